"""TEST-ONLY checks of the event-triggered re-solves of sensitivity-based MPC (do_mpc_amd/asmpc.py: select_device, set_law_members,
update_law_device, solve_members_device; closed_loop.BatchClosedLoopASMPC with settings.event_triggered), shared by the CPU suite
(host emulation of csrc/dompc_asmpc.hip) and the GPU suite: each check has the `hostemu=` switch of asmpc_common."""
import os
import re

import numpy as np

import asmpc_common as ac
import differentiator_batch_common as bc
from do_mpc_amd import asmpc as asmpc_mod
from do_mpc_amd.solver import STATS_DTYPE

SPAN = asmpc_mod.SELECT_SPAN             # loops per workgroup of the selection
# a wavefront edge, a workgroup edge, a batch long enough for the offsets across workgroups
SELECT_BATCHES = [1, 63, 64, 65, SPAN + 1, 3 * SPAN + 3]
SELECT_MASKS = [8, 3, 11]
MEMBER_SETS = [0, 1, 4, 5, 67]           # nothing, one, a full wavefront of the preparation, a partial one, all (descending)


def check_span_constant():
    text = open(os.path.join(os.path.dirname(asmpc_mod.__file__), "csrc", "dompc_asmpc_args.h")).read()
    threads, rounds = (int(re.search(rf"{k} = (\d+)", text).group(1)) for k in ("SELECT_THREADS", "SELECT_ROUNDS"))
    assert threads * rounds == SPAN and threads % 64 == 0


def _tensor(a, hostemu):
    import torch
    return torch.tensor(a, device="cpu" if hostemu else "cuda")


def _sync(hostemu):
    if not hostemu:
        import torch
        torch.cuda.synchronize()


def _patterns(B, rng):
    every_other, last, first = np.zeros(B, bool), np.zeros(B, bool), np.zeros(B, bool)
    every_other[::2], last[-1], first[0] = True, True, True
    return {"none": np.zeros(B, bool), "all": np.ones(B, bool), "every other": every_other, "only the last": last, "only the first": first,
            "random": rng.random(B) < 0.3}


def check_select(B, hostemu):
    """idx[:count] = flatnonzero(status & mask), count = its length, for statuses that also carry bit 2 and bits outside the mask"""
    a = ac.make_asmpc(ac.stub_mpc(4, 1), hostemu)
    rng = np.random.default_rng(1000 + B)
    for mask in SELECT_MASKS:
        a.settings.event_mask = mask
        bits = [b for b in (1, 2, 8) if mask & b]
        for what, want in _patterns(B, rng).items():
            status = np.zeros(B, dtype=np.int32)
            for b in np.flatnonzero(want):                    # a non-empty subset of the mask's bits
                chosen = [v for v in bits if rng.random() < 0.5] or [bits[int(rng.integers(len(bits)))]]
                status[b] = sum(chosen)
            status |= np.where(rng.random(B) < 0.5, 4, 0).astype(np.int32)                         # bit 2 must not select
            status |= (rng.integers(0, 16, B).astype(np.int32) & np.int32(11 & ~mask))               # nor a bit outside the mask
            expect = np.flatnonzero(status & mask)
            assert np.array_equal(expect, np.flatnonzero(want))
            st, idx, cnt = _tensor(status, hostemu), _tensor(np.full(B, -7, dtype=np.int32), hostemu), _tensor(np.full(1, -7, dtype=np.int32), hostemu)
            a.select_device(B, st.data_ptr(), idx.data_ptr(), cnt.data_ptr())
            _sync(hostemu)
            n = int(cnt.cpu().numpy()[0])
            assert n == expect.size, (B, mask, what, n, expect.size)
            assert np.array_equal(idx.cpu().numpy()[:n], expect), (B, mask, what)
            assert np.array_equal(st.cpu().numpy(), status)
    a.close()


# from workgroup SELECT_THREADS + 1 on (counted from 0), the strided sum over the counts of the workgroups before it takes a second
# round: 256 workgroups is the largest batch without one, 257 SPAN + 1 loops are 258 workgroups, the last with a single member
LARGE_SELECT_BATCHES = [256 * SPAN, 257 * SPAN + 1]


def check_select_large(B, hostemu):
    """check_select for batches of more than SELECT_THREADS workgroups, with the statuses drawn by array operations: count, idx[:count]
    = flatnonzero(status & mask), idx behind count untouched, status unchanged"""
    a = ac.make_asmpc(ac.stub_mpc(4, 1), hostemu)
    rng = np.random.default_rng(1000 + B)
    first_of_last = ((B - 1) // SPAN) * SPAN
    assert B > 256 * SPAN - 1 and first_of_last // SPAN >= 255
    for mask in (8, 11):
        a.settings.event_mask = mask
        bits = np.array([b for b in (1, 2, 8) if mask & b], dtype=np.int32)
        for what in ("none", "all", "only the last", "only the first of the last workgroup", "random"):
            want = np.zeros(B, bool)
            if what == "all":
                want[:] = True
            elif what == "only the last":
                want[-1] = True
            elif what == "only the first of the last workgroup":
                want[first_of_last] = True
            elif what == "random":
                want = rng.random(B) < 0.3
            # a non-empty subset of the mask's bits where wanted; bit 2 and bits outside the mask must not select
            subset = rng.integers(1, 2 ** bits.size, B)
            chosen = sum(((subset >> i) & 1).astype(np.int32) * bits[i] for i in range(bits.size))
            status = np.where(want, chosen, 0).astype(np.int32)
            status |= np.where(rng.random(B) < 0.5, 4, 0).astype(np.int32)
            status |= (rng.integers(0, 16, B).astype(np.int32) & np.int32(11 & ~mask))
            expect = np.flatnonzero(status & mask)
            assert np.array_equal(expect, np.flatnonzero(want))
            st, idx, cnt = _tensor(status, hostemu), _tensor(np.full(B, -7, dtype=np.int32), hostemu), _tensor(np.full(1, -7, dtype=np.int32), hostemu)
            a.select_device(B, st.data_ptr(), idx.data_ptr(), cnt.data_ptr())
            _sync(hostemu)
            n, got = int(cnt.cpu().numpy()[0]), idx.cpu().numpy()
            assert n == expect.size, (B, mask, what, n, expect.size)
            assert np.array_equal(got[:n], expect), (B, mask, what)
            assert np.all(got[n:] == -7), (B, mask, what)
            assert np.array_equal(st.cpu().numpy(), status)
    a.close()


def _same_law(La, Lb, cols=slice(None)):
    return all(np.array_equal(La[k][cols], Lb[k][cols], equal_nan=True) for k in ("x_ref", "u_ref", "M", "flags"))


def check_scatter(nx, nu, hostemu):
    """set_law, then set_law_members with fresh entries: the law = a fresh set_law of the merged arrays bit for bit, and every column
    that was not named is bit-equal to before"""
    B = 67
    merged = ac.record(nx, nu, B, seed=100 * nx + nu)
    a = ac.law_of(merged, hostemu)
    rng = np.random.default_rng(5)
    for n in MEMBER_SETS:
        before = a.law
        idx = np.arange(B)[::-1].copy() if n == B else rng.permutation(B)[:n]
        new = ac.record(nx, nu, n, seed=7000 + n)
        a.set_law_members(idx, new["x_prev"], new["u0"], new["J"], new["G"], new["ok"])
        assert a.batch == B
        for k in ("x_prev", "u0", "J", "G"):
            merged[k][idx] = new[k]
        fresh = ac.law_of(merged, hostemu)
        now, ref = a.law, fresh.law
        others = np.setdiff1d(np.arange(B), idx)
        assert _same_law(now, ref, idx), n
        assert _same_law(now, before, others), n
        assert _same_law(now, ref), n
        if n:
            assert np.array_equal(now["x_ref"][idx], new["x_prev"]) and not _same_law(now, before, idx)
        fresh.close()
    a.close()


def check_scatter_fallbacks(hostemu):
    """the fallbacks of asmpc_common.check_fallbacks through the scatter route: each flags its own column only"""
    base = ac.record(4, 2, 5, seed=11)
    good = ac.law_of(base, hostemu)
    Lg = good.law
    Ug, _ = good.make_step_batch(base["X"])
    other = ac.record(4, 2, 5, seed=12)
    for what, member, bit in (("singular", 1, 2), ("not ok", 2, 1), ("nan", 3, 1)):
        r = {k: v.copy() for k, v in base.items()}
        if what == "singular":
            r["G"][member] = np.eye(2) - np.array([[1.0, 2.0], [2.0, 4.0]])
        elif what == "not ok":
            r["ok"][member] = False
        else:
            r["J"][member, 1, 2] = np.nan
        expect = np.zeros(5, dtype=np.int32)
        expect[member] = bit
        others = [b for b in range(5) if b != member]
        # all five through the scatter, in another order, over a law of other numbers
        a = ac.law_of(other, hostemu)
        idx = np.array([3, 0, 4, 2, 1])
        a.set_law_members(idx, r["x_prev"][idx], r["u0"][idx], r["J"][idx], r["G"][idx], r["ok"][idx])
        L = a.law
        U, st = a.make_step_batch(r["X"])
        assert np.array_equal(L["flags"], expect) and np.array_equal(st, expect), (what, L["flags"], st)
        assert not L["M"][member].any() and np.array_equal(U[member], r["u0"][member]), what
        assert np.array_equal(L["M"][others], Lg["M"][others]) and np.array_equal(U[others], Ug[others]), what
        a.close()
        # the bad member alone into the good law: its column is flagged, the others are the good law's
        a = ac.law_of(base, hostemu)
        a.set_law_members([member], r["x_prev"][[member]], r["u0"][[member]], r["J"][[member]], r["G"][[member]], r["ok"][[member]])
        L = a.law
        assert np.array_equal(L["flags"], expect) and not L["M"][member].any() and _same_law(L, Lg, others), what
        a.close()
    good.close()


def check_member_refusals(hostemu):
    """duplicate or out-of-range members: ValueError on the host, the law stays as it is"""
    r = ac.record(4, 2, 5, seed=21)
    a = ac.law_of(r, hostemu)
    before = a.law
    new = ac.record(4, 2, 2, seed=22)
    for idx, word in (([1, 1], "distinct"), ([0, 5], "[0, 5)"), ([-1, 2], "[0, 5)")):
        try:
            a.set_law_members(idx, new["x_prev"], new["u0"], new["J"], new["G"])
        except ValueError as e:
            assert word in str(e), str(e)
        else:
            raise AssertionError(f"not refused: {idx}")
    assert _same_law(a.law, before)
    a.close()


# ---------------------------------------------------------------------------------------------- the loops
def check_all_selected_is_the_mpc_loop(make_mpc, name):
    """(GPU only: BatchClosedLoop has no host flavour.)  max_dx = 0 with a period that never comes: every step after the first selects
    all five members, idx the identity - the solve calls of BatchClosedLoop, and its u0 and x bit for bit"""
    from do_mpc_amd.closed_loop import BatchClosedLoop
    X0 = bc.batch_states(name)
    loop = ac.make_loop(make_mpc, name, False, 100, event_triggered=True, max_dx=0.0)
    ref = BatchClosedLoop(make_mpc(name, max_batch=5), ac.make_plant(name, False), X0)
    for k in range(3):
        r, q = loop.step(), ref.step()
        assert r["solved"] == (k == 0) and r["stats"]["success"].all() and q["stats"]["success"].all()
        du, dx = float(np.max(np.abs(r["u0"] - q["u0"]))), float(np.max(np.abs(r["x"] - q["x"])))
        print(f"{name} step {k}: max |u - u_mpc| = {du:.3e}, max |x - x_mpc| = {dx:.3e}, law status {r['law_status']}, resolved {r['resolved']}")
        assert np.array_equal(r["resolved"], np.arange(5) if k else np.zeros(0, dtype=int)), (k, r["resolved"])
        assert np.array_equal(r["u0"], q["u0"]) and np.array_equal(r["x"], q["x"]), (k, du, dx)


def check_nothing_selected_is_todays_loop(make_mpc, name, hostemu):
    on = ac.make_loop(make_mpc, name, hostemu, 3, event_triggered=True, max_dx=1e300).run(6, fused=False)
    off = ac.make_loop(make_mpc, name, hostemu, 3, max_dx=1e300).run(6, fused=False)
    assert ac.same_records(on, off)
    assert len(on["events"]) == 6 and all(e.size == 0 for e in on["events"]) and "events" not in off
    assert on["solve_steps"] == [0, 3]


def check_some_members_selected(make_mpc, name, hostemu):
    """an event that selects 0 < n < 5 members: their inputs and law columns are those of a solve of the same n members by calls that
    exist without the feature, the other members' are the event-free loop's - bit for bit"""
    import torch
    B = 5
    X0 = bc.batch_states(name)
    probe = ac.make_loop(make_mpc, name, hostemu, 100)
    xs = np.asarray(probe.mpc._x_scaling.master, float).reshape(-1)
    d = np.max(np.abs(probe.step()["x"] - X0) / xs, axis=1)
    ds = np.sort(d)
    assert ds[2] != ds[3], ds
    thr = 0.5 * (ds[2] + ds[3])
    ev = ac.make_loop(make_mpc, name, hostemu, 100, event_triggered=True, max_dx=thr)
    sh = ac.make_loop(make_mpc, name, hostemu, 100, max_dx=thr)
    r0, s0 = ev.step(), sh.step()
    assert r0["resolved"].size == 0 and all(np.array_equal(r0[k], s0[k]) for k in ("u0", "x", "law_status"))
    # the reference for step 1, from the shadow loop's own tensors
    idx = np.flatnonzero(d > thr)
    n = idx.size
    assert 0 < n < B and n == 2
    ps = sh.ps
    P = sh.P.clone()
    if ps.ntvp or ps.np_:
        tm = sh.t_mpc0 + sh.k * sh.dt_mpc
        row = sh._p_row.copy()
        row[ps.p_off_tvp:ps.p_off_p] = sh.mpc.tvp_fun(tm).master
        row[ps.p_off_p:ps.p_off_uprev] = sh.mpc.p_fun(tm).master
        P[:, ps.p_off_tvp:ps.p_off_uprev] = torch.from_numpy(row[ps.p_off_tvp:ps.p_off_uprev].copy()).to(sh.dev)
    P[:, :ps.nx] = sh.X
    P[:, ps.p_off_uprev:] = sh.U
    ix = torch.from_numpy(idx).to(sh.dev)
    e = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=sh.dev)      # noqa: E731
    second = ac.make_asmpc(make_mpc(name, max_batch=5), hostemu)
    second.settings.max_dx = thr
    second.solve_device(sh.guess[ix].contiguous(), P[ix].contiguous(), e(n, ps.n_opt_x), e(n, ps.n_g), e(n), e(n * STATS_DTYPE.itemsize, dt=torch.uint8))
    Xm, Um, stm = sh.X[ix].contiguous(), e(n, ps.nu), e(n, dt=torch.int32)
    second.make_step_batch_device(n, Xm.data_ptr(), Um.data_ptr(), stm.data_ptr())
    _sync(hostemu)
    u_ref, law_ref = Um.cpu().numpy(), second.law
    assert not (stm.cpu().numpy() & 8).any()
    # step 1
    r1, s1 = ev.step(), sh.step()
    assert not r1["solved"] and np.array_equal(r1["resolved"], idx), (r1["resolved"], idx)
    others = np.setdiff1d(np.arange(B), idx)
    du = float(np.max(np.abs(r1["u0"][idx] - u_ref)))
    print(f"{name}: distances {d}, max_dx = {thr:.6e}, selected {idx}, max |u - reference| = {du:.3e}, "
          f"max |u - shadow| of the selected = {np.max(np.abs(r1['u0'][idx] - s1['u0'][idx])):.3e}")
    assert np.array_equal(r1["u0"][idx], u_ref), du
    Le, Ls = ev.asmpc.law, sh.asmpc.law
    for k in ("x_ref", "u_ref", "M", "flags"):
        assert np.array_equal(Le[k][idx], law_ref[k]), k
        assert np.array_equal(Le[k][others], Ls[k][others]), k
    assert np.array_equal(r1["u0"][others], s1["u0"][others]) and np.array_equal(r1["x"][others], s1["x"][others])
    assert (s1["law_status"][idx] & 8).all() and not (s1["law_status"][others] & 8).any()
    assert (r1["law_status"][idx] & 16).all() and not (r1["law_status"][idx] & 8).any() and not (r1["law_status"][others] & 24).any()
    assert "stats" in r1 and r1["stats"]["success"][idx].all()
    # three more steps
    seen = set(idx.tolist())
    for k in range(2, 5):
        r, s = ev.step(), sh.step()
        m = r["resolved"]
        seen |= set(m.tolist())
        assert not (r["law_status"][m] & 8).any() and (r["law_status"][m] & 16).all(), (k, r["law_status"])
        rest = np.setdiff1d(np.arange(B), m)
        assert not (r["law_status"][rest] & 16).any()
        never = np.array(sorted(set(range(B)) - seen), dtype=int)
        assert np.array_equal(r["u0"][never], s["u0"][never]) and np.array_equal(r["x"][never], s["x"][never]), k
        print(f"{name} step {k}: resolved {m}, law status {r['law_status']}")
    second.close()


def check_make_step_event(make_mpc, name, hostemu, n=4):
    """ASMPC.make_step with max_dx = 0 and a period that never comes = resolve_every = 1 bit for bit: both solve on every call"""
    us = []
    for settings in (dict(event_triggered=True, max_dx=0.0, resolve_every=100), dict(resolve_every=1)):
        mpc = make_mpc(name)
        a = ac.make_asmpc(mpc, hostemu)
        for k, v in settings.items():
            setattr(a.settings, k, v)
        sim = ac.make_plant(name, hostemu)
        x0 = bc.batch_states(name)[0].reshape(-1, 1)
        mpc.x0 = x0
        mpc.u0 = np.zeros((mpc.model.n_u, 1))
        mpc.set_initial_guess()
        sim.x0 = x0
        for k in range(n):
            u = a.make_step(x0)
            x0 = sim.make_step(u)
        us.append((a.u_data.copy(), float(np.asarray(mpc._t0).ravel()[0])))
        a.close()
    assert us[0][0].shape[1] == n + 1 and np.array_equal(us[0][0], us[1][0]), np.max(np.abs(us[0][0] - us[1][0]))
    assert us[0][1] == us[1][1]                                   # (the controller's clock moved once per call in both)
    assert np.max(np.abs(us[0][0][:, 2] - us[0][0][:, 1])) > 0.0


def check_fused_is_refused(make_mpc, hostemu):
    loop = ac.make_loop(make_mpc, "batch_reactor", hostemu, 3, event_triggered=True)
    try:
        loop.run(2, fused=True)
    except NotImplementedError as e:
        assert "fused=False" in str(e), str(e)
    else:
        raise AssertionError("run(fused=True) with event_triggered was accepted")
