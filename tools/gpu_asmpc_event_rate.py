"""Rate and price of event-triggered re-solves in the device-resident sensitivity-based MPC loop (do_mpc_amd/asmpc.py,
closed_loop.BatchClosedLoopASMPC with settings.event_triggered) on one GPU, for batch_reactor and CSTR at B = 16 384 loops with resident
states.  Modelled on tools/gpu_asmpc_rate.py: the same states, the same warm-up, the configurations alternating in one process over
`--rounds` rounds, device events around at least `--seconds` of whole cycles after one warm-up cycle.

  * loop steps per second of run(n, fused=False) for the periodic modes (resolve_every in {1, 5, 20}, no events) beside the
    event-triggered mode (resolve_every so large that no period comes again after the first solve) at the values `--max-dx`, and for
    each event run the mean share of members re-solved per step over the timed steps.  The share of an event-triggered run is no
    constant - it falls as the loops settle -, so a rate belongs to its window.  Two windows: (a) the first `--window` = 20 steps of
    a fresh loop at the start states, for every configuration - the window the price is taken over, so that rate and price can be
    put side by side; its first step is the cold solve everywhere.  (b) for the event-triggered runs, the same loop going on after
    one more warm-up cycle, timed as tools/gpu_asmpc_rate.py times the periodic modes (whose rates in that steady regime are in
    profiles/asmpc_rate.txt).
  * the price, as profiles/asmpc_rate.txt states it for the periodic modes: max |u - u_mpc| over a 20-step loop of the five members of
    tests/differentiator_batch_common.batch_states, relative to the input range, u_mpc a fresh cold solve at the same state and
    previous input - for the periodic modes and for each max_dx, with the share of members re-solved there.
  * what the mode costs when it does nothing: the time of the selection alone (two launches) with nothing selected, beside the launch
    of the law step, at B = 16 384 and 262 144 on a synthetic law (n_x = 4, n_u = 1).

usage: python tools/gpu_asmpc_event_rate.py [--seconds 1.0] [--rounds 2] [--batch 16384] [--out profiles/asmpc_event_rate.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import asmpc_common as ac
import differentiator_batch_common as bc
from do_mpc_amd.asmpc import ASMPC
from do_mpc_amd.closed_loop import BatchClosedLoopASMPC
from do_mpc_amd.examples import CASES

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--window", type=int, default=20, help="control steps of a fresh loop that are timed: the window of the price")
ap.add_argument("--cycle", type=int, default=10, help="control steps per timed cycle of an event-triggered loop that goes on")
ap.add_argument("--periods", type=int, nargs="*", default=[1, 5, 20])
ap.add_argument("--max-dx", type=float, nargs="*", default=[0.03, 0.1, 0.3])
ap.add_argument("--cases", nargs="*", default=["batch_reactor", "CSTR"])
ap.add_argument("--select-batches", type=int, nargs="*", default=[16384, 262144])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asmpc_event_rate.txt"))
args = ap.parse_args()
lines = []
NEVER = 10 ** 9                                               # a period that does not come again


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(cycle, steps_per_cycle):
    """-> control steps per second: device events around whole cycles until args.seconds have been measured"""
    cycle()                                                   # warm-up: one cycle (the first solve is a cold one)
    torch.cuda.synchronize()
    total, n = 0.0, 0
    while total < args.seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cycle()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
        n += steps_per_cycle
    return n / total


say(f"# tools/gpu_asmpc_event_rate.py --seconds {args.seconds} --rounds {args.rounds} --batch {args.batch} --window {args.window} --cycle {args.cycle} "
    f"on {torch.cuda.get_device_name(0)}")
B = args.batch
for name in args.cases:
    ex = CASES[name]
    S = bc.batch_states(name)
    rng = np.random.default_rng(0)
    X0 = S[rng.integers(0, len(S), B)] * rng.uniform(0.99, 1.01, (B, S.shape[1]))
    mpc = ex.build_mpc(ex.build_model(), max_batch=B)
    sim = ac.make_plant(name, hostemu=False)
    say(f"## {name}, B = {B}: loop steps per second (loops x control steps / s), run(n, fused=False)")
    for rnd in range(args.rounds):
        for period, max_dx in [(p, None) for p in args.periods] + [(NEVER, v) for v in args.max_dx]:
            a = ASMPC(mpc)
            a.settings.resolve_every = period
            if max_dx is not None:
                a.settings.event_triggered, a.settings.max_dx = True, max_dx
            seen = {"law": 0, "plant": 0, "resolved": 0, "steps": 0}

            def count(r, steps):
                seen["law"] |= int(np.bitwise_or.reduce(r["law_status"].ravel()))
                seen["plant"] += int(r["plant_status"].sum())
                seen["resolved"] += sum(int(e.size) for e in r.get("events", []))
                seen["steps"] += steps

            # (a) the window the price below is taken over: the first args.window steps of a fresh loop at X0 (its first step is the cold
            #     solve in every configuration); the loop is built outside the timed region
            BatchClosedLoopASMPC(a, sim, X0).run(args.window, fused=False)        # warm-up: one cycle
            torch.cuda.synchronize()
            total, n = 0.0, 0
            while total < args.seconds:
                loop = BatchClosedLoopASMPC(a, sim, X0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = loop.run(args.window, fused=False)
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1) * 1e-3
                n += args.window
                count(r, args.window)
            rate = n / total
            name_ = f"resolve_every = {period}, no events" if max_dx is None else f"event-triggered, max_dx = {max_dx:g}"
            share = "" if max_dx is None else f" share of members re-solved per step {seen['resolved'] / (B * seen['steps']):.4f} |"
            say(f"| round {rnd} | steps 0 .. {args.window - 1} from the start | {name_} |{share} {B * rate:.4e} loop steps/s | {rate:.3f} control steps/s | "
                f"law status bits seen: {seen['law']:#x}, plant failures: {seen['plant']} |")
            # (b) the loop going on from there (as tools/gpu_asmpc_rate.py times the periodic modes): the share falls as the loops settle
            if max_dx is not None:
                seen.update(resolved=0, steps=0)
                first = [True]

                def cycle():
                    r = loop.run(args.cycle, fused=False)
                    if not first[0]:
                        count(r, args.cycle)
                    first[0] = False
                rate = timed(cycle, args.cycle)
                say(f"| round {rnd} | steps {args.window + args.cycle} .. {args.window + args.cycle + seen['steps'] - 1} of the same loop | {name_} | share of members "
                    f"re-solved per step {seen['resolved'] / (B * seen['steps']):.4f} | {B * rate:.4e} loop steps/s | {rate:.3f} control steps/s |")
            a.close()
    del mpc

say("## the price: max |u - u_mpc| over a 20-step loop of the five batch_states members, u_mpc a fresh cold solve at the same state and "
    "previous input (GPU); share: members re-solved by an event per step")
for name in args.cases:
    ex = CASES[name]
    fresh = ex.build_mpc(ex.build_model(), max_batch=5)
    lb, ub = fresh._u_lb.master, fresh._u_ub.master
    make = lambda n, **kw: CASES[n].build_mpc(CASES[n].build_model(), **kw)      # noqa: E731
    for period, max_dx in [(p, None) for p in args.periods] + [(NEVER, v) for v in args.max_dx]:
        loop = ac.make_loop(make, name, False, period, **({} if max_dx is None else {"event_triggered": True, "max_dx": max_dx}))
        x, u_prev = bc.batch_states(name), np.zeros((5, fresh.model.n_u))
        worst, worst_rel, failed, resolved = 0.0, 0.0, 0, 0
        for k in range(20):
            r = loop.step()
            q = fresh.make_step_batch(x, U_prev=u_prev)
            ok = q["stats"]["success"] != 0
            failed += int((~ok).sum())
            d = np.abs(r["u0"] - q["u0"])[ok]
            if d.size:
                worst = max(worst, float(d.max()))
                worst_rel = max(worst_rel, float((d / (ub - lb)).max()))
            resolved += int(r["resolved"].size) if max_dx is not None else 0
            x, u_prev = r["x"], r["u0"]
        what = f"resolve_every = {period}" if max_dx is None else f"event-triggered, max_dx = {max_dx:g} | share {resolved / 100.0:.2f}"
        say(f"| {name} | {what} | max |u - u_mpc| = {worst:.3e} | relative to the input range {worst_rel:.3e} | "
            f"fresh solves that failed: {failed} |")

say("## the mode when it does nothing: the selection alone (two launches, nothing selected) beside the launch of the law step, "
    "synthetic law n_x = 4, n_u = 1; microseconds per call, device events around 200 calls after 20")
for Bs in args.select_batches:
    r = ac.record(4, 1, Bs, seed=1)
    a = ac.law_of(r, False)
    dev = torch.device("cuda", 0)
    X = torch.tensor(r["x_prev"], device=dev)                 # at the expansion point: no status bit
    U = torch.empty((Bs, 1), dtype=torch.float64, device=dev)
    st, idx, cnt = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (Bs, Bs, 1))
    stream = torch.cuda.current_stream().cuda_stream
    calls = {"law step": lambda: a.make_step_batch_device(Bs, X.data_ptr(), U.data_ptr(), st.data_ptr(), stream=stream),
             "selection": lambda: a.select_device(Bs, st.data_ptr(), idx.data_ptr(), cnt.data_ptr(), stream=stream)}
    for rnd in range(args.rounds):
        for what, call in calls.items():
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                call()
            e1.record()
            torch.cuda.synchronize()
            assert int(cnt.item()) == 0 and not int(st.any().item())
            say(f"| round {rnd} | B = {Bs} | {what} | {e0.elapsed_time(e1) * 1e3 / 200:.2f} us per call |")
    a.close()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
