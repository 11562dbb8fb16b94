"""Rate and accuracy of the device-resident sensitivity-based MPC loop (do_mpc_amd/asmpc.py, closed_loop.BatchClosedLoopASMPC) on one
GPU, for batch_reactor and CSTR at B = 16 384 loops with resident states:

  * loop steps per second of BatchClosedLoopASMPC.run for resolve_every in {1, 5, 20}, fused (the steps between two solves in one
    launch) and step-wise, and of BatchClosedLoop (a full solve every step) on the same states - the configurations alternate in one
    process over `--rounds` rounds; device events around at least `--seconds` of whole control cycles after one warm-up cycle.  The
    time of run() includes its copies of the trajectories to the host, as BatchClosedLoop.step includes its own.
  * what the approximation costs: for each period max |u - u_mpc| over a 20-step loop of the five members of
    tests/differentiator_batch_common.batch_states, u_mpc a fresh cold solve at the same state and previous input (on the GPU).

usage: python tools/gpu_asmpc_rate.py [--seconds 1.0] [--rounds 2] [--batch 16384] [--out profiles/asmpc_rate.txt]"""
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
from do_mpc_amd.closed_loop import BatchClosedLoop, BatchClosedLoopASMPC
from do_mpc_amd.examples import CASES

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--periods", type=int, nargs="*", default=[1, 5, 20])
ap.add_argument("--cases", nargs="*", default=["batch_reactor", "CSTR"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asmpc_rate.txt"))
args = ap.parse_args()
lines = []


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


say(f"# tools/gpu_asmpc_rate.py --seconds {args.seconds} --rounds {args.rounds} --batch {args.batch} on {torch.cuda.get_device_name(0)}")
B = args.batch
for name in args.cases:
    ex = CASES[name]
    S = bc.batch_states(name)
    rng = np.random.default_rng(0)
    X0 = S[rng.integers(0, len(S), B)] * rng.uniform(0.99, 1.01, (B, S.shape[1]))
    mpc = ex.build_mpc(ex.build_model(), max_batch=B)
    sim = ac.make_plant(name, hostemu=False)
    say(f"## {name}, B = {B}: loop steps per second (loops x control steps / s)")
    for rnd in range(args.rounds):
        ref = BatchClosedLoop(mpc, sim, X0)
        rate = timed(lambda: ref.step(), 1)
        say(f"| round {rnd} | BatchClosedLoop (a solve every step) | {B * rate:.4e} loop steps/s | {rate:.3f} control steps/s |")
        for period in args.periods:
            for fused in (True, False):
                a = ASMPC(mpc)
                a.settings.resolve_every = period
                loop = BatchClosedLoopASMPC(a, sim, X0)
                bits = {"law": 0, "plant": 0}

                def cycle():
                    r = loop.run(period, fused=fused)
                    bits["law"] |= int(np.bitwise_or.reduce(r["law_status"].ravel()))
                    bits["plant"] += int(r["plant_status"].sum())
                rate = timed(cycle, period)
                say(f"| round {rnd} | BatchClosedLoopASMPC resolve_every = {period}, {'fused' if fused else 'step-wise'} | "
                    f"{B * rate:.4e} loop steps/s | {rate:.3f} control steps/s | law status bits seen: {bits['law']:#x}, plant failures: {bits['plant']} |")
                a.close()
    del mpc

say("## what the approximation costs: max |u - u_mpc| over a 20-step loop of the five batch_states members, u_mpc a fresh cold solve at the "
    "same state and previous input (GPU)")
for name in args.cases:
    ex = CASES[name]
    fresh = ex.build_mpc(ex.build_model(), max_batch=5)
    lb, ub = fresh._u_lb.master, fresh._u_ub.master
    for period in args.periods:
        loop = ac.make_loop(lambda n, **kw: CASES[n].build_mpc(CASES[n].build_model(), **kw), name, False, period)
        x, u_prev = bc.batch_states(name), np.zeros((5, fresh.model.n_u))
        worst, worst_rel, failed = 0.0, 0.0, 0
        for k in range(20):
            r = loop.step()
            q = fresh.make_step_batch(x, U_prev=u_prev)
            ok = q["stats"]["success"] != 0
            failed += int((~ok).sum())
            d = np.abs(r["u0"] - q["u0"])[ok]
            if d.size:
                worst = max(worst, float(d.max()))
                worst_rel = max(worst_rel, float((d / (ub - lb)).max()))
            x, u_prev = r["x"], r["u0"]
        say(f"| {name} | resolve_every = {period} | max |u - u_mpc| = {worst:.3e} | relative to the input range {worst_rel:.3e} | "
            f"fresh solves that failed: {failed} |")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
