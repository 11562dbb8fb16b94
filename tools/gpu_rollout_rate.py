"""Rate of the general plant rollout (csrc/dompc_plant.hip: dompc_plant_loop_kernel) on one GPU at B = 16 384 loops with resident states:

  * loop steps per second of BatchClosedLoopLQR.run(n) - per control step a handful of torch launches for the gain, one plant launch, a
    synchronisation and three copies to the host - and of run(n, fused=True) - n steps in one launch, one synchronisation, one copy - for
    oscillating_masses_lqr (discrete plant: launch-bound) and cstr_lqr (continuous plant: integrator-bound).  Both record the same
    trajectories on the host; the time includes those copies.
  * open loop: K control steps with given inputs as ONE call of Simulator.rollout_device against K calls of step_batch_device, on device
    buffers (what Simulator.simulate_batch does between its upload and its download), same two plants.

The paths alternate in one process over `--rounds` rounds; per path and round device events around at least `--seconds` of whole runs
after one discarded run.  The last lines give the ratios per round and how far the rounds are apart.

usage: python tools/gpu_rollout_rate.py [--seconds 1.0] [--rounds 3] [--batch 16384] [--steps 20] [--out profiles/rollout_rate.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lqr_common as lc
from do_mpc_amd.closed_loop import BatchClosedLoopLQR

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--steps", type=int, default=20, help="control steps per run / per open-loop call")
ap.add_argument("--cases", nargs="*", default=["oscillating_masses_lqr", "cstr_lqr"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_rate.txt"))
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(cycle, steps_per_cycle):
    """-> control steps per second: device events around whole cycles until args.seconds have been measured, after one discarded cycle"""
    cycle()
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


def spread(v):
    return (max(v) - min(v)) / (sum(v) / len(v))


say(f"# tools/gpu_rollout_rate.py --seconds {args.seconds} --rounds {args.rounds} --batch {args.batch} --steps {args.steps} "
    f"on {torch.cuda.get_device_name(0)}")
B, n = args.batch, args.steps
dev = torch.device("cuda", 0)
for name in args.cases:
    ex, plant, lqr = lc.example(name, hostemu=False)
    sim = ex.build_simulator(plant)
    if name == "cstr_lqr":
        lqr.set_setpoint(xss=ex.XSS, uss=ex.USS)
        X0 = ex.XSS.ravel()[None, :] * (1.0 + 0.01 * np.random.default_rng(0).uniform(-1, 1, (B, 4)))
    else:
        X0 = ex.X0[None, :] * (1.0 + 0.3 * np.random.default_rng(0).uniform(-1, 1, (B, 4)))
    m = sim.model
    say(f"## {name} ({m.model_type} plant), B = {B}, {n} control steps per run: loop steps per second (loops x control steps / s)")
    rates = {"step-wise": [], "fused": []}
    failures = 0
    loop = BatchClosedLoopLQR(lqr, sim, X0)                  # (one loop, set back to the start before every run: the law is formed once)
    X0_dev = loop.plant.X.clone()
    for rnd in range(args.rounds):
        for path in ("step-wise", "fused"):
            def cycle():
                global failures
                loop.plant.X.copy_(X0_dev)
                loop.U = torch.zeros_like(loop.U)
                loop.k = 0
                r = loop.run(n, fused=path == "fused")
                failures += int(r["plant_status"].sum())
            rate = timed(cycle, n)
            rates[path].append(rate)
            say(f"| round {rnd} | BatchClosedLoopLQR.run({n}{', fused=True' if path == 'fused' else ''}) | {B * rate:.4e} loop steps/s | "
                f"{rate:.2f} control steps/s |")
    ratio = [f / s for f, s in zip(rates["fused"], rates["step-wise"])]
    say(f"| {name} | fused / step-wise per round: {', '.join(f'{r:.2f}' for r in ratio)} | rounds apart by {spread(rates['step-wise']):.1%} "
        f"(step-wise) and {spread(rates['fused']):.1%} (fused) of their mean | plant failures: {failures} |")

    # open loop on device buffers: the inputs of the fused run above, replayed
    loop.plant.X.copy_(X0_dev)
    loop.U = torch.zeros_like(loop.U)
    loop.k = 0
    rec = loop.run(n, fused=True)
    U = torch.tensor(rec["u"], dtype=torch.float64, device=dev)
    Xt = torch.empty((n + 1, B, m.n_x), dtype=torch.float64, device=dev)
    Xt[0].copy_(torch.tensor(X0, dtype=torch.float64, device=dev))
    st = torch.zeros((n, B), dtype=torch.int32, device=dev)
    dummy = torch.zeros(8, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def one_call():
        sim.rollout_device(B, n, Xt.data_ptr(), U.data_ptr(), plant_status=st.data_ptr(), stream=stream)

    def k_calls():
        for k in range(n):
            sim.step_batch_device(B, Xt[k].data_ptr(), U[k].data_ptr(), dummy.data_ptr(), dummy.data_ptr(), Xt[k + 1].data_ptr(), 0,
                                  st[k].data_ptr(), shared_mask=2 | 4 | 8 | 16, stream=stream)
    rates = {"K launches": [], "one launch": []}
    for rnd in range(args.rounds):
        for path, cycle in (("K launches", k_calls), ("one launch", one_call)):
            rate = timed(cycle, n)
            rates[path].append(rate)
            say(f"| round {rnd} | open loop, {n} steps, {path} | {B * rate:.4e} loop steps/s | {rate:.2f} control steps/s |")
    one_call()
    torch.cuda.synchronize()
    x_one = Xt.cpu().numpy().copy()
    k_calls()
    torch.cuda.synchronize()
    same = np.array_equal(x_one.view(np.uint64), Xt.cpu().numpy().view(np.uint64))
    ratio = [f / s for f, s in zip(rates["one launch"], rates["K launches"])]
    say(f"| {name} | open loop, one launch / K launches per round: {', '.join(f'{r:.2f}' for r in ratio)} | rounds apart by "
        f"{spread(rates['K launches']):.1%} (K launches) and {spread(rates['one launch']):.1%} (one launch) of their mean | "
        f"trajectories of the two equal bit for bit: {same} |")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
