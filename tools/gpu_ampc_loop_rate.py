"""Rate of the fused approximate-MPC loop (csrc/dompc_ampc_loop.hip: dompc_ampc_loop_kernel) on one GPU, CSTR plant with the stored 1 x 50
network of the reference and with the default 3 x 50 network, B = 16 384 and 262 144 loops, 20 control steps per run:

  (a) loop steps per second of BatchClosedLoopAMPC.run(n) - per control step two launches, a synchronisation and three copies to the
      host: the yardstick - and of run(n, fused=True) - n steps in one launch, one synchronisation, one copy.  Both record the same
      trajectories on the host; the wall-clock time includes those copies.
  (b) on device buffers: ONE call of Simulator.rollout_ampc_device for n steps against n x (make_step_batch_device +
      step_batch_device) with no synchronisation in between - kernel time without the host's share; device events.

The paths alternate in one process over `--rounds` rounds; per path and round at least `--seconds` of whole runs after one discarded
run.  The last lines of a block give the ratios per round and how far the rounds are apart.

usage: python tools/gpu_ampc_loop_rate.py [--seconds 0.5] [--rounds 3] [--batches 16384 262144] [--steps 20] [--out profiles/ampc_loop_rate.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ampc_common as ac
from do_mpc_amd.closed_loop import BatchClosedLoopAMPC
from do_mpc_amd.examples import cstr_ampc as ex

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="*", default=[16384, 262144])
ap.add_argument("--steps", type=int, default=20, help="control steps per run / per device call")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ampc_loop_rate.txt"))
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(cycle, steps_per_cycle, events):
    """-> control steps per second over whole cycles until args.seconds have been measured, after one discarded cycle; `events`: device
    events around each cycle, else the wall clock around a cycle that ends synchronised"""
    cycle()
    torch.cuda.synchronize()
    total, n = 0.0, 0
    while total < args.seconds:
        if events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cycle()
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1) * 1e-3
        else:
            t0 = time.perf_counter()
            cycle()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        n += steps_per_cycle
    return n / total


def spread(v):
    return (max(v) - min(v)) / (sum(v) / len(v))


say(f"# tools/gpu_ampc_loop_rate.py --seconds {args.seconds} --rounds {args.rounds} --steps {args.steps} on {torch.cuda.get_device_name(0)}")
n = args.steps
dev = torch.device("cuda", 0)
nets = {"stored 1 x 50 (tanh)": ac.stored_cstr(hostemu=False),
        "default 3 x 50 (tanh)": ac.network(4, 2, True, hostemu=False, box=ac.CSTR_BOX, n_hidden_layers=3, n_neurons=50)}
sim = ex.build_simulator(ex.build_model())
for label, ampc in nets.items():
    for B in args.batches:
        rng = np.random.default_rng(0)
        X0 = ex.X0 * rng.uniform(0.95, 1.05, (B, 4))
        say(f"## CSTR plant, network {label}, B = {B}, {n} control steps per run")
        # ---- (a) the loop, records copied to the host
        loop = BatchClosedLoopAMPC(ampc, sim, X0, U_prev0=np.tile(ex.U0, (B, 1)))
        X0_dev, U0_dev = loop.plant.X.clone(), loop.U.clone()
        rates = {"step-wise": [], "fused": []}
        failures = 0
        for rnd in range(args.rounds):
            for path in ("step-wise", "fused"):
                def cycle():
                    global failures
                    loop.plant.X.copy_(X0_dev)
                    loop.U.copy_(U0_dev)
                    loop.k = 0
                    r = loop.run(n, fused=path == "fused")
                    failures += int(r["plant_status"].sum())
                rate = timed(cycle, n, events=False)
                rates[path].append(rate)
                say(f"| (a) round {rnd} | BatchClosedLoopAMPC.run({n}{', fused=True' if path == 'fused' else ''}) | {B * rate:.4e} loop steps/s | "
                    f"{1e6 / rate:.1f} us per control step |")
        ratio = [f / s for f, s in zip(rates["fused"], rates["step-wise"])]
        say(f"| (a) {label}, B = {B} | fused / step-wise per round: {', '.join(f'{r:.2f}' for r in ratio)} | rounds apart by "
            f"{spread(rates['step-wise']):.1%} (step-wise) and {spread(rates['fused']):.1%} (fused) of their mean | fused faster in every round: "
            f"{all(r > 1.0 for r in ratio)} | plant failures: {failures} |")
        # ---- (b) device buffers, no host copies
        Xt = torch.empty((n + 1, B, 4), dtype=torch.float64, device=dev)
        Ut = torch.empty((n, B, 2), dtype=torch.float64, device=dev)
        st = torch.zeros((n, B), dtype=torch.int32, device=dev)
        Xt[0].copy_(X0_dev)
        p_row = torch.tensor(np.asarray(sim.p_fun(0.0).master, float).reshape(-1), dtype=torch.float64, device=dev)
        p_rows = p_row.repeat(n, 1).contiguous()
        dummy = torch.zeros(8, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def one_call():
            sim.rollout_ampc_device(ampc, B, n, Xt.data_ptr(), Ut.data_ptr(), U_prev0=U0_dev.data_ptr(), p_rows=p_rows.data_ptr(),
                                    plant_status=st.data_ptr(), stream=stream)

        def pairs_of_calls():
            for k in range(n):
                ampc.make_step_batch_device(B, Xt[k].data_ptr(), (U0_dev if k == 0 else Ut[k - 1]).data_ptr(), Ut[k].data_ptr(), stream=stream)
                sim.step_batch_device(B, Xt[k].data_ptr(), Ut[k].data_ptr(), dummy.data_ptr(), p_row.data_ptr(), Xt[k + 1].data_ptr(), 0,
                                      st[k].data_ptr(), shared_mask=2 | 4 | 8 | 16, stream=stream)
        rates = {"2 n launches": [], "one launch": []}
        for rnd in range(args.rounds):
            for path, cycle in (("2 n launches", pairs_of_calls), ("one launch", one_call)):
                rate = timed(cycle, n, events=True)
                rates[path].append(rate)
                say(f"| (b) round {rnd} | device buffers, {n} steps, {path} | {B * rate:.4e} loop steps/s | {1e6 / rate:.1f} us per control step |")
        one_call()
        torch.cuda.synchronize()
        x_one, u_one = Xt.cpu().numpy().copy(), Ut.cpu().numpy().copy()
        pairs_of_calls()
        torch.cuda.synchronize()
        same = np.array_equal(x_one.view(np.uint64), Xt.cpu().numpy().view(np.uint64)) and np.array_equal(u_one.view(np.uint64), Ut.cpu().numpy().view(np.uint64))
        ratio = [f / s for f, s in zip(rates["one launch"], rates["2 n launches"])]
        say(f"| (b) {label}, B = {B} | one launch / 2 n launches per round: {', '.join(f'{r:.2f}' for r in ratio)} | rounds apart by "
            f"{spread(rates['2 n launches']):.1%} (2 n launches) and {spread(rates['one launch']):.1%} (one launch) of their mean | "
            f"trajectories of the two equal bit for bit: {same} |")
        del loop, Xt, Ut, st

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
