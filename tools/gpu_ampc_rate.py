"""Rate of the batched approximate-MPC step (do_mpc_amd/ampc.py, csrc/dompc_ampc.hip) on resident inputs, for the stored 1 x 50 network
of the reference (tests/golden/ampc_reference_cstr.pt) and the default 3 x 50 network, at B = 1, 1 024, 16 384 and 262 144: steps per
second of make_step_batch_device and, beside it, the same network's torch eager forward on the same device and inputs - scale, net,
rescale, clip: the reference's own device="cuda" path, what a user would otherwise run (about ten launches, two of them the
concatenation and the cast that the reference does on the host).  The per-launch time of the fused kernel includes the host side of
make_step_batch_device (the check of the parameters' version counters and the ctypes call).  Then the loop steps per second of
BatchClosedLoopAMPC (network -> CSTR plant).  Device events around at least `--seconds` of launches after a warm-up; the median of
`--repeats` such measurements.
usage: python tools/gpu_ampc_rate.py [--seconds 0.3] [--repeats 5] > profiles/ampc_rate.txt"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ampc_common as ac

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 1024, 16384, 262144])
ap.add_argument("--loop-batch", type=int, default=16384)
args = ap.parse_args()
dev = torch.device("cuda", 0)


def timed(launch, seconds, warm=5):
    """-> seconds per launch: device events around rounds of launches until `seconds` of them have been measured"""
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    total, n, per_round = 0.0, 0, 1
    while total < seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_round):
            launch()
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        total += dt
        n += per_round
        per_round = max(1, min(2000, int(0.25 * seconds / max(dt / per_round, 1e-7))))
    return total / n


def median(launch):
    return statistics.median(timed(launch, args.seconds) for _ in range(args.repeats))


print(f"# tools/gpu_ampc_rate.py --seconds {args.seconds} --repeats {args.repeats} on {torch.cuda.get_device_name(0)}")
stream = torch.cuda.current_stream().cuda_stream
nets = {"stored 1 x 50 (tanh)": ac.stored_cstr(hostemu=False),
        "default 3 x 50 (tanh)": ac.network(4, 2, True, hostemu=False, box=ac.CSTR_BOX, n_hidden_layers=3, n_neurons=50)}
for label, ampc in nets.items():
    net = copy.deepcopy(ampc.net).to(dev)
    lb, ub, lbu, ubu = (torch.tensor(a.reshape(1, -1), device=dev) for a in ampc._box())
    for B in args.batches:
        X, Up = ac.inputs(ampc, B, seed=1)
        dX, dU = torch.tensor(X, device=dev), torch.tensor(Up, device=dev)
        out = torch.empty((B, 2), dtype=torch.float64, device=dev)
        fused = lambda: ampc.make_step_batch_device(B, dX.data_ptr(), dU.data_ptr(), out.data_ptr(), stream=stream)      # noqa: E731

        @torch.no_grad()
        def eager(clip=True):
            # (the cat and the cast to float32 happen on the host in the reference's make_step, on one sample; here they are two of
            #  the about ten device launches of the baseline)
            x = torch.cat((dX, dU), dim=1).to(torch.float32)
            xs = ((x - lb) / (ub - lb)).type(torch.float32)
            y = net(xs) * (ubu - lbu) + lbu
            return torch.min(torch.max(y, lbu), ubu) if clip else y
        sf, se = median(fused), median(eager)
        # agreement of the two on the UNCLIPPED output (clipped, a network whose outputs all sit on a bound would agree trivially)
        ampc.make_step_batch_device(B, dX.data_ptr(), dU.data_ptr(), out.data_ptr(), stream=stream, clip_to_bounds=False)
        torch.cuda.synchronize()
        err = float(((out - eager(clip=False)).abs() / (ubu - lbu)).max())
        inside = float(((out > lbu) & (out < ubu)).double().mean())
        print(f"| {label} | B = {B} | fused kernel: {sf * 1e6:.1f} us per launch, {B / sf:.3e} steps/s | torch eager on the device: "
              f"{se * 1e6:.1f} us per step, {B / se:.3e} steps/s | x {se / sf:.1f} | unclipped: max |fused - eager| / (ubu - lbu) = {err:.1e}, {100 * inside:.0f} % of the outputs inside the bounds |", flush=True)

# the resident closed loop on the CSTR plant: two launches per control step
from do_mpc_amd.closed_loop import BatchClosedLoopAMPC
from do_mpc_amd.examples import cstr_ampc as ex
ampc = nets["stored 1 x 50 (tanh)"]
sim = ex.build_simulator(ex.build_model())
B = args.loop_batch
rng = np.random.default_rng(0)
loop = BatchClosedLoopAMPC(ampc, sim, ex.X0 * rng.uniform(0.95, 1.05, (B, 4)), U_prev0=np.tile(ex.U0, (B, 1)))
for _ in range(3):
    loop.step()
rates = []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    for _ in range(20):
        r = loop.step()
    rates.append(20 * B / (time.perf_counter() - t0))
print(f"| BatchClosedLoopAMPC, stored network -> CSTR plant | B = {B} | {statistics.median(rates):.3e} loop steps/s (wall clock, records copied "
      f"to the host every step) | plant status bits set: {int(r['plant_status'].sum())} |", flush=True)
