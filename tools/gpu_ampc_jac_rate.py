"""Time per launch of the batched network Jacobian (ApproxMPC.jacobian_batch_device, csrc/dompc_ampc.hip:dompc_ampc_jac_kernel) on
resident inputs beside the step (make_step_batch_device) and beside torch's Jacobian of the same network on the same device and inputs
- the tangent recursion do_mpc_amd.ampc.network_jacobian under no_grad (a handful of batched launches per layer; what the trainer's
Sobolev term runs) and torch.func.vmap(jacrev(net)) - for the stored 1 x 50 network of the reference and the default 3 x 50 network at
B = 16 384 and 262 144.  The three or four candidates of one row are measured in alternating rounds: every round times each of them
once (device events around enough launches for `--seconds` of work, after a warm-up of every one), `--rounds` rounds, the median and
the spread (min ... max) per candidate.  The fused launches include their host side (the check of the parameters' version counters and
the ctypes call).  torch's results are compared with the kernel's once per row.
usage: python tools/gpu_ampc_jac_rate.py [--seconds 0.5] [--rounds 7] > profiles/ampc_jac_rate.txt"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import ampc_common as ac
from do_mpc_amd.ampc import network_jacobian

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=0.5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--batches", type=int, nargs="*", default=[16384, 262144])
ap.add_argument("--no-jacrev", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tools/gpu_ampc_jac_rate.py measures on the GPU and found none")
dev = torch.device("cuda", 0)


def calibrate(launch, seconds, warm=3):
    """warm up, then -> launches that fill about `seconds`"""
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return max(3, min(20000, int(seconds / max(e0.elapsed_time(e1) * 1e-3 / 3, 1e-7))))


def timed(launch, n):
    """-> seconds per launch over n launches between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


print(f"# tools/gpu_ampc_jac_rate.py --seconds {args.seconds} --rounds {args.rounds} on {torch.cuda.get_device_name(0)}; "
      "us per launch: median (min ... max) over the alternating rounds")
stream = torch.cuda.current_stream().cuda_stream
nets = {"stored 1 x 50 (tanh)": ac.stored_cstr(hostemu=False),
        "default 3 x 50 (tanh)": ac.network(4, 2, True, hostemu=False, box=ac.CSTR_BOX, n_hidden_layers=3, n_neurons=50)}
for label, ampc in nets.items():
    net = copy.deepcopy(ampc.net).to(dev)
    lb, ub, lbu, ubu = (torch.tensor(a.reshape(1, -1), device=dev) for a in ampc._box())
    for B in args.batches:
        X, Up = ac.inputs(ampc, B, seed=1)
        dX, dU = torch.tensor(X, device=dev), torch.tensor(Up, device=dev)
        u, u2 = (torch.empty((B, 2), dtype=torch.float64, device=dev) for _ in range(2))
        jx, ju = torch.empty((B, 2, 4), dtype=torch.float64, device=dev), torch.empty((B, 2, 2), dtype=torch.float64, device=dev)
        xs = ((torch.cat((dX, dU), dim=1).to(torch.float32) - lb) / (ub - lb)).type(torch.float32)
        jac_of_one = torch.func.vmap(torch.func.jacrev(net))

        def step():
            ampc.make_step_batch_device(B, dX.data_ptr(), dU.data_ptr(), u2.data_ptr(), stream=stream, clip_to_bounds=False)

        def fused():
            ampc.jacobian_batch_device(B, dX.data_ptr(), dU.data_ptr(), u.data_ptr(), jx.data_ptr(), ju.data_ptr(), stream=stream)

        @torch.no_grad()
        def recursion():
            return network_jacobian(net, xs)[1]

        def jacrev():
            return jac_of_one(xs)
        cands = {"step kernel": step, "Jacobian kernel": fused, "torch tangent recursion": recursion}
        if not args.no_jacrev:
            cands["torch vmap(jacrev)"] = jacrev
        n = {k: calibrate(f, args.seconds) for k, f in cands.items()}
        t = {k: [] for k in cands}
        for _ in range(args.rounds):
            for k, f in cands.items():
                t[k].append(timed(f, n[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        # agreement: the kernel's Jacobian in the network's coordinates against torch's, and u against the step, bit for bit
        fused()
        step()
        torch.cuda.synchronize()
        J = torch.cat((jx, ju), dim=2) * (ub - lb).reshape(1, 1, -1) / (ubu - lbu).reshape(1, -1, 1)
        err = float((J - recursion().double()).abs().max())
        cells = " | ".join(f"{k}: {med[k] * 1e6:.1f} us ({min(t[k]) * 1e6:.1f} ... {max(t[k]) * 1e6:.1f}), {n[k]} launches per round" for k in cands)
        ratios = f"Jacobian / step = {med['Jacobian kernel'] / med['step kernel']:.2f}, recursion / Jacobian = {med['torch tangent recursion'] / med['Jacobian kernel']:.1f}"
        if not args.no_jacrev:
            ratios += f", vmap(jacrev) / Jacobian = {med['torch vmap(jacrev)'] / med['Jacobian kernel']:.1f}"
        print(f"| {label} | B = {B} | {cells} | {ratios} | {B / med['Jacobian kernel']:.3e} Jacobians/s | max |kernel - recursion| = {err:.1e}, "
              f"u equal to the step's: {bool(torch.equal(u, u2))} |", flush=True)
