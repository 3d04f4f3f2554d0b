#!/usr/bin/env python3
"""The four power-iteration steps of ONE train-mode f-call of RealSN_SimpleCNN (shipped weights, 40 x 40 maps) on the device: the
composed torch operations of the reference's pre-forward hook (networks/provable/model/conv_sn_chen.py:29-50 - conv2d, flip, permute,
and normalize()'s float(torch.sqrt(...)), i.e. two host synchronisations per layer) against R1 of csrc/realsn.hip (4 launches per layer,
none).  And the gradient of the four normalised weights for a given upstream gradient: autograd's backward through the composed
last two lines of the step against R2 (2 launches per layer).  HIP events after warm-up, the median of the repeats; every repeat starts
from the same weight_u.  Prints one line per measurement and a JSON line.

    python tools/realsn_bench.py [--reps 50] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, checkpoint  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.networks.simplecnn import RealSNConv2d  # noqa: E402


def timed(fn, reps, warmup, before=None):
    """Median ms of fn(state) over `reps` runs; before() -> state runs untimed in front of each."""
    ms = []
    for i in range(warmup + reps):
        state = before() if before is not None else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def composed_normalize(t, eps):
    norm = max(float(torch.sqrt(torch.sum(t * t))), eps)           # (the host synchronisation of the composed form)
    return t / norm


def composed_step(W, u, sigma, eps=1e-12):
    """One step as composed torch operations, as the reference writes it; -> (weight, u, v, cur_sigma), weight on the tape of W."""
    with torch.no_grad():
        v = composed_normalize(F.conv2d(u.flip(2, 3), W.permute(1, 0, 2, 3), padding=1), eps).flip(2, 3)
        u = composed_normalize(F.conv2d(v, W, padding=1), eps).clone()
        v = v.clone()
    cur_sigma = torch.sum(u * F.conv2d(v, W, padding=1))
    return W / cur_sigma * sigma, u, v, cur_sigma


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "realsn_bench needs a GPU"
    solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 10)
    convs = [m for m in solver.nonlinear_op.modules() if isinstance(m, RealSNConv2d)]
    Ws = [m.weight_orig.detach().clone().requires_grad_(True) for m in convs]
    us = [m.weight_u.detach().clone() for m in convs]
    sig = [float(m.sigma) for m in convs]
    g = torch.Generator(device="cuda").manual_seed(0)
    Gs = [torch.randn(W.shape, device="cuda", generator=g) for W in Ws]
    wss = [_hip.realsn_workspace(W.shape[1], W.shape[0], u.shape[2], u.shape[3], "cuda") for W, u in zip(Ws, us)]
    out = {"layers": [list(W.shape) for W in Ws], "map": list(us[0].shape[2:]), "reps": a.reps}

    def fresh_u(_=None):
        return [u.clone() for u in us]

    def power_composed(u0):
        with torch.no_grad():
            return [composed_step(W, u, s) for W, u, s in zip(Ws, u0, sig)]

    def power_device(u0):
        return [_hip.realsn_power(W.detach(), u, 1, s, 1e-12, workspace=ws) for W, u, s, ws in zip(Ws, u0, sig, wss)]

    out["power_composed_ms"] = timed(power_composed, a.reps, a.warmup, fresh_u)
    out["power_device_ms"] = timed(power_device, a.reps, a.warmup, fresh_u)
    out["power_device_launches"] = 4 * len(Ws)

    def taped(_=None):
        return [composed_step(W, u, s)[0] for W, u, s in zip(Ws, us, sig)]

    def grad_autograd(weights):
        return torch.autograd.grad(weights, Ws, Gs)

    kept = [_hip.realsn_power(W.detach(), u.clone(), 1, s, 1e-12, workspace=ws) for W, u, s, ws in zip(Ws, us, sig, wss)]

    def grad_device(_):
        return [_hip.realsn_grad(G, W.detach(), k[1], k[2], k[3], s, workspace=ws) for G, W, k, s, ws in zip(Gs, Ws, kept, sig, wss)]

    out["grad_autograd_ms"] = timed(grad_autograd, a.reps, a.warmup, taped)
    out["grad_device_ms"] = timed(grad_device, a.reps, a.warmup)
    out["grad_device_launches"] = 2 * len(Ws)
    # the two forms compute the same thing
    want = torch.autograd.grad(taped(), Ws, Gs)
    out["grad_rel_l2_device_vs_autograd"] = max(float((d - w).norm() / w.norm()) for d, w in zip(grad_device(None), want))
    print(f"power step x {len(Ws)} layers, one f-call:  composed torch {out['power_composed_ms']:.3f} ms   R1 {out['power_device_ms']:.3f} ms "
          f"({out['power_device_launches']} launches)   x{out['power_composed_ms'] / out['power_device_ms']:.1f}")
    print(f"weight gradient x {len(Ws)} layers:         autograd       {out['grad_autograd_ms']:.3f} ms   R2 {out['grad_device_ms']:.3f} ms "
          f"({out['grad_device_launches']} launches)   x{out['grad_autograd_ms'] / out['grad_device_ms']:.1f}   "
          f"(relative L2 between them {out['grad_rel_l2_device_vs_autograd']:.2e})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
