#!/usr/bin/env python3
"""The denoiser's weight gradients in a training step's backward, autograd (the torch module on the tape: MIOpen backward-data and
backward-weights) against device (DEQFixedPoint.parameter_backward = "device": vjp.DenoiserParamGrads, csrc/wgrad.hip), for SimpleCNN with its
shipped weights at 256 x 256 x 8 and 1 or 8 measurements per call.  Times, with HIP events after warm-up, the median of the repeats:
    taped     the taped call z = f(z*) itself (device: the kernel forward that keeps activations and masks, and the weight packs)
    backward  torch.autograd.grad of that call w.r.t. every conv weight, for a given upstream gradient (a fresh taped call per repeat)
    W0        one 64 -> 64 weight gradient alone (and its TFLOP/s against the 157.3 TF fp32 matrix peak)
    W1        one edge-layer weight gradient alone, both forms
Prints one line per (batch, path) and a JSON line.

    python tools/wgrad_bench.py [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deqsci_amd  # noqa: E402
from deqsci_amd import _hip, checkpoint, vjp  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402

F32_MATRIX_PEAK_TF = 157.3


def timed(fn, reps, warmup, before=None):
    """Median ms of fn(state) over `reps` runs; before() -> state runs untimed in front of each."""
    ms = []
    for i in range(warmup + reps):
        state = before() if before is not None else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = "cuda"
    solver, _ = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 12)
    net = solver.nonlinear_op
    weights = vjp.conv_weights(net)
    out = {"denoiser": "SimpleCNN", "H": 256, "W": 256, "B": 8, "wgrad_chain": _hip.WGRAD_CHAIN, "rows": []}
    for bsz in (1, 8):
        g = torch.Generator(device=dev).manual_seed(bsz)
        Phi = (torch.rand(bsz, 256, 256, 8, device=dev, generator=g) < 0.5).float()
        Ps = deqsci_amd.phi_sum(Phi)
        gt = torch.rand(bsz, 256, 256, 8, device=dev, generator=g)
        y = (gt * Phi).sum(-1)
        z = deqsci_amd.initial_point(y, Phi, Ps, None).clone()
        up = torch.randn_like(gt)
        calls = {"autograd": lambda: solver(z, y, Phi, Ps), "device": lambda: solver.forward_param_device(z, y, Phi, Ps)}
        grads = {p: torch.autograd.grad(call(), weights, up) for p, call in calls.items()}
        rel = [float((d - r).double().norm() / r.double().norm()) for d, r in zip(grads["device"], grads["autograd"])]
        for path, call in calls.items():
            t_fwd = timed(lambda _: call(), a.reps, a.warmup)
            t_bwd = timed(lambda zt: torch.autograd.grad(zt, weights, up), a.reps, a.warmup, before=call)
            row = {"bsz": bsz, "path": path, "taped_ms": t_fwd, "backward_ms": t_bwd,
                   "rel_l2_device_vs_autograd": rel if path == "device" else None}
            out["rows"].append(row)
            print(f"bsz {bsz} {path:8s}: taped call {t_fwd:8.3f} ms   backward (all weight gradients) {t_bwd:8.3f} ms"
                  + (f"   rel-L2 vs autograd per weight {', '.join('%.1e' % r for r in rel)}" if path == "device" else ""))
        n = bsz * 8
        x = torch.randn(n, 64, 256, 256, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        gg = torch.randn(n, 64, 256, 256, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        s = torch.randn(n, 1, 256, 256, device=dev, generator=g)
        ws = _hip.wgrad_workspace(n, 256, 256, dev)
        t_w0 = timed(lambda _: _hip.wgrad_c64_c64(x, gg, ws), a.reps, a.warmup)
        t_w1 = [timed(lambda _: _hip.wgrad_c1_c64(s, gg, flip, ws), a.reps, a.warmup) for flip in (0, 1)]
        tf = 2.0 * 9 * 64 * 64 * n * 256 * 256 / (t_w0 * 1e-3) / 1e12
        out["rows"].append({"bsz": bsz, "path": "kernels", "w0_ms": t_w0, "w0_tflops": tf, "w0_of_peak": tf / F32_MATRIX_PEAK_TF,
                            "w1_flip0_ms": t_w1[0], "w1_flip1_ms": t_w1[1], "workspace_mib": ws.numel() * 8 / 2 ** 20})
        print(f"bsz {bsz} kernels : W0 {t_w0:8.3f} ms = {tf:6.1f} TFLOP/s ({100 * tf / F32_MATRIX_PEAK_TF:.0f} % of {F32_MATRIX_PEAK_TF} TF)"
              f"   W1 flip 0 {t_w1[0]:.3f} ms, flip 1 {t_w1[1]:.3f} ms   workspace {ws.numel() * 8 / 2 ** 20:.0f} MiB")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
