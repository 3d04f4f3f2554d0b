#!/usr/bin/env python3
"""The denoiser's weight gradients in a training step's backward, autograd (the torch module on the tape: MIOpen backward-data and
backward-weights) against device (DEQFixedPoint.parameter_backward = "device": vjp.DenoiserParamGrads, csrc/wgrad.hip), for SimpleCNN with its
shipped weights at 256 x 256 x 8 and 1 or 8 measurements per call.  --denoiser ffdnet (shipped weights) and --denoiser DnCNN --loadpath W
(17 layers with BatchNorm) time "autograd" against "device+bn" (the frozen-BatchNorm path: csrc/wgrad_bn.hip, gamma and beta included).
Times, with HIP events after warm-up, the median of the repeats:
    taped     the taped call z = f(z*) itself (device: the kernel forward that keeps activations and masks, and the weight packs)
    backward  torch.autograd.grad of that call w.r.t. every parameter the device answers for, for a given upstream gradient (a fresh
              taped call per repeat)
    W0        one 64 -> 64 weight gradient alone (and its TFLOP/s against the 157.3 TF fp32 matrix peak)
    W1        one edge-layer weight gradient alone, both forms
    W0-BN     (ffdnet, DnCNN) the 64 -> 64 weight gradient with its two BatchNorm sums, next to W0 on the same data
    W2        (ffdnet) one pixel-(un)shuffled edge-layer weight gradient alone, both forms, and the bytes it reads per second
Prints one line per (batch, path) and a JSON line.

    python tools/wgrad_bench.py [--denoiser SimpleCNN|ffdnet|DnCNN] [--loadpath W] [--reps 10] [--warmup 2]
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


def kernels_ffdnet(out, bsz, g, a):
    """W0 and W0-BN on the same half-resolution activations, W2 in both forms on the full-resolution image."""
    dev, n = "cuda", bsz * 8
    x = torch.randn(n, 64, 128, 128, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    gg = torch.randn(n, 64, 128, 128, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    w, scale = torch.randn(64, 64, 3, 3, device=dev, generator=g), torch.randn(64, device=dev, generator=g)
    img, sigma = torch.randn(n, 1, 256, 256, device=dev, generator=g), torch.rand(n, device=dev, generator=g)
    ws, wsb = _hip.wgrad_workspace(n, 128, 128, dev), _hip.wgrad_bn_workspace(n, 128, 128, dev)
    t_w0 = timed(lambda _: _hip.wgrad_c64_c64(x, gg, ws), a.reps, a.warmup)
    t_bn = timed(lambda _: _hip.wgrad_c64_c64_bn(x, gg, w, scale, wsb), a.reps, a.warmup)
    t_w2 = [timed(lambda _: _hip.wgrad_shuffle(img, gg, which, sigma, wsb), a.reps, a.warmup) for which in (0, 1)]
    tf = lambda ms: 2.0 * 9 * 64 * 64 * n * 128 * 128 / (ms * 1e-3) / 1e12
    read = (gg.numel() + img.numel()) * 4                        # bytes W2's first launch reads once: the activation and the image
    out["rows"].append({"bsz": bsz, "path": "kernels", "w0_ms": t_w0, "w0_tflops": tf(t_w0), "w0bn_ms": t_bn, "w0bn_tflops": tf(t_bn),
                        "w2_which0_ms": t_w2[0], "w2_which1_ms": t_w2[1], "w2_read_mib": read / 2 ** 20,
                        "w2_which0_gbs": read / (t_w2[0] * 1e-3) / 1e9, "w2_which1_gbs": read / (t_w2[1] * 1e-3) / 1e9,
                        "workspace_mib": wsb.numel() * 8 / 2 ** 20})
    print(f"bsz {bsz} kernels  : W0 {t_w0:7.3f} ms = {tf(t_w0):5.1f} TFLOP/s   W0-BN {t_bn:7.3f} ms = {tf(t_bn):5.1f} TFLOP/s ({t_bn / t_w0:.3f} x W0)"
          f"   W2 which 0 {t_w2[0]:.3f} ms, which 1 {t_w2[1]:.3f} ms reading {read / 2 ** 20:.0f} MiB = {read / (t_w2[0] * 1e-3) / 1e9:.0f} / "
          f"{read / (t_w2[1] * 1e-3) / 1e9:.0f} GB/s   workspace {wsb.numel() * 8 / 2 ** 20:.0f} MiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--denoiser", default="SimpleCNN", choices=["SimpleCNN", "ffdnet", "DnCNN"])
    ap.add_argument("--loadpath", default=None, help="weights (DnCNN has no shipped ones; default for the others: the shipped weights)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = "cuda"
    bn = a.denoiser != "SimpleCNN"
    device = "device+bn" if bn else "device"
    loadpath = a.loadpath or {"SimpleCNN": checkpoint.shipped("cnn"), "ffdnet": checkpoint.shipped("ffdnet_gray")}.get(a.denoiser)
    solver, _ = build_pipeline(a.denoiser, loadpath, 12)
    net = solver.nonlinear_op
    weights = vjp.grad_parameters(net) if bn else vjp.conv_weights(net)
    out = {"denoiser": a.denoiser, "H": 256, "W": 256, "B": 8, "wgrad_chain": _hip.WGRAD_CHAIN, "parameters": len(weights), "rows": []}
    for bsz in (1, 8):
        g = torch.Generator(device=dev).manual_seed(bsz)
        Phi = (torch.rand(bsz, 256, 256, 8, device=dev, generator=g) < 0.5).float()
        Ps = deqsci_amd.phi_sum(Phi)
        gt = torch.rand(bsz, 256, 256, 8, device=dev, generator=g)
        y = (gt * Phi).sum(-1)
        z = deqsci_amd.initial_point(y, Phi, Ps, None).clone()
        up = torch.randn_like(gt)

        def fresh(call):
            solver.noise_sigma = None                          # FFDNet: every call at the first noise level, on both paths
            return call()
        calls = {"autograd": lambda: fresh(lambda: solver(z, y, Phi, Ps)),
                 device: lambda: fresh(lambda: solver.forward_param_device(z, y, Phi, Ps, frozen_bn=bn))}
        grads = {p: torch.autograd.grad(call(), weights, up) for p, call in calls.items()}
        rel = [float((d - r).double().norm() / r.double().norm()) for d, r in zip(grads[device], grads["autograd"])]
        for path, call in calls.items():
            t_fwd = timed(lambda _: call(), a.reps, a.warmup)
            t_bwd = timed(lambda zt: torch.autograd.grad(zt, weights, up), a.reps, a.warmup, before=call)
            row = {"bsz": bsz, "path": path, "taped_ms": t_fwd, "backward_ms": t_bwd,
                   "rel_l2_device_vs_autograd": rel if path == device else None}
            out["rows"].append(row)
            print(f"bsz {bsz} {path:9s}: taped call {t_fwd:8.3f} ms   backward (all {len(weights)} gradients) {t_bwd:8.3f} ms"
                  + (f"   rel-L2 vs autograd per parameter: max {max(rel):.1e}, median {statistics.median(rel):.1e}" if path == device else ""))
        if a.denoiser == "ffdnet":
            kernels_ffdnet(out, bsz, g, a)
            continue
        n = bsz * 8
        x = torch.randn(n, 64, 256, 256, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        gg = torch.randn(n, 64, 256, 256, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
        s = torch.randn(n, 1, 256, 256, device=dev, generator=g)
        ws = _hip.wgrad_workspace(n, 256, 256, dev)
        t_w0 = timed(lambda _: _hip.wgrad_c64_c64(x, gg, ws), a.reps, a.warmup)
        if bn:
            w, scale = torch.randn(64, 64, 3, 3, device=dev, generator=g), torch.randn(64, device=dev, generator=g)
            wsb = _hip.wgrad_bn_workspace(n, 256, 256, dev)
            t_bn = timed(lambda _: _hip.wgrad_c64_c64_bn(x, gg, w, scale, wsb), a.reps, a.warmup)
            out["rows"].append({"bsz": bsz, "path": "kernels-bn", "w0bn_ms": t_bn, "w0bn_over_w0": t_bn / t_w0})
            print(f"bsz {bsz} kernels  : W0-BN {t_bn:8.3f} ms ({t_bn / t_w0:.3f} x W0)")
        t_w1 = [timed(lambda _: _hip.wgrad_c1_c64(s, gg, flip, ws), a.reps, a.warmup) for flip in (0, 1)]
        tf = 2.0 * 9 * 64 * 64 * n * 256 * 256 / (t_w0 * 1e-3) / 1e12
        out["rows"].append({"bsz": bsz, "path": "kernels", "w0_ms": t_w0, "w0_tflops": tf, "w0_of_peak": tf / F32_MATRIX_PEAK_TF,
                            "w1_flip0_ms": t_w1[0], "w1_flip1_ms": t_w1[1], "workspace_mib": ws.numel() * 8 / 2 ** 20})
        print(f"bsz {bsz} kernels : W0 {t_w0:8.3f} ms = {tf:6.1f} TFLOP/s ({100 * tf / F32_MATRIX_PEAK_TF:.0f} % of {F32_MATRIX_PEAK_TF} TF)"
              f"   W1 flip 0 {t_w1[0]:.3f} ms, flip 1 {t_w1[1]:.3f} ms   workspace {ws.numel() * 8 / 2 ** 20:.0f} MiB")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
