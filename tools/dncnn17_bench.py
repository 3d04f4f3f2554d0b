#!/usr/bin/env python3
"""DnCNN-17 on the engine, path by path: one f-call of the denoiser and a 30-iteration reconstruction of 8 measurements of 256 x 256 x 8
(64 images per f-call), HIP-event timed, on

    w16 stack launch   the default: 1->64 layer, the 15 middle layers as ONE conv_w16 launch, 64->1 layer, per slice of the batch
    w16 per layer      stack=False: the same kernels, a launch per layer (what a 17-layer plugin took before the stack launch existed)
    s16 stack launch   stack_kernel="s16": the direct split-fp16 kernel's stack launch

    python tools/dncnn17_bench.py [--loadpath tests/golden/dncnn_noise15.npz] [--iters 30] [--bsz 8] [--launches 20] [--repeats 3]

The f-call is timed over rotating inputs (consecutive calls read different iterates, as in tools/kernel_bench.py); the measurements are
traffic's, cycled to --bsz.  Prints one JSON object per path and a markdown table (profiles/dncnn17.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.engine import DEQSCIEngine  # noqa: E402
from deqsci_amd.harness import load_test_data  # noqa: E402

PATHS = {"w16 stack launch": {}, "w16 per layer": {"stack": False}, "s16 stack launch": {"stack_kernel": "s16"}}


def events_ms(fn, n, warm):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loadpath", default=os.path.join(ROOT, "tests", "golden", "dncnn_noise15.npz"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--bsz", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sets", type=int, default=3, help="rotating inputs of the f-call")
    args = ap.parse_args()
    dev = "cuda"
    d = load_test_data(os.path.join(ROOT, "data", "test_gray", "traffic_cacti.mat"))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"]))[None].to(dev)
    meas = np.ascontiguousarray(d["meas"].transpose(2, 0, 1))
    y = torch.from_numpy(meas[[i % meas.shape[0] for i in range(args.bsz)]]).contiguous().to(dev)
    net = build_pipeline("DnCNN", args.loadpath, args.iters)[0].nonlinear_op
    H, W, B = Phi.shape[1:]
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.rand(args.bsz, B, H, W, device=dev, generator=g) for _ in range(args.sets)]
    rows, recs = [], {}
    for name, kw in PATHS.items():
        eng = DEQSCIEngine(net, max_iter=args.iters, use_graph=False, **kw)
        rec = eng.reconstruct(y, Phi)                                    # (warms every kernel up, measures the ranges, builds the stacks)
        info = eng.last_info
        if info["denoiser_path"] != name or info["stack_timeouts"]:
            raise SystemExit(f"{name}: the engine took {info['denoiser_path']!r} (stack time-outs: {info['stack_timeouts']})")
        recs[name] = rec.clone()
        den = eng.den
        fcall = events_ms(lambda i: den.run(zs[i % len(zs)], 1), args.launches, 3)
        if den.stack_timed_out():
            raise SystemExit(f"{name}: a stack launch timed out while it was timed")
        run = sorted(events_ms(lambda i: eng.reconstruct(y, Phi), 1, 0) for _ in range(args.repeats))[args.repeats // 2]
        row = {"path": name, "fcall_ms": round(fcall, 4), "reconstruction_ms": round(run, 2), "iters": args.iters, "bsz": args.bsz,
               "f_calls": eng.last_info["f_calls"], "frames_per_s": round(args.bsz * B / (run * 1e-3), 1), "res": eng.last_info["res"],
               "device": torch.cuda.get_device_name(0)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    same = torch.equal(recs["w16 stack launch"], recs["w16 per layer"])
    print(json.dumps({"w16 stack launch == w16 per layer, bit for bit": same}))
    base = rows[1]
    print(f"\n| path | f-call ({args.bsz * B} images {H} x {W}), ms | {args.iters}-iteration reconstruction of {args.bsz} measurements, ms | frames/s | vs w16 per layer |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['path']} | {r['fcall_ms']:.3f} | {r['reconstruction_ms']:.1f} | {r['frames_per_s']:.1f} | {base['reconstruction_ms'] / r['reconstruction_ms']:.3f} x |")


if __name__ == "__main__":
    main()
