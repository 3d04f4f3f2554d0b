"""What snapshots= and trace= cost: one reconstruction (180 iterations, 256x256x8) with no option, with five snapshots, and with the
trace (residual + PSNR), timed with HIP events after warm-up, at 1 and 8 measurements per call.  Prints ONE JSON line.

    python tools/horizons_bench.py [--denoiser ffdnet] [--iters 180] [--reps 5] [--table]

--table also prints (to stderr) the PSNR-vs-horizon table of the three shipped clips from one run per denoiser, as INTEGRATION.md has it.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deqsci_amd import checkpoint, harness                    # noqa: E402
from deqsci_amd.cli import build_pipeline                     # noqa: E402
from deqsci_amd.engine import DEQSCIEngine                    # noqa: E402

SNAPSHOTS = (10, 30, 60, 100, 140)
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "test_gray")


def batch(n, dev):
    clips = [harness.as_clip(c) for c in harness.SCITestDataset(DATA)]
    picks = [(c, m) for c in clips for m in harness.scored_measurements(c['file'], c['meas'].shape[-1])]
    picks = [p for p in picks if "traffic" in p[0]['file']][:1] if n == 1 else picks[:n]
    y = torch.stack([c['meas'][..., m] for c, m in picks]).contiguous().to(dev)
    Phi = torch.stack([c['mask'] for c, _ in picks]).contiguous().to(dev)
    gt = torch.stack([c['gt'][..., 8 * m:8 * m + 8] for c, m in picks]).contiguous().to(dev)
    return y, Phi, gt


def time_ms(fn, reps, warmup=3):
    for _ in range(warmup):                                   # (eager call, graph capture, first replay)
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--denoiser", default="ffdnet", choices=["ffdnet", "SimpleCNN"])
    ap.add_argument("--iters", type=int, default=180)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    weights = {"ffdnet": "ffdnet_gray", "SimpleCNN": "cnn"}
    solver, _ = build_pipeline(args.denoiser, checkpoint.shipped(weights[args.denoiser]), args.iters, device=dev)
    snaps = tuple(k for k in SNAPSHOTS if k < args.iters)
    out = {"tool": "horizons_bench", "denoiser": args.denoiser, "iters": args.iters, "snapshots": list(snaps), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "unit": "ms per reconstruct() call, median"}
    for n in (1, 8):
        y, Phi, gt = batch(n, dev)
        eng = DEQSCIEngine(solver.nonlinear_op, max_iter=args.iters, lam=1e-2, tol=1e-5)
        base = time_ms(lambda: eng.reconstruct(y, Phi), args.reps)
        snap = time_ms(lambda: eng.reconstruct(y, Phi, snapshots=snaps), args.reps)
        trace = time_ms(lambda: eng.reconstruct(y, Phi, trace=True, gt=gt), args.reps)
        out[f"bsz{n}"] = {"plain_ms": round(base, 3), "snapshots_ms": round(snap, 3), "trace_ms": round(trace, 3),
                          "snapshots_rel": round(snap / base - 1, 4), "trace_rel": round(trace / base - 1, 4),
                          "snapshots_expected_rel": round(len(snaps) / (args.iters + 1), 4), "graph": bool(eng.last_info["graph"])}
    if args.table:
        clips = list(harness.SCITestDataset(DATA))
        for kind in ("ffdnet", "SimpleCNN"):
            _, deq = build_pipeline(kind, checkpoint.shipped(weights[kind]), args.iters, device=dev)
            avg, results = harness.evaluate(deq, clips, device=dev, batch=False, snapshots=snaps)
            for K in snaps:
                print(kind, K, " ".join("%s %.2f" % (r.name.split("_")[0], sum(r.snapshots[K]["psnr"]) / len(r.snapshots[K]["psnr"]))
                                        for r in results), "avg %.2f" % harness.horizon_means(results)[K][0], file=sys.stderr)
            print(kind, args.iters, " ".join("%s %.2f" % (r.name.split("_")[0], r.mean_psnr) for r in results), "avg %.2f" % avg, file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
