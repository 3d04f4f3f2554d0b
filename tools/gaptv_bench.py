#!/usr/bin/env python3
"""GAP-TV on the device (csrc/tv.hip): wall time per call of _hip.gaptv at 1 and 8 measurements per call, 256 x 256 x 8, the
reference's settings (40 GAP iterations, step 1, TV weight 0.3, at most 30 Chambolle iterations, eps 2e-4), timed with HIP events
around each call after warm-up.  The inputs are the shipped clips' 8 scored measurements with their own masks, so the early stops fire
as they do in evaluation.  Prints one line per batch size and a JSON line.

    python tools/gaptv_bench.py [--reps 10] [--warmup 2]

Under `rocprofv3 --kernel-trace --stats -- python tools/gaptv_bench.py --reps 2` the stats file gives the split between the kernels.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, phi_sum  # noqa: E402
from deqsci_amd.harness import load_test_data, scored_measurements  # noqa: E402


def inputs(dev):
    ys, Phis = [], []
    for clip in ("drop8", "runner8", "traffic"):
        d = load_test_data(os.path.join(ROOT, "data", "test_gray", f"{clip}_cacti.mat"))
        ids = scored_measurements(clip, d["meas"].shape[-1])
        ys.append(torch.from_numpy(np.ascontiguousarray(d["meas"][..., ids].transpose(2, 0, 1))))
        Phis.append(torch.from_numpy(d["mask"])[None].expand(len(ids), -1, -1, -1))
    y = torch.cat(ys).to(dev)
    Phi = torch.cat(Phis).contiguous().to(dev)
    return y, Phi, phi_sum(Phi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    y, Phi, Ps = inputs("cuda")
    res = {}
    for bsz in (1, 8):
        args = (y[:bsz].contiguous(), Phi[:bsz].contiguous(), Ps[:bsz].contiguous())
        for _ in range(a.warmup):
            _hip.gaptv(*args)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, stop = _hip.gaptv(*args, return_stop=True)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        tv_iters = int(stop.sum()) + int((stop < 30).sum())              # launches that did work per plane: stop index + 1 where it fired
        res[bsz] = {"ms_median": med, "ms_min": float(min(times)), "ms_max": float(max(times)),
                    "chambolle_plane_iters": tv_iters, "reps": a.reps}
        print(f"gaptv 256x256x8, {bsz} measurement(s) per call: median {med:.2f} ms (min {min(times):.2f}, max {max(times):.2f}) "
              f"over {a.reps} calls, {med / bsz:.2f} ms per measurement; {tv_iters} plane-iterations of Chambolle did work")
    print(json.dumps({"gaptv_bench": res}))


if __name__ == "__main__":
    main()
