#!/usr/bin/env python3
"""Generate tests/golden/ssim.npz by IMPORTING the reference's pytorch_ssim (CPU, through ref_shims.py) and running its own
code.  Like make_golden.py it runs only where the reference is mounted, and it stores data only: the values the reference
computes from seeded inputs (and hashes of those inputs).

    python tests/golden/make_ssim_golden.py

Contents (data only; the synthetic inputs are not stored - tests/test_ssim.py rebuilds them with `pair` below, whose only source of
randomness is numpy's RandomState, a stream numpy keeps fixed, and checks them against the stored hashes):
  pair{i}_sha                         sha256 prefix of the float32 bytes of img1 then img2 of pair i
  pair{i}_w{ws}_avg / _img            pytorch_ssim.ssim(img1, img2, window_size=ws, size_average=True / False), ws = 7, 11, for the
                                      seeded NCHW pairs in [0,1] of shapes (1,1,7,9) (smaller than the window), (2,1,37,53),
                                      (1,3,64,64), (4,1,256,256); img2 is a noisy, slightly smoothed copy of img1
  rec_{tag}_{clip}_m0                 per-frame SSIM (window 11, size_average=True) of the reference's own reconstruction in
                                      e2e_{tag}_rec.npz, clamped to [0,1], against the clip's ground truth; each frame a
                                      (1,1,H,W) image
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()
sys.path.insert(0, ref_shims.REFERENCE_ROOT)

import pytorch_ssim  # noqa: E402  (the reference's)
from utils.sci_dataloader import load_test_data  # noqa: E402

DATA = ref_shims.REFERENCE_ROOT + "/data/test_gray/"
SHAPES = [(1, 1, 7, 9), (2, 1, 37, 53), (1, 3, 64, 64), (4, 1, 256, 256)]
WINDOWS = (7, 11)
RECS = {"SimpleCNN_anderson_180": ("drop8", "runner8", "traffic"), "ffdnet_anderson_30": ("traffic",)}


def pair(i):
    """Seeded NCHW pair i (numpy float64 arithmetic, rounded to float32 once; restated in tests/test_ssim.py)."""
    shape = SHAPES[i]
    rs = np.random.RandomState(20261015 + i)
    x = rs.random_sample(shape)
    nb = sum(np.roll(np.roll(x, dy, axis=2), dx, axis=3) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    y = np.clip(0.7 * x + 0.3 * nb + 0.05 * rs.standard_normal(shape), 0.0, 1.0)
    return x.astype(np.float32), y.astype(np.float32)


def sha(x, y):
    return hashlib.sha256(x.tobytes() + y.tobytes()).hexdigest()[:16]


def main():
    out = {}
    for i in range(len(SHAPES)):
        xn, yn = pair(i)
        out[f"pair{i}_sha"] = np.array(sha(xn, yn))
        x, y = torch.from_numpy(xn), torch.from_numpy(yn)
        for ws in WINDOWS:
            with torch.no_grad():
                out[f"pair{i}_w{ws}_avg"] = pytorch_ssim.ssim(x, y, window_size=ws, size_average=True).numpy()
                out[f"pair{i}_w{ws}_img"] = pytorch_ssim.ssim(x, y, window_size=ws, size_average=False).numpy()
    for tag, clips in RECS.items():
        recs = np.load(os.path.join(HERE, f"e2e_{tag}_rec.npz"))
        for clip in clips:
            gt = torch.from_numpy(load_test_data(DATA + f"{clip}_cacti.mat")["gt"])
            rec = torch.from_numpy(recs[f"{clip}_m0"][0]).clamp(0, 1)                     # (H,W,8)
            vals = []
            for b in range(rec.shape[-1]):
                with torch.no_grad():
                    vals.append(float(pytorch_ssim.ssim(rec[None, None, :, :, b].contiguous(), gt[None, None, :, :, b].contiguous(),
                                                        window_size=11, size_average=True)))
            out[f"rec_{tag}_{clip}_m0"] = np.array(vals, dtype=np.float32)
            print(tag, clip, "mean SSIM over the frames of m0: %.5f" % np.mean(vals))
    np.savez_compressed(os.path.join(HERE, "ssim.npz"), **out)
    print("wrote", os.path.join(HERE, "ssim.npz"), len(out), "arrays")


if __name__ == "__main__":
    main()
