#!/usr/bin/env python3
"""Generate tests/golden/gaptv.npz by IMPORTING the reference's GAP_TV_rec (utils/cg_utils.py, through ref_shims.py) and running its
own code on CPU.  Like make_golden.py it runs only where the reference is mounted, and it stores data only.

    python tests/golden/make_gaptv_golden.py              -> gaptv.npz
    python tests/golden/make_gaptv_golden.py --shapes     -> gaptv_shapes.npz

The reference calls skimage.restoration.denoise_tv_chambolle (scikit-image 0.17.2), which is not installed here.  This script replaces
cg_utils.denoise_tv_chambolle with `denoise_tv_chambolle` below: a float64 restatement, line by line, of skimage 0.17.2's
_denoise_tv_chambolle_nd and its multichannel loop.  The TV part of every value in this file therefore rests on that restatement, not on
skimage itself.  The restatement also records, per call, the iteration the early stop fired at and the stop-test margin.

Contents (data only; the seeded small case's inputs are not stored - tests/test_gaptv.py rebuilds them with `small_case` below, whose
only source of randomness is numpy's RandomState, a stream numpy keeps fixed, and checks them against the stored hash):
  ids                       "clip:measurement" of the 8 scored measurements of the shipped clips (drop8:0, runner8:0, traffic:0..5)
  psnr_ref                  (8,) cg_utils.psnr of the reference's float32 result against the measurement's gt (the line it prints
                            uses its float64 f: the same to the two printed decimals)
  psnr                      (8,) the harness's PSNR of the reference's float32 result: clamp to [0,1], float32 difference, float64 mean
  stop                      (8, 40, 8) int32, per (measurement, outer iteration, frame): the Chambolle iteration the stop fired at, or
                            n_iter_max (30) if it never fired
  margin                    (8, 40, 8) |E_prev - E| - eps * E_init of the last stop test of the call (negative when it fired)
  tie                       (8, 40, 8) min over the call's stop tests of | |E_prev - E| - eps * E_init | / (eps * E_init): how close the
                            call came to stopping elsewhere
  rec_drop8_0_crop, rec_traffic_0_crop   the reference's float32 output in the window CROP (rows 104:152, columns 96:160, all 8
                            frames; the full 256 x 256 x 8 outputs are too large to keep: the tests hold the device to the float64
                            restatement on the full frames and to the reference here)
  rec_drop8_0_frames, rec_traffic_0_frames   (8, 2) float64 per frame of the full output: sum and sum of squares
  clip_mean_psnr            (3,) the mean of `psnr` per clip, in file order; its mean is the CLI's Total Average
  small_sha                 sha256 prefix of the float32 bytes of y, Phi of the seeded case (37 x 53 x 8, mask in [0,1], maxiter 5)
  small_rec64               its output (1,37,53,8) before the reference's final cast to float32 (the last TV call's float64 result;
                            the reference returns exactly its float32 rounding)
  small_stop, small_margin, small_tie   its per-call records (1, 5, 8)
  deq_rec_crop, deq_rec_frames, deq_psnr   the reference's DEQFixedPoint (SimpleCNN, cnn.ckpt, Anderson m=5 beta=1 lam=1e-2, 10 iterations, tol 1e-5)
                            on drop8:0 started from its GAP-TV point (40 iterations, step 1, TV weight 0.3): its reconstruction in
                            CROP, per-frame sum and sum of squares of the full one, and its PSNR

gaptv_shapes.npz (--shapes): the seeded cases of SHAPES (ragged sizes, B from 1 to 128, binary, non-binary and zero-sum-pixel masks,
a step and a TV weight other than the defaults).  Inputs are rebuilt by `shape_case` (restated in tests/test_gaptv_edges.py) and
checked by hash; per case <name>:
  <name>_params             (H, W, B, maxiter, step_size, tv_weight, seed) float64
  <name>_sha                sha256 prefix of the float32 bytes of y, Phi
  <name>_rec64              the float64 result of the last TV call (1,H,W,B)
  <name>_stop, <name>_margin, <name>_tie   the per-call records (1, maxiter, B), as above
Every seed was picked so that no stop test comes within 1e-9 eps E_init of a tie (min tie >= 1e-9).
"""
import hashlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()
sys.path.insert(0, ref_shims.REFERENCE_ROOT)

from utils import cg_utils  # noqa: E402  (the reference's)
from utils.sci_dataloader import load_test_data  # noqa: E402

DATA = ref_shims.REFERENCE_ROOT + "/data/test_gray/"
CLIPS = (("drop8", [0]), ("runner8", [0]), ("traffic", list(range(6))))
MAXITER, STEP, TV_WEIGHT, N_ITER_MAX, EPS = 40, 1, 0.3, 30, 2e-4
SMALL = (37, 53, 8, 5)                                       # H, W, B, maxiter
CROP = (slice(None), slice(104, 152), slice(96, 160), slice(None))   # the stored window of a (1,256,256,8) output

RECORD = []                                                  # (stop, margin, tie) per channel of every call
LAST = []                                                    # the float64 result of the last denoise_tv_chambolle call


def _tv_nd(image, weight=0.1, eps=2.e-4, n_iter_max=200):
    """skimage 0.17.2 _denoise_tv_chambolle_nd, restated in float64 numpy; appends (stop, margin, tie) to RECORD."""
    ndim = image.ndim
    p = np.zeros((image.ndim, ) + image.shape, dtype=image.dtype)
    g = np.zeros_like(p)
    d = np.zeros_like(image)
    i = 0
    stop, margin, tie = n_iter_max, np.nan, np.inf
    while i < n_iter_max:
        if i > 0:
            d = -p.sum(0)
            slices_d = [slice(None), ] * ndim
            slices_p = [slice(None), ] * (ndim + 1)
            for ax in range(ndim):
                slices_d[ax] = slice(1, None)
                slices_p[ax + 1] = slice(0, -1)
                slices_p[0] = ax
                d[tuple(slices_d)] += p[tuple(slices_p)]
                slices_d[ax] = slice(None)
                slices_p[ax + 1] = slice(None)
            out = image + d
        else:
            out = image
        E = (d ** 2).sum()
        slices_g = [slice(None), ] * (ndim + 1)
        for ax in range(ndim):
            slices_g[ax + 1] = slice(0, -1)
            slices_g[0] = ax
            g[tuple(slices_g)] = np.diff(out, axis=ax)
            slices_g[ax + 1] = slice(None)
        norm = np.sqrt((g ** 2).sum(axis=0))[np.newaxis, ...]
        E += weight * norm.sum()
        tau = 1. / (2. * ndim)
        norm *= tau / weight
        norm += 1.
        p -= tau * g
        p /= norm
        E /= float(image.size)
        if i == 0:
            E_init = E
            E_previous = E
        else:
            margin = np.abs(E_previous - E) - eps * E_init
            tie = min(tie, abs(margin) / (eps * E_init))
            if np.abs(E_previous - E) < eps * E_init:
                stop = i
                break
            else:
                E_previous = E
        i += 1
    RECORD.append((stop, margin, tie))
    return out


def denoise_tv_chambolle(image, weight=0.1, eps=2.e-4, n_iter_max=200, multichannel=False):
    """skimage 0.17.2 denoise_tv_chambolle for float input."""
    if multichannel:
        out = np.zeros_like(image)
        for c in range(image.shape[-1]):
            out[..., c] = _tv_nd(image[..., c], weight, eps, n_iter_max)
    else:
        out = _tv_nd(image, weight, eps, n_iter_max)
    LAST[:] = [out.copy()]
    return out


cg_utils.denoise_tv_chambolle = denoise_tv_chambolle


def small_case():
    """The seeded case (numpy float64 arithmetic, rounded to float32 once; restated in tests/test_gaptv.py) -> y (1,H,W), Phi (1,H,W,B)
    float32; the mask is a non-binary float in [0,1]."""
    H, W, B, _ = SMALL
    rs = np.random.RandomState(20261016)
    x = rs.random_sample((1, H, W, B))
    x = (x + np.roll(x, 1, axis=1) + np.roll(x, 1, axis=2)) / 3.0
    Phi = rs.random_sample((1, H, W, B)).astype(np.float32)
    y = np.sum(x * Phi, axis=3).astype(np.float32)
    return y, Phi


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype=np.float32).tobytes() for a in arrays)).hexdigest()[:16]


def frames(rec):
    """(8, 2) float64: per frame of a (1,H,W,8) output, the sum and the sum of squares of its float32 values."""
    r = rec[0].astype(np.float64)
    return np.stack([r.sum(axis=(0, 1)), (r * r).sum(axis=(0, 1))], axis=1)


def harness_psnr(rec, gt):
    d = np.clip(rec, 0, 1).astype(np.float32) - gt.astype(np.float32)
    return 10.0 * np.log10(1.0 / np.mean(d * d, dtype=np.float64))


def run(y, Phi, gt, maxiter, step=STEP, tv_weight=TV_WEIGHT):
    """The reference's GAP_TV_rec on one measurement (batch 1) -> (float32 result, PSNR printed, (maxiter, B) records)."""
    Ps = torch.sum(Phi, axis=3)
    Ps[Ps == 0] = 1
    del RECORD[:]
    ref_shims.PSNR_LOG.clear()
    rec = cg_utils.GAP_TV_rec(y, Phi, Ps, gt, cg_utils.A_, cg_utils.At_, maxiter=maxiter, step_size=step, tv_weight=tv_weight)
    f64 = cg_utils.psnr(rec.numpy().astype(np.float64), gt)                # (the print used the float64 f)
    B = Phi.shape[-1]
    rs = np.array(RECORD, dtype=object).reshape(maxiter, B, 3)
    return rec.numpy(), f64, rs


def main():
    out = {}
    ids, psnr_ref, psnr, stop, margin, tie, clip_mean = [], [], [], [], [], [], []
    drop_gap = None
    for clip, ms in CLIPS:
        d = load_test_data(DATA + f"{clip}_cacti.mat")
        Phi = torch.from_numpy(d["mask"])[None]
        per = []
        for m in ms:
            t0 = time.time()
            y = torch.from_numpy(np.ascontiguousarray(d["meas"][..., m]))[None]
            gt = d["gt"][..., 8 * m:8 * (m + 1)][None]
            rec, pr, rs = run(y, Phi, gt, MAXITER)
            ids.append(f"{clip}:{m}")
            psnr_ref.append(pr)
            psnr.append(harness_psnr(rec, gt))
            per.append(psnr[-1])
            stop.append(rs[..., 0].astype(np.int32))
            margin.append(rs[..., 1].astype(np.float64))
            tie.append(rs[..., 2].astype(np.float64))
            if m == 0 and clip in ("drop8", "traffic"):
                out[f"rec_{clip}_0_crop"] = rec[CROP].astype(np.float32)
                out[f"rec_{clip}_0_frames"] = frames(rec)
            if m == 0 and clip == "drop8":
                drop_gap = (y, Phi, gt, rec)
            print(f"{clip}:{m} GAP-TV PSNR {pr:.4f} (harness {psnr[-1]:.4f}), stop fired in {(stop[-1] < N_ITER_MAX).sum()} of "
                  f"{stop[-1].size} calls, min tie {tie[-1].min():.2e}, {time.time() - t0:.1f} s", flush=True)
        clip_mean.append(float(np.mean(per)))
    out.update(ids=np.array(ids), psnr_ref=np.array(psnr_ref), psnr=np.array(psnr), stop=np.stack(stop), margin=np.stack(margin),
               tie=np.stack(tie), clip_mean_psnr=np.array(clip_mean))

    y, Phi = small_case()
    H, W, B, it = SMALL
    gt = np.zeros((1, H, W, B), np.float32)
    rec, _, rs = run(torch.from_numpy(y), torch.from_numpy(Phi), gt, it)
    out.update(small_sha=np.array(sha(y, Phi)), small_rec64=LAST[0].astype(np.float64), small_stop=rs[None, ..., 0].astype(np.int32),
               small_margin=rs[None, ..., 1].astype(np.float64), small_tie=rs[None, ..., 2].astype(np.float64))

    import make_golden                                                     # the reference's DEQ builders (cnn.ckpt)
    y, Phi, gt, x0 = drop_gap
    Ps = torch.sum(Phi, axis=3)
    Ps[Ps == 0] = 1
    torch.manual_seed(0)
    _, deq = make_golden.build_deq("SimpleCNN", 10)
    rec = deq.forward(y, Phi, Ps, initial_point=torch.from_numpy(x0), train_flag=False).detach().numpy()
    out.update(deq_rec_crop=rec[CROP].astype(np.float32), deq_rec_frames=frames(rec), deq_psnr=np.float64(harness_psnr(rec, gt)))
    print("DEQ SimpleCNN Anderson 10 from GAP-TV on drop8:0: PSNR %.4f" % out["deq_psnr"])
    np.savez_compressed(os.path.join(HERE, "gaptv.npz"), **out)
    print("wrote", os.path.join(HERE, "gaptv.npz"), os.path.getsize(os.path.join(HERE, "gaptv.npz")), "bytes")


# name, H, W, B, maxiter, step_size, tv_weight, mask, seed: B = 1, 5 (< 8: left to right), 13 (the 8-sum loop and a tail of 5), 16 (two
# rounds, no tail), 128 (sixteen rounds, MAX_FRAMES); 17 x 130 is three 64-column tiles, the last ragged, and two 16-row tiles
SHAPES = (("b1", 19, 23, 1, 6, 1.0, 0.3, "float", 1),
          ("b5", 17, 130, 5, 4, 1.0, 0.3, "binary", 2),
          ("b13", 11, 23, 13, 4, 1.0, 0.3, "zeros", 3),
          ("b16", 9, 21, 16, 4, 1.5, 0.3, "float", 4),
          ("b128", 5, 7, 128, 3, 1.0, 0.1, "binary", 5))


def shape_case(H, W, B, mask, seed):
    """A seeded case (numpy float64 arithmetic, rounded to float32 once; restated in tests/test_gaptv_edges.py) -> y (1,H,W),
    Phi (1,H,W,B) float32.  mask: "float" uniform in [0,1), "binary" 0/1, "zeros" uniform with column 0 and the centre pixel zero
    in every frame (Phi_sum 0 there, replaced by 1)."""
    rs = np.random.RandomState(seed)
    x = rs.random_sample((1, H, W, B))
    x = (x + np.roll(x, 1, axis=1) + np.roll(x, 1, axis=2)) / 3.0
    u = rs.random_sample((1, H, W, B))
    Phi = (u < 0.5).astype(np.float32) if mask == "binary" else u.astype(np.float32)
    if mask == "zeros":
        Phi[0, :, 0, :] = 0
        Phi[0, H // 2, W // 2, :] = 0
    y = np.sum(x * Phi, axis=3).astype(np.float32)
    return y, Phi


def shapes():
    out = {}
    for name, H, W, B, it, step, weight, mask, seed in SHAPES:
        t0 = time.time()
        y, Phi = shape_case(H, W, B, mask, seed)
        _, _, rs = run(torch.from_numpy(y), torch.from_numpy(Phi), np.zeros((1, H, W, B), np.float32), it, step, weight)
        tie = rs[..., 2].astype(np.float64)
        assert tie.min() >= 1e-9, (name, tie.min())
        out.update({f"{name}_params": np.array([H, W, B, it, step, weight, seed], np.float64), f"{name}_sha": np.array(sha(y, Phi)),
                    f"{name}_rec64": LAST[0].astype(np.float64), f"{name}_stop": rs[None, ..., 0].astype(np.int32),
                    f"{name}_margin": rs[None, ..., 1].astype(np.float64), f"{name}_tie": tie[None]})
        print(f"{name}: {H}x{W}x{B}, {it} iterations, stops {sorted(set(rs[..., 0].ravel().tolist()))}, min tie {tie.min():.2e}, "
              f"{time.time() - t0:.1f} s", flush=True)
    path = os.path.join(HERE, "gaptv_shapes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    shapes() if sys.argv[1:] == ["--shapes"] else main()
