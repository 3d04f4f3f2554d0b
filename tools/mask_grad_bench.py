#!/usr/bin/env python3
"""The mask's gradient (Phi.requires_grad: a learnable coded aperture), timed two ways.

  step     the backward of the taped GAP step z1 = z + At((y - A z) / Phi_sum) with y, Phi and Phi_sum on the tape, at 256 x 256 x 8 and
           1 or 8 measurements, a mask per sample and one shared mask: the fused path (operators.gap_update -> G1, one launch of
           csrc/sci_grad.hip) against the composition z + At_torch_((y - A_torch_(z, Phi)) / Phi_sum, Phi) through the operator-level
           autograd (G2 launches and torch's elementwise backward).  torch.autograd.grad for a given upstream gradient, a fresh forward
           (untimed) per repeat, HIP events, the median.
  G1       deqsci_gap_update_grad_f32 alone at bsz = 64 (a working set above 512 MiB), on buffer sets that rotate so that no launch finds
           its inputs in the Infinity Cache, HIP events around `--launches` back-to-back launches (five such windows: the median and the spread): GB/s on the algorithmic bytes -
           (16B + 12) per pixel for the mask outputs, (20B + 16) with gz and gy; a shared mask reads and writes its (4B + 4) + (4B + 4)
           once, not per sample - and the fraction of the 8 TB/s peak, next to K3 (deqsci_gap_update_f32, (12B + 8)) in the same harness.
Prints one line per row, a markdown table and a JSON line.

    python tools/mask_grad_bench.py [--reps 20] [--warmup 3] [--launches 200] [--sets 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, operators  # noqa: E402
from deqsci_amd.operators import A_torch_, At_torch_  # noqa: E402

HBM_PEAK_GBS = 8000.0
H, W, B = 256, 256, 8
DEV = "cuda"


def timed(fn, reps, warmup, before):
    ms = []
    for i in range(warmup + reps):
        state = before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def step_rows(a, rows):
    gen = torch.Generator(device=DEV).manual_seed(0)
    for bsz in (1, 8):
        for shared in (False, True):
            nm = 1 if shared else bsz
            z = torch.randn(bsz, H, W, B, device=DEV, generator=gen)
            g = torch.randn(bsz, H, W, B, device=DEV, generator=gen)
            Phi = (0.1 + 0.9 * torch.rand(nm, H, W, B, device=DEV, generator=gen)).requires_grad_(True)
            y = A_torch_(torch.rand(bsz, H, W, B, device=DEV, generator=gen), Phi.detach()).requires_grad_(True)
            Ps = _hip.phi_sum(Phi.detach()).requires_grad_(True)
            fused = lambda: operators.gap_update(z, y, Phi, Ps)
            composed = lambda: z + At_torch_((y - A_torch_(z, Phi)) / Ps, Phi)
            back = lambda out: torch.autograd.grad(out, [y, Phi, Ps], g)
            gf, gc = back(fused()), back(composed())
            worst = max(float((p - q).norm() / q.norm()) for p, q in zip(gf, gc))
            t_f, t_c = timed(back, a.reps, a.warmup, fused), timed(back, a.reps, a.warmup, composed)
            rows.append({"what": "step", "bsz": bsz, "shared": shared, "fused_ms": t_f, "composed_ms": t_c, "rel_diff": worst})
            print(f"step bsz {bsz} {'shared' if shared else 'per-sample'}: fused {t_f * 1e3:8.1f} us   composed {t_c * 1e3:8.1f} us   "
                  f"({t_c / t_f:.2f} x)   the two agree to {worst:.1e}")


def g1_rows(a, rows):
    bsz, P = 64, H * W
    gen = torch.Generator(device=DEV).manual_seed(1)
    sets = []
    for _ in range(a.sets):
        s = {"z": torch.randn(bsz, H, W, B, device=DEV, generator=gen), "g": torch.randn(bsz, H, W, B, device=DEV, generator=gen),
             "Phi": 0.1 + 0.9 * torch.rand(bsz, H, W, B, device=DEV, generator=gen), "y": torch.rand(bsz, H, W, device=DEV, generator=gen)}
        s["Ps"] = _hip.phi_sum(s["Phi"])
        s["out"] = (torch.empty(bsz, H, W, B, device=DEV), torch.empty(bsz, H, W, device=DEV),
                    torch.empty(bsz, H, W, B, device=DEV), torch.empty(bsz, H, W, device=DEV))
        sets.append(s)

    def run(name, launch, nbytes, blocks):
        for i in range(10):
            launch(sets[i % a.sets])
        windows = []
        for _ in range(5):                                       # five windows of `launches` launches: the median, and the spread
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(a.launches):
                launch(sets[i % a.sets])
            e1.record()
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        us = statistics.median(windows)
        gbs = nbytes / (us * 1e-6) / 1e9
        rows.append({"what": name, "bsz": bsz, "us": us, "us_min": min(windows), "us_max": max(windows), "mib": nbytes / 2 ** 20, "gbs": gbs,
                     "of_peak": gbs / HBM_PEAK_GBS, "blocks": blocks})
        print(f"{name:34s}: {us:8.1f} us ({min(windows):.1f} .. {max(windows):.1f})   {nbytes / 2 ** 20:7.1f} MiB   {gbs:7.0f} GB/s = {gbs / HBM_PEAK_GBS:.2f} of peak   ({blocks} workgroups)")

    blk = -(-(P * (B // 4)) // 1024)
    run("K3 gap_update", lambda s: _hip.gap_update(s["z"], s["Phi"], s["y"], s["Ps"], out=s["out"][2]), bsz * P * (12 * B + 8), blk * bsz)
    run("G1 per sample, gPhi + gs", lambda s: _hip.gap_update_grad(s["z"], s["Phi"], s["g"], s["y"], s["Ps"], (True, True, False, False), s["out"]),
        bsz * P * (16 * B + 12), blk * bsz)
    run("G1 per sample, gPhi + gs + gz + gy", lambda s: _hip.gap_update_grad(s["z"], s["Phi"], s["g"], s["y"], s["Ps"], (True, True, True, True), s["out"]),
        bsz * P * (20 * B + 16), blk * bsz)
    sh = lambda s, need: _hip.gap_update_grad(s["z"], s["Phi"][:1], s["g"], s["y"], s["Ps"][:1], need,
                                              (s["out"][0][:1], s["out"][1][:1], s["out"][2], s["out"][3]))
    run("G1 shared, gPhi + gs", lambda s: sh(s, (True, True, False, False)), bsz * P * (8 * B + 4) + P * (8 * B + 8), blk)
    run("G1 shared, gPhi + gs + gz + gy", lambda s: sh(s, (True, True, True, True)), bsz * P * (12 * B + 8) + P * (8 * B + 8), blk)
    for n in (1, 8):                                             # the shared launch at the step's own sizes: P LP / 1024 = 128 workgroups
        z, g, y = sets[0]["z"][:n], sets[0]["g"][:n], sets[0]["y"][:n]
        for shared in (False, True):
            m = 1 if shared else n
            Phi, Ps = sets[0]["Phi"][:m], sets[0]["Ps"][:m]
            out = (sets[0]["out"][0][:m], sets[0]["out"][1][:m], None, None)
            nbytes = n * P * (8 * B + 4) + m * P * (8 * B + 8)
            t = timed(lambda _: _hip.gap_update_grad(z, Phi, g, y, Ps, (True, True, False, False), out), a.reps, a.warmup, lambda: None)
            rows.append({"what": "G1 small", "bsz": n, "shared": shared, "us": t * 1e3, "mib": nbytes / 2 ** 20, "blocks": blk * m})
            print(f"G1 bsz {n} {'shared' if shared else 'per-sample'} (cache-warm, one launch): {t * 1e3:7.1f} us   {nbytes / 2 ** 20:6.1f} MiB   {blk * m} workgroups")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--sets", type=int, default=3)
    a = ap.parse_args()
    rows = []
    step_rows(a, rows)
    g1_rows(a, rows)
    print("\n| what | bsz | time | MiB | GB/s | of 8 TB/s | workgroups |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if r["what"] == "step":
            print(f"| step backward, {'shared' if r['shared'] else 'per-sample'} mask | {r['bsz']} | fused {r['fused_ms'] * 1e3:.1f} us, composed {r['composed_ms'] * 1e3:.1f} us | | | | |")
        elif r["what"] == "G1 small":
            print(f"| G1 one launch, {'shared' if r['shared'] else 'per-sample'} mask | {r['bsz']} | {r['us']:.1f} us | {r['mib']:.1f} | | | {r['blocks']} |")
        else:
            print(f"| {r['what']} | {r['bsz']} | {r['us']:.1f} us | {r['mib']:.1f} | {r['gbs']:.0f} | {r['of_peak']:.2f} | {r['blocks']} |")
    print(json.dumps({"tool": "mask_grad_bench", "shape": [H, W, B], "launches": a.launches, "sets": a.sets, "rows": rows}))


if __name__ == "__main__":
    main()
