#!/usr/bin/env python3
"""Time one Broyden step on the device: the HIP step kernels (csrc/broyden.hip: four launches) against the same step written with
torch contractions on a history stored in the reference's layout ((bsz,N,1,L) / (bsz,L,N,1), history index innermost).

    python tools/broyden_bench.py [--steps 200] [--warmup 20] [--out FILE.md]

Per (bsz, t) at N = 256 x 256 x 8: microseconds per step from device events around `--steps` steps, and the algorithmic bytes
4 N (5 t + 13) bsz over that time against the 8 TB/s HBM peak.  At bsz = 8 the steps rotate over several workspaces so that the
history read by a step (2 t bsz N floats, at least 300 MB) was not left in the 256 MiB Infinity Cache by the previous one; at bsz = 1
the solver itself re-reads one history of at most 113 MB step after step, so one workspace is what it sees.  Needs an MI355X."""
import argparse
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deqsci_amd import _hip  # noqa: E402

N = 256 * 256 * 8
L = 27
PEAK = 8.0e12


def timed(fn, steps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def hip_step(bsz, t, sets):
    g = torch.Generator(device="cuda").manual_seed(0)
    state = []
    for _ in range(sets):
        ws = _hip.BroydenWorkspace(bsz, N, L, "cuda")
        ws.U.normal_(generator=g).mul_(N ** -0.5)
        ws.V.normal_(generator=g)
        rows = [torch.randn(bsz, N, device="cuda", generator=g) for _ in range(4)]
        state.append((ws, rows, torch.empty(bsz, N, device="cuda"), torch.empty(bsz, N, device="cuda")))
    slot = t % L

    def step(i):
        ws, (dx, g0, g1, x), upd, xn = state[i % sets]
        _hip.broyden_dots(ws, dx, g0, g1, t)
        _hip.broyden_update(ws, dx, g0, g1, t, slot, upd, x=x, x_next=xn)
    return step


def einsum_step(bsz, t, sets):
    """The same step with torch contractions on a history stored the reference's way: hist_u (bsz,N,1,L) with the history index innermost,
    hist_v (bsz,L,N,1).  Written from the algorithm (tests/broyden_f64.py: step_f64) on (bsz,N,L) / (bsz,L,N) views of those buffers."""
    g = torch.Generator(device="cuda").manual_seed(0)
    state = []
    for _ in range(sets):
        hist_u = torch.randn(bsz, N, 1, L, device="cuda", generator=g) * N ** -0.5
        hist_v = torch.randn(bsz, L, N, 1, device="cuda", generator=g)
        state.append((hist_u, hist_v, [torch.randn(bsz, N, device="cuda", generator=g) for _ in range(4)]))
    slot = t % L
    filled = max(t, slot + 1)

    def step(i):
        hist_u, hist_v, (dx, g0, g1, x) = state[i % sets]
        Um, Vm = hist_u.squeeze(2), hist_v.squeeze(3)                # (bsz,N,L) strided by L, (bsz,L,N)
        dg = g1 - g0
        coef_a = torch.einsum("bn,bnl->bl", dx, Um[:, :, :t])
        coef_b = torch.einsum("bln,bn->bl", Vm[:, :t], dg)
        v_row = torch.einsum("bl,bln->bn", coef_a, Vm[:, :t]) - dx
        w_row = dx + dg - torch.einsum("bnl,bl->bn", Um[:, :, :t], coef_b)
        u_row = w_row / (v_row * dg).sum(1, keepdim=True)
        Vm[:, slot] = torch.nan_to_num(v_row, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
        Um[:, :, slot] = torch.nan_to_num(u_row, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
        coef_c = torch.einsum("bln,bn->bl", Vm[:, :filled], g1)
        return x + (g1 - torch.einsum("bnl,bl->bn", Um[:, :, :filled], coef_c))
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("broyden_bench needs an MI355X: a CPU run measures nothing")
    lines = ["| bsz | t | workspaces | HIP us/step | algorithmic GB | TB/s | of 8 TB/s | einsum us/step | einsum / HIP |", "|---|---|---|---|---|---|---|---|---|"]
    for bsz in (1, 8):
        for t in (9, 27):
            sets = 1 if bsz == 1 else (3 if t == 9 else 2)
            hip_us = timed(hip_step(bsz, t, sets), a.steps, a.warmup)
            torch.cuda.empty_cache()
            ein_us = timed(einsum_step(bsz, t, sets), max(a.steps // 4, 10), max(a.warmup // 4, 3))
            torch.cuda.empty_cache()
            nbytes = 4 * N * (5 * t + 13) * bsz
            rate = nbytes / (hip_us * 1e-6)
            lines.append(f"| {bsz} | {t} | {sets} | {hip_us:.1f} | {nbytes / 1e9:.3f} | {rate / 1e12:.2f} | {rate / PEAK:.2f} | {ein_us:.1f} | {ein_us / hip_us:.1f} |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    text += f"\n{torch.cuda.get_device_name(0)}, torch {torch.__version__}, {a.steps} steps after {a.warmup} warm-up steps, device events.\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
