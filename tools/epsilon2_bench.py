#!/usr/bin/env python3
"""Time one epsilon2 step on the device: the HIP step kernels (csrc/epsilon2.hip: four launches) against the same step written as the
reference's torch expressions (solvers/new_equilibrium_utils_yaping.py:199-206 without the f-calls and the .item() read-backs).

    python tools/epsilon2_bench.py [--steps 200] [--warmup 20] [--out FILE.md]

At bsz = 8, N = 256 x 256 x 8: microseconds per step from device events around `--steps` steps, and the algorithmic bytes 28 N bsz
(three rows read, then three read and one written) over that time against the 8 TB/s HBM peak.  The steps rotate over several sets of
rows, as tools/broyden_bench.py does, so that a step's rows (67 MB) were not left in the 256 MiB Infinity Cache by the step before; one set
is timed as well: that is what the solver's loop sees between two f-calls that do not evict it.  Needs an MI355X."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deqsci_amd import _hip  # noqa: E402

BSZ, SHAPE = 8, (256, 256, 8)
N = SHAPE[0] * SHAPE[1] * SHAPE[2]
PEAK = 8.0e12
LAM = 1e-4


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


def rows(sets):
    g = torch.Generator(device="cuda").manual_seed(0)
    out = []
    for _ in range(sets):
        x = torch.randn(BSZ, N, device="cuda", generator=g)
        fx = x + 0.3 * torch.randn(BSZ, N, device="cuda", generator=g)
        ffx = fx + 0.2 * torch.randn(BSZ, N, device="cuda", generator=g)
        out.append((x, fx, ffx, torch.empty(BSZ, N, device="cuda")))
    return out


def hip_step(sets):
    state = rows(sets)
    ws = _hip.Epsilon2Workspace(BSZ, N, "cuda")

    def step(i):
        x, fx, ffx, xn = state[i % sets]
        _hip.epsilon2_norms(ws, x, fx, ffx)
        _hip.epsilon2_update(ws, x, fx, ffx, xn, LAM)
    return step


def torch_step(sets):
    """The step as the reference writes it, on (bsz, H, W, B) tensors; the two norms of the residual stay on the device."""
    state = [tuple(t.view(BSZ, *SHAPE) for t in s[:3]) for s in rows(sets)]

    def l2(t):
        return torch.sum(t ** 2, dim=[1, 2, 3], keepdim=True)

    def step(i):
        x, f_x, f_fx = state[i % sets]
        delta_x = f_x - x
        delta_f = f_fx - f_x
        delta2_x = delta_f - delta_x
        x_new = f_x + (delta_f * l2(delta_x) - delta_x * l2(delta_f)) / (l2(delta2_x) + LAM)
        return (x_new - x).norm(), x_new.norm()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("epsilon2_bench needs an MI355X: a CPU run measures nothing")
    lines = ["| bsz | N | sets of rows | HIP us/step | algorithmic GB | TB/s | of 8 TB/s | torch us/step | torch / HIP |", "|---|---|---|---|---|---|---|---|---|"]
    nbytes = 28 * N * BSZ
    for sets in (6, 1):
        hip_us = timed(hip_step(sets), a.steps, a.warmup)
        torch.cuda.empty_cache()
        ref_us = timed(torch_step(sets), a.steps, a.warmup)
        torch.cuda.empty_cache()
        rate = nbytes / (hip_us * 1e-6)
        lines.append(f"| {BSZ} | {N} | {sets} | {hip_us:.1f} | {nbytes / 1e9:.3f} | {rate / 1e12:.2f} | {rate / PEAK:.2f} | {ref_us:.1f} | {ref_us / hip_us:.1f} |")
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
