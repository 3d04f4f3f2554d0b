#!/usr/bin/env python3
"""BatchNorm2d in train mode on the device (csrc/bn_train.hip) against the torch module, at 256 x 256 x 8 with 1 and 8 measurements per
call - FFDNet with the shipped weights in .train(), what the reference's training script runs:

  f-call      one train-mode f-call of the engine's denoiser: the module (MIOpen; train_bn="module") against train_bn="device"
              (head kernel -> 13 x [fp32 Winograd raw convolution -> T1 -> T2] -> tail kernel)
  taped call  the taped call and its backward for a seeded upstream gradient: the module on autograd's tape against
              autograd.denoiser_noise(train_bn=True) (parameter_backward = "device+bn-train")
  T1 .. T4    each kernel alone on an (n,64,128,128) activation, n = 8 and 64 images, with the bytes it has to move (T1 reads c twice,
              T2 reads and writes, T3 reads two, T4 reads two and writes one) over its time

HIP events after a warm-up, the median of 10 repeats, two runs of everything.  Prints one line per measurement and a JSON line; the
numbers go to profiles/bn_train.md with the board they were measured on.  No threshold: both defaults stay "module" / "autograd".

    python tools/bn_train_bench.py [--reps 10] [--warmup 3] [--runs 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, autograd as ag, checkpoint, vjp  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.engine import _Denoiser  # noqa: E402

H = W = 256
B = 8


def timed(fn, reps, warmup, before=None):
    """Median ms of fn(state) over `reps` runs; before() -> state runs untimed in front of each."""
    ms = []
    for i in range(warmup + reps):
        state = before() if before is not None else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def fcall_and_taped(bsz, a, out):
    net = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), 10)[0].nonlinear_op.train()
    n = bsz * B
    gen = torch.Generator(device="cuda").manual_seed(bsz)
    z1 = torch.rand(bsz, B, H, W, device="cuda", generator=gen)
    v = torch.randn(n, 1, H, W, device="cuda", generator=gen)
    dens = {mode: _Denoiser(net, train_bn=mode) for mode in ("module", "device")}
    for den in dens.values():
        den.prepare(4, "cuda", n_img=n)
    assert dens["device"]._route(n, H, W, "cuda", "fast", False) == "train bn per layer" and dens["module"]._route(n, H, W, "cuda", "fast", False) == "module"
    with torch.no_grad():
        for mode, den in dens.items():
            out[f"fcall_{mode}_ms_bsz{bsz}"] = timed(lambda _, den=den: den.run(z1, 1), a.reps, a.warmup)
        d = dens["device"].run(z1, 1)[0]
        m = dens["module"].run(z1, 1)[0]
        out[f"fcall_rel_l2_bsz{bsz}"] = float((d - m).norm() / m.norm())
    x = z1.view(n, 1, H, W)
    sigma = dens["device"].sigma_table[1:2].expand(n)
    params = vjp.grad_parameters(net, train_bn=True)

    def taped_module(_):
        return torch.autograd.grad(net(x, sigma), params, v)

    def taped_device(_):
        return torch.autograd.grad(ag.denoiser_noise(net, x, sigma, train_bn=True), params, v)

    out[f"taped_autograd_ms_bsz{bsz}"] = timed(taped_module, a.reps, a.warmup)
    out[f"taped_device_ms_bsz{bsz}"] = timed(taped_device, a.reps, a.warmup)
    out[f"taped_grad_rel_l2_bsz{bsz}"] = max(float((p - q).norm() / q.norm()) for p, q in zip(taped_device(None), taped_module(None)))
    print(f"bsz {bsz} ({n} images of {H} x {W}): f-call module {out[f'fcall_module_ms_bsz{bsz}']:.3f} ms, train_bn='device' "
          f"{out[f'fcall_device_ms_bsz{bsz}']:.3f} ms (rel L2 {out[f'fcall_rel_l2_bsz{bsz}']:.1e});  taped call + backward autograd "
          f"{out[f'taped_autograd_ms_bsz{bsz}']:.3f} ms, 'device+bn-train' {out[f'taped_device_ms_bsz{bsz}']:.3f} ms "
          f"(gradients rel L2 {out[f'taped_grad_rel_l2_bsz{bsz}']:.1e})")


def kernels(n, a, out):
    h = w = H // 2                                                     # FFDNet's 64 -> 64 layers run at half resolution
    gen = torch.Generator(device="cuda").manual_seed(n)
    c = torch.randn(n, 64, h, w, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, 64, h, w, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    gamma, beta = torch.rand(64, device="cuda", generator=gen) + 0.5, torch.randn(64, device="cuda", generator=gen)
    rm, rv, nbt = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    P = n * h * w
    ws, rec = _hip.bn_train_workspace(P, "cuda"), torch.empty(128, dtype=torch.float64, device="cuda")
    y, mask, dc = torch.empty_like(c), torch.empty((n, h, w), dtype=torch.int64, device="cuda"), torch.empty_like(c)
    _hip.bn_train_stats(c, rm, rv, nbt, 0.1, record=rec, workspace=ws)
    grec = _hip.bn_train_grad_stats(gy, c, rec, 1e-5, ws)[2]
    act = P * 64 * 4
    runs = {"T1": (lambda _: _hip.bn_train_stats(c, rm, rv, nbt, 0.1, record=rec, workspace=ws), 2 * act),
            "T2": (lambda _: _hip.bn_train_apply(c, rec, gamma, beta, 1e-5, relu=True, out=y, mask=mask), 2 * act + P * 8),
            "T3": (lambda _: _hip.bn_train_grad_stats(gy, c, rec, 1e-5, ws), 2 * act),
            "T4": (lambda _: _hip.bn_train_grad_apply(gy, c, rec, grec, gamma, 1e-5, out=dc), 3 * act)}
    line = []
    for name, (fn, nbytes) in runs.items():
        ms = timed(fn, a.reps, a.warmup)
        out[f"{name}_ms_n{n}"], out[f"{name}_TBps_n{n}"] = ms, nbytes / (ms * 1e-3) / 1e12
        line.append(f"{name} {ms * 1e3:.1f} us ({out[f'{name}_TBps_n{n}']:.2f} TB/s)")
    print(f"n = {n} images of {h} x {w} x 64 ({act / 2**20:.0f} MiB): " + ", ".join(line))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bn_train_bench needs a GPU"
    for run in range(a.runs):
        out = {"run": run, "device": torch.cuda.get_device_name(0), "shape": [H, W, B], "reps": a.reps}
        for bsz in (1, 8):
            fcall_and_taped(bsz, a, out)
        for n in (8, 64):
            kernels(n, a, out)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
