#!/usr/bin/env python3
"""The four power-iteration steps of ONE train-mode f-call of RealSN_SimpleCNN (shipped weights, 40 x 40 maps) on the device: the
composed torch operations of the reference's pre-forward hook (networks/provable/model/conv_sn_chen.py:29-50 - conv2d, flip, permute,
and normalize()'s float(torch.sqrt(...)), i.e. two host synchronisations per layer) against R1 of csrc/realsn.hip (4 launches per layer,
none).  And the gradient of the four normalised weights for a given upstream gradient: autograd's backward through the composed
last two lines of the step against R2 (2 launches per layer).  HIP events after warm-up, the median of the repeats; every repeat starts
from the same weight_u.  Prints one line per measurement and a JSON line.

Then the train-mode device paths at 256 x 256 x 8 with 1 and 8 measurements per call (a second JSON line):

  packs       R3 alone per layer shape (every pack of the layer, one launch) against the host packers making the same packs
  f-call      one train-mode f-call of the engine's denoiser: the module (power step on csrc/realsn.hip, convolutions on MIOpen) against
              train_realsn="device" (R1 in place, R3, first-layer stencil, fp32 64->64 kernels, last-layer kernel)
  taped call  the taped call and its backward for a seeded upstream gradient: the module on autograd's tape against
              autograd.denoiser_noise(train_realsn=True) (parameter_backward = "device+realsn")

No threshold: the defaults stay "module" / "autograd"; the numbers go to profiles/realsn.md with the board they were measured on.

    python tools/realsn_bench.py [--reps 50] [--warmup 5] [--train-reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, autograd as ag, checkpoint, vjp  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.engine import _Denoiser  # noqa: E402
from deqsci_amd.networks.simplecnn import RealSNConv2d  # noqa: E402

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


def composed_normalize(t, eps):
    norm = max(float(torch.sqrt(torch.sum(t * t))), eps)           # (the host synchronisation of the composed form)
    return t / norm


def composed_step(W, u, sigma, eps=1e-12):
    """One step as composed torch operations, as the reference writes it; -> (weight, u, v, cur_sigma), weight on the tape of W."""
    with torch.no_grad():
        v = composed_normalize(F.conv2d(u.flip(2, 3), W.permute(1, 0, 2, 3), padding=1), eps).flip(2, 3)
        u = composed_normalize(F.conv2d(v, W, padding=1), eps).clone()
        v = v.clone()
    cur_sigma = torch.sum(u * F.conv2d(v, W, padding=1))
    return W / cur_sigma * sigma, u, v, cur_sigma


def train_net():
    net = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 10)[0].nonlinear_op.train()
    for p in net.parameters():
        p.requires_grad_(True)
    return net


def fcall_and_taped(bsz, reps, warmup, out):
    """One train-mode f-call of the engine's denoiser, module against train_realsn="device", and the taped call with its backward,
    autograd against autograd.denoiser_noise(train_realsn=True), on bsz measurements of 256 x 256 x 8.  Every path runs its own copy of
    the net (each call advances weight_u)."""
    n = bsz * B
    gen = torch.Generator(device="cuda").manual_seed(bsz)
    z1 = torch.rand(bsz, B, H, W, device="cuda", generator=gen)
    v = torch.randn(n, 1, H, W, device="cuda", generator=gen)
    dens = {mode: _Denoiser(train_net(), train_realsn=mode) for mode in ("module", "device")}
    for den in dens.values():
        den.prepare(4, "cuda", n_img=n)
    assert dens["device"]._route(n, H, W, "cuda", "fast", False) == "train realsn per layer" and dens["module"]._route(n, H, W, "cuda", "fast", False) == "module"
    with torch.no_grad():
        for mode, den in dens.items():
            out[f"fcall_{mode}_ms_bsz{bsz}"] = timed(lambda _, den=den: den.run(z1, 1), reps, warmup)
        nets = [train_net(), train_net()]
        d = _Denoiser(nets[0], train_realsn="device").run(z1, 1)[0]
        m = _Denoiser(nets[1], train_realsn="module").run(z1, 1)[0]
        out[f"fcall_rel_l2_bsz{bsz}"] = float((d - m).norm() / m.norm())
    x = z1.view(n, 1, H, W)
    net_a, net_d = train_net(), train_net()

    def taped_module(_):
        return torch.autograd.grad(net_a(x), vjp.grad_parameters(net_a, train_realsn=True), v)

    def taped_device(_):
        return torch.autograd.grad(ag.denoiser_noise(net_d, x, train_realsn=True), vjp.grad_parameters(net_d, train_realsn=True), v)

    out[f"taped_autograd_ms_bsz{bsz}"] = timed(taped_module, reps, warmup)
    out[f"taped_device_ms_bsz{bsz}"] = timed(taped_device, reps, warmup)
    net_a, net_d = train_net(), train_net()
    out[f"taped_grad_rel_l2_bsz{bsz}"] = max(float((p - q).norm() / q.norm()) for p, q in zip(taped_device(None), taped_module(None)))
    print(f"bsz {bsz} ({n} images of {H} x {W}): train-mode f-call module {out[f'fcall_module_ms_bsz{bsz}']:.3f} ms, train_realsn='device' "
          f"{out[f'fcall_device_ms_bsz{bsz}']:.3f} ms (rel L2 {out[f'fcall_rel_l2_bsz{bsz}']:.1e});  taped call + backward autograd "
          f"{out[f'taped_autograd_ms_bsz{bsz}']:.3f} ms, 'device+realsn' {out[f'taped_device_ms_bsz{bsz}']:.3f} ms "
          f"(gradients rel L2 {out[f'taped_grad_rel_l2_bsz{bsz}']:.1e})")


def packs(reps, warmup, out):
    """R3 alone per layer shape - every pack of the layer in one launch - against the host packers making the same packs."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    for cin, cout in ((1, 64), (64, 64), (64, 1)):
        w = torch.randn(cout, cin, 3, 3, device="cuda", generator=gen)
        bufs = _hip.realsn_pack_buffers(cin, cout, "cuda")
        if (cin, cout) == (64, 64):
            host = lambda _: (_hip.pack_winograd_weights(w), _hip.pack_winograd44_weights(w), _hip.pack_winograd_weights(vjp._transposed(w)))
        elif cin == 1:
            host = lambda _: (_hip.pack_c1_to_64_weights(w), _hip.pack_c64_to_1_weights(vjp._transposed(w)))
        else:
            host = lambda _: (_hip.pack_c64_to_1_weights(w), _hip.pack_c1_to_64_weights(vjp._transposed(w)))
        tag = f"{cin}x{cout}"
        out[f"pack_host_ms_{tag}"] = timed(host, reps, warmup)
        out[f"pack_r3_ms_{tag}"] = timed(lambda _: _hip.realsn_pack(w, *bufs), reps, warmup)
        print(f"packs of a ({cout},{cin},3,3) weight: host packers {out[f'pack_host_ms_{tag}'] * 1e3:.1f} us, R3 {out[f'pack_r3_ms_{tag}'] * 1e3:.1f} us (one launch)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-reps", type=int, default=10, help="repeats of the 256 x 256 x 8 f-call and taped-call measurements (0: skip them)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "realsn_bench needs a GPU"
    solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 10)
    convs = [m for m in solver.nonlinear_op.modules() if isinstance(m, RealSNConv2d)]
    Ws = [m.weight_orig.detach().clone().requires_grad_(True) for m in convs]
    us = [m.weight_u.detach().clone() for m in convs]
    sig = [float(m.sigma) for m in convs]
    g = torch.Generator(device="cuda").manual_seed(0)
    Gs = [torch.randn(W.shape, device="cuda", generator=g) for W in Ws]
    wss = [_hip.realsn_workspace(W.shape[1], W.shape[0], u.shape[2], u.shape[3], "cuda") for W, u in zip(Ws, us)]
    out = {"layers": [list(W.shape) for W in Ws], "map": list(us[0].shape[2:]), "reps": a.reps}

    def fresh_u(_=None):
        return [u.clone() for u in us]

    def power_composed(u0):
        with torch.no_grad():
            return [composed_step(W, u, s) for W, u, s in zip(Ws, u0, sig)]

    def power_device(u0):
        return [_hip.realsn_power(W.detach(), u, 1, s, 1e-12, workspace=ws) for W, u, s, ws in zip(Ws, u0, sig, wss)]

    out["power_composed_ms"] = timed(power_composed, a.reps, a.warmup, fresh_u)
    out["power_device_ms"] = timed(power_device, a.reps, a.warmup, fresh_u)
    out["power_device_launches"] = 4 * len(Ws)

    def taped(_=None):
        return [composed_step(W, u, s)[0] for W, u, s in zip(Ws, us, sig)]

    def grad_autograd(weights):
        return torch.autograd.grad(weights, Ws, Gs)

    kept = [_hip.realsn_power(W.detach(), u.clone(), 1, s, 1e-12, workspace=ws) for W, u, s, ws in zip(Ws, us, sig, wss)]

    def grad_device(_):
        return [_hip.realsn_grad(G, W.detach(), k[1], k[2], k[3], s, workspace=ws) for G, W, k, s, ws in zip(Gs, Ws, kept, sig, wss)]

    out["grad_autograd_ms"] = timed(grad_autograd, a.reps, a.warmup, taped)
    out["grad_device_ms"] = timed(grad_device, a.reps, a.warmup)
    out["grad_device_launches"] = 2 * len(Ws)
    # the two forms compute the same thing
    want = torch.autograd.grad(taped(), Ws, Gs)
    out["grad_rel_l2_device_vs_autograd"] = max(float((d - w).norm() / w.norm()) for d, w in zip(grad_device(None), want))
    print(f"power step x {len(Ws)} layers, one f-call:  composed torch {out['power_composed_ms']:.3f} ms   R1 {out['power_device_ms']:.3f} ms "
          f"({out['power_device_launches']} launches)   x{out['power_composed_ms'] / out['power_device_ms']:.1f}")
    print(f"weight gradient x {len(Ws)} layers:         autograd       {out['grad_autograd_ms']:.3f} ms   R2 {out['grad_device_ms']:.3f} ms "
          f"({out['grad_device_launches']} launches)   x{out['grad_autograd_ms'] / out['grad_device_ms']:.1f}   "
          f"(relative L2 between them {out['grad_rel_l2_device_vs_autograd']:.2e})")
    print(json.dumps(out))
    if a.train_reps > 0:
        # the train-mode device paths (train_realsn="device", "device+realsn") at 256 x 256 x 8 with 1 and 8 measurements, and R3 alone
        out = {"device": torch.cuda.get_device_name(0), "shape": [H, W, B], "reps": a.train_reps}
        packs(a.reps, a.warmup, out)
        for bsz in (1, 8):
            fcall_and_taped(bsz, a.train_reps, 3, out)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
