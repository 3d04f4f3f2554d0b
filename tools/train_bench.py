#!/usr/bin/env python3
"""One training step at 256 x 256 x 8, and_maxiters 30, for SimpleCNN and FFDNet (shipped weights, train mode) at batch 1 and 8:
the all-autograd step (nn.MSELoss, loss.item(), the PSNR on the host, torch.optim.Adam - the reference's step) against the all-device
step (training.configure_training(deq, "device"), autograd.mse_loss_stats with its one read-back, optim.DeviceAdam).
HIP events after warm-up, the median of the repeats.  The parts of a step:
    solve      the no-tape fixed-point solve inside deq.forward (the solver call, or the engine's solve where the train-mode f-calls run there)
    taped      the rest of deq.forward: the taped call z = f(z*), f0 = f(z0), the device map
    hook       the implicit backward's solve inside loss.backward()
    param      the rest of loss.backward(): the loss gradient and the denoiser's weight gradients
    glue       loss, NaN check and batch PSNR as the loop takes them (autograd: MSELoss, .item(), clip + copy to the host + PSNR there)
    optimizer  optimizer.step()
and L1 / L2 alone against what they replace: the composed torch expressions for loss, gradient, clamped squared error and non-finite count,
and torch.optim.Adam.step() (its default multi-tensor form and foreach=False) on the same parameter tensors.
Clipping by global norm (--parts clip), on each denoiser's parameter list: L3 alone (_hip.grad_norm); L2c against L2 (_hip.adam_step with and
without the statistics); and the clipped optimizer step DeviceAdam(max_grad_norm=...).step() against torch.nn.utils.clip_grad_norm_ followed
by DeviceAdam.step() on the same gradients in the same process, with the launches of each.
Prints one line per (denoiser, batch, backend) and a JSON line.

    python tools/train_bench.py [--denoisers SimpleCNN,ffdnet] [--batches 1,8] [--iters 30] [--reps 10] [--warmup 2] [--parts steps,kernels,clip]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deqsci_amd  # noqa: E402
from deqsci_amd import _hip, checkpoint, harness, solvers, training  # noqa: E402
from deqsci_amd.autograd import mse_loss_stats  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.optim import DeviceAdam  # noqa: E402

WEIGHTS = {"SimpleCNN": "cnn", "ffdnet": "ffdnet_gray", "RealSN_SimpleCNN": "rsn_cnn"}
PARTS = ("total", "solve", "taped", "hook", "param", "glue", "optimizer")


class Span:
    """HIP events around a piece of host code; .ms after a synchronise"""

    def __init__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        self.e0.record()
        return self

    def __exit__(self, *a):
        self.e1.record()
        return False

    @property
    def ms(self):
        return self.e0.elapsed_time(self.e1)


def timed(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        with Span() as s:
            fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.ms)
    return statistics.median(ms)


def step_parts(kind, backend, bsz, iters, reps, warmup):
    dev = "cuda"
    solver, deq = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), iters)
    solver.nonlinear_op.train()
    cfg = training.configure_training(deq, backend)
    device = backend == "device"
    opt = (DeviceAdam if device else torch.optim.Adam)(solver.parameters(), lr=1e-6)       # (a small lr: every repeat on nearly the same weights)
    loss_fn = torch.nn.MSELoss(reduction="mean")
    g = torch.Generator(device=dev).manual_seed(bsz)
    Phi = (torch.rand(bsz, 256, 256, 8, device=dev, generator=g) < 0.5).float()
    gt = torch.rand(bsz, 256, 256, 8, device=dev, generator=g)
    y = (gt * Phi).sum(-1)
    Ps = deqsci_amd.phi_sum(Phi)
    spans = []                                                   # the solver calls of the step in progress
    real_solver = deq.solver

    def solver_fn(*a, **k):
        with Span() as s:
            out = real_solver(*a, **k)
        spans.append(s)
        return out
    eng = deq._train_solve_engine()
    if eng is not None:                                          # the train-mode f-calls run on the engine: its solve is the forward's solver call
        real_solve = eng.solve

        def solve_fn(*a, **k):
            with Span() as s:
                out = real_solve(*a, **k)
            spans.append(s)
            return out
        eng.solve = solve_fn
    # (DEQFixedPoint picks the engine by `self.solver is andersonexp`: the timed wrapper takes that name for the length of this run)
    deq.solver = solvers.andersonexp = solver_fn
    try:
        return _measure(kind, backend, bsz, cfg, solver, deq, opt, loss_fn, (y, Phi, Ps, gt), spans, device, reps, warmup)
    finally:
        solvers.andersonexp = real_solver


def _measure(kind, backend, bsz, cfg, solver, deq, opt, loss_fn, data, spans, device, reps, warmup):
    y, Phi, Ps, gt = data
    rows = {p: [] for p in PARTS}
    last = {}
    for i in range(warmup + reps):
        del spans[:]
        with Span() as total:
            opt.zero_grad()
            with torch.no_grad():
                x0 = deqsci_amd.initial_point(y, Phi, Ps, gt)
            with Span() as fwd:
                rec = deq.forward(y, Phi, Ps, initial_point=x0)
            n_fwd = len(spans)
            with Span() as glue:
                if device:
                    loss, stats = mse_loss_stats(rec, gt)
                    host = stats.cpu()
                    value, psnr = float(host[0]) / rec.numel(), 10.0 * math.log10(rec.numel() / float(host[1]))
                else:
                    loss = loss_fn(rec, gt)
                    value = loss.item()
                    psnr = harness.psnr(rec.clip(0, 1).cpu().detach().numpy(), gt.cpu().detach().numpy())
                assert not math.isnan(value)
            with Span() as bwd:
                loss.backward()
            with Span() as step:
                opt.step()
        torch.cuda.synchronize()
        if i >= warmup:
            solve = sum(s.ms for s in spans[:n_fwd])
            hook = sum(s.ms for s in spans[n_fwd:])
            for name, v in (("total", total.ms), ("solve", solve), ("taped", fwd.ms - solve), ("hook", hook), ("param", bwd.ms - hook),
                            ("glue", glue.ms), ("optimizer", step.ms)):
                rows[name].append(v)
        last = {"loss": value, "psnr": psnr, "backward_path": deq.last_backward_path, "parameter_path": deq.last_parameter_path}
    med = {p: statistics.median(v) for p, v in rows.items()}
    return {"denoiser": kind, "bsz": bsz, "backend": backend, "implicit_backward": cfg.implicit_backward, "parameter_backward": cfg.parameter_backward,
            "engine_options": cfg.engine_options, "reasons": cfg.reasons, "parameters": len(list(solver.parameters())), **{p + "_ms": med[p] for p in PARTS}, **last}


def kernels_alone(kind, bsz, reps, warmup):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(3)
    rec = torch.rand(bsz, 256, 256, 8, device=dev, generator=g) * 1.2 - 0.1
    gt = torch.rand(bsz, 256, 256, 8, device=dev, generator=g)
    total = rec.numel()
    ws = _hip.mse_workspace(total, dev)

    def composed():
        d = rec - gt
        loss = (d * d).mean()
        grad = d * (2.0 / total)
        dc = rec.clamp(0, 1) - gt
        return loss, grad, (dc * dc).sum(dtype=torch.float64), (~torch.isfinite(d)).sum()
    t_l1 = timed(lambda: _hip.mse_stats_grad(rec, gt, workspace=ws), reps, warmup)
    t_l1_torch = timed(composed, reps, warmup)
    solver, _ = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), 3)
    params = list(solver.parameters())
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g)
    out = {"denoiser": kind, "bsz": bsz, "l1_ms": t_l1, "l1_torch_ms": t_l1_torch, "l1_gbs": 12.0 * total / (t_l1 * 1e-3) / 1e9,
           "tensors": len(params), "weights": sum(p.numel() for p in params)}
    for name, opt in (("l2_ms", DeviceAdam(params, lr=1e-6)), ("adam_foreach_ms", torch.optim.Adam(params, lr=1e-6)),
                      ("adam_single_ms", torch.optim.Adam(params, lr=1e-6, foreach=False))):
        out[name] = timed(opt.step, reps, warmup)
    return out


def clip_rows(kind, reps, warmup, max_norm=1e-3):
    """max_norm far below the gradients' norm: the coefficient is below 1 in every repeat, for torch's in-place scaling too"""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    solver, _ = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), 3)
    shapes = [p.shape for p in solver.parameters()]

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g)) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=g)
        return ps
    ps = params()
    grads = [p.grad for p in ps]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    stats = torch.empty(3 + len(ps), device=dev, dtype=torch.float64)
    ws = _hip.grad_norm_workspace(grads)
    out = {"denoiser": kind, "tensors": len(ps), "weights": sum(p.numel() for p in ps), "max_norm": max_norm,
           "l3_launches": _hip.grad_norm_launches(len(ps))}
    out["l3_ms"] = timed(lambda: _hip.grad_norm(grads, max_norm, stats=stats, workspace=ws), reps, warmup)
    with torch.no_grad():
        out["l2_ms"] = timed(lambda: _hip.adam_step(ps, grads, ms, vs, 1, 1e-6, (0.9, 0.999), 1e-8), reps, warmup)
        out["l2c_ms"] = timed(lambda: _hip.adam_step(ps, grads, ms, vs, 1, 1e-6, (0.9, 0.999), 1e-8, stats=stats), reps, warmup)
    fused = DeviceAdam(params(), lr=1e-6, max_grad_norm=max_norm)
    pt = params()
    plain = DeviceAdam(pt, lr=1e-6)

    def composed():
        torch.nn.utils.clip_grad_norm_(pt, max_norm)
        plain.step()
    out["clipped_step_ms"] = timed(fused.step, reps, warmup)
    out["clipped_step_launches"] = fused.last_launches
    out["torch_clip_plus_step_ms"] = timed(composed, reps, warmup)
    out["torch_clip_ms"] = timed(lambda: torch.nn.utils.clip_grad_norm_(pt, max_norm), reps, warmup)
    # the launches of torch's clip_grad_norm_, counted by the profiler (one step, behind the timed ones)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        torch.nn.utils.clip_grad_norm_(pt, max_norm)
        torch.cuda.synchronize()
    out["torch_clip_launches"] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--denoisers", default="SimpleCNN,ffdnet")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="steps,kernels,clip")
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = {"H": 256, "W": 256, "B": 8, "and_maxiters": a.iters, "reps": a.reps, "steps": [], "kernels": [], "clip": []}
    for kind in a.denoisers.split(","):
        if "clip" in parts:
            c = clip_rows(kind, a.reps, a.warmup)
            out["clip"].append(c)
            print(f"{kind:9s} clip {c['tensors']} tensors, {c['weights']} weights: L3 {c['l3_ms']:.4f} ms ({c['l3_launches']} launches);   L2c {c['l2c_ms']:.4f} ms vs L2 "
                  f"{c['l2_ms']:.4f} ms;   clipped DeviceAdam.step {c['clipped_step_ms']:.4f} ms ({c['clipped_step_launches']} launches) vs torch clip_grad_norm_ + "
                  f"DeviceAdam.step {c['torch_clip_plus_step_ms']:.4f} ms (clip_grad_norm_ alone {c['torch_clip_ms']:.4f} ms, {c['torch_clip_launches']} launches)", flush=True)
        for bsz in (int(b) for b in a.batches.split(",")):
            for backend in (("autograd", "device") if "steps" in parts else ()):
                r = step_parts(kind, backend, bsz, a.iters, a.reps, a.warmup)
                out["steps"].append(r)
                print(f"{kind:9s} bsz {bsz} {backend:8s}: step {r['total_ms']:9.2f} ms = solve {r['solve_ms']:8.2f} + taped {r['taped_ms']:7.2f} + hook "
                      f"{r['hook_ms']:8.2f} + param {r['param_ms']:7.2f} + glue {r['glue_ms']:6.3f} + optimizer {r['optimizer_ms']:6.3f}   "
                      f"(implicit {r['implicit_backward']}, parameter {r['parameter_backward']}; loss {r['loss']:.5f})", flush=True)
            if "kernels" not in parts:
                continue
            k = kernels_alone(kind, bsz, a.reps, a.warmup)
            out["kernels"].append(k)
            print(f"{kind:9s} bsz {bsz} alone   : L1 {k['l1_ms']:.4f} ms ({k['l1_gbs']:.0f} GB/s) vs composed torch {k['l1_torch_ms']:.4f} ms;   L2 {k['tensors']} tensors "
                  f"{k['l2_ms']:.4f} ms vs torch Adam foreach {k['adam_foreach_ms']:.4f} ms, single-tensor {k['adam_single_ms']:.4f} ms", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
