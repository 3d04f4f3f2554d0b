"""DeviceAdam: torch.optim.Adam's step for all parameter tensors of a group in one launch per table of _hip.ADAM_MAX_TENSORS tensors
(csrc/train.hip L2) instead of a dozen elementwise launches per tensor.

The arithmetic is the reference's torch-1.9 F.adam, per element in fp32, every operation rounded separately, in this order:

    m = m * beta1 + g * (1 - beta1)
    v = v * beta2 + (g * g) * (1 - beta2)
    den = sqrt(v) / sqrt(1 - beta2^t) + eps
    p = p - (lr / (1 - beta1^t)) * (m / den)

with the scalars computed in double on the host and rounded to fp32 once.  No weight decay, no amsgrad, no maximize: refused.
State and state_dict() are laid out as the installed torch.optim.Adam's (per parameter `step` - a 0-d fp32 CPU tensor -, `exp_avg`,
`exp_avg_sq`; the same param_group keys), so either optimizer loads the other's state_dict; an integer `step` (a checkpoint of the
reference's torch 1.9) is accepted.  CPU parameters take the same order of operations in torch (`adam_reference_step_`).

The kernel writes the parameters through raw pointers, which autograd's version counters do not see; every updated parameter's
counter is bumped after the launch (torch.autograd.graph.increment_version: host only, no launch), because DEQSCIEngine decides from
(data_ptr, _version) whether its packed and folded weights are stale.

Clipping (this build's; the reference trains without it, and it is off by default).  clip_grad_norm_ is torch's function on the device:
the global 2-norm of the gradients (csrc/train.hip L3: float64 sums in a fixed order, tests/clip_ref.py), the coefficient
coef = fp32(min(1, max_norm / (norm + 1e-6))) and the count of non-finite elements stay on the device, and L3s scales the gradients
in place - unless one of them holds a NaN or an Inf, where nothing is scaled.  DeviceAdam(max_grad_norm=...) fuses the scaling into the
step (L2c: g * coef in registers, p.grad untouched) and SKIPS a step whose gradient is not finite: not a word of p, exp_avg or
exp_avg_sq is written.  The host does not learn of the skip (no synchronisation), so state['step'] advances all the same: after a
skipped step the bias corrections are those of one step further on - the one deviation from "the step did not happen".
"""
import math

import numpy as np
import torch

from . import _hip


def adam_reference_step_(p, g, m, v, step, lr, betas, eps):
    """One step of the order above on fp32 CPU tensors, in place in p, m, v (the CPU path of DeviceAdam; what L2 equals bit for bit).
    The square root goes through float64: torch's CPU fp32 sqrt may be a vector library's, within an ulp but not correctly rounded,
    and the float64 root of an fp32 number rounds to the correctly rounded fp32 root."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc2s, step_size = _hip.adam_scalars(int(step), float(lr), (b1, b2))
    m.mul_(b1).add_(g * (1.0 - b1))
    v.mul_(b2).add_((g * g) * (1.0 - b2))
    den = (v.double().sqrt().float() / bc2s).add_(float(eps))
    p.sub_((m / den) * step_size)


# ----------------------------------------------------------------------------- the gradient norm on the host, in L3's order
_TB, _WAVE, _P = 256, 64, 4                                   # csrc/rows.hpp: the workgroup, the wave; csrc/train.hip: PER_THREAD


def _workgroup_sum(v):
    """v[..., 256] float64, one value per thread -> the workgroup's sum: the wave's xor butterfly, then the four waves in order"""
    w = v.reshape(v.shape[:-1] + (_TB // _WAVE, _WAVE))
    lanes = np.arange(_WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _tensor_sum(t):
    """t: float64 terms of one tensor, flat -> their sum in L3's order: per chunk of 4096 thread tid adds the terms of its float4 groups
    q = 0..3 at (q * 256 + tid) * 4 in order, then the workgroup's sum; the chunk sums by thread i adding chunks i, i + 256, ..."""
    chunk = _TB * 4 * _P
    n = -(-t.size // chunk)
    pad = np.zeros(n * chunk)
    pad[:t.size] = t
    g = pad.reshape(n, _P, _TB, 4)
    acc = np.zeros((n, _TB))
    for q in range(_P):
        for k in range(4):
            acc = acc + g[:, q, :, k]
    part = _workgroup_sum(acc)
    trips = -(-n // _TB)
    pad = np.zeros(trips * _TB)
    pad[:n] = part
    acc = np.zeros(_TB)
    for r in range(trips):
        acc = acc + pad[r * _TB:(r + 1) * _TB]
    return float(_workgroup_sum(acc))


def host_grad_stats(grads, max_norm):
    """L3 on CPU tensors -> stats (3 + n,) float64: the norm, coef, the number of non-finite elements, every tensor's own norm"""
    sums, count = [], 0.0
    with np.errstate(all="ignore"):
        for g in grads:
            a = g.detach().reshape(-1).numpy().astype(np.float64)
            sums.append(_tensor_sum(a * a))
            count += float(np.count_nonzero(~np.isfinite(a)))         # (a sum of zeros and ones: exact in every order)
        total = 0.0
        for s in sums:
            total = total + s
        norm = math.sqrt(total) if total >= 0 else float("nan")
        c = np.float64(max_norm) / np.float64(norm + 1e-6)
        coef = float(np.float32(1.0 if c >= 1.0 else c))
        return torch.tensor([norm, coef, count] + [float(np.sqrt(np.float64(s))) for s in sums], dtype=torch.float64)


def _grads_of(parameters, what):
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if g.is_sparse or g.dtype != torch.float32:
            raise NotImplementedError(f"{what}: dense float32 gradients only, got {'sparse ' if g.is_sparse else ''}{g.dtype}")
        if not g.is_contiguous():
            raise NotImplementedError(f"{what}: gradients must be contiguous (they are scaled in place through raw pointers)")
    devices = {g.device for g in grads}
    if len(devices) > 1:
        raise NotImplementedError(f"{what}: the gradients lie on {len(devices)} devices ({', '.join(sorted(str(d) for d in devices))}); the global "
                                  "norm is formed on one device without a host synchronisation")
    return grads


def _check_max_norm(max_norm, what):
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"{what}: max_norm must be >= 0, got {max_norm!r}")
    return max_norm


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, *, return_stats=False):
    """torch.nn.utils.clip_grad_norm_ (its signature) -> the total norm, a 0-d float64 tensor on the gradients' device.  On the device:
    L3 + L3s, _hip.grad_norm_launches(n) + ceil(n / 64) launches and no synchronisation.  On the CPU: the same order in numpy.
    Where a gradient holds a NaN or an Inf nothing is scaled (torch would multiply every gradient by a NaN coefficient).
    norm_type: 2 only.  error_if_nonfinite=True reads the statistics back and raises as torch does.
    return_stats=True (this build's): the whole statistics instead - norm, coef, the non-finite count, the per-tensor norms."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"clip_grad_norm_: norm_type={norm_type!r} is not implemented (the 2-norm only)")
    max_norm = _check_max_norm(max_norm, "clip_grad_norm_")
    grads = _grads_of(parameters, "clip_grad_norm_")
    if not grads:
        stats = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    elif grads[0].is_cuda:
        stats = _hip.grad_norm(grads, max_norm)
        _hip.grad_scale_(grads, stats)
    else:
        stats = host_grad_stats(grads, max_norm)
        if float(stats[2]) == 0.0 and float(stats[1]) != 1.0:
            coef = float(stats[1])
            with torch.no_grad():
                for g in grads:
                    g.mul_(coef)
    if error_if_nonfinite:
        host = stats[:3].cpu()                                        # the only path that reads back
        if float(host[2]) > 0 or not math.isfinite(float(host[0])):
            raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                               "clipped. To disable this error and leave the gradients as they are, set `error_if_nonfinite=False`")
    return stats if return_stats else stats[0]


class DeviceAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, max_grad_norm=None):
        if weight_decay != 0:
            raise NotImplementedError("DeviceAdam: weight decay is not implemented (the reference trains without it)")
        if amsgrad:
            raise NotImplementedError("DeviceAdam: amsgrad is not implemented (the reference trains without it)")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("DeviceAdam: lr must be a Python number (the kernel takes it from the host)")
        # the installed Adam's own checks of lr, betas, eps - and its param_group keys, so that each loads the other's state_dict
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)
        self.last_launches = 0
        # an attribute, not a param_group key: state_dict() stays torch.optim.Adam's
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, "DeviceAdam")
        self.last_grad_stats = None                                   # with max_grad_norm: the step's statistics, on the parameters' device

    @staticmethod
    def _refuse(group):
        for key, what in (("weight_decay", "weight decay"), ("amsgrad", "amsgrad"), ("maximize", "maximize"),
                          ("decoupled_weight_decay", "decoupled weight decay")):
            if group.get(key):
                raise NotImplementedError(f"DeviceAdam: {what} is not implemented (param_group {key}={group[key]!r})")

    def grad_norm(self):
        """The last step's global gradient norm as a Python float (reads back: a synchronisation); None before the first clipped step."""
        return None if self.last_grad_stats is None else float(self.last_grad_stats[0])

    def _clip_stats(self):
        """L3 over every parameter of every group that has a gradient -> (stats, launches); refusals before anything is launched"""
        max_norm = _check_max_norm(self.max_grad_norm, "DeviceAdam.max_grad_norm")
        params = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        devices = sorted({str(p.device) for p in params})
        if len(devices) > 1:
            raise NotImplementedError(f"DeviceAdam: max_grad_norm with parameters on {len(devices)} devices ({', '.join(devices)}): the global norm "
                                      "is formed on one device without a host synchronisation")
        for p in params:
            if p.grad.is_sparse:
                raise RuntimeError("DeviceAdam does not support sparse gradients")
            if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                raise NotImplementedError(f"DeviceAdam: float32 parameters only, got {p.dtype}")
        if not params:
            return torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), 0
        if not params[0].is_cuda:
            return host_grad_stats([p.grad for p in params], max_norm), 0
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
        return _hip.grad_norm(grads, max_norm), _hip.grad_norm_launches(len(grads))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.last_launches = 0
        stats = None
        if self.max_grad_norm is not None:
            for group in self.param_groups:
                self._refuse(group)
            stats, self.last_launches = self._clip_stats()
            self.last_grad_stats = stats
            if not stats.is_cuda:                                     # the CPU path: the same decision, taken here
                skip, coef = float(stats[2]) > 0, float(stats[1])
        for group in self.param_groups:
            self._refuse(group)
            lr, betas, eps = float(group["lr"]), tuple(float(b) for b in group["betas"]), float(group["eps"])
            device = {}                                               # device -> ([p], [g], [m], [v], [step])
            for p in group["params"]:
                if p.grad is None:
                    continue                                          # skipped, its step does not advance (as in torch)
                if p.grad.is_sparse:
                    raise RuntimeError("DeviceAdam does not support sparse gradients")
                if p.dtype != torch.float32:
                    raise NotImplementedError(f"DeviceAdam: float32 parameters only, got {p.dtype}")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                t = int(state["step"]) + 1                           # (a CPU tensor or an int: no device read)
                state["step"] = torch.tensor(float(t), dtype=torch.float32)      # (also on a skipped step: see the module's docstring)
                if not p.is_cuda:
                    if stats is None:
                        adam_reference_step_(p, p.grad, state["exp_avg"], state["exp_avg_sq"], t, lr, betas, eps)
                    elif not skip:
                        adam_reference_step_(p, p.grad * coef, state["exp_avg"], state["exp_avg_sq"], t, lr, betas, eps)
                    continue
                if not (p.is_contiguous() and state["exp_avg"].is_contiguous() and state["exp_avg_sq"].is_contiguous()):
                    raise NotImplementedError("DeviceAdam: parameters and their state must be contiguous")
                lists = device.setdefault(p.device, ([], [], [], [], []))
                for lst, item in zip(lists, (p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), state["exp_avg"], state["exp_avg_sq"], t)):
                    lst.append(item)
            for ps, gs, ms, vs, ts in device.values():
                self.last_launches += _hip.adam_step(ps, gs, ms, vs, ts, lr, betas, eps, stats=stats)
                torch.autograd.graph.increment_version(ps)           # the kernel wrote through raw pointers: see the module's docstring
        return loss
