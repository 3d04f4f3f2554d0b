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
"""
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


class DeviceAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
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

    @staticmethod
    def _refuse(group):
        for key, what in (("weight_decay", "weight decay"), ("amsgrad", "amsgrad"), ("maximize", "maximize"),
                          ("decoupled_weight_decay", "decoupled weight decay")):
            if group.get(key):
                raise NotImplementedError(f"DeviceAdam: {what} is not implemented (param_group {key}={group[key]!r})")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.last_launches = 0
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
                state["step"] = torch.tensor(float(t), dtype=torch.float32)
                if not p.is_cuda:
                    adam_reference_step_(p, p.grad, state["exp_avg"], state["exp_avg_sq"], t, lr, betas, eps)
                    continue
                if not (p.is_contiguous() and state["exp_avg"].is_contiguous() and state["exp_avg_sq"].is_contiguous()):
                    raise NotImplementedError("DeviceAdam: parameters and their state must be contiguous")
                lists = device.setdefault(p.device, ([], [], [], [], []))
                for lst, item in zip(lists, (p, p.grad if p.grad.is_contiguous() else p.grad.contiguous(), state["exp_avg"], state["exp_avg_sq"], t)):
                    lst.append(item)
            for ps, gs, ms, vs, ts in device.values():
                self.last_launches += _hip.adam_step(ps, gs, ms, vs, ts, lr, betas, eps)
                torch.autograd.graph.increment_version(ps)           # the kernel wrote through raw pointers: see the module's docstring
        return loss
