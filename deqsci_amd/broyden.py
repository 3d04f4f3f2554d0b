"""Broyden's method on the device: the reference's quasi-Newton fixed-point solver, backed by the HIP step kernels of csrc/broyden.hip.

    broyden(g, x0, threshold=9, eps=1e-5, ls=False) -> (x, |g(x)|)      solvers/broyd_equilibrium_utils.py:117-181
    broyden_fixed_point(f, x0, threshold=9, eps=1e-5) -> (z, res)       the (f, x0, **kw) shape DEQFixedPoint's solvers have

Same name, arguments, call shape of g and return value as the reference.  The history lives in two planar buffers (bsz, L, N) with
contiguous rows instead of the reference's (bsz,N,1,L) / (bsz,L,N,1) pair; a step is four launches (inner products, their second
stage, the rank-one update, the new direction) and one read-back of the squared norms, the host loop's only synchronisation.
"""
import math

import torch

from . import _hip


def broyden(g, x0, threshold=9, eps=1e-5, ls=False):
    """Solve g(x) = 0 by Broyden's (good) method with a limited history of L = min(threshold, 27) rank-one terms.

    g is called with tensors of shape (bsz, N, 1) and returns that shape, as in the reference.  The objective that stops the
    iteration is the reference's: the 2-norm of g(x) over the WHOLE batch (one number, so the samples of a batch stop together and a
    sample's result depends on what it is batched with); the per-sample norms of the returned iterate are in
    `broyden.last_info["res_per_sample"]`.  Returns (the iterate with the lowest objective, reshaped like x0; that objective).
    The norms are summed in float64 on the device; the low-rank combinations are fp32, as the reference's.
    `broyden.last_info`: nstep, g_calls, lowest_step, trace (the objective per step), res_per_sample.
    ls=True (the reference's Armijo line search, unused by its drivers) is not implemented."""
    if ls:
        raise NotImplementedError("broyden: ls=True (the Armijo line search of the reference's line_search / scalar_search_armijo) is not "
                                  "implemented; the reference's default and every driver of it use ls=False")
    shape = x0.shape
    bsz = shape[0]
    x = _hip.f32c(x0.detach()).reshape(bsz, -1).clone()
    N = x.shape[1]
    L = min(int(threshold), _hip.BROYDEN_MAX_L)
    calls = 0

    def call(xf):
        nonlocal calls
        calls += 1
        return _hip.f32c(g(xf.view(bsz, N, 1))).reshape(bsz, N)

    ws = _hip.BroydenWorkspace(bsz, N, max(L, 1), x.device)

    def norms():
        """per-sample |gx_new|^2 of the last broyden_dots (float64) -> (objective, per-sample norms): the step's one synchronisation"""
        gg = ws.table[:, _hip.BROYDEN_GG].cpu()
        return math.sqrt(float(gg.sum())), [math.sqrt(v) for v in gg.tolist()]

    gx = call(x)
    _hip.broyden_dots(ws, gx, gx, gx, 0)
    objective, per_sample = norms()
    init_objective = objective
    trace = [objective]
    lowest, lowest_x, lowest_step, lowest_per_sample = objective, x.clone(), 0, per_sample
    update = gx.clone()                                  # the step about to be taken (the next dx); rewritten in place by the kernels
    other = torch.add(x, update)                         # the first step has no history: x1 = x0 + g(x0)
    nstep = 0
    while objective >= eps and nstep < threshold:
        x, other = other, x                              # the new iterate; the previous one's buffer receives the next
        gx_new = call(x)
        nstep += 1
        t = min(nstep - 1, L)
        _hip.broyden_dots(ws, update, gx, gx_new, t)
        objective, per_sample = norms()
        trace.append(objective)
        if objective < lowest:
            lowest_x.copy_(x)                            # a device copy, taken when the host sees a new minimum
            lowest, lowest_step, lowest_per_sample = objective, nstep, per_sample
        if objective < eps:
            break
        if objective < 3 * eps and nstep > 30 and max(trace[-30:]) / min(trace[-30:]) < 1.3:
            break                                        # hardly any progress in the last 30 steps
        if objective > init_objective * 1e6:
            break
        if nstep >= threshold:
            break                                        # (the reference forms one more update here and never uses it)
        _hip.broyden_update(ws, update, gx, gx_new, t, (nstep - 1) % L, update, x=x, x_next=other)
        gx = gx_new
    broyden.last_info = {"nstep": nstep, "g_calls": calls, "lowest_step": lowest_step, "trace": trace, "res_per_sample": lowest_per_sample}
    return lowest_x.reshape(shape), lowest


broyden.last_info = None


def broyden_fixed_point(f, x0, threshold=9, eps=1e-5):
    """The fixed point z = f(z) by `broyden` on g = f - id: the (f, x0, **kwargs) -> (z, res) solver DEQFixedPoint takes, e.g.
    DEQFixedPoint(f, broyden_fixed_point, threshold=30, eps=1e-5) (forward and, with a tape, the implicit backward).  res is the
    2-norm of f(z) - z over the whole batch."""
    shape = x0.shape

    def g(xf):
        z = xf.view(shape)
        return (f(z) - z).reshape(shape[0], -1, 1)
    return broyden(g, x0, threshold=threshold, eps=eps)
