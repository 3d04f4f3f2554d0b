"""The vector epsilon-algorithm on the device: the reference's history-free accelerator (Aitken's delta-squared extrapolation of
x, f(x), f(f(x))), backed by the HIP step kernels of csrc/epsilon2.hip.

    epsilon2(f, x0, max_iter=50, tol=1e-2, lam=1e-4) -> (x, residual)      solvers/new_equilibrium_utils_yaping.py:194-211

Same name, arguments and return value as the reference, and the (f, x0, **kw) -> (z, res) shape DEQFixedPoint's solvers have.  Its state
is three rows - x, f(x), f(f(x)) - and two iterate buffers that take turns; an iteration is two f-calls, four launches (the three squared
norms, their second stage, the extrapolated point with its two norms, their second stage) and one read-back of the float64 table
(bsz, 5), the host loop's only synchronisation.
"""
import math

import torch

from . import _hip


def _host_step(x, f_x, f_fx, lam):
    """One iteration's arithmetic in torch for tensors that are not on a HIP device: fp32 differences, float64 sums, the fp32 update in
    the reference's operation order -> (x_new, the (bsz, 5) table as nested lists)."""
    dx = f_x - x
    df = f_fx - f_x
    d2 = df - dx
    sq = lambda t: t.double().square().sum(dim=1, keepdim=True)
    sa, sb, sc = sq(dx), sq(df), sq(d2)
    x_new = f_x + (df * sa.float() - dx * sb.float()) / (sc.float() + lam)
    return x_new, torch.cat([sa, sb, sc, sq(x_new - x), sq(x_new)], dim=1).tolist()


def epsilon2(f, x0, max_iter=50, tol=1e-2, lam=1e-4):
    """The fixed point of f by the vector epsilon-algorithm.  Per iteration, with f_x = f(x), f_fx = f(f_x), dx = f_x - x, df = f_fx - f_x,
    d2 = df - dx (fp32):  x <- f_x + (df |dx|^2 - dx |df|^2) / (|d2|^2 + lam),  the squared norms PER SAMPLE (over every dimension but
    the first; summed in float64, rounded to fp32), the update elementwise in fp32 in this operation order.  The iteration stops when
    |x_new - x| / |x_new| over the WHOLE batch (one number, as in the reference: the samples of a batch stop together) falls below tol.

    f is called with tensors shaped like x0 (any shape of at least two dimensions; a sample is everything behind the first).  Returns
    (the extrapolated point - not an output of f - shaped like x0, fp32; the last residual).  As in the reference: max_iter <= 0 raises
    UnboundLocalError, |x_new| = 0 raises ZeroDivisionError, and a residual that is not finite does not stop the loop.
    `epsilon2.last_info`: iterations, f_calls, trace (the residual per iteration), res_per_sample (|x_new - x| / |x_new| of each sample
    at the last iteration).  Tensors that are not on a HIP device take the same steps written in torch."""
    if x0.dim() < 2:
        raise ValueError(f"epsilon2: x0 must have a batch dimension and at least one more, got shape {tuple(x0.shape)}")
    shape = x0.shape
    bsz = shape[0]
    x = _hip.f32c(x0.detach()).reshape(bsz, -1)
    N = x.shape[1]
    device = x.is_cuda
    calls = 0

    def call(v):
        nonlocal calls
        calls += 1
        return _hip.f32c(f(v.view(shape)).detach()).reshape(bsz, N)

    if device and max_iter > 0:
        ws = _hip.Epsilon2Workspace(bsz, N, x.device)
        bufs = [torch.empty_like(x), torch.empty_like(x)]
    trace, rows = [], None
    for k in range(max_iter):
        f_x = call(x)
        f_fx = call(f_x)
        if device:
            x_new = bufs[k % 2]                          # x is x0 or the other buffer
            _hip.epsilon2_norms(ws, x, f_x, f_fx)
            _hip.epsilon2_update(ws, x, f_x, f_fx, x_new, lam)
            rows = ws.table.tolist()                     # the iteration's one read-back
        else:
            x_new, rows = _host_step(x, f_x, f_fx, lam)
        step = math.sqrt(sum(r[_hip.EPSILON2_STEP] for r in rows))
        size = math.sqrt(sum(r[_hip.EPSILON2_NEW] for r in rows))
        residual = step / size                           # ZeroDivisionError at |x_new| = 0, as the reference's .item() / .item()
        trace.append(residual)
        x = x_new
        if residual < tol:
            break
    if rows is None:
        raise UnboundLocalError("local variable 'residual' referenced before assignment")
    per_sample = [math.sqrt(r[_hip.EPSILON2_STEP]) / math.sqrt(r[_hip.EPSILON2_NEW]) if r[_hip.EPSILON2_NEW] > 0 else float("nan") for r in rows]
    epsilon2.last_info = {"iterations": len(trace), "f_calls": calls, "trace": trace, "res_per_sample": per_sample}
    return x.view(shape), residual


epsilon2.last_info = None
