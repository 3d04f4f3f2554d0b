"""Restatements for the training tests (csrc/train.hip, deqsci_amd/optim.py).  A helper module, not a test.

  adam_f32_step   L2's order of operations in numpy float32: what the device must equal BIT FOR BIT
  adam_f64_step   the same step in float64, with exact (double) constants
  adam_bound_step the running bound on |fp32 - float64| of that order, rounding by rounding
  mse_stats       L1: the gradient in fp32 and the statistics in csrc/rows.hpp's order (rows_order.sum_workgroup, P = 4): BIT FOR BIT
  mse_stats_f64   the statistics of the same fp32 terms summed exactly enough (math.fsum)

The order (the reference's torch-1.9 F.adam), every operation rounded separately:
    m = m * b1 + g * (1 - b1);  v = v * b2 + (g * g) * (1 - b2);  den = sqrt(v) / bc2s + eps;  p = p - step_size * (m / den)
with b1, 1 - b1, b2, 1 - b2, bc2s = sqrt(1 - b2^t), step_size = lr / (1 - b1^t), eps computed in double and rounded to fp32 once.
"""
import math

import numpy as np

import rows_order

P = 4                                   # csrc/train.hip: PER_THREAD
CHUNK = rows_order.chunk(P)             # 4096 = DEQSCI_TRAIN_CHUNK
ADAM_MAX_TENSORS = 64                   # DEQSCI_ADAM_MAX_TENSORS
U = 2.0 ** -24                          # fp32's unit roundoff

# The roundings of one step and element, stage by stage (a constant rounded to fp32 counts as one):
#   m:   b1, m * b1, 1 - b1, g * (1 - b1), the sum                      5, each at most U x S_m,  S_m = b1 |m| + (1 - b1) |g|
#   v:   b2, v * b2, g * g, 1 - b2, (g * g) * (1 - b2), the sum         6, each at most U x S_v,  S_v = b2 v + (1 - b2) g^2
#   den: sqrt, bc2s, the division, eps, the sum                         5, each at most U x den
#   q = m / den                                                         1
#   d = step_size * q: step_size, the product                           2
#   p - d                                                               1
ADAM_ROUNDINGS = {"m": 5, "v": 6, "den": 5, "q": 1, "d": 2, "p": 1}
assert sum(ADAM_ROUNDINGS.values()) == 20
SECOND_ORDER = 1.01                     # (1 + U)^k - 1 <= 1.01 k U for the k <= 100 roundings of five steps: the bound below is first order


def adam_scalars(t, lr, betas):
    b1, b2 = betas
    return math.sqrt(1.0 - b2 ** t), lr / (1.0 - b1 ** t)


def adam_f32_step(p, g, m, v, t, lr, betas, eps):
    """-> (p, m, v) after step t >= 1, float32 arrays in, float32 arrays out (the inputs are not modified)."""
    f = np.float32
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    b1, b2 = betas
    bc2s, step_size = adam_scalars(t, lr, betas)
    with np.errstate(all="ignore"):
        m = m * f(b1) + g * f(1.0 - b1)
        v = v * f(b2) + (g * g) * f(1.0 - b2)
        den = np.sqrt(v) / f(bc2s) + f(eps)
        p = p - f(step_size) * (m / den)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adam_f64_step(p, g, m, v, t, lr, betas, eps):
    b1, b2 = betas
    bc2s, step_size = adam_scalars(t, lr, betas)
    g = g.astype(np.float64)
    m = m * b1 + g * (1.0 - b1)
    v = v * b2 + (g * g) * (1.0 - b2)
    den = np.sqrt(v) / bc2s + eps
    return p - step_size * (m / den), m, v


def adam_bound_step(e, before, after, g, t, lr, betas, eps):
    """The bound on |fp32 - float64| after step t from the bound e = (e_p, e_m, e_v) before it, first order in U, from the float64 run's
    values `before` = (p, m, v) and `after` = (p, m, v): every rounding of ADAM_ROUNDINGS at most U times the magnitude its stage sums."""
    b1, b2 = betas
    bc2s, step_size = adam_scalars(t, lr, betas)
    R = ADAM_ROUNDINGS
    g = np.abs(g.astype(np.float64))
    (_, m0, v0), (p1, m1, v1) = before, after
    e_p, e_m, e_v = e
    e_m = b1 * e_m + R["m"] * U * (b1 * np.abs(m0) + (1.0 - b1) * g)
    e_v = b2 * e_v + R["v"] * U * (b2 * v0 + (1.0 - b2) * g * g)
    root = np.sqrt(v1)
    e_root = np.divide(e_v, 2.0 * root, out=np.zeros_like(root), where=root > 0)           # (v = 0 only where every g was 0: exact)
    den = root / bc2s + eps
    e_den = e_root / bc2s + R["den"] * U * den
    q = m1 / den
    e_q = e_m / den + np.abs(m1) * e_den / den ** 2 + R["q"] * U * np.abs(q)
    e_d = step_size * e_q + R["d"] * U * np.abs(step_size * q)
    e_p = e_p + e_d + R["p"] * U * np.abs(p1)
    return e_p, e_m, e_v


def clamp01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)        # NaN stays NaN, as the kernel's


def mse_terms(rec, gt):
    """-> (grad fp32, the fp32 squares d * d and dc * dc, the non-finite flags) of flat float32 arrays."""
    assert rec.dtype == gt.dtype == np.float32 and rec.ndim == gt.ndim == 1
    with np.errstate(all="ignore"):
        d = rec - gt
        grad = d * np.float32(2.0 / rec.size)
        dc = clamp01(rec) - gt
        return grad, d * d, dc * dc, ~np.isfinite(d)


def mse_stats(rec, gt):
    """-> (grad, stats[3] float64): what deqsci_mse_stats_grad_f32 must give bit for bit (stage 2 by one workgroup: sum_workgroup)."""
    grad, sq, sqc, bad = mse_terms(rec, gt)
    with np.errstate(all="ignore"):
        stats = np.array([rows_order.sum_workgroup(t.astype(np.float64)[None], P)[0] for t in (sq, sqc, bad)])
    return grad, stats


def mse_stats_f64(rec, gt):
    _, sq, sqc, bad = mse_terms(rec, gt)
    return np.array([math.fsum(sq.astype(np.float64)), math.fsum(sqc.astype(np.float64)), float(bad.sum())])
