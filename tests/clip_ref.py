"""The order of csrc/train.hip's L3 (the global gradient norm), restated on tests/rows_order.py: what deqsci_grad_norm_f32 and the CPU paths
of deqsci_amd.optim must equal BIT FOR BIT.  A helper module, not a test.

  1. per tensor, every element widened to float64 and squared (exact), each chunk of 4096 summed in rows.hpp's stage-1 order with P = 4;
  2. the tensor's chunk partials in the stage-2 order of a workgroup - together rows_order.sum_workgroup;
  3. the tensors' sums added one after the other in list order, in float64.
  stats[0] = sqrt(sum); stats[1] = fp32(c >= 1 ? 1 : c), c = max_norm / (stats[0] + 1e-6) in float64; stats[2] = the non-finite elements;
  stats[3 + i] = sqrt(tensor i's sum).
"""
import math

import numpy as np

import rows_order
import train_ref as tr

P = tr.P


def tensor_sums(grads):
    """-> (the float64 sum of squares per tensor in the restated order, the non-finite count per tensor)"""
    sums, bad = [], []
    with np.errstate(all="ignore"):
        for g in grads:
            assert g.dtype == np.float32
            a = g.ravel().astype(np.float64)
            sums.append(float(rows_order.sum_workgroup((a * a)[None], P)[0]))
            bad.append(float(rows_order.sum_workgroup((~np.isfinite(a)).astype(np.float64)[None], P)[0]))
    return sums, bad


def coef_of(norm, max_norm):
    """fp32(min(1, max_norm / (norm + 1e-6))), the division in float64, ONE rounding to fp32 -> that fp32's value as a Python float"""
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
        return float(np.float32(1.0 if c >= 1.0 else c))


def grad_stats(grads, max_norm):
    """-> stats (3 + n,) float64 of a list of float32 arrays"""
    sums, bad = tensor_sums(grads)
    total, count = 0.0, 0.0
    for s, b in zip(sums, bad):
        total = total + s
        count = count + b
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(total)))
        return np.array([norm, coef_of(norm, max_norm), count] + [float(np.sqrt(np.float64(s))) for s in sums], dtype=np.float64)


def exact_sum_of_squares(grads):
    """math.fsum of the exact float64 squares"""
    return math.fsum(float(x) * float(x) for g in grads for x in g.ravel().astype(np.float64))


def clipped(grads, coef):
    """g * coef, one fp32 rounding per element"""
    return [g * np.float32(coef) for g in grads]
