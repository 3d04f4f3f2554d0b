"""Float64 restatements of csrc/bn_train.hip (T1 .. T4) in the order of operations include/deqsci_hip.h states, with the error bounds the
tests hold the kernels to - counted from that text, never from what the kernels give.  numpy, CPU; shared by tests/test_bn_train_gpu.py.

u = 2^-53 is float64's unit roundoff, v = 2^-24 fp32's.  A float64 sum of P terms is within (P - 1) u of sum |terms| of the exact one.
"""
import functools

import numpy as np

U, V = 2.0 ** -53, 2.0 ** -24
CHUNK, MAX_WG = 128, 1024                 # DEQSCI_BN_TRAIN_CHUNK, DEQSCI_BN_TRAIN_MAX_WG
TINY = 2.0 ** -149                        # the smallest fp32 subnormal: a result rounded there is off by at most this
EPS, MOMENTUM = 1e-5, 0.1                 # torch's defaults, FFDNet's and the DnCNN's


def split(P):
    """(chunk, workgroups) of the kernels' first stage for P pixels, as the header states it."""
    chunk = CHUNK
    if -(-P // chunk) > MAX_WG:
        chunk = -(-(-(-P // MAX_WG)) // 16) * 16
    return chunk, -(-P // chunk)


# shapes (n, H, W): P = 2; ragged, one workgroup, 105 pixels; the smallest kind with more than one workgroup AND a thread that owns more than
# one pixel - 135 pixels = one full chunk of 128 (16 pixels per step: 8 per thread) and a second workgroup with 7; 49 workgroups, the last
# partly filled; and one past MAX_WG * CHUNK pixels, where the chunk grows (144 pixels, 916 workgroups)
SHAPES = ((1, 1, 2), (3, 5, 7), (3, 5, 9), (3, 40, 52))
BIG = (1, 363, 363)
assert split(2) == (128, 1) and split(105) == (128, 1) and split(135) == (128, 2) and split(3 * 40 * 52) == (128, 49)
assert split(363 * 363) == (144, 916) and 363 * 363 > CHUNK * MAX_WG
CASES = ("signed", "constant", "offset")


@functools.lru_cache(maxsize=None)
def data(shape, case, seed=0):
    """(c, gy, gamma, beta, running_mean, running_var): c, gy (P, 64) fp32.  signed: N(0,1) scaled per channel over four decades;
    constant: channel 7 holds one value (var = 0) and channel 9 is all zeros; offset: c = 1000 + 1e-2 N(0,1), where E[c^2] - mean^2 has no
    digit left.  gamma has an exact zero (3) and negative entries (7, 20, 41); gy is zero on a third of its entries, as behind a ReLU."""
    P = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(1000 * seed + P)
    c = rng.standard_normal((P, 64)).astype(np.float32)
    if case == "offset":
        c = (1000.0 + 1e-2 * c).astype(np.float32)
    else:
        c *= (10.0 ** rng.uniform(-2, 2, 64)).astype(np.float32)
    if case == "constant":
        c[:, 7] = np.float32(0.75)
        c[:, 9] = 0.0
    gy = (rng.standard_normal((P, 64)) * (rng.random((P, 64)) > 1 / 3)).astype(np.float32)
    gamma = (0.5 + rng.random(64)).astype(np.float32)
    gamma[3] = 0.0
    gamma[[7, 20, 41]] *= -1.0
    beta = (0.2 * rng.standard_normal(64)).astype(np.float32)
    rm, rv = (0.3 * rng.standard_normal(64)).astype(np.float32), (0.5 + rng.random(64)).astype(np.float32)
    for a in (c, gy, gamma, beta, rm, rv):
        a.setflags(write=False)
    return c, gy, gamma, beta, rm, rv


@functools.lru_cache(maxsize=None)
def stats(shape, case):
    """T1's reference: (mean, var, mean |c|) per channel.  Extended precision where numpy has it (x86: 64-bit mantissa), pairwise float64
    sums otherwise and for BIG - either way far inside the bound the kernel is held to."""
    c = data(shape, case)[0]
    wide = np.longdouble if c.shape[0] <= 1 << 14 else np.float64
    x = c.astype(wide)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, np.abs(x).mean(0)


def stats_bounds(P, var, mean_abs):
    """|mean - ref| and |var - ref| allowed: P 2^-52 relative to mean |c| and to the variance ITSELF - the worst case of a float64 sum of P
    terms (2 (P - 1) u would do for the sums alone; the centring and the squares of the second pass are covered by the rest)."""
    return P * 2.0 ** -52 * mean_abs, P * 2.0 ** -52 * var


def running(rm, rv, mean, var, P, momentum=MOMENTUM):
    """torch's update in float64 (the header's expression); the kernel's fp32 result is within one fp32 rounding of it."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    return (1.0 - momentum) * rm.astype(np.float64) + momentum * mean, (1.0 - momentum) * rv.astype(np.float64) + momentum * (var * P / (P - 1))


def one_rounding(ref):
    """|fp32 result - float64 ref| allowed when the result is ref rounded once (and ref itself carries a few u)."""
    return V * np.abs(ref) * (1 + 2.0 ** -20) + TINY


def apply(c, record, gamma, beta, eps=EPS, relu=True):
    """T2 -> (y float64, bound): inv = 1 / sqrt(var + eps), a = gamma inv, y = a (c - mean) + beta, ReLU.  The kernel rounds 6 times in
    float64 on the way to a d (add, sqrt, divide, gamma inv, c - mean, the fma) - at most 8 u (|a d| + |beta|) with this restatement's own
    rounding - and once to fp32."""
    mean, var = record[:64], record[64:]
    a = gamma.astype(np.float64) * (1.0 / np.sqrt(var + eps))
    ad = a * (c.astype(np.float64) - mean)
    y = ad + beta.astype(np.float64)
    bound = V * np.abs(y) + 8 * U * (np.abs(ad) + np.abs(beta.astype(np.float64))) + TINY
    return (np.maximum(y, 0.0) if relu else y), bound


def mask_words(y):
    """deqsci_relu_mask_pack_f32's words of a (P, 64) activation: bit ch = (y > 0)."""
    bits = (y > 0).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=1).view(np.int64)


def grad_stats(gy, c, record, eps=EPS):
    """T3 -> (dbeta, dgamma, bound_dbeta, bound_dgamma) in float64 (extended sums where numpy has them).  P - 1 additions per sum; dgamma
    has 8 more roundings per term or in all (c - mean, the product, add / sqrt / divide of inv, the scaling, this restatement's own)."""
    P = c.shape[0]
    wide = np.longdouble if P <= 1 << 14 else np.float64
    mean, var = record[:64].astype(wide), record[64:].astype(wide)
    g, d = gy.astype(wide), c.astype(wide) - mean
    inv = 1.0 / np.sqrt(var + eps)
    dbeta, dgamma = g.sum(0), inv * (g * d).sum(0)
    return (dbeta.astype(np.float64), dgamma.astype(np.float64), np.asarray((P + 1) * U * np.abs(g).sum(0), np.float64),
            np.asarray((P + 8) * U * inv * np.abs(g * d).sum(0), np.float64))


def grad_apply(gy, c, record, grad_record, gamma, eps=EPS):
    """T4 -> (dc float64, bound): k1 = dbeta / P, k2 = dgamma inv / P, a = gamma inv, dc = a ((gy - k1) - (c - mean) k2).  Each of the three
    terms reaches the result through at most 14 float64 roundings (inv 3, a 1, k2 2, c - mean 1, the product 1, two subtractions, the
    scaling, and this restatement's own) - 16 u |a| (|gy| + |k1| + |d k2|) - and the result is rounded once to fp32."""
    P = c.shape[0]
    mean, var = record[:64], record[64:]
    inv = 1.0 / np.sqrt(var + eps)
    a, k1, k2 = gamma.astype(np.float64) * inv, grad_record[:64] / P, grad_record[64:] * inv / P
    g, d = gy.astype(np.float64), c.astype(np.float64) - mean
    dc = a * ((g - k1) - d * k2)
    bound = V * np.abs(dc) + 16 * U * np.abs(a) * (np.abs(g) + np.abs(k1) + np.abs(d * k2)) + TINY
    return dc, bound
