"""An independent numpy restatement of csrc/noise.hip for the tests (it does not import deqsci_amd.noise): Philox4x32-10 with python
integers, the normals in float64, and kernel N2's order of operations emulated in fp32 on GIVEN normals."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
# (counter, key, result): the known answers of Philox4x32-10
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((5, 0, 7, 0), (1234, 0), (289107249, 2204080987, 1141931367, 543250339)),          # group 5 of seq 7, seed 1234
)
# (sigma, gain, bits, full_scale): the grid of the sensor model; full_scale None = not used (no quantiser)
GRID = ((5 / 255, 0.0, 0, None), (0.0, 0.01, 0, None), (5 / 255, 0.01, 8, 8.0), (2 / 255, 0.003, 12, 3.5), (0.0, 0.0, 0, None))
NORMAL_MAX = math.sqrt(-2.0 * math.log(2.0 ** -24))                                    # u >= 2^-24: |n| <= 5.768...


def philox_scalar(counter, key):
    """One block, python integers."""
    c0, c1, c2, c3 = (int(v) & MASK32 for v in counter)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, k0, k1):
    """Arrays of uint64 holding 32-bit words (c2, c3, k0, k1 may be scalars) -> four arrays of uint32."""
    u = np.uint64
    c0, c1 = np.asarray(c0, u), np.asarray(c1, u)
    c2, c3 = np.broadcast_to(np.asarray(c2, u), c0.shape), np.broadcast_to(np.asarray(c3, u), c0.shape)
    k0, k1 = u(k0), u(k1)
    for _ in range(10):
        p0, p1 = u(M0) * c0, u(M1) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ k0, p1 & u(MASK32), (p0 >> u(32)) ^ c3 ^ k1, p0 & u(MASK32)
        k0, k1 = (k0 + u(W0)) & u(MASK32), (k1 + u(W1)) & u(MASK32)
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def words(seqs, n, seed):
    """(bsz, ceil(n / 4), 4) uint32: what kernel N0 writes for the sequence numbers `seqs` (python integers) and the 64-bit seed."""
    groups = -(-int(n) // 4)
    g = np.arange(groups, dtype=np.uint64)
    out = np.empty((len(seqs), groups, 4), np.uint32)
    for k, seq in enumerate(seqs):
        seq = int(seq)
        w = philox(g & np.uint64(MASK32), g >> np.uint64(32), seq & MASK32, seq >> 32, int(seed) & MASK32, (int(seed) >> 32) & MASK32)
        for i in range(4):
            out[k, :, i] = w[i]
    return out


def _sincospi(t):
    """sin(pi t), cos(pi t) in float64 for t in (0, 2), reduced to |f| <= 1/4 exactly before pi enters"""
    q = np.floor(2.0 * t + 0.5)
    f = np.pi * (t - q / 2.0)
    s0, c0 = np.sin(f), np.cos(f)
    q = q.astype(np.int64) % 4
    s = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
    c = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
    return s, c


def normals64(w, n):
    """(bsz, groups, 4) uint32 words -> (bsz, n) float64 normals, the formulas of include/deqsci_hip.h in float64."""
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert u.min() > 0.0 and u.max() < 1.0
    out = np.empty(w.shape, np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        s, c = _sincospi(2.0 * u[..., a + 1])
        out[..., a], out[..., a + 1] = r * c, r * s
    return out.reshape(w.shape[0], -1)[:, :int(n)]


def sensor_f32(y, nrm, sigma, gain, bits, full_scale):
    """Kernel N2 on the normals `nrm`: fp32, every operation rounded on its own, element by element in the stated order."""
    f = np.float32
    y, nrm = np.asarray(y, f), np.asarray(nrm, f)
    assert y.shape == nrm.shape
    out = y.copy()
    ok = np.isfinite(y)                                                  # NaN and +-Inf pass through untouched
    yy, nn = y[ok], nrm[ok]
    p = np.where(yy > 0, yy, f(0))
    v = f(gain) * p
    v = v + f(sigma) * f(sigma)
    d = np.sqrt(v)
    t = d * nn
    o = yy + t
    assert o.dtype == f and v.dtype == f
    if bits > 0:
        L = f((1 << bits) - 1)
        c = o / f(full_scale)
        c = np.where(c > 0, c, f(0))
        c = np.where(c < 1, c, f(1))
        q = np.rint(c * L)
        o = (q / L) * f(full_scale)
        assert o.dtype == f
    out[ok] = o
    return out


def ramp(bsz, n):
    """The sensor tests' input: a ramp over [-0.5, 9] (negative values, mid-range, saturation) holding a NaN, a +Inf and a -Inf."""
    y = np.linspace(-0.5, 9.0, bsz * n, dtype=np.float64).astype(np.float32).reshape(bsz, n)
    flat = y.reshape(-1)
    if flat.size >= 8:
        flat[flat.size // 7], flat[flat.size // 3], flat[flat.size // 2] = np.nan, np.inf, -np.inf
    return y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def moments(x):
    """The statistics of the issue, each in units of its own standard error under N(0,1): mean, variance, third and fourth moment, and
    the autocorrelations at lags 1 and 4."""
    x = np.asarray(x, np.float64).reshape(-1)
    N = x.size
    m = x.mean()
    z = x - m
    var = (z * z).mean()
    out = {"mean": abs(m) * math.sqrt(N), "var": abs(var - 1.0) * math.sqrt(N / 2.0), "m3": abs((z ** 3).mean()) * math.sqrt(N / 6.0),
           "m4": abs((z ** 4).mean() - 3.0) * math.sqrt(N / 24.0)}
    for lag in (1, 4):
        out["lag%d" % lag] = abs((z[:-lag] * z[lag:]).mean() / var) * math.sqrt(N)
    return out


def correlation(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return abs((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean())) * math.sqrt(a.size)
