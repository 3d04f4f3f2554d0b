"""The summation order of csrc/rows.hpp, restated in numpy for float64 terms t[s, e]: what the device's planar-row sums (sqerr_rows,
power_step, the Broyden and epsilon2 tables) must equal BIT FOR BIT.  A helper module, not a test.

Stage 1, chunk c (CHUNK = 256 * 4 * P elements), thread tid: acc = 0.0; for q = 0..P-1, for k = 0..3: acc += t[c*CHUNK + (q*256 + tid)*4 + k]
(nothing past N: the zeros padded here add +0.0 to an accumulator that started at +0.0 and so is never -0.0 - the same bits); then per
wave six butterfly steps v[l] = v[l] + v[l ^ o], o = 32..1, on all 64 lanes at once; then ((w0 + w1) + w2) + w3 over the four waves.
Stage 2 over a sample's chunk sums: by a workgroup (thread i adds chunks i, i + 256, ... in order from 0.0, then the same block sum), or
by one wave (lane l adds chunks l, l + 64, ..., then the butterfly)."""
import numpy as np

TB, WAVE = 256, 64


def chunk(P):
    return TB * 4 * P


def _butterfly(v):
    """v[..., 64] per lane -> the sum every lane ends with"""
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _block_sum(v):
    """v[..., 256] per thread -> the workgroup's sum"""
    w = _butterfly(v.reshape(v.shape[:-1] + (TB // WAVE, WAVE)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _strided(p, lanes):
    """p[s, n] -> acc[s, lanes]: lane i adds p[i], p[i + lanes], ... in order from 0.0"""
    trips = -(-p.shape[1] // lanes)
    pad = np.zeros((p.shape[0], trips * lanes))
    pad[:, :p.shape[1]] = p
    acc = np.zeros((p.shape[0], lanes))
    for r in range(trips):
        acc = acc + pad[:, r * lanes:(r + 1) * lanes]
    return acc


def chunk_sums(t, P):
    """Stage 1: terms t[s, N] float64 -> the chunk partials [s, ceil(N / CHUNK)]"""
    assert t.dtype == np.float64 and t.ndim == 2
    n = -(-t.shape[1] // chunk(P))
    pad = np.zeros((t.shape[0], n * chunk(P)))
    pad[:, :t.shape[1]] = t
    g = pad.reshape(t.shape[0], n, P, TB, 4)
    acc = np.zeros((t.shape[0], n, TB))
    for q in range(P):
        for k in range(4):
            acc = acc + g[:, :, q, :, k]
    return _block_sum(acc)


def fold_workgroup(p):
    return _block_sum(_strided(p, TB))


def fold_wave(p):
    return _butterfly(_strided(p, WAVE))


def sum_workgroup(t, P):
    """the Broyden and epsilon2 tables, power_step"""
    return fold_workgroup(chunk_sums(t, P))


def sum_wave(t, P):
    """sqerr_rows"""
    return fold_wave(chunk_sums(t, P))
