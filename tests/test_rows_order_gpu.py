"""GPU: the float64 sums over planar rows (csrc/rows.hpp) against their order restated in numpy (tests/rows_order.py), BIT FOR BIT: the
squared error, the power step, the epsilon2 table and the Broyden table.  The terms are formed in numpy exactly as the kernels form them
(fp32 differences and squares where the kernel rounds to fp32, exact float64 products of converted floats elsewhere), so nothing but the
order of the additions is left to differ - and a later edit that changes that order fails here, whatever its accuracy.

Sizes: 1 and 3 (one ragged group), a chunk less and plus one element (the seam between two workgroups), two chunks and three (a strided
trip of the first stage's grid is not needed: the grid covers 65536 chunks), and 257 chunks + 5 once per family, where the second
stage's workgroup takes a second trip (for the squared error's wave, 65 chunks do that and 257 take five).  One case per family reads one
row 4 bytes past a 16-byte boundary: the element-by-element path."""
import numpy as np
import pytest
import torch

import rows_order as ro

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip

DEV = "cuda"
F64 = np.float64
SIZES = ["1", "3", "chunk-1", "chunk+1", "2chunk+3"]


def _n(kind, P):
    c = ro.chunk(P)
    return {"1": 1, "3": 3, "chunk-1": c - 1, "chunk+1": c + 1, "2chunk+3": 2 * c + 3, "257chunk+5": 257 * c + 5}[kind]


def _dev(a, offset=0):
    """numpy fp32 array -> a device tensor `offset` floats past a 16-byte boundary"""
    buf = torch.empty(a.size + 4, device=DEV, dtype=torch.float32)
    t = buf[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * offset
    return t


def _randn(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def _cases(P):
    """(bsz, N, offset of one input row) of a family whose chunks hold 1024 P elements"""
    return ([(bsz, _n(k, P), 0) for bsz in (1, 3) for k in SIZES] + [(2, _n("257chunk+5", P), 0), (3, _n("2chunk+3", P) + 1, 1)])


def _ids(cases):
    return [f"bsz{b}-N{n}-off{o}" for b, n, o in cases]


# ----------------------------------------------------------------------------- sqerr_rows (csrc/trace.hip): P = 4, the wave's second stage
def _sqerr_terms(x, gt, clamp):
    d = (np.clip(x, np.float32(0), np.float32(1)) if clamp else x) - gt
    sq = d * d
    assert sq.dtype == np.float32
    return sq.astype(F64)


@pytest.mark.parametrize("bsz,N,off", _cases(4), ids=_ids(_cases(4)))
def test_sqerr_rows_sums_in_the_stated_order(bsz, N, off):
    assert _hip.load().deqsci_sqerr_workspace_bytes(1, ro.chunk(4) + 1) == 16                  # the chunk this file assumes
    x = _randn(N + bsz, bsz, N) * np.float32(0.8) + np.float32(0.5)                            # values outside [0,1] on both sides
    gt = np.random.RandomState(N).rand(bsz, N).astype(np.float32)
    dx, dgt = _dev(x, off), _dev(gt)
    hist = torch.zeros(bsz, 3, N, device=DEV)
    hist[:, 1] = dx
    for clamp in (True, False):
        want = ro.sum_wave(_sqerr_terms(x, gt, clamp), 4)
        assert np.array_equal(_hip.sqerr_rows(dx, dgt, clamp_x=clamp).cpu().numpy(), want), clamp
        assert np.array_equal(_hip.sqerr_rows(hist[:, 1], dgt, clamp_x=clamp).cpu().numpy(), want), clamp     # a slot of a (bsz, 3, N) history


# ----------------------------------------------------------------------------- power_step (csrc/jacobian.hip J2): P = 4, the workgroup's
@pytest.mark.parametrize("bsz,N,off", _cases(4), ids=_ids(_cases(4)))
def test_power_step_sums_in_the_stated_order(bsz, N, off):
    assert _hip.load().deqsci_power_workspace_bytes(1, ro.chunk(4) + 1) == 32
    w, v = _randn(N + 1, bsz, N), _randn(N + 2, bsz, N)
    dw, dv = _dev(w, off), _dev(v)
    w64, v64 = w.astype(F64), v.astype(F64)
    want_a, want_b = ro.sum_workgroup(w64 * w64, 4), ro.sum_workgroup(v64 * w64, 4)
    for prev in (dv, None):
        row = torch.zeros(bsz, 2, dtype=torch.float64, device=DEV)
        out = _hip.power_step(dw, prev, torch.empty_like(dw), row)
        tab = row.cpu().numpy()
        assert np.array_equal(tab[:, 0], want_a)
        assert np.array_equal(tab[:, 1], want_b) if prev is not None else np.isnan(tab[:, 1]).all()
        want_v = (w64 * (1.0 / np.sqrt(tab[:, 0]))[:, None]).astype(np.float32)                # the device's own a: one float64 product, one rounding
        assert np.array_equal(out.cpu().numpy(), want_v)


# ----------------------------------------------------------------------------- epsilon2 (csrc/epsilon2.hip): P = 2, the workgroup's
@pytest.mark.parametrize("bsz,N,off", _cases(2), ids=_ids(_cases(2)))
def test_epsilon2_table_sums_in_the_stated_order(bsz, N, off):
    assert _hip.epsilon2_chunk() == ro.chunk(2)
    x = _randn(N + 3, bsz, N)
    fx = (x + np.float32(0.3) * _randn(N + 4, bsz, N)).astype(np.float32)
    ffx = (fx + np.float32(0.2) * _randn(N + 5, bsz, N)).astype(np.float32)
    dx_, df_ = fx - x, ffx - fx
    d2_ = df_ - dx_
    assert d2_.dtype == np.float32
    ws = _hip.Epsilon2Workspace(bsz, N, DEV)
    rows = (_dev(x), _dev(fx, off), _dev(ffx))
    xn = torch.empty(bsz, N, device=DEV)
    _hip.epsilon2_norms(ws, *rows)
    _hip.epsilon2_update(ws, *rows, xn, 1e-4)
    tab, xn = ws.table.cpu().numpy(), xn.cpu().numpy()
    step = xn - x                                                                              # fp32, from the device's own x_new
    assert step.dtype == np.float32
    for col, v in enumerate((dx_, df_, d2_, step, xn)):
        assert np.array_equal(tab[:, col], ro.sum_workgroup(v.astype(F64) ** 2, 2)), col


# ----------------------------------------------------------------------------- Broyden (csrc/broyden.hip): P = 2, the workgroup's
def _broyden_cases():
    c = ro.chunk(2)
    small = [(bsz, _n(k, 2), t, 0) for bsz in (1, 3) for k in SIZES for t in (0, 1, 27)]
    return small + [(2, 257 * c + 5, 1, 0), (3, 2 * c + 4, 27, 1)]


@pytest.mark.parametrize("bsz,N,t,off", _broyden_cases(), ids=[f"bsz{b}-N{n}-t{t}-off{o}" for b, n, t, o in _broyden_cases()])
def test_broyden_table_sums_in_the_stated_order(bsz, N, t, off):
    assert _hip.broyden_chunk() == ro.chunk(2)
    A, B, C, GG, D, CN = _hip.BROYDEN_A, _hip.BROYDEN_B, _hip.BROYDEN_C, _hip.BROYDEN_GG, _hip.BROYDEN_D, _hip.BROYDEN_CNEW
    L = 27 if t == 27 else t + 1                                                               # t = 27: the first wrapped step, row 0
    slot = t % L
    U, V = _randn(N + 6, bsz, L, N) / np.float32(np.sqrt(N)), _randn(N + 7, bsz, L, N)
    dx, g0, g1 = _randn(N + 8, bsz, N), _randn(N + 9, bsz, N), _randn(N + 10, bsz, N)
    dg = g1 - g0
    assert dg.dtype == np.float32 and U.dtype == np.float32
    ws = _hip.BroydenWorkspace(bsz, N, L, DEV)
    ws.U.copy_(torch.from_numpy(U))
    ws.V.copy_(torch.from_numpy(V))
    ddx, dg0, dg1 = _dev(dx, off), _dev(g0), _dev(g1)
    _hip.broyden_dots(ws, ddx, dg0, dg1, t)
    tab = ws.table.cpu().numpy().copy()
    dx64, dg64, g164 = dx.astype(F64), dg.astype(F64), g1.astype(F64)
    for j in range(t):
        Uj, Vj = U[:, j].astype(F64), V[:, j].astype(F64)
        assert np.array_equal(tab[:, A + j], ro.sum_workgroup(dx64 * Uj, 2)), ("a", j)
        assert np.array_equal(tab[:, B + j], ro.sum_workgroup(Vj * dg64, 2)), ("b", j)
        assert np.array_equal(tab[:, C + j], ro.sum_workgroup(Vj * g164, 2)), ("c", j)
    assert np.array_equal(tab[:, GG], ro.sum_workgroup(g164 * g164, 2))
    _hip.broyden_update(ws, ddx, dg0, dg1, t, slot, torch.empty(bsz, N, device=DEV))
    tab = ws.table.cpu().numpy()
    vT = ws.V[:, slot].cpu().numpy()                                                           # the device's stored row (no NaN to zero here)
    assert np.isfinite(vT).all()
    assert np.array_equal(tab[:, D], ro.sum_workgroup(vT.astype(F64) * dg64, 2))
    assert np.array_equal(tab[:, CN], ro.sum_workgroup(vT.astype(F64) * g164, 2))
