"""GPU: the Anderson step kernels (csrc/anderson.hip) one by one against float64 references of the same operation, at the smallest shapes
where each code path exists.  K4 residual_store (exact outputs, bounded block sums, every seam of the sweeps), K5+K6 anderson_solve (the
persistent float64 Gram through the ring's wrap, the residuals and the arrival ticket, the bordered LU in float64 and in fp32), K7
anderson_mix and anderson_mix_gap (every instantiation and both fallbacks).  Every bound is the operation count of the kernel times the
unit roundoff of fp32, u = 2^-24, on the sum of the magnitudes (first-order, Higham's gamma_k), or - the fp32 LU - a multiple measured
on LAPACK's sgesv for the same systems; profiles/anderson_step_kernels.md has the table of shapes, paths, bounds and measured err / bound."""
import ctypes

import numpy as np
import pytest
import torch

import sci_ops_ref as so

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip
    from test_gpu_parity import make_case

DEV = "cuda"
HWB, BHW = 0, 1
U = 2.0 ** -24                                                 # unit roundoff of fp32
STREAM_MIN_BYTES = 64 << 20                                    # (csrc/common.hpp: from here on K4 / K7 use non-temporal loads and stores)
NAN = float("nan")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, device=DEV, generator=gen)


def _chunk(ws):
    """Elements per K4 block (chunk_elems): N / nchunks, rounded up to whole 1024-element sweeps, two at least."""
    per = -(-ws.N // ws.nchunks)
    return max(2048, -(-per // 1024) * 1024)


def _k4_ops(chunk):
    """Roundings on the way of one product into a block sum: chunk / 256 fused multiply-adds of a lane (chunk / 1024 sweeps of a float4),
    six wave-shuffle adds, three LDS adds.  (The float64 finish over the blocks adds nothing visible.)"""
    return chunk // 256 + 9


def _state(ws):
    """(bsz, 80) float64: the 8 x 8 Gram, |F_slot|^2, |G_slot|^2 of the last call."""
    return ws.gram[:ws.bsz * 80].view(ws.bsz, 80).clone()


def _dots(a, rows):
    """float64 <a, rows_j> and sum |a_i rows_ji| for a (bsz, N), rows (bsz, r, N), both fp32 on the device."""
    a = a.double().unsqueeze(1)
    ex = torch.empty(rows.shape[:2], device=rows.device, dtype=torch.float64)
    mag = torch.empty_like(ex)
    for j in range(rows.shape[1]):                             # (row by row: the largest case is 128 x 262148)
        p = a[:, 0] * rows[:, j].double()
        ex[:, j] = p.sum(-1)
        mag[:, j] = p.abs().sum(-1)
    return ex, mag


def _ratio(got, exact, bound):
    """max |got - exact| / bound; an error where the bound is zero must be zero."""
    err = (got - exact).abs()
    assert torch.isfinite(got).all()
    assert (err[bound == 0] == 0).all()
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ----------------------------------------------------------------------------- K4
# (bsz, N, m, nchunks, chunk): the path each reaches is in profiles/anderson_step_kernels.md
K4_SHAPES = [(2, 5, 8, 1, 2048), (1, 105, 8, 1, 2048), (3, 2051, 8, 2, 2048),      # scalar path (N % 4 != 0): one block, two blocks
             (1, 4, 8, 1, 2048),                                                  # a single float4
             (2, 1028, 8, 1, 2048),                                               # one sweep + a tail of one float4
             (1, 2048, 8, 1, 2048),                                               # exactly one two-sweep trip
             (3, 2052, 8, 2, 2048),                                               # a second block of 4 elements
             (2, 7172, 8, 4, 2048),                                               # 3.5 blocks
             (128, 262148, 2, 86, 3072)]                                          # three sweeps per block, 86 blocks, streaming cache policy


def _k4_workspace(bsz, N, m, nchunks, chunk):
    ws = _hip.AndersonWorkspace(bsz, N, m, DEV)
    assert ws.nchunks == nchunks and _chunk(ws) == chunk       # (a retuned chunk_elems must not silently empty a case)
    assert (bsz * N * 4 * (1 + 4) >= STREAM_MIN_BYTES) == (bsz == 128)     # the streaming policy: from the first call on, or never
    return ws


@pytest.mark.parametrize("bsz,N,m,nchunks,chunk", K4_SHAPES)
def test_k4_outputs_are_exact_and_its_sums_bounded_through_the_rings_wrap(bsz, N, m, nchunks, chunk):
    """m + 3 calls in the loop's order (slot k % m, n_filled = min(k + 1, m)), noise on the odd calls, x_next on the first, x_cur != 0.
    F, G, x_next are single IEEE operations: bit for bit.  The whole n x n float64 Gram, |F|^2 and |G|^2 after every call against the
    float64 sums over the stored fp32 rows: |got - exact| <= (chunk / 256 + 9) u sum_i |G_a[i] G_b[i]| - after the wrap that includes the
    rows last refreshed m - 1 calls ago."""
    ws = _k4_workspace(bsz, N, m, nchunks, chunk)
    gen = _gen(N + bsz)
    K = _k4_ops(chunk)
    x_next = torch.full((bsz, N), NAN, device=DEV)
    worst = 0.0
    for k in range(m + 3):
        slot, nf = k % m, min(k + 1, m)
        z1, x_cur = _randn(gen, bsz, N), _randn(gen, bsz, N)
        noise = 0.1 * _randn(gen, bsz, N) if k % 2 else None
        F0, G0 = ws.F.clone(), ws.G.clone()
        _hip.residual_store(ws, z1, noise, x_cur, slot, nf, x_next if k == 0 else None)
        f = z1 - noise if noise is not None else z1
        assert torch.equal(ws.F[:, slot], f), k
        assert torch.equal(ws.G[:, slot], f - x_cur), k
        if k == 0:
            assert torch.equal(x_next, f)
        F0[:, slot], G0[:, slot] = ws.F[:, slot], ws.G[:, slot]
        assert torch.equal(ws.F, F0) and torch.equal(ws.G, G0), k          # (the other slots are untouched)
        del F0, G0
        _hip.anderson_solve(ws, slot, nf, 0, 1e-2, 1e-5)
        st = _state(ws)
        gram = st[:, :64].view(bsz, 8, 8)
        for a in range(nf):
            ex, mag = _dots(ws.G[:, a], ws.G[:, :nf])
            worst = max(worst, _ratio(gram[:, a, :nf], ex, K * U * mag))
            if a == slot:
                worst = max(worst, _ratio(st[:, 65], ex[:, slot], K * U * mag[:, slot]))
        ff, _ = _dots(ws.F[:, slot], ws.F[:, slot:slot + 1])
        worst = max(worst, _ratio(st[:, 64], ff[:, 0], K * U * ff[:, 0]))
    print(f"K4 ring ({bsz}, {N}) m={m} chunk={chunk} nchunks={nchunks}: max err / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("bsz,N,m,nchunks,chunk", K4_SHAPES)
def test_k4_drops_and_doubles_no_element_at_any_seam(bsz, N, m, nchunks, chunk):
    """Random data would hide one element dropped or read twice at a seam of the sweeps.  So: a history of 1e-3 randn with the value 1000 at
    ONE index of every row - the first and last element, both sides of every float4 / sweep / trip / block boundary - one index at a time.
    The product at that index is 1e6 of a sum of 1e6: losing or doubling it is 1e6 / bound ~ 1e6 times over the same bound as above."""
    m = min(m, 3)
    ws = _k4_workspace(bsz, N, m, nchunks, chunk)
    gen = _gen(7 * N + bsz)
    K = _k4_ops(chunk)
    ws.G.copy_(1e-3 * _randn(gen, bsz, m, N))
    z1, x_cur = 1e-3 * _randn(gen, bsz, N), 1e-3 * _randn(gen, bsz, N)
    slot = 1 if m > 1 else 0
    worst = 0.0
    seams = sorted({i for i in (0, 3, 4, 1019, 1023, 1024, 2047, 2048, chunk - 1, chunk, N - 4, N - 1) if 0 <= i < N})
    for idx in seams:
        keep_g, keep_z = ws.G[:, :, idx].clone(), z1[:, idx].clone()
        ws.G[:, :, idx] = 1000.0
        z1[:, idx] = 1000.0
        _hip.residual_store(ws, z1, None, x_cur, slot, m, None)
        _hip.anderson_solve(ws, slot, m, 0, 1e-2, 1e-5)
        st = _state(ws)
        assert float(ws.G[:, slot, idx].min()) > 999.0
        ex, mag = _dots(ws.G[:, slot], ws.G)
        assert float(ex.min()) > 9.9e5                          # (the spike is what the sums are made of)
        r = _ratio(st[:, :64].view(bsz, 8, 8)[:, slot, :m], ex, K * U * mag)
        r = max(r, _ratio(st[:, 65], ex[:, slot], K * U * mag[:, slot]))
        ff, _ = _dots(ws.F[:, slot], ws.F[:, slot:slot + 1])
        r = max(r, _ratio(st[:, 64], ff[:, 0], K * U * ff[:, 0]))
        assert r <= 1.0, (idx, r)
        worst = max(worst, r)
        ws.G[:, :, idx] = keep_g
        z1[:, idx] = keep_z
    print(f"K4 seams ({bsz}, {N}) chunk={chunk}: {len(seams)} indices, max err / bound {worst:.4f}")


# ----------------------------------------------------------------------------- K5 + K6
@pytest.mark.parametrize("bsz", [1, 3, 9])
def test_solve_residuals_ticket_and_n0(bsz):
    """res[row, 1 + s] = sqrt(|G_s|^2) / (eps + sqrt(|F_s|^2)) and the batch-wide res[row, 0] (bsz = 1: the copy; bsz > 1: the last block to
    draw the arrival ticket, which resets itself - five calls in a row on one workspace) against the float64 sums over the stored rows.
    Both sums are of positive terms, each within (chunk / 256 + 9) u RELATIVE; the square root halves that, numerator and denominator
    add up to the whole again, and the result is rounded to fp32 once: |got - want| <= ((chunk / 256 + 9) u + 2^-23) want.
    The rows of `res` that were not asked for stay as they were, and n = 0 leaves alpha alone."""
    N, m, eps = 2052, 3, 1e-5
    ws = _hip.AndersonWorkspace(bsz, N, m, DEV, res_rows=4)
    assert ws.nchunks == 2 and _chunk(ws) == 2048
    rel = _k4_ops(2048) * U + 2.0 ** -23
    gen = _gen(100 + bsz)
    ws.res.fill_(-7.0)
    ws.alpha.fill_(NAN)
    eps32 = float(np.float32(eps))
    worst = 0.0
    for k, row in enumerate((0, 3, 1, 0, 3)):
        slot, nf = k % m, min(k + 1, m)
        scale = 1e-4 * (1 + torch.arange(bsz, device=DEV).view(bsz, 1))            # (eps is 0.2 % of |F| here: it is checked too)
        z1, x_cur = scale * _randn(gen, bsz, N), scale * _randn(gen, bsz, N)
        _hip.residual_store(ws, z1, None, x_cur, slot, nf, None)
        before = ws.res.clone()
        _hip.anderson_solve(ws, slot, nf, 0, 1e-2, eps, res_row=row)
        after = ws.res.clone()
        gg = (ws.G[:, slot].double() ** 2).sum(-1)
        ff = (ws.F[:, slot].double() ** 2).sum(-1)
        want = torch.cat([(gg.sum().sqrt() / (eps32 + ff.sum().sqrt())).view(1), gg.sqrt() / (eps32 + ff.sqrt())])
        worst = max(worst, _ratio(after[row].double(), want, rel * want))
        if bsz == 1:
            assert after[row, 0] == after[row, 1]
        others = [r for r in range(4) if r != row]
        assert torch.equal(after[others], before[others])
        assert torch.isnan(ws.alpha).all()
    print(f"solve residuals bsz={bsz}: max err / bound {worst:.4f}")
    assert worst <= 1.0


def _lu_rows(kind, bsz, m, N, gen):
    if kind == "independent":
        return _randn(gen, bsz, m, N)
    if kind == "late":                                         # late in the iteration: a common vector, a 5 % ramp, 0.3 of noise
        return (_randn(gen, bsz, 1, N) * (1 + 0.05 * torch.arange(m, device=DEV).view(1, m, 1)) + 0.3 * _randn(gen, bsz, m, N)) * 1e-2
    if kind == "repeated":                                     # one row exactly twice: G G^T is singular, lam alone separates the two
        x = _randn(gen, bsz, m, N) * 1e-2                      # (scaled so that fp32 still sees lam = 1e-4 next to |G|^2 ~ 0.2: the fp32 LU runs on these too)
        x[:, 1] = x[:, 0]
        return x
    raise ValueError(kind)


LU_CASES = [("independent", 1e-2), ("independent", 1e-4), ("independent", 0.0), ("late", 1e-2), ("late", 1e-4), ("repeated", 1e-4)]
LU_BSZ, LU_N, LU_M = 2, 2052, 8


def _bordered(gram, lam, dtype):
    """[[0, 1^T], [1, G G^T + lam I]] for gram (bsz, n, n), formed in `dtype` as the kernel forms it (lam is the fp32 the C ABI takes)."""
    bsz, n, _ = gram.shape
    H = np.zeros((bsz, n + 1, n + 1), dtype=dtype)
    H[:, 0, 1:] = 1
    H[:, 1:, 0] = 1
    H[:, 1:, 1:] = gram.astype(dtype) + (np.float32(lam) * np.eye(n, dtype=np.float32)).astype(dtype)
    return H


def _solve64(H):
    """alpha (bsz, n) of the bordered system in float64, and cond_inf(H) per sample."""
    H = H.astype(np.float64)
    rhs = np.zeros(H.shape[:2] + (1,))
    rhs[:, 0] = 1
    sol = np.linalg.solve(H, rhs)[:, 1:, 0]
    return sol, np.array([np.linalg.cond(h, np.inf) for h in H])


@pytest.mark.parametrize("kind,lam", LU_CASES)
def test_solve_float64_lu_vs_numpy(kind, lam):
    """The bordered (n + 1) x (n + 1) system, n = 1..8, from the kernel's OWN float64 Gram, against numpy.linalg.solve:
    |alpha - want| <= u |want| (alpha is stored as fp32) + 64 cond_inf(H) 2^-53 |want|_inf (a backward-stable float64 LU of at most 9
    rows; 64 covers the growth and the constant of the forward bound).  Entries n..7 of alpha are exactly 0."""
    bsz, N, m = LU_BSZ, LU_N, LU_M
    ws = _hip.AndersonWorkspace(bsz, N, m, DEV)
    assert ws.nchunks == 2
    rows = _lu_rows(kind, bsz, m, N, _gen(5))
    zero = torch.zeros(bsz, N, device=DEV)
    worst = 0.0
    for k in range(m):
        n = k + 1
        _hip.residual_store(ws, rows[:, k].contiguous(), None, zero, k, n, None)
        ws.alpha.fill_(NAN)
        _hip.anderson_solve(ws, k, n, n, lam, 1e-5)
        gram = _state(ws)[:, :64].view(bsz, 8, 8)[:, :n, :n].cpu().numpy()
        want, cond = _solve64(_bordered(gram, lam, np.float64))
        got = ws.alpha.cpu().numpy().astype(np.float64)
        assert np.array_equal(got[:, n:], np.zeros((bsz, 8 - n)))
        bound = U * np.abs(want) + (64 * cond * 2.0 ** -53 * np.abs(want).max(1))[:, None]
        assert np.isfinite(got).all()
        worst = max(worst, float((np.abs(got[:, :n] - want) / bound).max()))
    print(f"float64 LU {kind} lam={lam:g}: max err / bound {worst:.4f}")
    assert worst <= 1.0


_LU32 = {}


def _lu32_measurements():
    """For every LU case, n = 1..8 and both fp32 entries of the solve - gram32= (the caller's fp32 torch.bmm block) and ref=True (the
    kernel's own fp32 Gram, read back from gram32_state) -: the system built from those fp32 values as the kernel builds it, its float64
    solution, and the errors of the kernel and of LAPACK's sgesv (torch.linalg.solve in fp32 on the CPU, what the reference calls) as
    multiples of (n + 1) u cond_inf(H) |want|_inf.  Computed once, shared by the tests below."""
    if _LU32:
        return _LU32
    bsz, N, m = LU_BSZ, LU_N, LU_M
    out = {"gram32": [], "ref": []}
    for kind, lam in LU_CASES:
        rows = _lu_rows(kind, bsz, m, N, _gen(5))
        zero = torch.zeros(bsz, N, device=DEV)
        for entry in ("gram32", "ref"):
            ws = _hip.AndersonWorkspace(bsz, N, m, DEV)
            for k in range(m):
                n = k + 1
                _hip.residual_store(ws, rows[:, k].contiguous(), None, zero, k, n, None, ref=(entry == "ref"))
                ws.alpha.fill_(NAN)
                if entry == "gram32":
                    g32 = torch.bmm(ws.G[:, :n], ws.G[:, :n].mT).contiguous()
                    _hip.anderson_solve(ws, k, n, n, lam, 1e-5, gram32=g32)
                else:
                    _hip.anderson_solve(ws, k, n, n, lam, 1e-5, ref=True)
                    g32 = ws.gram32_state()[:, :n, :n]
                H32 = _bordered(g32.cpu().numpy(), lam, np.float32)
                want, cond = _solve64(H32)
                rhs = torch.zeros(bsz, n + 1, 1)
                rhs[:, 0] = 1
                sgesv = torch.linalg.solve(torch.from_numpy(H32), rhs)[:, 1:, 0].numpy().astype(np.float64)
                got = ws.alpha.cpu().numpy().astype(np.float64)
                unit = (n + 1) * U * cond * np.abs(want).max(1)
                out[entry].append(dict(kind=kind, lam=lam, n=n, tail_zero=bool(np.array_equal(got[:, n:], np.zeros((bsz, 8 - n)))),
                                       kernel=float((np.abs(got[:, :n] - want).max(1) / unit).max()),
                                       sgesv=float((np.abs(sgesv - want).max(1) / unit).max())))
    _LU32.update(out)
    return _LU32


@pytest.mark.parametrize("entry", ["gram32", "ref"])
def test_solve_fp32_lu_within_four_times_sgesv(entry):
    """The fp32 LU (partial pivoting, a reciprocal-multiply for the factors) has no tolerance that can be derived exactly, so it is
    measured against the reference's own solver: sgesv's largest error over these systems, as a multiple of
    (n + 1) u cond_inf(H) |want|_inf, times 4 (another but equally valid order of the elimination) is the gate for every system."""
    meas = _lu32_measurements()
    every = meas["gram32"] + meas["ref"]
    assert all(np.isfinite(c["sgesv"]) for c in every)
    gate = 4 * max(c["sgesv"] for c in every)
    worst = max(meas[entry], key=lambda c: c["kernel"])
    print(f"fp32 LU {entry}: sgesv max multiple {gate / 4:.4f} -> gate {gate:.4f}; kernel max multiple {worst['kernel']:.4f} at {worst['kind']} lam={worst['lam']:g} n={worst['n']}")
    for c in meas[entry]:
        assert c["tail_zero"], c
        assert np.isfinite(c["kernel"]) and c["kernel"] <= gate, (c, gate)


def test_step_kernels_refuse_bad_calls():
    lib = _hip.load()
    ws = _hip.AndersonWorkspace(1, 64, 5, DEV)
    z = torch.zeros(1, 64 + 4, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    g32 = torch.zeros(1, 1, 1, device=DEV)
    solve = lambda nf, n, g: lib.deqsci_anderson_solve_gram_f32(p(ws.partials), p(ws.gram), p(ws.alpha), p(ws.res), 1, 64, 5, 0, nf, n, 1e-2, 1e-5, g, None)
    store = lambda z1, slot, nf: lib.deqsci_residual_store_f32(z1, None, p(z), p(ws.F), p(ws.G), None, p(ws.partials), 1, 64, 5, slot, nf, None)
    assert store(p(z), 0, 1) == 0
    assert solve(1, 1, p(g32)) == 0
    assert solve(1, 0, p(g32)) == -2                            # a Gram block and nothing to solve
    assert solve(1, 2, None) == -2                              # n > n_filled
    assert store(p(z), 1, 1) == -2                              # slot >= n_filled
    assert store(ctypes.c_void_p(z.data_ptr() + 4), 0, 1) == -3    # z1 off by one float
    assert lib.deqsci_anderson_mix_f32(p(ws.F), p(ws.G), p(ws.alpha), p(z), 1.0, 0, 1, 64, 5, None) == -2      # mix of nothing
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- K7
def _fill_history(ws, n, gen, f_rand=False):
    """History rows and coefficients written directly; rows n.. and alpha[:, n:] are NaN: they must not be read."""
    bsz, m, N = ws.F.shape
    ws.F.copy_(torch.rand(bsz, m, N, device=DEV, generator=gen) if f_rand else _randn(gen, bsz, m, N))
    ws.G.copy_(0.1 * _randn(gen, bsz, m, N) if f_rand else _randn(gen, bsz, m, N))
    ws.alpha[:, :n] = (1 + 0.3 * _randn(gen, bsz, n)) / n     # (either sign at n = 8; the sum stays near 1)
    ws.F[:, n:] = NAN
    ws.G[:, n:] = NAN
    ws.alpha[:, n:] = NAN


def _mix_reference(ws, n, beta):
    """sum a_i F_i - omb sum a_i G_i in float64 (omb = 1 - beta in fp32, as the launcher forms it) and the bound per element: n fused
    multiply-adds per sum and one for the combination - (n + 2) u (sum |a_i F_i| + |omb| sum |a_i G_i|) - or, beta = 1, n u sum |a_i F_i|."""
    omb = float(np.float32(1) - np.float32(beta))
    a = ws.alpha[:, :n].double().unsqueeze(2)
    want = torch.zeros(ws.bsz, ws.N, device=DEV, dtype=torch.float64)
    mag = torch.zeros_like(want)
    for i in range(n):
        t = a[:, i] * ws.F[:, i].double()
        want += t
        mag += t.abs()
    if omb == 0.0:
        return want, n * U * mag
    for i in range(n):
        t = omb * a[:, i] * ws.G[:, i].double()
        want -= t
        mag += t.abs()
    return want, (n + 2) * U * mag


@pytest.mark.parametrize("bsz,N", [(2, 5), (1, 105), (3, 1028), (2, 2052), (8, 1 << 19)])
def test_mix_flat_vs_float64(bsz, N):
    """The flat kernel's scalar (N % 4 != 0) and vector paths, one block and more, and at 8 x 2^19 with n = 5 the streaming policy;
    m = 8, n < m and n = m, beta = 1 (the shortcut that skips G: G is all NaN then), 0.7 and 0."""
    m = 8
    ws = _hip.AndersonWorkspace(bsz, N, m, DEV)
    gen = _gen(N)
    worst = 0.0
    for n in ((5,) if N == 1 << 19 else (1, 2, 5, 8)):
        assert (bsz * N * 4 * (n + 1) >= STREAM_MIN_BYTES) == (N == 1 << 19)
        for beta in (1.0, 0.7, 0.0):
            _fill_history(ws, n, gen)
            if beta == 1.0:
                ws.G.fill_(NAN)
            x = torch.full((bsz, N), NAN, device=DEV)
            _hip.anderson_mix(ws, x, beta, n)
            want, bound = _mix_reference(ws, n, beta)
            r = _ratio(x.double(), want, bound)
            assert r <= 1.0, (n, beta, r)
            worst = max(worst, r)
    print(f"mix flat ({bsz}, {N}) {'vector' if N % 4 == 0 else 'scalar'}: max err / bound {worst:.4f}")


# ----------------------------------------------------------------------------- K7 + K3
# (layout, B, H, W, fused)
MG_CASES = ([(HWB, B, 5, 7, True) for B in (4, 8, 16, 32)] +                       # LP = 1, 2, 4, 8: tail lanes of the UNR = 2 loop (Q < 512)
            [(HWB, 8, 33, 31, True)] +                                             # more than one block
            [(HWB, 5, 5, 7, False), (HWB, 12, 5, 7, False)] +                      # any other B: the two unfused kernels
            [(BHW, B, H, W, True) for B in (4, 8, 16) for (H, W) in ((6, 6), (34, 30))] +      # BT = 4, 8, 16: one block with idle lanes, several blocks
            [(BHW, 8, 5, 7, False)] +                                              # P % 4 != 0: unfused
            [(BHW, 32, 6, 6, False), (BHW, 5, 6, 6, False)])                       # any other B: unfused


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("layout,B,H,W,fused", MG_CASES)
def test_mix_gap_every_instantiation_vs_float64(layout, B, H, W, fused, shared):
    """x_out held as the flat mix is; z1 against x + Phi^T ((y - Phi x) / Phi_sum) in float64 formed from the kernel's own fp32 x_out, to the
    derived running-error bound of the GAP step (tests/sci_ops_ref.py: ref_gap - the fused kernels do the step's operations one for one, the
    planar one summing its frame column through LDS, and the bound does not depend on the order of a sum); where the case is fused, x_out is bit-equal to anderson_mix on the same workspace; and
    the step lands on the data: Phi z1 = y to 2e-5 where the mask has a non-zero sum.  Binary masks with all-zero pixels (Phi_sum = 1
    there), shared and per sample, bsz = 3."""
    bsz, m, P = 3, 8, H * W
    N = P * B
    assert fused == ((layout == HWB and B in (4, 8, 16, 32)) or (layout == BHW and P % 4 == 0 and B in (4, 8, 16)))
    if layout == HWB and fused:
        assert (P * (B // 4) > 512) == (P > 35)                # (one block of 2 x 256 quads with clamped tail lanes, or several)
    Phi, Phie, _, _, y, Ps = make_case(bsz, H, W, B, seed=B * H + W, shared=shared)
    lay = (lambda t: t) if layout == HWB else (lambda t: t.permute(0, 3, 1, 2).contiguous())
    dPhi, dy, dPs = lay(Phi).to(DEV), y.to(DEV), Ps.to(DEV)
    assert (dPs == 1).any() and (Phi.sum(3) == 0).any()
    shape = (bsz, H, W, B) if layout == HWB else (bsz, B, H, W)
    fdim = 3 if layout == HWB else 1
    Phid = lay(Phie).to(DEV).double()
    ws = _hip.AndersonWorkspace(bsz, N, m, DEV)
    gen = _gen(N + layout)
    worst = worst_gap = 0.0
    for n in (1, 5, 8):
        for beta in (1.0, 0.7, 0.0):
            _fill_history(ws, n, gen, f_rand=True)
            if beta == 1.0:
                ws.G.fill_(NAN)
            x_out, z1 = torch.full(shape, NAN, device=DEV), torch.full(shape, NAN, device=DEV)
            _hip.anderson_mix_gap(ws, beta, n, dPhi, dy, dPs, x_out, z1, layout)
            want, bound = _mix_reference(ws, n, beta)
            r = _ratio(x_out.view(bsz, N).double(), want, bound)
            assert r <= 1.0, (n, beta, r)
            worst = max(worst, r)
            if fused:
                x_flat = torch.full((bsz, N), NAN, device=DEV)
                _hip.anderson_mix(ws, x_flat, beta, n)
                assert torch.equal(x_out.view(bsz, N), x_flat), (n, beta)
            lg = lambda t: so.from_layout(t, layout)            # (n, P, B), the layout sci_ops_ref speaks
            ex, bd = so.ref_gap(lg(x_out), lg(dPhi), dy.view(bsz, P), dPs.reshape(-1, P))
            rg = _ratio(lg(z1).double(), ex, bd)
            assert rg <= 1.0, (n, beta, rg)
            worst_gap = max(worst_gap, rg)
            miss = ((Phid * z1.double()).sum(fdim) - dy.double()).abs()
            assert float(miss[Phid.sum(fdim) != 0].max()) < 2e-5, (n, beta)
    print(f"mix+GAP {'HWB' if layout == HWB else 'BHW'} B={B} {H}x{W} {'fused' if fused else 'unfused'} shared={shared}: x_out max err / bound {worst:.4f}, z1 {worst_gap:.4f}")
