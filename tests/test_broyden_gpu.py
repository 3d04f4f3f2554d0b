"""GPU: Broyden's method on the device - the step kernels of csrc/broyden.hip against float64, stage by stage with derived bounds; the
solver against the float64 restatement (tests/broyden_f64.py) on the reference's toy cases (tests/golden/broyden_toy.npz); and
DEQFixedPoint with broyden_fixed_point through the real map, forward and implicit backward.

Bounds of the step-kernel tests.  The inner products are exact products summed in float64: they agree with numpy's float64 sums to
1e-12 x sum |a_i b_i| (both sides err by a few units of 2^-53 per level of their summation trees).  A combination of r rows with
fp32-rounded coefficients, summed in fp32 term by term, errs per element by at most (r + 3) 2^-24 x sum_j |c_j| |row_j| (one rounding
of the coefficient, one of the product, at most r + 1 of the running sum, each 2^-24 relative).  vT, u and the update are held to
(t + 3) 2^-23 x sum_j |c_j| |row_j| plus one ulp of the result, t the number of old rows: vT and w have r = t, u adds the rounding of d
and the division (t + 5 units of 2^-24), the update has r = t + 1 rows when the history fills (t + 4 units); 2 (t + 3) covers each.  Each stage is held to the float64 value computed from the inputs that stage read on the device (its coefficients from the
float64 table, the rows from memory), so a bound never has to absorb the cancellation of an earlier stage."""
import copy
import os

import numpy as np
import pytest
import torch

import broyden_f64 as bf
from conftest import GOLDEN, ROOT, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint
    from deqsci_amd.cli import build_pipeline

DEV = "cuda"
L = 27
U23 = 2.0 ** -23


def _state(bsz, N, seed, t, L=L):
    """A seeded step state on the device: a workspace of L rows whose first t are filled, dx, gx_old, gx_new, x."""
    r = np.random.RandomState(seed)
    ws = _hip.BroydenWorkspace(bsz, N, L, DEV)
    ws.U[:, :t] = torch.from_numpy((r.randn(bsz, t, N) / np.sqrt(N)).astype(np.float32)).to(DEV)
    ws.V[:, :t] = torch.from_numpy(r.randn(bsz, t, N).astype(np.float32)).to(DEV)
    rows = [torch.from_numpy(r.randn(bsz, N).astype(np.float32)).to(DEV) for _ in range(4)]
    return ws, rows


def _ulp(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def _run_step(ws, dx, g0, g1, x, t, slot):
    """dots + update on the device; -> everything the checks need, as float64 numpy (inputs as they were BEFORE the step)."""
    n = lambda v: v.detach().cpu().numpy().astype(np.float64)
    U0, V0 = n(ws.U), n(ws.V)
    _hip.broyden_dots(ws, dx, g0, g1, t)
    tab_dots = ws.table.cpu().numpy().copy()
    upd, xn = torch.empty_like(dx), torch.empty_like(dx)
    _hip.broyden_update(ws, dx, g0, g1, t, slot, upd, x=x, x_next=xn)
    torch.cuda.synchronize()
    return {"U0": U0, "V0": V0, "dx": n(dx), "g1": n(g1), "dg": (g1 - g0).cpu().numpy().astype(np.float64), "x": x.cpu().numpy(),
            "tab_dots": tab_dots, "tab": ws.table.cpu().numpy().copy(), "U": n(ws.U), "V": n(ws.V), "upd": n(upd), "upd32": upd.cpu().numpy(),
            "xn32": xn.cpu().numpy()}


def _within(got, want, mag, rows, what):
    err = np.abs(got - want)
    bound = (rows + 3) * U23 * mag + _ulp(want)
    worst = float((err / bound).max())
    print(f"    {what}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (what, worst)


def _check_step(o, t, slot):
    A, B, C, GG, D, CN = _hip.BROYDEN_A, _hip.BROYDEN_B, _hip.BROYDEN_C, _hip.BROYDEN_GG, _hip.BROYDEN_D, _hip.BROYDEN_CNEW
    U0, V0, dx, g1, dg = o["U0"][:, :t], o["V0"][:, :t], o["dx"], o["g1"], o["dg"]
    tab = o["tab"]

    def dots_close(got, x, y, what):
        want, size = np.einsum("b...n,b...n->b...", x, y), np.einsum("b...n,b...n->b...", np.abs(x), np.abs(y))
        worst = float((np.abs(got - want) / (1e-12 * size + 1e-300)).max()) if want.size else 0.0
        print(f"    {what}: worst error / (1e-12 sum|a b|) {worst:.3f}")
        assert worst <= 1.0, (what, worst)
    dots_close(tab[:, A:A + t], dx[:, None], U0, "a")
    dots_close(tab[:, B:B + t], V0, dg[:, None], "b")
    dots_close(tab[:, C:C + t], V0, g1[:, None], "c")
    dots_close(tab[:, GG], g1, g1, "gg")
    assert np.array_equal(o["tab_dots"][:, :GG + 1], tab[:, :GG + 1])                 # the update leaves the products alone
    # the rank-one rows, from the float64 coefficients the kernel read
    a, b, c = tab[:, A:A + t], tab[:, B:B + t], tab[:, C:C + t]
    vT = -dx + np.einsum("bj,bjn->bn", a, V0)
    _within(o["V"][:, slot], vT, np.abs(dx) + np.einsum("bj,bjn->bn", np.abs(a), np.abs(V0)), t, "vT")
    w = dx - (np.einsum("bj,bjn->bn", b, U0) - dg)
    mag_w = np.abs(dx) + np.abs(dg) + np.einsum("bj,bjn->bn", np.abs(b), np.abs(U0))
    vT_dev = o["V"][:, slot]
    dots_close(tab[:, D], vT_dev, dg, "d")
    dots_close(tab[:, CN], vT_dev, g1, "c_new")
    d, cn = tab[:, D], tab[:, CN]
    _within(o["U"][:, slot], w / d[:, None], mag_w / np.abs(d)[:, None], t, "u")
    # the new direction, from the rows in memory after the step: the t old rows less a replaced one, and the new row with c_new
    rows = max(t, slot + 1)
    cc = np.zeros((dx.shape[0], rows))
    cc[:, :t] = c
    cc[:, slot] = cn
    Un = o["U"][:, :rows]
    upd = g1 - np.einsum("bj,bjn->bn", cc, Un)
    _within(o["upd"], upd, np.abs(g1) + np.einsum("bj,bjn->bn", np.abs(cc), np.abs(Un)), t, "update")
    assert np.array_equal(o["xn32"], o["x"] + o["upd32"])                               # one fp32 addition
    keep = [j for j in range(o["U"].shape[1]) if j != slot]
    assert np.array_equal(o["U"][:, keep], o["U0"][:, keep]) and np.array_equal(o["V"][:, keep], o["V0"][:, keep])      # only row `slot` is written


def _chunk():
    return _hip.broyden_chunk()


@pytest.mark.parametrize("t", [0, 1, 5, 27])
@pytest.mark.parametrize("n_kind", ["1200", "2051", "3chunks+7"])
@pytest.mark.parametrize("bsz", [1, 3])
def test_step_kernels_against_float64(bsz, n_kind, t):
    N = {"1200": 1200, "2051": 2051, "3chunks+7": 3 * _chunk() + 7}[n_kind]
    ws, (dx, g0, g1, x) = _state(bsz, N, 1000 * bsz + t, t)
    slot = t % L                                          # t = 27: the first wrapped step, row 0
    _check_step(_run_step(ws, dx, g0, g1, x, t, slot), t, slot)


def test_step_kernels_wrap_in_the_middle_and_ragged_vector_rows():
    """t = 27 with the slot in the middle of the history: the row it replaces feeds vT and w but not the update.  N = 3 chunks + 8: the
    float4 path with a last chunk that is nearly empty."""
    N = 3 * _chunk() + 8
    ws, (dx, g0, g1, x) = _state(3, N, 77, 27)
    o = _run_step(ws, dx, g0, g1, x, 27, 13)
    _check_step(o, 27, 13)
    want = bf.step_f64(o["U0"], o["V0"], o["dx"], None, o["g1"], 27, 13, dg=o["dg"])
    assert rel_l2(o["upd"], want["update"]) < 1e-3        # (end to end, through d's cancellation: the old row 13 is not in it)
    with_old = o["g1"] - np.einsum("bj,bjn->bn", o["tab"][:, _hip.BROYDEN_C:_hip.BROYDEN_C + 27], o["U0"])
    assert rel_l2(o["upd"], with_old - o["tab"][:, _hip.BROYDEN_CNEW, None] * o["U"][:, 13]) > 1e-2


def test_step_kernels_do_not_depend_on_alignment_or_batch():
    """The same rows at a 4-byte offset (every access element by element) and as sample 0 of a batch of two copies: the same bits."""
    N, t = 2 * _chunk() + 1032, 5
    ws, (dx, g0, g1, x) = _state(1, N, 5, t)
    base = _run_step(ws, dx, g0, g1, x, t, t)
    ws1, _ = _state(1, N, 5, t)
    off = [torch.empty(N + 1, device=DEV)[1:].view(1, N).copy_(v) for v in (dx, g0, g1, x)]
    assert all(v.data_ptr() % 16 == 4 for v in off)
    o1 = _run_step(ws1, *off, t, t)
    ws2, _ = _state(1, N, 5, t)
    big = _hip.BroydenWorkspace(2, N, L, DEV)
    big.U[:], big.V[:] = ws2.U, ws2.V
    o2 = _run_step(big, *[v.repeat(2, 1).contiguous() for v in (dx, g0, g1, x)], t, t)
    for k in ("tab", "U", "V", "upd32", "xn32"):
        assert np.array_equal(base[k], o1[k]), k
        assert np.array_equal(base[k][0], o2[k][0]) and np.array_equal(o2[k][0], o2[k][1]), k


def test_step_kernels_zero_denominator_and_nan():
    """Sample 1: gx_new = gx_old, so d = 0 - u = dx / 0 keeps its infinities, and 0 / 0 becomes 0.  Sample 2: a NaN in dx - vT and u are
    all NaN before they are zeroed.  Sample 0 is what it is alone."""
    N, t = 1200, 5
    ws, (dx, g0, g1, x) = _state(3, N, 9, t)
    g1[1] = g0[1]
    dx[1, 5] = 0.0
    dx[2, 7] = float("nan")
    o = _run_step(ws, dx, g0, g1, x, t, t)
    assert o["tab"][1, _hip.BROYDEN_D] == 0.0 and np.isnan(o["tab"][2, _hip.BROYDEN_D])
    u1 = o["U"][1, t]
    assert u1[5] == 0.0 and np.isinf(np.delete(u1, 5)).all() and np.array_equal(np.sign(np.delete(u1, 5)), np.sign(np.delete(o["dx"][1], 5)))
    assert not np.isnan(o["V"][1, t]).any()
    assert not o["U"][2, t].any() and not o["V"][2, t].any()
    ws0, _ = _state(3, N, 9, t)
    alone = _hip.BroydenWorkspace(1, N, L, DEV)
    alone.U[:], alone.V[:] = ws0.U[:1], ws0.V[:1]
    o0 = _run_step(alone, *[v[:1].contiguous() for v in (dx, g0, g1, x)], t, t)
    for k in ("tab", "U", "V", "upd32", "xn32"):
        assert np.array_equal(o[k][0], o0[k][0]), k
    assert np.isfinite(o["upd32"][0]).all()


def test_step_kernels_at_the_workload_row_length():
    """Launch geometry: bsz = 2, N = 256 x 256 x 8 (256 chunks per sample), t = 9 (a history of 10 rows keeps the host copies small)."""
    ws, (dx, g0, g1, x) = _state(2, 256 * 256 * 8, 3, 9, L=10)
    _check_step(_run_step(ws, dx, g0, g1, x, 9, 9), 9, 9)


# ----------------------------------------------------------------------------- the solver
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "broyden_toy.npz")))


@pytest.fixture(scope="module")
def f64_runs(golden):
    out = {}
    for name in bf.CASES:
        f, shape, threshold, eps = bf.case_map(golden, name, torch.float64)
        out[name] = bf.broyden_f64(bf.as_g_numpy(f, shape), golden[f"{name}/x0"], threshold, eps)
    return out


def _device_run(golden, name):
    f, shape, threshold, eps = bf.case_map(golden, name, torch.float32, DEV)
    g, seen = bf.as_g(f, shape), []

    def watched(x):
        seen.append(tuple(x.shape))
        return g(x)
    x, res = deqsci_amd.broyden(watched, torch.from_numpy(golden[f"{name}/x0"]).to(DEV), threshold=threshold, eps=eps)
    return x, res, seen, dict(deqsci_amd.broyden.last_info)


@pytest.mark.parametrize("name", sorted(bf.CASES))
def test_solver_reproduces_the_float64_restatement(golden, f64_runs, name):
    x64, res64, info64 = f64_runs[name]
    x, res, seen, info = _device_run(golden, name)
    shape, eps = bf.CASES[name][1], bf.CASES[name][5]
    dist = rel_l2(x.cpu().numpy(), x64)
    print(f"{name}: device vs float64 {dist:.3e} (reference vs float64 {float(golden[f'{name}/ref_vs_f64']):.3e}), g calls {info['g_calls']}, "
          f"res {res:.6e} (float64 {res64:.6e})")
    assert tuple(x.shape) == shape and x.dtype == torch.float32
    assert set(seen) == {(shape[0], int(np.prod(shape[1:])), 1)}                       # g's call shape is the reference's
    assert dist <= max(10 * float(golden[f"{name}/ref_vs_f64"]), 1e-7)
    assert info["g_calls"] == len(seen) == info64["g_calls"] == int(golden[f"{name}/ref_g_calls"])
    assert info["lowest_step"] == info64["lowest_step"]
    if bool(golden[f"{name}/eps_stop"]):
        assert res < eps and abs(res - res64) <= 0.01 * res64
    assert abs(np.sqrt(sum(v * v for v in info["res_per_sample"])) - res) <= 1e-12 * res and len(info["res_per_sample"]) == shape[0]


def test_solver_is_deterministic(golden):
    a = _device_run(golden, "a")
    b = _device_run(golden, "a")
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[3]["trace"] == b[3]["trace"]


# ----------------------------------------------------------------------------- through the stack
def _crop(size=32):
    from deqsci_amd.harness import load_test_data
    d = load_test_data(os.path.join(ROOT, "data", "test_gray", "traffic_cacti.mat"))
    sl = (slice(96, 96 + size), slice(64, 64 + size))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"][sl]))[None]
    y = torch.from_numpy(np.ascontiguousarray(d["meas"][sl][..., 0]))[None]
    return y, Phi


def _deq(kind, weights, threshold=8, eps=1e-5):
    solver, _ = build_pipeline(kind, checkpoint.shipped(weights), threshold)
    return solver, deqsci_amd.DEQFixedPoint(solver, deqsci_amd.broyden_fixed_point, threshold=threshold, eps=eps)


def test_deq_forward_against_float64_host():
    y, Phi = _crop()
    solver, deq = _deq("SimpleCNN", "cnn")
    dy, dPhi = y.to(DEV), Phi.to(DEV)
    dPs = deqsci_amd.phi_sum(dPhi)
    with torch.no_grad():
        rec = deq.forward(dy, dPhi, dPs, initial_point=deqsci_amd.initial_point(dy, dPhi, dPs, None), train_flag=False)
    assert deq._engine is None and isinstance(deq.forward_res, float)
    # the same construction in float64 on the host: f(z) = z1 - D(z1), z1 = z + At((y - A z) / Phi_sum), then the wrapper's extra f call
    net = copy.deepcopy(solver.nonlinear_op).cpu().double().eval()
    y64, Phi64 = y.double(), Phi.double()
    Ps64 = Phi64.sum(-1)
    Ps64[Ps64 == 0] = 1
    shape = tuple(Phi.shape)

    def f(z):
        z1 = z + ((y64 - (z * Phi64).sum(-1)) / Ps64)[..., None] * Phi64
        zp = z1.permute(0, 3, 1, 2).reshape(-1, 1, shape[1], shape[2])
        return z1 - net(zp).view(shape[0], shape[3], shape[1], shape[2]).permute(0, 2, 3, 1)
    with torch.no_grad():
        x0 = (y64[..., None] * Phi64).numpy()
        z64, res64, info64 = bf.broyden_f64(bf.as_g_numpy(f, shape), x0, 8, 1e-5)
        want = f(torch.from_numpy(z64)).numpy()
    dist = rel_l2(rec.cpu().numpy(), want)
    print(f"DEQFixedPoint + broyden_fixed_point, SimpleCNN 32x32x8: rel-L2 vs float64 host {dist:.3e}, res {deq.forward_res:.4e} (float64 {res64:.4e})")
    assert dist <= 1e-4
    assert deqsci_amd.broyden.last_info["g_calls"] == info64["g_calls"]


def test_deq_implicit_backward_device_against_autograd():
    y, Phi = _crop()
    grads = {}
    for mode in ("device", "autograd"):
        solver, deq = _deq("SimpleCNN", "cnn")
        deq.implicit_backward = mode
        dy, dPhi = y.to(DEV).requires_grad_(), Phi.to(DEV)
        dPs = deqsci_amd.phi_sum(dPhi)
        rec = deq(dy, dPhi, dPs, initial_point=deqsci_amd.initial_point(dy.detach(), dPhi, dPs, None))
        rec.square().mean().backward()
        assert deq.last_backward_path == mode and deq.backward_fallback_reason is None
        assert isinstance(deq.backward_res, float) and np.isfinite(deq.backward_res)
        grads[mode] = (dy.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in solver.named_parameters()})
    dist = rel_l2(grads["device"][0], grads["autograd"][0])
    print(f"implicit backward with broyden_fixed_point: input gradient, device vs autograd {dist:.3e}")
    assert np.abs(grads["autograd"][0]).max() > 0 and dist <= 1e-4
    for k, gk in grads["autograd"][1].items():
        assert rel_l2(grads["device"][1][k], gk) <= 1e-4, k


def test_deq_forward_ffdnet_runs():
    """No parity gate: FFDNet's sigma falls with every call, so f is not one map and the secant pairs mix maps."""
    y, Phi = _crop()
    _, deq = _deq("ffdnet", "ffdnet_gray")
    dy, dPhi = y.to(DEV), Phi.to(DEV)
    dPs = deqsci_amd.phi_sum(dPhi)
    with torch.no_grad():
        rec = deq.forward(dy, dPhi, dPs, initial_point=deqsci_amd.initial_point(dy, dPhi, dPs, None), train_flag=False)
    info = deqsci_amd.broyden.last_info
    assert info["nstep"] == 8 and info["g_calls"] == 9
    assert tuple(rec.shape) == tuple(Phi.shape) and bool(torch.isfinite(rec).all()) and np.isfinite(deq.forward_res)
