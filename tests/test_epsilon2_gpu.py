"""GPU: the vector epsilon-algorithm on the device - the step kernels of csrc/epsilon2.hip against float64, stage by stage; the solver
against the float64 restatement (tests/epsilon2_f64.py) on the reference's toy cases (tests/golden/epsilon2_toy.npz); DEQFixedPoint with
epsilon2 through the real map, forward and implicit backward; and the command line.

Bounds of the step-kernel tests.  The five sums are sums of exact float64 squares of fp32 numbers, added in float64 in a tree of at most
2^28 / chunk second-stage terms; numpy's float64 sum of the same squares differs from them by a few units of 2^-53 per level of either
tree, so 2^-40 relative (8192 units of 2^-53) holds both with room.  x_new = f_x + (df a - dx b) / c is five fp32 operations: the two
products, their difference and the quotient err by 2^-24 relative each (3 units of 2^-24 of (|df| a + |dx| b) / c to first order), the
final sum by 2^-24 of |x_new| <= |f_x| + (|df| a + |dx| b) / c; 4 x 2^-23 x (|f_x| + (|df| a + |dx| b) / c) is twice that.  Each stage is
held to the float64 value computed from what that stage read on the device (a, b, c as the kernel rounds them from the float64 table), so
no bound has to absorb an earlier stage's rounding."""
import os
import shutil

import numpy as np
import pytest
import torch

import epsilon2_f64 as ef
from conftest import GOLDEN, ROOT, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint
    from deqsci_amd.cli import build_pipeline

DEV = "cuda"
REL40 = 2.0 ** -40
U23 = 2.0 ** -23
GUARD = 64                       # floats (doubles) of NaN on either side of every output: 256 (512) bytes, so the alignment stays


def _guarded(n, dtype=torch.float32, offset=0):
    """(a view of n elements inside a NaN-filled buffer, `offset` elements past a 16-byte boundary; the buffer)"""
    buf = torch.full((2 * GUARD + offset + n,), float("nan"), device=DEV, dtype=dtype)
    return buf[GUARD + offset:GUARD + offset + n], buf


def _guards_intact(buf, n, offset=0):
    return bool(torch.isnan(buf[:GUARD + offset]).all()) and bool(torch.isnan(buf[GUARD + offset + n:]).all())


def _rows(bsz, N, seed, spike_at=None):
    """Seeded x, f_x, f_fx (bsz, N) fp32 numpy of a contracting sequence; spike_at: that element of f_x of every sample 1e4 times the rest."""
    r = np.random.RandomState(seed)
    x = r.randn(bsz, N).astype(np.float32)
    fx = (x + 0.3 * r.randn(bsz, N)).astype(np.float32)
    if spike_at is not None:
        fx[:, spike_at] = 1e4
    ffx = (fx + 0.2 * r.randn(bsz, N)).astype(np.float32)
    return x, fx, ffx


def _run(x, fx, ffx, lam=1e-4, offsets=(0, 0, 0, 0)):
    """norms + update on the device for numpy rows; every output sits between NaN guards.  offsets: elements past a 16-byte boundary
    of x, f_x, f_fx, x_new.  -> dict of numpy results (table after the norms, table after the update, x_new)."""
    bsz, N = x.shape
    dev = []
    for v, off in zip((x, fx, ffx), offsets):
        t, _ = _guarded(bsz * N, offset=off)
        t.copy_(torch.from_numpy(v).reshape(-1))
        assert t.data_ptr() % 16 == 4 * (off % 4)
        dev.append(t.view(bsz, N))
    ws = _hip.Epsilon2Workspace(bsz, N, DEV)
    table, tbuf = _guarded(bsz * 5, torch.float64)
    part, pbuf = _guarded(ws.partials.numel(), torch.float64)
    ws.table, ws.partials = table.view(bsz, 5), part
    xn, xbuf = _guarded(bsz * N, offset=offsets[3])
    _hip.epsilon2_norms(ws, *dev)
    tab_norms = ws.table.cpu().numpy().copy()
    _hip.epsilon2_update(ws, *dev, xn.view(bsz, N), lam)
    torch.cuda.synchronize()
    assert _guards_intact(xbuf, bsz * N, offsets[3]) and _guards_intact(tbuf, bsz * 5) and _guards_intact(pbuf, part.numel())
    for t, v in zip(dev, (x, fx, ffx)):
        assert np.array_equal(t.cpu().numpy(), v)                                          # the inputs are read only
    return {"tab_norms": tab_norms, "tab": ws.table.cpu().numpy().copy(), "xn": xn.view(bsz, N).cpu().numpy().copy()}


def _close40(got, want, what):
    worst = float((np.abs(got - want) / (REL40 * np.abs(want) + 1e-300)).max())
    print(f"    {what}: worst error / (2^-40 relative) {worst:.4f}")
    assert worst <= 1.0, (what, worst)


def _check(o, x, fx, ffx, lam=1e-4):
    """Every stage of one step against float64 on what the stage read.  -> (worst sum error / bound, worst x_new error / bound, whether
    x_new equals the numpy float32 restatement bit for bit)."""
    dx, df = fx - x, ffx - fx                                                              # fp32, rounded as the reference's tensors are
    d2 = df - dx
    assert dx.dtype == df.dtype == d2.dtype == np.float32
    sq = lambda v: (v.astype(np.float64) ** 2).sum(1)
    tab = o["tab"]
    assert np.isnan(o["tab_norms"][:, 3:]).all() and np.array_equal(o["tab_norms"][:, :3], tab[:, :3])      # each call writes its own columns
    for col, v, what in ((0, dx, "sum dx^2"), (1, df, "sum df^2"), (2, d2, "sum d2^2")):
        _close40(tab[:, col], sq(v), what)
    # the update from the kernel's own fp32 a, b, c
    a, b = tab[:, 0].astype(np.float32)[:, None], tab[:, 1].astype(np.float32)[:, None]
    c = (tab[:, 2].astype(np.float32) + np.float32(lam))[:, None]
    assert c.dtype == np.float32
    a64, b64, c64, dx64, df64, fx64 = (v.astype(np.float64) for v in (a, b, c, dx, df, fx))
    want = fx64 + (df64 * a64 - dx64 * b64) / c64
    bound = 4 * U23 * (np.abs(fx64) + (np.abs(df64) * a64 + np.abs(dx64) * b64) / c64)
    worst = float((np.abs(o["xn"] - want) / (bound + 1e-300)).max())
    x32 = fx + (df * a - dx * b) / c
    assert x32.dtype == np.float32
    same = np.array_equal(o["xn"], x32)
    print(f"    x_new: worst error / bound {worst:.4f}; differs from the numpy float32 restatement in {int((o['xn'] != x32).sum())} of {x32.size} elements")
    assert worst <= 1.0, worst
    assert same
    step = o["xn"] - x
    assert step.dtype == np.float32
    _close40(tab[:, 3], sq(step), "sum (x_new - x)^2")
    _close40(tab[:, 4], sq(o["xn"]), "sum x_new^2")


def _chunk():
    return _hip.epsilon2_chunk()


N_KINDS = ["1", "3", "1200", "chunk-1", "chunk", "chunk+1", "2chunk+3"]


def _n(kind):
    c = _chunk()
    return {"1": 1, "3": 3, "1200": 1200, "chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "2chunk+3": 2 * c + 3}[kind]


@pytest.mark.parametrize("n_kind", N_KINDS)
@pytest.mark.parametrize("bsz", [1, 3])
def test_step_kernels_against_float64(bsz, n_kind):
    N = _n(n_kind)
    x, fx, ffx = _rows(bsz, N, 100 * bsz + len(n_kind) + N % 7)
    o = _run(x, fx, ffx)
    _check(o, x, fx, ffx)
    if bsz == 3:                                           # a sample's results do not depend on what else is in the batch
        for s in range(3):
            alone = _run(x[s:s + 1], fx[s:s + 1], ffx[s:s + 1])
            assert np.array_equal(alone["tab"][0], o["tab"][s]) and np.array_equal(alone["xn"][0], o["xn"][s]), s


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_step_kernels_scalar_path_gives_the_same_bits(which):
    """One row 4 bytes past a 16-byte boundary (x, f_x, f_fx or x_new) forces the element-by-element path: the same bits as the float4
    path, and held to float64 on its own.  N = 2 chunks + 1032: a multiple of 4, so only the base decides."""
    N = 2 * _chunk() + 1032
    x, fx, ffx = _rows(2, N, 5)
    base = _run(x, fx, ffx)
    off = [0, 0, 0, 0]
    off[which] = 1
    o = _run(x, fx, ffx, offsets=tuple(off))
    _check(o, x, fx, ffx)
    assert np.array_equal(base["tab"], o["tab"]) and np.array_equal(base["xn"], o["xn"])


def test_step_kernels_spike_at_every_chunk_seam():
    """An element 1e4 times the rest, one index at a time, on either side of every seam between two workgroups' chunks (and at both ends of
    the row): it is counted once, in float64, whichever thread, wave or workgroup it falls to."""
    c = _chunk()
    N = 2 * c + 3
    for at in (0, c - 1, c, 2 * c - 1, 2 * c, N - 1):
        print(f"  spike at {at}")
        x, fx, ffx = _rows(1, N, 40 + at % 11, spike_at=at)
        _check(_run(x, fx, ffx), x, fx, ffx)


def test_step_kernels_fixed_point_is_exact():
    """x = f_x = f_fx (one buffer for all three) and lam > 0: the sums are 0, x_new == f_x bit for bit and the residual is 0."""
    N = _chunk() + 5
    x = _rows(2, N, 8)[0]
    o = _run(x, x, x, lam=1e-4)
    assert np.array_equal(o["xn"], x) and not o["tab"][:, :4].any()
    _close40(o["tab"][:, 4], (x.astype(np.float64) ** 2).sum(1), "sum x_new^2")
    xd = torch.from_numpy(x).to(DEV)
    ws = _hip.Epsilon2Workspace(2, N, DEV)
    out = torch.empty_like(xd)
    _hip.epsilon2_norms(ws, xd, xd, xd)
    _hip.epsilon2_update(ws, xd, xd, xd, out, 1e-4)
    assert torch.equal(out, xd)
    with pytest.raises(_hip.DeqsciHipError, match="-4"):
        _hip.epsilon2_update(ws, xd, xd, xd, xd, 1e-4)     # x_new may alias none of the inputs
    got, res = deqsci_amd.epsilon2(lambda z: z, xd.view(2, N, 1, 1))
    assert res == 0.0 and torch.equal(got.view(2, N), xd) and deqsci_amd.epsilon2.last_info["f_calls"] == 2


def test_step_kernels_at_the_workload_row_length():
    """Launch geometry: bsz = 2, N = 256 x 256 x 8 (256 chunks per sample)."""
    x, fx, ffx = _rows(2, 256 * 256 * 8, 3)
    _check(_run(x, fx, ffx), x, fx, ffx)


# ----------------------------------------------------------------------------- the solver
@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "epsilon2_toy.npz")))


@pytest.fixture(scope="module")
def f64_runs(golden):
    out = {}
    for name in ef.CASES:
        f, shape, max_iter, tol, lam = ef.case_map(golden, name, torch.float64)
        out[name] = ef.epsilon2_f64(ef.as_numpy_map(f), golden[f"{name}/x0"], max_iter, tol, lam)
    return out


def _device_run(golden, name):
    f, shape, max_iter, tol, lam = ef.case_map(golden, name, torch.float32, DEV)
    seen = []

    def watched(x):
        seen.append(tuple(x.shape))
        return f(x)
    with torch.no_grad():
        x, res = deqsci_amd.epsilon2(watched, torch.from_numpy(golden[f"{name}/x0"]).to(DEV), max_iter=max_iter, tol=tol, lam=lam)
    return x, res, seen, dict(deqsci_amd.epsilon2.last_info)


@pytest.mark.parametrize("name", sorted(ef.CASES))
def test_solver_reproduces_the_float64_restatement(golden, f64_runs, name):
    x64, res64, info64 = f64_runs[name]
    x, res, seen, info = _device_run(golden, name)
    shape, (max_iter, tol, lam) = ef.MAPS[name][1], ef.CASES[name]
    dist = rel_l2(x.cpu().numpy(), x64)
    print(f"{name}: device vs float64 {dist:.3e} (reference vs float64 {float(golden[f'{name}/ref_vs_f64']):.3e}), f calls {info['f_calls']}, "
          f"res {res:.6e} (float64 {res64:.6e})")
    assert tuple(x.shape) == shape and x.dtype == torch.float32 and x.is_cuda
    assert set(seen) == {shape}                                                        # f's call shape is x0's
    assert dist <= max(10 * float(golden[f"{name}/ref_vs_f64"]), 1e-6)
    assert info["f_calls"] == len(seen) == info64["f_calls"] == int(golden[f"{name}/ref_f_calls"]) == 2 * info["iterations"]
    assert info["trace"][-1] == res and len(info["trace"]) == info["iterations"]
    if bool(golden[f"{name}/tol_stop"]):                                               # the stop happens where the golden says
        assert res < tol <= info["trace"][-2] and abs(res - res64) <= 0.01 * res64
    else:
        assert info["iterations"] == max_iter and res >= tol
    assert len(info["res_per_sample"]) == shape[0] and all(np.isfinite(v) for v in info["res_per_sample"])


def test_solver_is_deterministic_and_keeps_the_edge_behaviour(golden):
    a = _device_run(golden, "a")
    b = _device_run(golden, "a")
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[3]["trace"] == b[3]["trace"]
    calls = []
    with pytest.raises(UnboundLocalError, match="residual"):
        deqsci_amd.epsilon2(lambda z: calls.append(1) or z, torch.ones(1, 4, device=DEV), max_iter=0)
    assert not calls
    with pytest.raises(ZeroDivisionError):
        deqsci_amd.epsilon2(lambda z: torch.zeros_like(z), torch.zeros(2, 3, 4, device=DEV), max_iter=5)
    x, res = deqsci_amd.epsilon2(lambda z: z * float("nan"), torch.ones(2, 3, 4, device=DEV), max_iter=3)
    assert np.isnan(res) and deqsci_amd.epsilon2.last_info["f_calls"] == 6 and bool(torch.isnan(x).all())


# ----------------------------------------------------------------------------- through the stack
def _crop(size=32):
    from deqsci_amd.harness import load_test_data
    d = load_test_data(os.path.join(ROOT, "data", "test_gray", "traffic_cacti.mat"))
    sl = (slice(96, 96 + size), slice(64, 64 + size))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"][sl]))[None]
    y = torch.from_numpy(np.ascontiguousarray(d["meas"][sl][..., 0]))[None]
    return y, Phi


def _deq(max_iter=6, tol=1e-9, lam=1e-4):
    solver, _ = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), max_iter)
    return solver, deqsci_amd.DEQFixedPoint(solver, deqsci_amd.epsilon2, max_iter=max_iter, tol=tol, lam=lam)


def test_deq_forward_against_the_torch_loop():
    """DEQFixedPoint(..., epsilon2, max_iter=6, tol=1e-9, lam=1e-4), SimpleCNN on a 32 x 32 x 8 crop: 12 f-calls of the solver and the
    wrapper's two, and the same reconstruction as the loop written with torch expressions on the device, to 1e-5 relative L2."""
    y, Phi = _crop()
    solver, deq = _deq()
    dy, dPhi = y.to(DEV), Phi.to(DEV)
    dPs = deqsci_amd.phi_sum(dPhi)
    x0 = deqsci_amd.initial_point(dy, dPhi, dPs, None)
    count = [0]
    hook = solver.register_forward_hook(lambda *a: count.__setitem__(0, count[0] + 1))
    with torch.no_grad():
        rec = deq.forward(dy, dPhi, dPs, initial_point=x0, train_flag=False)
    hook.remove()
    info = deqsci_amd.epsilon2.last_info
    assert deq._engine is None and isinstance(deq.forward_res, float)
    assert info["f_calls"] == 12 and info["iterations"] == 6 and count[0] == 12 + 2

    def l2(t):
        return torch.sum(t ** 2, dim=[1, 2, 3], keepdim=True)
    with torch.no_grad():
        f = lambda z: solver(z, dy, dPhi, dPs)
        x = x0
        for _ in range(6):
            f_x = f(x)
            dx = f_x - x
            df = f(f_x) - f_x
            d2 = df - dx
            x_new = f_x + (df * l2(dx) - dx * l2(df)) / (l2(d2) + 1e-4)
            res = (x_new - x).norm().item() / x_new.norm().item()
            x = x_new
        want = f(x)
    dist = rel_l2(rec.cpu().numpy(), want.cpu().numpy())
    print(f"DEQFixedPoint + epsilon2, SimpleCNN 32x32x8: rel-L2 vs the torch loop {dist:.3e}, res {deq.forward_res:.4e} (torch loop {res:.4e})")
    assert tuple(rec.shape) == tuple(Phi.shape) and dist <= 1e-5


def test_deq_implicit_backward_device_against_autograd():
    """The taped forward and its hook with epsilon2 as the solver of g = J^T g + grad, J^T v by the HIP kernels and by autograd: two
    evaluations of the same products that differ by fp32 rounding (1e-6), through the same 6 iterations; held to the 1e-4 that holds the
    same comparison with Broyden's method."""
    y, Phi = _crop()
    grads = {}
    for mode in ("device", "autograd"):
        solver, deq = _deq()
        deq.implicit_backward = mode
        dy, dPhi = y.to(DEV).requires_grad_(), Phi.to(DEV)
        dPs = deqsci_amd.phi_sum(dPhi)
        rec = deq(dy, dPhi, dPs, initial_point=deqsci_amd.initial_point(dy.detach(), dPhi, dPs, None))
        rec.square().mean().backward()
        assert deq.last_backward_path == mode and deq.backward_fallback_reason is None
        assert isinstance(deq.backward_res, float) and np.isfinite(deq.backward_res)
        assert deqsci_amd.epsilon2.last_info["f_calls"] == 12
        grads[mode] = (dy.grad.cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in solver.named_parameters()})
    dist = rel_l2(grads["device"][0], grads["autograd"][0])
    print(f"implicit backward with epsilon2: input gradient, device vs autograd {dist:.3e}")
    assert np.abs(grads["autograd"][0]).max() > 0 and dist <= 1e-4
    for k, gk in grads["autograd"][1].items():
        assert rel_l2(grads["device"][1][k], gk) <= 1e-4, k


def test_cli_runs_epsilon2_end_to_end(tmp_path, capsys):
    from deqsci_amd.cli import main as cli_main
    clips = tmp_path / "clips"
    clips.mkdir()
    shutil.copy(os.path.join(ROOT, "data", "test_gray", "drop8_cacti.mat"), clips / "drop8_cacti.mat")
    avg = cli_main(["--denoiser", "SimpleCNN", "--testpath", str(clips) + "/", "--savepath", str(tmp_path / "out") + "/", "--solver", "epsilon2",
                    "--and_maxiters", "4", "--inference", "True"])
    out = capsys.readouterr().out
    info = deqsci_amd.epsilon2.last_info
    print(out)
    assert "solver: epsilon2 (lam=0.0001, max_iter=4, tol=0.01)" in out and "Total Average PSNR" in out and "drop8_cacti.mat" in out
    assert np.isfinite(avg) and 1 <= info["iterations"] <= 4 and info["f_calls"] == 2 * info["iterations"]
    assert os.listdir(tmp_path / "out")
