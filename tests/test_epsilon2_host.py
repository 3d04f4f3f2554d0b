"""CPU: the vector epsilon-algorithm - the float64 restatement (tests/epsilon2_f64.py) against the reference's own runs
(tests/golden/epsilon2_toy.npz, made by tests/golden/make_epsilon2_golden.py), the C ABI's argument validation, the command line, and
the reference's edge behaviour on the host path of deqsci_amd.epsilon2."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import epsilon2_f64 as ef
from conftest import GOLDEN, ROOT, rel_l2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "epsilon2_toy.npz")))


@pytest.mark.parametrize("name", sorted(ef.CASES))
def test_float64_restatement_reproduces_the_reference(golden, name):
    f, shape, max_iter, tol, lam = ef.case_map(golden, name, torch.float64)
    x, res, info = ef.epsilon2_f64(ef.as_numpy_map(f), golden[f"{name}/x0"], max_iter, tol, lam)
    dist = rel_l2(golden[f"{name}/ref_x"], x)
    print(f"{name}: ref vs float64 {dist:.3e} (stored {float(golden[f'{name}/ref_vs_f64']):.3e}), f calls {info['f_calls']}, res {res:.6e}")
    assert dist <= max(10 * float(golden[f"{name}/ref_vs_f64"]), 1e-7)
    assert info["f_calls"] == int(golden[f"{name}/ref_f_calls"])
    if bool(golden[f"{name}/tol_stop"]):
        assert res < tol and abs(res - float(golden[f"{name}/ref_res"])) <= 0.01 * float(golden[f"{name}/ref_res"])


def test_golden_holds_its_conditions(golden):
    """What make_epsilon2_golden.py asserted when it wrote the file: equal f-call counts, and every tol stop more than 1 % of tol away
    from tol at the stopping iteration and at the one before."""
    for name, (max_iter, tol, lam) in ef.CASES.items():
        assert int(golden[f"{name}/ref_f_calls"]) == int(golden[f"{name}/f64_f_calls"])
        assert tuple(golden[f"{name}/x0"].shape) == ef.MAPS[name][1]
        assert (int(golden[f"{name}/max_iter"]), float(golden[f"{name}/tol"]), float(golden[f"{name}/lam"])) == (max_iter, tol, lam)
        if bool(golden[f"{name}/tol_stop"]):
            last, before = float(golden[f"{name}/f64_res"]), float(golden[f"{name}/f64_res_before"])
            assert last < tol and abs(last - tol) > 0.01 * tol and abs(before - tol) > 0.01 * tol and before >= tol
        assert 0 < float(golden[f"{name}/ref_vs_f64"]) < 1e-6
    assert not bool(golden["a/tol_stop"]) and all(bool(golden[f"{n}/tol_stop"]) for n in "bcd")
    assert [int(golden[f"{n}/ref_f_calls"]) for n in "abcd"] == [24, 12, 8, 68]          # a: all 12 iterations
    assert golden["c/x0"][0].size == 1200


@pytest.mark.parametrize("name", sorted(ef.CASES))
def test_host_path_follows_the_float64_restatement(golden, name):
    """deqsci_amd.epsilon2 on CPU tensors (the torch restatement with float64 sums) against float64: the reference's own distance."""
    import deqsci_amd
    f64, shape, max_iter, tol, lam = ef.case_map(golden, name, torch.float64)
    x64, res64, info64 = ef.epsilon2_f64(ef.as_numpy_map(f64), golden[f"{name}/x0"], max_iter, tol, lam)
    f32 = ef.case_map(golden, name, torch.float32)[0]
    with torch.no_grad():
        x, res = deqsci_amd.epsilon2(f32, torch.from_numpy(golden[f"{name}/x0"]), max_iter=max_iter, tol=tol, lam=lam)
    info = deqsci_amd.epsilon2.last_info
    assert tuple(x.shape) == shape and x.dtype == torch.float32
    assert rel_l2(x.numpy(), x64) <= max(10 * float(golden[f"{name}/ref_vs_f64"]), 1e-6)
    assert info["f_calls"] == info64["f_calls"] == 2 * info["iterations"] and len(info["trace"]) == info["iterations"]
    assert info["trace"][-1] == res and len(info["res_per_sample"]) == shape[0]


def test_cabi_validation_codes():
    from deqsci_amd import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 4096)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    x, fx, ffx, xn, tab, ws = (p16 + 1024 * k for k in range(6))        # six disjoint 1 KiB regions

    def norms(x=x, fx=fx, ffx=ffx, tab=tab, ws=ws, bsz=1, N=8):
        return lib.deqsci_epsilon2_norms_f32(x, fx, ffx, tab, ws, bsz, N, None)

    def update(x=x, fx=fx, ffx=ffx, xn=xn, tab=tab, ws=ws, bsz=1, N=8, lam=1e-4):
        return lib.deqsci_epsilon2_update_f32(x, fx, ffx, xn, tab, ws, bsz, N, lam, None)
    # NULL
    for k in ("x", "fx", "ffx", "tab", "ws"):
        assert norms(**{k: None}) == -1 and update(**{k: None}) == -1, k
    assert update(xn=None) == -1
    assert lib.deqsci_epsilon2_norms_f32(None, None, None, None, None, 0, 0, None) == -1            # NULL is checked first
    # sizes
    for kw in (dict(bsz=0), dict(bsz=-1), dict(N=0), dict(N=-4), dict(N=(1 << 28) + 1)):
        assert norms(**kw) == -2 and update(**kw) == -2, kw
    assert norms(bsz=0, x=x + 2) == -2                                   # ... before alignment
    # misaligned
    assert norms(x=x + 2) == -3 and norms(ffx=ffx + 1) == -3 and norms(tab=tab + 4) == -3 and norms(ws=ws + 4) == -3
    assert update(xn=xn + 3) == -3 and update(fx=fx + 2) == -3 and update(tab=tab + 4) == -3 and update(ws=ws + 4) == -3
    assert update(bsz=70000, xn=xn + 2) == -3                            # ... before the unsupported cases
    # unsupported
    assert norms(bsz=70000) == -4 and update(bsz=70000) == -4
    assert update(xn=x) == -4 and update(xn=fx) == -4 and update(xn=ffx) == -4 and update(xn=x + 28) == -4 and update(xn=ffx - 28) == -4
    assert update(bsz=2, N=8, xn=x + 32) == -4                           # sample 0 of x_new is sample 1 of x
    # the workspace
    wsb = lib.deqsci_epsilon2_workspace_bytes
    assert wsb(0, 1024) == 0 and wsb(1, 0) == 0 and wsb(1, (1 << 28) + 1) == 0 and wsb(70000, 1024) == 0
    chunk = _hip.epsilon2_chunk()
    assert chunk > 0 and chunk % 4 == 0
    assert wsb(8, 256 * 256 * 8) == 8 * (256 * 256 * 8 // chunk) * 3 * 8
    assert wsb(1, chunk) == 3 * 8 and wsb(1, chunk + 1) == 2 * 3 * 8 and wsb(1, 1 << 28) == ((1 << 28) // chunk) * 3 * 8
    assert _hip.EPSILON2_NEW + 1 == _hip.EPSILON2_TABLE_STRIDE == 5
    hdr = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    assert "#define DEQSCI_EPSILON2_TABLE_STRIDE 5" in hdr


def test_cli_builds_the_chosen_solver():
    import deqsci_amd
    from deqsci_amd import cli
    from deqsci_amd.harness import solver_line
    args = cli.parser().parse_args(["--solver", "epsilon2", "--denoiser", "SimpleCNN", "--and_maxiters", "7", "--eps2_tol", "1e-3", "--eps2_lam", "1e-6"])
    assert args.solver == "epsilon2" and args.eps2_tol == 1e-3 and args.eps2_lam == 1e-6
    _, deq = cli.build_pipeline(args.denoiser, None, args.and_maxiters, args.and_m, args.and_beta, device="cpu", solver_name=args.solver,
                                eps2_tol=args.eps2_tol, eps2_lam=args.eps2_lam)
    assert deq.solver is deqsci_amd.epsilon2 and deq.kwargs == {"max_iter": 7, "tol": 1e-3, "lam": 1e-6}
    assert deq._engine_for() is None                                    # the generic path
    assert solver_line(deq) == "solver: epsilon2 (lam=1e-06, max_iter=7, tol=0.001)"
    args = cli.parser().parse_args(["--solver", "epsilon2"])
    assert (args.eps2_tol, args.eps2_lam) == (1e-2, 1e-4)
    _, deq = cli.build_pipeline("SimpleCNN", None, args.and_maxiters, device="cpu", solver_name="epsilon2")
    assert deq.kwargs == {"max_iter": 100, "tol": 1e-2, "lam": 1e-4}
    # picard: forward_iteration on the engine
    args = cli.parser().parse_args(["--solver", "picard", "--and_maxiters", "25", "--snapshots", "5,10"])
    assert args.solver == "picard" and args.snapshots == (5, 10)
    _, deq = cli.build_pipeline("SimpleCNN", None, args.and_maxiters, device="cpu", solver_name=args.solver)
    assert deq.solver is deqsci_amd.forward_iteration and deq.kwargs == {"max_iter": 25, "tol": 1e-5}
    assert solver_line(deq) == "solver: forward_iteration (max_iter=25, tol=1e-05)"
    # the default stays what it is
    args = cli.parser().parse_args([])
    assert args.solver == "anderson"
    _, deq = cli.build_pipeline("SimpleCNN", None, 30, device="cpu")
    assert deq.solver is deqsci_amd.andersonexp and deq.kwargs == {"m": 5, "beta": 1.0, "lam": 1e-2, "max_iter": 30, "tol": 1e-5}
    with pytest.raises(ValueError):
        cli.build_pipeline("SimpleCNN", None, 30, device="cpu", solver_name="neumann")


def test_cli_help_lists_the_new_flags():
    """(--help formats every help string with %: a bare per-cent sign in one of them used to make it raise)"""
    from deqsci_amd import cli
    text = cli.parser().format_help()
    assert "--eps2_tol" in text and "--eps2_lam" in text and "{anderson,broyden,epsilon2,picard}" in text and "4 % faster" in text


@pytest.mark.parametrize("extra", [["--snapshots", "10"], ["--trace", "t.json"]])
def test_cli_refuses_engine_extras_with_epsilon2(extra, capsys):
    from deqsci_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--solver", "epsilon2"] + extra)
    assert e.value.code == 2
    assert "not available with --solver epsilon2" in capsys.readouterr().err           # the parse-time rule, not argparse's own refusals
    args = cli.parser().parse_args(["--solver", "epsilon2"])                            # ... and without the extras it parses
    assert args.solver == "epsilon2" and args.snapshots is None and args.trace is None


def test_cli_picard_snapshots_follow_the_picard_rule(capsys):
    """Picard can stop at horizon 1; Anderson's smallest is 3.  (Both refusals come before any device is touched.)"""
    from deqsci_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--solver", "anderson", "--and_maxiters", "10", "--snapshots", "1"])
    assert "smallest horizon" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cli.main(["--solver", "picard", "--and_maxiters", "10", "--snapshots", "0"])
    assert "smallest horizon of the picard iteration is 1" in str(e.value.code)


def test_unexpected_keyword_fails():
    import deqsci_amd
    from deqsci_amd import cli
    solver, _ = cli.build_pipeline("SimpleCNN", None, 5, device="cpu")
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.epsilon2, max_iter=2, m=5)
    assert deq._engine_for() is None
    with pytest.raises(TypeError, match="unexpected keyword argument 'm'"), torch.no_grad():
        deq.forward(torch.zeros(1, 8, 8), torch.ones(1, 8, 8, 4), torch.ones(1, 8, 8), initial_point=torch.zeros(1, 8, 8, 4), train_flag=False)


def test_engine_only_message_on_the_generic_path():
    from deqsci_amd import cli
    _, deq = cli.build_pipeline("SimpleCNN", None, 10, device="cpu", solver_name="epsilon2")
    deq.snapshots = (5,)
    with pytest.raises(NotImplementedError, match="engine's path only"), torch.no_grad():
        deq.forward(torch.zeros(1, 8, 8), torch.ones(1, 8, 8, 4), torch.ones(1, 8, 8), initial_point=torch.zeros(1, 8, 8, 4), train_flag=False)


# ----------------------------------------------------------------------------- the reference's edge behaviour, host path
def test_no_iteration_raises_unbound_local_error():
    import deqsci_amd
    calls = []
    for max_iter in (0, -3):
        with pytest.raises(UnboundLocalError, match="residual"):
            deqsci_amd.epsilon2(lambda x: calls.append(1) or x, torch.ones(1, 4), max_iter=max_iter)
    assert not calls


def test_zero_iterate_raises_zero_division_error():
    import deqsci_amd
    with pytest.raises(ZeroDivisionError):
        deqsci_amd.epsilon2(lambda x: torch.zeros_like(x), torch.zeros(2, 3, 4), max_iter=5)


def test_non_finite_residual_does_not_stop_the_loop():
    import deqsci_amd
    calls = []

    def f(x):
        calls.append(tuple(x.shape))
        return x * float("nan")
    x, res = deqsci_amd.epsilon2(f, torch.ones(2, 3, 4), max_iter=4, tol=1e-2)
    assert math.isnan(res) and len(calls) == 8 and set(calls) == {(2, 3, 4)} and bool(torch.isnan(x).all())
    assert deqsci_amd.epsilon2.last_info["iterations"] == 4 and all(math.isnan(v) for v in deqsci_amd.epsilon2.last_info["trace"])


def test_fixed_point_and_shapes_on_the_host_path():
    """x = f(x): dx = df = 0, so x_new = f_x exactly and the residual is 0 - one iteration, two calls.  Any x0 of two or more
    dimensions; one dimension is refused."""
    import deqsci_amd
    for shape in ((3, 5), (2, 3, 4), (2, 2, 3, 2, 2)):
        x0 = torch.randn(*shape, generator=torch.Generator().manual_seed(1))
        x, res = deqsci_amd.epsilon2(lambda z: z.clone(), x0)
        assert res == 0.0 and torch.equal(x, x0) and deqsci_amd.epsilon2.last_info["f_calls"] == 2
        assert deqsci_amd.epsilon2.last_info["res_per_sample"] == [0.0] * shape[0]
    with pytest.raises(ValueError, match="at least one more"):
        deqsci_amd.epsilon2(lambda z: z, torch.ones(4))
