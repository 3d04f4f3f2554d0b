"""CPU: Broyden's method - the float64 restatement (tests/broyden_f64.py) against the reference's own runs (tests/golden/broyden_toy.npz,
made by tests/golden/make_broyden_golden.py), the C ABI's argument validation, and the command line."""
import ctypes
import os

import numpy as np
import pytest
import torch

import broyden_f64 as bf
from conftest import GOLDEN, rel_l2


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "broyden_toy.npz")))


@pytest.mark.parametrize("name", sorted(bf.CASES))
def test_float64_restatement_reproduces_the_reference(golden, name):
    f, shape, threshold, eps = bf.case_map(golden, name, torch.float64)
    x, res, info = bf.broyden_f64(bf.as_g_numpy(f, shape), golden[f"{name}/x0"], threshold, eps)
    dist = rel_l2(golden[f"{name}/ref_x"], x)
    print(f"{name}: ref vs float64 {dist:.3e} (stored {float(golden[f'{name}/ref_vs_f64']):.3e}), g calls {info['g_calls']}, res {res:.6e}")
    assert dist <= max(10 * float(golden[f"{name}/ref_vs_f64"]), 1e-7)
    assert info["g_calls"] == int(golden[f"{name}/ref_g_calls"])
    if bool(golden[f"{name}/eps_stop"]):
        assert res < eps and abs(res - float(golden[f"{name}/ref_res"])) <= 0.01 * float(golden[f"{name}/ref_res"])


def test_golden_holds_its_conditions(golden):
    """What make_broyden_golden.py asserted when it wrote the file: equal g-call counts, an eps stop in b and d, and a wrap in d."""
    for name in bf.CASES:
        assert int(golden[f"{name}/ref_g_calls"]) == int(golden[f"{name}/f64_g_calls"])
        assert tuple(golden[f"{name}/x0"].shape) == bf.CASES[name][1]
    assert bool(golden["b/eps_stop"]) and bool(golden["d/eps_stop"]) and not bool(golden["a/eps_stop"])
    assert int(golden["a/ref_g_calls"]) == 13                          # all 12 steps
    assert int(golden["d/ref_g_calls"]) - 1 > bf.MAX_L + 1             # rows 0.. are rewritten and used
    assert golden["c/x0"][0].size == 1200


def test_cabi_validation_codes():
    from deqsci_amd import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 4096)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    U, V, dx, g0, g1, x, xn, up, tab, ws = (p16 + 1024 * k for k in range(10))      # ten disjoint 1 KiB regions

    def dots(U=U, V=V, dx=dx, g0=g0, g1=g1, tab=tab, ws=ws, bsz=1, N=8, L=3, t=1):
        return lib.deqsci_broyden_dots_f32(U, V, dx, g0, g1, tab, ws, bsz, N, L, t, None)

    def update(U=U, V=V, dx=dx, g0=g0, g1=g1, x=x, xn=xn, up=up, tab=tab, ws=ws, bsz=1, N=8, L=3, t=1, slot=1):
        return lib.deqsci_broyden_update_f32(U, V, dx, g0, g1, x, xn, up, tab, ws, bsz, N, L, t, slot, None)
    # NULL
    for k in ("U", "V", "dx", "g0", "g1", "tab", "ws"):
        assert dots(**{k: None}) == -1 and update(**{k: None}) == -1, k
    assert update(up=None) == -1 and update(x=None) == -1               # x_next without x
    # sizes
    for kw in (dict(bsz=0), dict(bsz=-1), dict(N=0), dict(L=0), dict(L=28, t=0), dict(t=4), dict(t=-1)):
        assert dots(**kw) == -2 and update(**{**kw, "slot": 0}) == -2, kw
    assert update(slot=3) == -2 and update(slot=-1) == -2 and update(t=0, slot=1) == -2       # slot >= L; rows t .. slot - 1 were never filled
    assert update(t=2, slot=1) == -2 and update(t=2, slot=0) == -2                             # slot < t only once the history is full (t == L)
    assert lib.deqsci_broyden_dots_f32(None, None, None, None, None, None, None, 1, 8, 28, 0, None) == -1      # NULL is checked first
    # misaligned
    assert dots(U=U + 2) == -3 and dots(g1=g1 + 1) == -3 and dots(tab=tab + 4) == -3 and dots(ws=ws + 4) == -3
    assert update(up=up + 2) == -3 and update(xn=xn + 3) == -3 and update(tab=tab + 4) == -3
    # unsupported
    assert dots(bsz=70000) == -4 and update(bsz=70000) == -4
    assert update(up=U + 32) == -4 and update(up=V) == -4 and update(xn=U) == -4 and update(dx=V + 32) == -4       # aliasing with a history row
    assert update(up=xn) == -4
    # the workspace
    assert lib.deqsci_broyden_workspace_bytes(0, 1024, 27) == 0 and lib.deqsci_broyden_workspace_bytes(1, 0, 27) == 0
    assert lib.deqsci_broyden_workspace_bytes(1, (1 << 28) + 1, 1) == 0 and dots(N=(1 << 28) + 1) == -4 and update(N=(1 << 28) + 1) == -4
    assert lib.deqsci_broyden_workspace_bytes(1, 1024, 28) == 0 and lib.deqsci_broyden_workspace_bytes(1, 1024, 0) == 0
    chunk = _hip.broyden_chunk()
    assert chunk > 0 and chunk % 4 == 0
    assert lib.deqsci_broyden_workspace_bytes(8, 256 * 256 * 8, 27) == 8 * (256 * 256 * 8 // chunk) * _hip.BROYDEN_TABLE_STRIDE * 8
    assert lib.deqsci_broyden_workspace_bytes(1, chunk + 1, 1) == 2 * _hip.BROYDEN_TABLE_STRIDE * 8
    assert _hip.BROYDEN_CNEW + 1 == _hip.BROYDEN_TABLE_STRIDE and _hip.BROYDEN_GG == 3 * _hip.BROYDEN_MAX_L


def test_line_search_is_refused():
    import deqsci_amd
    with pytest.raises(NotImplementedError, match="line search"):
        deqsci_amd.broyden(lambda x: x, torch.zeros(1, 4), ls=True)


def test_cli_builds_the_chosen_solver():
    import deqsci_amd
    from deqsci_amd import cli
    args = cli.parser().parse_args(["--solver", "broyden", "--denoiser", "SimpleCNN", "--and_maxiters", "40", "--broyden_eps", "1e-4"])
    assert args.solver == "broyden" and args.broyden_threshold is None and args.broyden_eps == 1e-4
    _, deq = cli.build_pipeline(args.denoiser, None, args.and_maxiters, args.and_m, args.and_beta, device="cpu", solver_name=args.solver,
                                broyden_threshold=args.broyden_threshold, broyden_eps=args.broyden_eps)
    assert deq.solver is deqsci_amd.broyden_fixed_point and deq.kwargs == {"threshold": 40, "eps": 1e-4}
    assert deq._engine_for() is None                                    # the generic path
    args = cli.parser().parse_args(["--solver", "broyden", "--broyden_threshold", "15"])
    _, deq = cli.build_pipeline("SimpleCNN", None, args.and_maxiters, device="cpu", solver_name=args.solver, broyden_threshold=args.broyden_threshold,
                                broyden_eps=args.broyden_eps)
    assert deq.kwargs == {"threshold": 15, "eps": 1e-5}
    from deqsci_amd.harness import solver_line
    assert solver_line(deq) == "solver: broyden_fixed_point (eps=1e-05, threshold=15)"
    args = cli.parser().parse_args([])
    assert args.solver == "anderson"
    _, deq = cli.build_pipeline("SimpleCNN", None, 30, device="cpu")
    assert deq.solver is deqsci_amd.andersonexp and deq.kwargs == {"m": 5, "beta": 1.0, "lam": 1e-2, "max_iter": 30, "tol": 1e-5}
    with pytest.raises(ValueError):
        cli.build_pipeline("SimpleCNN", None, 30, device="cpu", solver_name="neumann")


@pytest.mark.parametrize("extra", [["--snapshots", "10"], ["--trace", "t.json"]])
def test_cli_refuses_engine_extras_with_broyden(extra, capsys):
    from deqsci_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--solver", "broyden"] + extra)
    assert e.value.code == 2
    assert "not available with --solver broyden" in capsys.readouterr().err            # the parse-time rule, not argparse's own refusals
    args = cli.parser().parse_args(["--solver", "broyden"])                             # ... and without the extras it parses
    assert args.solver == "broyden" and args.snapshots is None and args.trace is None


def test_engine_only_message_names_the_solver():
    from deqsci_amd import cli
    _, deq = cli.build_pipeline("SimpleCNN", None, 10, device="cpu", solver_name="broyden")
    deq.snapshots = (5,)
    y = torch.zeros(1, 8, 8)
    with pytest.raises(NotImplementedError, match="broyden_fixed_point"), torch.no_grad():
        deq.forward(y, torch.ones(1, 8, 8, 4), torch.ones(1, 8, 8), initial_point=torch.zeros(1, 8, 8, 4), train_flag=False)
