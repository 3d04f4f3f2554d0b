"""CPU: the Jacobian diagnostics' host statements (deqsci_amd/vjp.py plan_jvp / plan_vjp / ffdnet_plan_*, deqsci_amd/jacobian.py
power_report_host) in float64 against tests/golden/jacobian.npz (the reference's Jacobian: tests/golden/make_golden_jacobian.py) and
torch.autograd.functional, the interface's refusals, the C ABI's argument checks and the register report of csrc/jacobian.hip."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, rel_l2
from deqsci_amd import checkpoint, jacobian, vjp
from deqsci_amd.cli import SHIPPED, build_denoiser, build_pipeline, parser

CASES = {"SimpleCNN": "SimpleCNN", "RealSN_SimpleCNN": "RealSN_SimpleCNN", "ffdnet_s0": "ffdnet", "ffdnet_s1": "ffdnet"}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "jacobian.npz"))


def _net(case):
    kind = CASES.get(case, case)
    solver, _ = build_pipeline(kind, checkpoint.shipped(SHIPPED[kind]), device="cpu")
    return solver.nonlinear_op.eval().double()              # (float64 before the plan folds the BatchNorm)


def _op(gold, case, part, **kw):
    g = lambda k: torch.from_numpy(np.asarray(gold[f"{case}/{part}_{k}"], dtype=np.float64))
    sigma = float(gold[f"{case}/{part}_sigma"]) if CASES[case] == "ffdnet" else None
    return jacobian.HostMapJacobian(_net(case), g("z"), g("y"), g("Phi"), g("Phi_sum"), sigma=sigma, **kw), g


@pytest.mark.parametrize("case", list(CASES))
def test_products_against_the_reference(gold, case):
    op, g = _op(gold, case, "a")
    Jv = op.jv(g("v"))
    assert rel_l2(Jv, g("Jv")) <= 1e-9
    JTw = op.jtv(g("w"))
    if CASES[case] != "ffdnet":                    # the reference's own autograd; FFDNet's returns zero, its transpose is pinned by the dense case
        assert rel_l2(JTw, g("JTw")) <= 1e-9
    lhs, rhs = float((g("w") * Jv).sum()), float((JTw * g("v")).sum())
    assert abs(lhs - rhs) <= 1e-9 * float(g("w").norm() * Jv.norm())
    assert abs(lhs - float(gold[f"{case}/a_wJv"])) <= 1e-9 * float(g("w").norm() * Jv.norm())


@pytest.mark.parametrize("case", list(CASES))
def test_products_against_the_dense_jacobian_and_its_transpose(gold, case):
    op, g = _op(gold, case, "b")
    P = g("probes")
    bsz, H, W, B = op.shape
    for k in range(P.shape[1]):
        v = P[:, k].reshape(op.shape)
        assert rel_l2(op.jv(v).reshape(-1), g("J_probes")[:, k]) <= 1e-9
        assert rel_l2(op.jtv(v).reshape(-1), g("JT_probes")[:, k]) <= 1e-9
        x = P[:, k].reshape(bsz * B, 1, H, W)
        assert rel_l2(op.denoiser.jvp(x).reshape(-1), g("JD_probes")[:, k]) <= 1e-9
        assert rel_l2(op.denoiser.vjp(x).reshape(-1), g("JDT_probes")[:, k]) <= 1e-9


@pytest.mark.parametrize("kind", ["SimpleCNN", "RealSN_SimpleCNN", "ffdnet"])
def test_plans_equal_autograd_functional_on_random_inputs(kind):
    net = _net(kind)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 1, 12, 10, generator=g, dtype=torch.float64)
    v, w = (torch.randn(2, 1, 12, 10, generator=g, dtype=torch.float64) for _ in range(2))
    if kind == "ffdnet":
        L, sg = vjp.ffdnet_plan(net), 0.17
        f = lambda t: vjp.ffdnet_plan_forward(L, t, sg)[0]
        assert rel_l2(f(x).detach(), net(x, torch.full((2,), sg, dtype=torch.float64)).detach()) <= 1e-12
        jv, jtw = vjp.ffdnet_plan_jvp(L, x, sg, v)[0], vjp.ffdnet_plan_vjp(L, x, sg, w)[0]
    else:
        L, _ = vjp.host_plan(net)
        f = net
        jv, jtw = vjp.plan_jvp(L, x, v)[0], vjp.plan_vjp(L, x, w)[0]
    assert rel_l2(jv, torch.autograd.functional.jvp(f, x, v)[1].detach()) <= 1e-12
    assert rel_l2(jtw, torch.autograd.functional.vjp(f, x, w)[1].detach()) <= 1e-12


def test_ffdnet_plan_refuses_odd_sizes():
    L = vjp.ffdnet_plan(_net("ffdnet"))
    x = torch.zeros(1, 1, 7, 8, dtype=torch.float64)
    for fn in (vjp.ffdnet_plan_jvp, vjp.ffdnet_plan_vjp):
        with pytest.raises(ValueError, match="even"):
            fn(L, x, 0.1, x)


@pytest.mark.parametrize("case", list(CASES))
def test_power_report_host_on_the_dense_case(gold, case):
    op, g = _op(gold, case, "b")
    n_iters, window = int(gold[f"{case}/b_n_iters"]), int(gold[f"{case}/b_window"])
    rep = jacobian.power_report_host(op, op.shape, n_iters=n_iters, window=window, seed=0)
    for mine, theirs in (("lipschitz_f_history", "lip_hist"), ("rho_f_growth", "growth"), ("rho_f_rayleigh", "rayleigh"),
                         ("lipschitz_denoiser_history", "lipd_hist")):
        assert rep[mine].shape == (n_iters, 1)
        assert rel_l2(rep[mine][:, 0], gold[f"{case}/b_{theirs}"]) <= 1e-9, mine
    assert abs(rep["rho_f"][0] - float(gold[f"{case}/b_rho"])) <= 1e-9 * float(gold[f"{case}/b_rho"])
    for key, sv in (("lipschitz_f", "svd_J"), ("lipschitz_denoiser", "svd_JD")):
        smax = float(gold[f"{case}/b_{sv}"][0])
        assert 0.99 * smax <= rep[key][0] <= smax * (1 + 1e-9), (key, rep[key][0], smax)
        h = rep[key + "_history"][:, 0]
        assert np.all(np.diff(h) >= -1e-12 * smax), key            # non-decreasing
    # the golden's own numbers hang together: rho <= sigma_max
    rho_dense = np.abs(gold[f"{case}/b_eig_J_re"] + 1j * gold[f"{case}/b_eig_J_im"]).max()
    assert rho_dense <= float(gold[f"{case}/b_svd_J"][0]) * (1 + 1e-12)


def test_power_report_is_per_sample_and_reports_nan_for_a_dead_sample(gold):
    """Two samples, the second with an all-zero Jacobian for f (Phi_sum trick: P = 0 is not available, so a zero map is used)."""
    class Op:
        class denoiser:
            jvp = staticmethod(lambda v: 0.5 * v)
            vjp = staticmethod(lambda v: 0.5 * v)
        scale = torch.tensor([2.0, 0.0], dtype=torch.float64).view(2, 1, 1, 1)
        jv = classmethod(lambda c, v: v * c.scale)
        jtv = classmethod(lambda c, v: v * c.scale)
    rep = jacobian.power_report_host(Op, (2, 4, 4, 2), n_iters=5, window=2)
    assert rep["lipschitz_f"][0] == pytest.approx(2.0, rel=1e-12) and rep["rho_f"][0] == pytest.approx(2.0, rel=1e-12)
    assert np.isnan(rep["lipschitz_f"][1]) and np.isnan(rep["rho_f"][1])
    assert np.allclose(rep["lipschitz_denoiser"], 0.5, rtol=1e-12)
    with pytest.raises(ValueError, match="window"):
        jacobian.power_report_host(Op, (2, 4, 4, 2), n_iters=5, window=6)
    with pytest.raises(ValueError, match="of="):
        jacobian.power_report_host(Op, (2, 4, 4, 2), of=("g",))


def test_interface_flags_defaults_and_refusals():
    from deqsci_amd import DEQFixedPoint, andersonexp, harness
    from deqsci_amd.networks import DnCNN, FFDNet
    from deqsci_amd.operators import A_torch_, At_torch_
    from deqsci_amd.solvers import EquilibriumProxGradSCI
    p = parser()
    d = p.parse_args([])
    assert d.jacobian is None and d.jacobian_json is None
    assert p.parse_args(["--jacobian"]).jacobian == 30 and p.parse_args(["--jacobian", "12"]).jacobian == 12
    assert p.parse_args(["--jacobian_json", "x.json"]).jacobian_json == "x.json"
    # the hook's view of FFDNet is unchanged
    ff = FFDNet(1, tag="ffdnet").eval()
    ok, why = vjp.eligibility(ff)
    assert ok and "detaches its input" in why
    assert vjp.jacobian_eligibility(ff) == (True, "FFDNet: through the input")
    assert vjp.jacobian_eligibility(FFDNet(3, tag="ffdnet").eval())[0] is False
    assert vjp.jacobian_eligibility(build_denoiser("RealSN_SimpleCNN").train())[0] is False

    class FakeCuda(torch.Tensor):
        is_cuda = True
    x = torch.zeros(1, 1, 4, 4).as_subclass(FakeCuda)
    assert vjp.DenoiserVJP(ff, x).zero is True
    # refusals
    custom = EquilibriumProxGradSCI(lambda z, P: A_torch_(z, P), At_torch_, build_denoiser("SimpleCNN").eval(), eta=0.2)
    with pytest.raises(NotImplementedError, match="custom A / At"):
        DEQFixedPoint(custom, andersonexp, m=5).jacobian_report(None, None, None, None)
    bn = EquilibriumProxGradSCI(A_torch_, At_torch_, DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").train(), eta=0.2)
    with pytest.raises(NotImplementedError, match="BatchNorm2d"):
        DEQFixedPoint(bn, andersonexp, m=5).jacobian_report(None, None, None, None)
    with pytest.raises(ValueError, match="device_jacobian"):
        bn.device_jacobian(None, None, None, None)
    with pytest.raises(ValueError, match="gaptv"):
        harness.evaluate(None, [], method="gaptv", jacobian={"n_iters": 5})


def test_cabi_argument_checks_without_a_gpu():
    from deqsci_amd import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 256)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    q16 = p16 + 256
    assert lib.deqsci_ffdnet_head_masked_f32(None, p16, p16, q16, 1, 4, 4, None) == -1
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16, None, q16, 1, 4, 4, None) == -1
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16, p16, q16, 1, 0, 4, None) == -2
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16, p16, q16, 0, 4, 4, None) == -2
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16, p16 + 4, q16, 1, 4, 4, None) == -3
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16 + 4, p16, q16, 1, 4, 4, None) == -3
    assert lib.deqsci_ffdnet_head_masked_f32(p16, p16, p16, q16, 70000, 4, 4, None) == -4
    assert lib.deqsci_power_step_f32(None, p16, p16, q16, 1, 64, q16, None) == -1
    assert lib.deqsci_power_step_f32(p16, None, p16, None, 1, 64, q16, None) == -1
    assert lib.deqsci_power_step_f32(p16, p16, p16, q16, -1, 64, q16, None) == -2
    assert lib.deqsci_power_step_f32(p16, p16, p16, q16, 70000, 64, q16, None) == -2
    assert lib.deqsci_power_step_f32(p16 + 2, p16, p16, q16, 1, 64, q16, None) == -3
    assert lib.deqsci_power_step_f32(p16, p16, p16, q16 + 4, 1, 64, q16, None) == -3
    assert lib.deqsci_power_step_f32(None, None, None, None, 0, 64, None, None) == 0          # nothing to do
    assert lib.deqsci_power_workspace_bytes(0, 1 << 20) == 0
    assert lib.deqsci_power_workspace_bytes(-1, 8) == 0
    assert lib.deqsci_power_workspace_bytes(8, 256 * 256 * 8) == 8 * 128 * 2 * 8
    assert lib.deqsci_power_workspace_bytes(1, 1) == 16


_RESOURCES = r"Function Name: (\S*%s\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)"


def _compile_with_resource_report(src_name, tmp_path):
    src = os.path.join(ROOT, "deqsci_amd", "csrc", src_name)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deqsci_amd", "csrc"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage",
           "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(tmp_path)
    return out.stderr, open(tmp_path / asm[0]).read()


def test_masked_head_kernel_has_no_spills(tmp_path):
    """J1 keeps 4 x 36 weights per lane in registers for the whole tile (144 of them, as the head keeps 180): a spill would put a scratch
    access into the 36-FMA inner loop.  Both tile sizes: no scratch, no spills; the loop is packed FMAs."""
    report, text = _compile_with_resource_report("jacobian.hip", tmp_path)
    kernels = re.findall(_RESOURCES % "ffdnet_head_masked_kernel", report, flags=re.S)
    assert len(kernels) == 2, report[-2000:]
    for name, vgprs, scratch, sspill, vspill in kernels:
        assert int(vgprs) <= 256 and (int(scratch), int(sspill), int(vspill)) == (0, 0, 0), (name, vgprs, scratch, sspill, vspill)
    assert text.count("v_pk_fma_f32") >= 2 * 72
    assert "scratch_" not in text
