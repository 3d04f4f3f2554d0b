"""CPU: the host side of the device weight gradients (deqsci_amd/vjp.py: plan_param_grads, param_eligibility) and the argument
validation of csrc/wgrad.hip's entry points, which happens before any launch."""
import os

import pytest
import torch

from conftest import ROOT
from deqsci_amd import _hip, checkpoint, vjp
from deqsci_amd.cli import build_denoiser, build_pipeline
from deqsci_amd.networks import DnCNN, FFDNet


def _seeded_dncnn(layers, seed):
    g = torch.Generator().manual_seed(seed)
    net = DnCNN(1, num_of_layers=layers, lip=0.0, no_bn=True, tag="denoiser")
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.weight.shape[1])) ** 0.5
    return net.eval()


def _net(kind):
    if kind == "SimpleCNN":
        return build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4, device="cpu")[0].nonlinear_op
    return _seeded_dncnn(6, 5)


@pytest.mark.parametrize("kind", ["SimpleCNN", "DnCNN6"])
def test_plan_param_grads_equals_float64_autograd(kind):
    net = _net(kind).double()
    ok, why = vjp.param_eligibility(net)
    assert ok, why
    layers, why = vjp.host_plan(net)
    assert layers is not None, why
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 1, 24, 20, generator=g, dtype=torch.float64)
    v = torch.randn(3, 1, 24, 20, generator=g, dtype=torch.float64)
    weights = vjp.conv_weights(net)
    assert len(weights) == len(layers) == (4 if kind == "SimpleCNN" else 6)
    want = torch.autograd.grad(net(x), weights, v)
    got, masks = vjp.plan_param_grads(layers, x, v)
    assert len(got) == len(want) and len(masks) == len(layers) - 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == torch.float64
        assert float((a - b).norm() / b.norm()) <= 1e-12, i
    # handed the masks of that pass, it is the same statement
    again, _ = vjp.plan_param_grads(layers, x, v, masks=masks)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_param_eligibility_rules_and_reasons():
    for net in (build_denoiser("SimpleCNN").eval(), build_denoiser("SimpleCNN").train(), _seeded_dncnn(6, 1), _seeded_dncnn(2, 1),
                _seeded_dncnn(17, 1)):
        ok, why = vjp.param_eligibility(net)
        assert ok, why
    ok, why = vjp.param_eligibility(FFDNet(1, tag="ffdnet").eval())
    assert not ok and "FFDNet" in why
    for bn in (DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").eval(),
               DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").train()):
        ok, why = vjp.param_eligibility(bn)
        assert not ok and "BatchNorm2d" in why
    ok, why = vjp.param_eligibility(build_denoiser("RealSN_SimpleCNN").eval())
    assert not ok and "RealSNConv2d" in why
    ok, why = vjp.param_eligibility(DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="conv2d").eval())
    assert not ok and "'conv2d'" in why

    class Plugin(torch.nn.Module):
        tag = "denoiser"

    ok, why = vjp.param_eligibility(Plugin())
    assert not ok and "Plugin" in why
    wide = _seeded_dncnn(4, 1)
    wide.dncnn[2] = torch.nn.Conv2d(64, 64, kernel_size=5, padding=2, bias=False)
    ok, why = vjp.param_eligibility(wide)
    assert not ok and "3x3" in why
    biased = _seeded_dncnn(4, 1)
    biased.dncnn[2] = torch.nn.Conv2d(64, 64, kernel_size=3, padding=1, bias=True)
    ok, why = vjp.param_eligibility(biased)
    assert not ok and "bias" in why
    shapes = _seeded_dncnn(4, 1)
    shapes.dncnn[2] = torch.nn.Conv2d(64, 32, kernel_size=3, padding=1, bias=False)
    shapes.dncnn[4] = torch.nn.Conv2d(32, 64, kernel_size=3, padding=1, bias=False)
    ok, why = vjp.param_eligibility(shapes)
    assert not ok and "layer shapes" in why
    no_relu = _seeded_dncnn(4, 1)
    del no_relu.dncnn[3]
    ok, why = vjp.param_eligibility(no_relu)
    assert not ok and "ReLU" in why


def test_deq_switch_defaults_and_unknown_value():
    import deqsci_amd
    solver, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4, device="cpu")
    assert deq.parameter_backward == "autograd" and deq.last_parameter_path is None and deq.parameter_fallback_reason is None
    assert solver.device_param_eligibility()[0] is True
    other = deqsci_amd.EquilibriumProxGradSCI(lambda x, Phi: x, lambda y, Phi: y, solver.nonlinear_op, eta=0.2)
    ok, why = other.device_param_eligibility()
    assert not ok and "custom A / At" in why
    deq.parameter_backward = "hip"
    with pytest.raises(ValueError, match="parameter_backward"):
        deq._taped_call(None, None, None, None)


def test_wgrad_entry_points_validate_before_any_launch():
    lib = _hip.load()
    assert _hip.WGRAD_CHAIN == 4096
    hdr = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    assert "#define DEQSCI_WGRAD_CHAIN %d\n" % _hip.WGRAD_CHAIN in hdr
    wsb = lib.deqsci_wgrad_workspace_bytes
    assert wsb(0, 4, 4) == 0 and wsb(1, 0, 4) == 0 and wsb(1, 4, -1) == 0 and wsb(-3, 4, 4) == 0
    assert wsb(1, 1 << 21, 4) == 0 and wsb(1 << 20, 1 << 20, 64) == 0                 # beyond the kernels' offsets
    assert wsb(1, 1, 1) >= 9 * 64 * 64 * 8 and wsb(1, 1, 1) % 8 == 0
    assert wsb(64, 256, 256) <= 256 * 9 * 64 * 64 * 8                                   # bounded: it does not grow with the batch
    far = 1 << 40                                                                       # addresses only: validation dereferences nothing
    w0, w1 = lib.deqsci_wgrad3x3_c64_c64_f32, lib.deqsci_wgrad3x3_c1_c64_f32
    x, g, dw, ws = far, far + (1 << 24), far + (2 << 24), far + (3 << 24)
    # NULL -> -1
    assert w0(None, g, dw, 1, 4, 4, ws, None) == -1 and w0(x, None, dw, 1, 4, 4, ws, None) == -1
    assert w0(x, g, None, 1, 4, 4, ws, None) == -1 and w0(x, g, dw, 1, 4, 4, None, None) == -1
    assert w1(None, g, dw, 0, 1, 4, 4, ws, None) == -1 and w1(x, None, dw, 0, 1, 4, 4, ws, None) == -1
    assert w1(x, g, None, 1, 1, 4, 4, ws, None) == -1 and w1(x, g, dw, 1, 1, 4, 4, None, None) == -1
    # sizes -> -2
    assert w0(x, g, dw, 0, 4, 4, ws, None) == -2 and w0(x, g, dw, 1, 0, 4, ws, None) == -2 and w0(x, g, dw, 1, 4, -4, ws, None) == -2
    assert w1(x, g, dw, 0, 0, 4, 4, ws, None) == -2 and w1(x, g, dw, 1, 1, -1, 4, ws, None) == -2 and w1(x, g, dw, 0, 1, 4, 0, ws, None) == -2
    # alignment -> -3
    assert w0(x + 4, g, dw, 1, 4, 4, ws, None) == -3 and w0(x, g + 8, dw, 1, 4, 4, ws, None) == -3
    assert w0(x, g, dw + 2, 1, 4, 4, ws, None) == -3 and w0(x, g, dw, 1, 4, 4, ws + 4, None) == -3
    assert w1(x + 2, g, dw, 0, 1, 4, 4, ws, None) == -3 and w1(x, g + 1, dw, 0, 1, 4, 4, ws, None) == -3
    assert w1(x, g, dw, 0, 1, 4, 4, ws + 4, None) == -3
    # overlap / unsupported -> -4
    assert w0(x, g, x, 1, 4, 4, ws, None) == -4 and w0(x, g, g + 64, 1, 4, 4, ws, None) == -4          # dw inside an input
    assert w0(x, g, dw, 1, 4, 4, x, None) == -4 and w0(x, g, dw, 1, 4, 4, g + 8, None) == -4           # workspace over an input
    assert w0(x, g, dw, 1, 4, 4, dw + 8, None) == -4                                                   # workspace over dw
    assert w0(x, g, dw, 1, 1 << 21, 4, ws, None) == -4 and w0(x, g, dw, 1 << 20, 1 << 20, 64, ws, None) == -4
    assert w1(x, g, x, 0, 1, 4, 4, ws, None) == -4 and w1(x, g, g + 64, 1, 1, 4, 4, ws, None) == -4
    assert w1(x, g, dw, 0, 1, 4, 4, x, None) == -4 and w1(x, g, dw, 1, 1, 4, 4, g, None) == -4
    assert w1(x, g, dw, 2, 1, 4, 4, ws, None) == -4 and w1(x, g, dw, -1, 1, 4, 4, ws, None) == -4      # flip is 0 or 1
    assert w1(x, g, dw, 0, 1, 4, 1 << 21, ws, None) == -4


def test_wgrad_kernels_compile_without_spills(tmp_path):
    """csrc/wgrad.hip's W0 holds 9 x 16 accumulators per lane beside the next tile's loads: a spilled register would be a memory round trip
    in front of the matrix instructions (seen while writing it: 144 addresses of the flush kept across the tile loop, 164 spills).  Every
    kernel of the file compiles for gfx950 with no spill and no per-lane stack, and W0's code is matrix instructions.  (Cross-compiles
    without a GPU, ~10 s.)"""
    import re
    import subprocess
    src = os.path.join(ROOT, "deqsci_amd", "csrc", "wgrad.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deqsci_amd", "csrc"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage",
           "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    found = re.findall(r"Function Name: (\S*wgrad\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+)"
                       r".*?VGPRs Spill: (\d+)", out.stderr, flags=re.S)
    assert len(found) == 3, out.stderr[-2000:]                    # wgrad_c64_kernel, wgrad_c1_kernel, wgrad_sum_kernel
    for name, vgprs, agprs, stack, sspill, vspill in found:
        assert int(vgprs) + int(agprs) <= 512 and (int(stack), int(sspill), int(vspill)) == (0, 0, 0), (name, vgprs, agprs, stack, sspill, vspill)
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(tmp_path)
    assert open(tmp_path / asm[0]).read().count("v_mfma_f32_32x32x2_f32") >= 9
