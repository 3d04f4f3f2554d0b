"""DnCNN-17 on the device: the 15 middle layers as ONE conv_w16 stack launch per slice between the HIP 1->64 and 64->1 layers
(engine._Denoiser._sliced), against the same layers launched one by one, a float64 stack, and the reference's own runs
(tests/golden/dncnn17.npz, make_dncnn_golden.py: traffic measurement 0, the 64 x 64 x 8 crop, 10 and K iterations).

Shapes this small take Winograd F(2x2,3x3) under the default policy (less than a block tile per CU: _hip.conv64_kernel_for), so the
tests of the stack path pin the split-fp16 kernels with _hip.FORCE_CONV64 as the tools do; at 256 x 256 x 8 the policy picks them itself
(the command-line test below).

Measured on an MI355X (profiles/dncnn17.md): against the float64 stack 7.2e-7 (fp32 kernels 1.1e-6); one f-call against golden (a)
1.0e-6 (MIOpen's fp32 stack: 9.7e-7); end to end 2.9e-7 at 10 iterations and 3.5e-6 at K = 17 (stack_kernel="s16": 3.2e-7, 1.7e-5)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deqsci_amd import _hip
from deqsci_amd.cli import build_pipeline
from deqsci_amd.engine import DEQSCIEngine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WEIGHTS = os.path.join(GOLDEN, "dncnn_noise15.npz")
DEV = "cuda"


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def psnr(rec, gt):
    return float(10 * np.log10(1.0 / np.mean((np.clip(np.asarray(rec, dtype=np.float64), 0, 1) - np.asarray(gt, dtype=np.float64)) ** 2)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "dncnn17.npz"))


@pytest.fixture(scope="module")
def net():
    return build_pipeline("DnCNN", WEIGHTS, 10)[0].nonlinear_op


@pytest.fixture
def split16():
    old = _hip.FORCE_CONV64
    _hip.FORCE_CONV64 = "s16"
    yield
    _hip.FORCE_CONV64 = old


def _den(net, n_img, **kw):
    """The engine's denoiser prepared as reconstruct() prepares it for f-calls of n_img images."""
    den = DEQSCIEngine(net, max_iter=8, use_graph=False, **kw).den
    den.prepare(16, DEV, n_img=n_img)
    return den


def _float64_stack(den, x):
    h = x.double()
    for w, b, relu in den.fast:
        h = torch.nn.functional.conv2d(h, w.double(), None if b is None else b.double(), padding=1)
        h = torch.relu(h) if relu else h
    return h


@pytest.mark.parametrize("kernel,per_layer", [("w16", "w16 per layer (behind a stack time-out)"), ("s16", "per layer")])
@pytest.mark.parametrize("n,H,W,per_launch", [(2, 24, 24, None), (3, 40, 72, None), (33, 16, 16, None), (33, 16, 16, 32)])
def test_stack_launch_is_bit_identical_to_per_layer_launches(net, split16, n, H, W, per_launch, kernel, per_layer):
    """(2, 24 x 24) a single tile per image; (3, 40 x 72) ragged, several tiles; (33, 16 x 16) as one launch and in slices of 32 images
    (the second slice one image: head, stack launch and tail at an offset into the batch and its range slots).  The per-layer side is
    what the engine falls back to behind a stack time-out."""
    g = torch.Generator(device=DEV).manual_seed(n * H + W)
    z = torch.rand(1, n, H, W, device=DEV, generator=g)
    den = _den(net, n, stack_kernel=kernel)
    den.stack_per_launch = per_launch
    den.run(z, 0, calibrate=True)                              # the first f-call: the ranges, measured on the direct kernels layer by layer
    got = den.run(z, 1)[0].clone()
    assert den.last_path == kernel + " stack launch" and den.stack_launches == 1 and not den.stack_timed_out()
    den.stack, den.per_layer_w16 = False, True                 # (what the engine sets behind a time-out)
    want = den.run(z, 1)[0]
    assert den.last_path == per_layer and den.stack_launches == 1
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and torch.equal(got, want)


def test_stack_launch_against_float64_and_per_image_ranges(net, gold, split16):
    """The shipped weights on the golden's input: no further from the float64 stack than 1.25 x the fp32 kernels (conv64="fast32"), the
    project's rule for the split-fp16 layers; and - range slots are per image - an image's output alone = in the batch, bit for bit."""
    z = torch.from_numpy(gold["a_x"]).to(DEV).view(1, 8, 64, 64)
    den = _den(net, 8)
    den.run(z, 0, calibrate=True)
    got = den.run(z, 1)[0]
    assert den.last_path == "w16 stack launch"
    ref = _float64_stack(den, z.view(8, 1, 64, 64)).view(1, 8, 64, 64)
    _hip.FORCE_CONV64 = None                                   # (the fixture's pin would override "fast32" too; it restores the old value)
    f32 = _den(net, 8, conv64="fast32")
    got32 = f32.run(z, 0, calibrate=True)[0]
    _hip.FORCE_CONV64 = "s16"
    e16, e32 = float((got.double() - ref).norm() / ref.norm()), float((got32.double() - ref).norm() / ref.norm())
    print(f"vs float64: w16 stack launch {e16:.3e}  fp32 kernels {e32:.3e}")
    assert f32.last_path == "per layer" and e16 <= 1.25 * e32
    for j in (0, 5):
        one = _den(net, 1)
        zj = z[:, j:j + 1].contiguous()
        one.run(zj, 0, calibrate=True)
        assert torch.equal(one.run(zj, 1)[0], got[:, j:j + 1]) and one.last_path == "w16 stack launch"


def test_one_fcall_against_the_reference(net, gold, split16):
    """Golden (a): the reference's DnCNN (CPU, fp32) on the GAP output of the crop; the project's per-f-call gate, 1e-5 - should 17
    layers not meet it, 1.25 x what MIOpen's fp32 conv2d stack (the module itself on the device) is from the same golden."""
    x = torch.from_numpy(gold["a_x"]).to(DEV)
    den = _den(net, 8)
    den.run(x.view(1, 8, 64, 64), 0, calibrate=True)
    got = den.run(x.view(1, 8, 64, 64), 1)[0].view(8, 1, 64, 64)
    with torch.no_grad():
        mi = net(x)
    e, e_mi = rel_l2(got.cpu().numpy(), gold["a_out"]), rel_l2(mi.cpu().numpy(), gold["a_out"])
    print(f"one f-call vs golden (a): w16 stack launch {e:.3e}  MIOpen fp32 module {e_mi:.3e}")
    assert den.last_path == "w16 stack launch" and (e <= 1e-5 or e <= 1.25 * e_mi)


def _problem(gold):
    return (torch.from_numpy(gold[k]).to(DEV) for k in ("y", "Phi", "Phi_sum", "x0"))


def _gates(rec, gold, iters):
    e = rel_l2(rec.cpu().numpy(), gold[f"b{iters}_rec"])
    dp = abs(psnr(rec.cpu().numpy(), gold["gt"]) - float(gold[f"b{iters}_psnr"]))
    return e, dp


@pytest.fixture(scope="module")
def stack_recs(net, gold):
    """{iterations: the stack-launch engine's eager reconstruction} - computed once, shared by the tests below."""
    out = {}
    old = _hip.FORCE_CONV64
    _hip.FORCE_CONV64 = "s16"
    try:
        y, Phi, Ps, x0 = _problem(gold)
        for iters in (10, int(gold["K"])):
            eng = DEQSCIEngine(net, max_iter=iters, use_graph=False)
            rec = eng.reconstruct(y, Phi, Ps, initial_point=x0)
            assert eng.last_info["denoiser_path"] == "w16 stack launch" and eng.last_info["stack_timeouts"] == 0
            assert eng.last_info["stack_launches"] == eng.last_info["f_calls"] - 1
            out[iters] = (rec.clone(), eng.last_info["res"])
    finally:
        _hip.FORCE_CONV64 = old
    return out


@pytest.mark.parametrize("which", [10, "K"])
def test_end_to_end_against_the_reference(net, gold, split16, stack_recs, which):
    """Golden (b): the reference's EquilibriumProxGradSCI + andersonexp on the crop at 10 and at K iterations (K = 17: the largest horizon
    at which the reference's own run, perturbed by 1e-7, stays within 1e-5 of itself): <= 1e-4 rel-L2 and <= 0.01 dB, through the engine
    (eager, and hipGraph replay bit-identical to it) and through the drop-in DEQFixedPoint."""
    iters = int(gold["K"]) if which == "K" else 10
    y, Phi, Ps, x0 = _problem(gold)
    rec, res = stack_recs[iters]
    e, dp = _gates(rec, gold, iters)
    print(f"{iters} iterations, engine (w16 stack launch): rel-L2 {e:.3e}  PSNR difference {dp:.4f} dB  res {res:.4e} (reference {float(gold[f'b{iters}_res']):.4e})")
    assert e <= 1e-4 and dp <= 0.01
    eng = DEQSCIEngine(net, max_iter=iters, use_graph=True)
    for _ in range(3):                                          # eager, capture + replay, replay
        again = eng.reconstruct(y, Phi, Ps, initial_point=x0)
    assert eng.last_info["graph"] and eng.last_info["denoiser_path"] == "w16 stack launch" and torch.equal(again, rec)
    deq = build_pipeline("DnCNN", WEIGHTS, iters)[1]
    z = deq.forward(y, Phi, Ps, initial_point=x0, train_flag=False)
    e, dp = _gates(z, gold, iters)
    print(f"{iters} iterations, DEQFixedPoint: rel-L2 {e:.3e}  PSNR difference {dp:.4f} dB")
    assert e <= 1e-4 and dp <= 0.01


@pytest.mark.parametrize("which", [10, "K"])
def test_timeout_fallback_and_s16_stack_stay_within_the_gates(net, gold, split16, stack_recs, which):
    """Behind a stack time-out (the engine's own state for it, set by hand: nothing waits here) the 15 layers go out one by one on the
    same kernel with the same ranges - the stack launch's bits; stack_kernel="s16" runs them as one launch of the direct kernel."""
    iters = int(gold["K"]) if which == "K" else 10
    y, Phi, Ps, x0 = _problem(gold)
    eng = DEQSCIEngine(net, max_iter=iters, use_graph=False)
    eng.den.stack, eng.den.per_layer_w16, eng._stack_off_for = False, True, 4
    rec = eng.reconstruct(y, Phi, Ps, initial_point=x0)
    assert eng.last_info["denoiser_path"] == "w16 per layer (behind a stack time-out)" and eng.last_info["stack_launches"] == 0
    assert torch.equal(rec, stack_recs[iters][0])
    s16 = DEQSCIEngine(net, max_iter=iters, use_graph=False, stack_kernel="s16")
    rec = s16.reconstruct(y, Phi, Ps, initial_point=x0)
    e, dp = _gates(rec, gold, iters)
    print(f"{iters} iterations, s16 stack launch: rel-L2 {e:.3e}  PSNR difference {dp:.4f} dB")
    assert s16.last_info["denoiser_path"] == "s16 stack launch" and s16.last_info["stack_launches"] == s16.last_info["f_calls"] - 1
    assert e <= 1e-4 and dp <= 0.01


def test_default_policy_on_the_crop_stays_within_the_gates(net, gold):
    """Without the pin: 8 images of 64 x 64 are less than a block tile per CU, the 64->64 layers take Winograd F(2x2,3x3) layer by layer."""
    y, Phi, Ps, x0 = _problem(gold)
    eng = DEQSCIEngine(net, max_iter=10, use_graph=False)
    e, dp = _gates(eng.reconstruct(y, Phi, Ps, initial_point=x0), gold, 10)
    assert eng.last_info["denoiser_path"] == "per layer" and e <= 1e-4 and dp <= 0.01


def test_cli_smoke(tmp_path):
    """--denoiser DnCNN --loadpath ... on one shipped clip at 256 x 256 x 8, 3 iterations: the reference-shaped lines."""
    data = tmp_path / "clips"
    data.mkdir()
    os.symlink(os.path.join(ROOT, "data", "test_gray", "drop8_cacti.mat"), data / "drop8_cacti.mat")
    env = dict(os.environ)
    env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, "-m", "deqsci_amd.cli", "--denoiser", "DnCNN", "--loadpath", WEIGHTS, "--and_maxiters", "3",
           "--testpath", str(data) + "/", "--savepath", str(tmp_path / "out") + "/"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert "loaded dict!" in lines and any("drop8" in ln for ln in lines)
    total = [ln for ln in lines if ln.startswith("--------------------------------- Total Average PSNR: ")]
    assert len(total) == 1 and np.isfinite(float(total[0].split(": ")[-1].split()[0]))
