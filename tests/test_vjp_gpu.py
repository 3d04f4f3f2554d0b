"""GPU: the DEQ's implicit backward on the HIP kernels - the ReLU-mask pack, the masked epilogues, DenoiserVJP against float64 autograd,
an adjointness dot test, and DEQFixedPoint(implicit_backward="device") against the reference's own training run (tests/golden/backward*.npz)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint, vjp
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.networks import DnCNN

DEV = "cuda"


def _unpack(mask):
    """(n,H,W) int64 words -> (n,64,H,W) bool."""
    bits = torch.arange(64, device=mask.device).view(1, 64, 1, 1)
    return ((mask.unsqueeze(1) >> bits) & 1).bool()


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (3, 37, 29), (2, 64, 65)])
def test_relu_mask_pack_is_bit_equal(n, H, W):
    g = torch.Generator(device=DEV).manual_seed(n * H + W)
    a = torch.randn(n, 64, H, W, device=DEV, generator=g)
    a[:, ::5] = 0.0
    a[:, 1::7] = -0.0
    a[:, 62, 1::2] = float("nan")                              # NaN blocks (ReLU(NaN) > 0 is false)
    a = a.contiguous(memory_format=torch.channels_last)
    m = _hip.relu_mask_pack(a)
    assert m.shape == (n, H, W) and m.dtype == torch.int64
    assert torch.equal(_unpack(m), a > 0)


def _masked_case(n, H, W, kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "zeros":
        mb = torch.zeros(n, 64, H, W, dtype=torch.bool, device=DEV)
    elif kind == "ones":
        mb = torch.ones(n, 64, H, W, dtype=torch.bool, device=DEV)
    else:
        mb = torch.rand(n, 64, H, W, device=DEV, generator=g) < 0.5
    m = _hip.relu_mask_pack(torch.where(mb, 1.0, -1.0).contiguous(memory_format=torch.channels_last))
    assert torch.equal(_unpack(m), mb)
    return g, mb, m


SHAPES = [(1, 8, 8), (3, 37, 29), (2, 5, 70), (8, 256, 256)]


@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_winograd_masked_vs_float64(n, H, W, kind):
    g, mb, m = _masked_case(n, H, W, kind, seed=H * W + n)
    x = torch.randn(n, 64, H, W, device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
    w = torch.randn(64, 64, 3, 3, device=DEV, generator=g) * 0.05
    got = _hip.conv3x3_c64_winograd_masked(x, _hip.pack_winograd_weights(w), m)
    assert got.is_contiguous(memory_format=torch.channels_last)
    want = Fn.conv2d(x.double(), w.double(), padding=1) * mb
    if kind == "zeros":
        assert torch.equal(got, torch.zeros_like(got))
    else:
        assert _rel(got, want) < 1e-6
        assert torch.equal(got[~mb], torch.zeros_like(got[~mb]))
    if kind == "ones":                                        # all-one mask = the unmasked kernel without bias / ReLU, bit for bit
        assert torch.equal(got, _hip.conv3x3_c64_winograd(x, _hip.pack_winograd_weights(w), None, False))


@pytest.mark.parametrize("n,H,W", SHAPES)
@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_c1_to_64_masked_vs_float64(n, H, W, kind):
    g, mb, m = _masked_case(n, H, W, kind, seed=7 * H + W + n)
    x = torch.randn(n, 1, H, W, device=DEV, generator=g)
    w = torch.randn(64, 1, 3, 3, device=DEV, generator=g) * 0.2
    got = _hip.conv3x3_c1_to_64_masked(x, _hip.pack_c1_to_64_weights(w), m)
    want = Fn.conv2d(x.double(), w.double(), padding=1) * mb
    if kind == "zeros":
        assert torch.equal(got, torch.zeros_like(got))
    else:
        assert _rel(got, want) < 1e-6
    if kind == "ones":
        assert torch.equal(got, _hip.conv3x3_c1_to_64(x, _hip.pack_c1_to_64_weights(w), relu=False))


def test_masked_entry_points_refuse_bad_arguments():
    lib = _hip.load()
    x = torch.zeros(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    u = _hip.pack_winograd_weights(torch.zeros(64, 64, 3, 3, device=DEV))
    m = torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV)
    y = torch.empty_like(x)
    assert lib.deqsci_conv3x3_c64_winograd_masked_f32(x.data_ptr(), u.data_ptr(), None, y.data_ptr(), 1, 4, 4, None) == -1
    assert lib.deqsci_conv3x3_c64_winograd_masked_f32(x.data_ptr(), u.data_ptr(), m.data_ptr() + 4, y.data_ptr(), 1, 4, 4, None) == -3
    assert lib.deqsci_conv3x3_c64_winograd_masked_f32(x.data_ptr(), u.data_ptr(), m.data_ptr(), x.data_ptr(), 1, 4, 4, None) == -4
    assert lib.deqsci_relu_mask_pack_f32(x.data_ptr(), None, 16, None) == -1
    assert lib.deqsci_relu_mask_pack_f32(x.data_ptr(), m.data_ptr(), -1, None) == -2
    assert lib.deqsci_conv3x3_c1_to_64_masked_f32(x.data_ptr(), u.data_ptr(), None, y.data_ptr(), 1, 4, 4, None) == -1
    with pytest.raises(_hip.DeqsciHipError, match="mask"):
        _hip.conv3x3_c64_winograd_masked(x, u, torch.zeros(1, 4, 5, dtype=torch.int64, device=DEV))


def _net(kind):
    if kind == "SimpleCNN":
        s, _ = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4)
        return s.nonlinear_op
    if kind == "RealSN_SimpleCNN":
        s, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 4)
        return s.nonlinear_op
    g = torch.Generator().manual_seed(5)
    net = DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag="denoiser")
    for mod in net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.data = torch.randn(mod.weight.shape, generator=g) * (2.0 / (9 * mod.weight.shape[1])) ** 0.5
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data = 0.5 + torch.rand(64, generator=g)
            mod.bias.data = 0.1 * torch.randn(64, generator=g)
            mod.running_mean = 0.1 * torch.randn(64, generator=g)
            mod.running_var = 0.5 + torch.rand(64, generator=g)
    return net.eval().to(DEV)


class _FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, h):
        return h * self.mask


def _masked_module(net, masks):
    """A float64 copy of the module with every ReLU replaced by `h * mask` (the device forward's decisions): its autograd is J_D^T with
    those masks.  (A float64 forward decides the units within rounding of 0 differently from any fp32 forward - MIOpen's as well.)"""
    m64 = copy.deepcopy(net).double()
    seq, k = m64.dncnn, 0
    for i, mod in enumerate(list(seq)):
        if isinstance(mod, torch.nn.ReLU):
            seq[i] = _FixedMask(_unpack(masks[k]).double())
            k += 1
    assert k == len(masks)
    return m64


@pytest.mark.parametrize("kind", ["SimpleCNN", "RealSN_SimpleCNN", "DnCNN17"])
@pytest.mark.parametrize("n,H,W", [(3, 24, 20), (8, 64, 64), (8, 256, 256)])
def test_denoiser_vjp_vs_float64_autograd(kind, n, H, W):
    net = _net(kind)
    g = torch.Generator(device=DEV).manual_seed(n + H)
    x = torch.rand(n, 1, H, W, device=DEV, generator=g)
    v = torch.randn(n, 1, H, W, device=DEV, generator=g)
    jd = vjp.DenoiserVJP(net, x)
    got = jd(v)
    assert got.shape == v.shape and got.dtype == torch.float32
    m64 = _masked_module(net, jd.masks)
    x64 = x.double().requires_grad_()
    want = torch.autograd.grad(m64(x64), x64, v.double())[0]
    assert _rel(got, want) <= 1e-5, _rel(got, want)
    # the masks are the float64 forward's up to units within rounding of zero
    layers, _ = vjp.host_plan(net)
    with torch.no_grad():
        _, masks64 = vjp.plan_vjp([(w.double(), None if b is None else b.double(), r) for w, b, r in layers], x.double(), v.double())
    flips = sum(int((_unpack(m) != m64_).sum()) for m, m64_ in zip(jd.masks, masks64))
    assert flips <= 1e-5 * sum(m.numel() for m in masks64), flips
    # the same map again (the masks are fixed): bit for bit
    assert torch.equal(jd(v), got)


def test_denoiser_vjp_adjointness_against_float64_jvp():
    """<J^T v, u> (device) = <v, J u> with J u a float64 torch.func.jvp of the module under the device forward's masks."""
    net = _net("DnCNN17")
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.rand(2, 1, 40, 33, device=DEV, generator=g)
    u = torch.randn(2, 1, 40, 33, device=DEV, generator=g)
    v = torch.randn(2, 1, 40, 33, device=DEV, generator=g)
    jd = vjp.DenoiserVJP(net, x)
    m64 = _masked_module(net, jd.masks)
    _, ju = torch.func.jvp(m64, (x.double(),), (u.double(),))
    lhs = float((jd(v).double() * u.double()).sum())
    rhs = float((v.double() * ju).sum())
    assert abs(lhs - rhs) <= 1e-5 * (jd(v).double().norm() * u.double().norm()).item(), (lhs, rhs)


def test_denoiser_vjp_ffdnet_is_zero_and_refusals():
    s, _ = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), 4)
    x = torch.rand(4, 1, 16, 16, device=DEV)
    jd = vjp.DenoiserVJP(s.nonlinear_op, x, torch.full((4,), 0.1, device=DEV))
    assert jd.zero and torch.equal(jd(torch.randn_like(x)), torch.zeros_like(x))
    with pytest.raises(ValueError, match="BatchNorm2d"):
        vjp.DenoiserVJP(DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").to(DEV).train(), x)


def _golden_run(kind, mode, monkeypatch=None):
    g = np.load(os.path.join(GOLDEN, "backward.npz" if kind == "SimpleCNN" else "backward_ffdnet.npz"))
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    solver, _ = build_pipeline(kind, checkpoint.shipped("cnn" if kind == "SimpleCNN" else "ffdnet_gray"), 12)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=12, tol=1e-9)
    deq.implicit_backward = mode
    Phi, y, Ps, gt = G(g["Phi"]), G(g["y"]), G(g["Phi_sum"]), G(g["gt"])
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt))
    loss = torch.nn.functional.mse_loss(rec, gt)
    solver.zero_grad()
    calls = []
    if monkeypatch is not None:
        real = torch.autograd.grad
        monkeypatch.setattr(torch.autograd, "grad", lambda *a, **k: calls.append(1) or real(*a, **k))
    loss.backward()
    if monkeypatch is not None:
        monkeypatch.undo()
    return g, solver, deq, rec, loss, calls


@pytest.mark.parametrize("kind", ["SimpleCNN", "ffdnet"])
def test_device_implicit_backward_vs_reference_golden(kind, monkeypatch):
    g, solver, deq, rec, loss, calls = _golden_run(kind, "device", monkeypatch)
    assert deq.last_backward_path == "device" and deq.backward_fallback_reason is None
    assert calls == [], "torch.autograd.grad was called inside the device hook"
    assert rel_l2(rec.detach().cpu().numpy(), g["rec"]) < 1e-4
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * float(g["loss"])
    assert abs(deq.forward_res - float(g["forward_res"])) < 1e-2 * float(g["forward_res"])
    assert abs(deq.backward_res - float(g["backward_res"])) < 1e-2 * float(g["backward_res"])
    for name, p in solver.named_parameters():
        assert rel_l2(p.grad.cpu().numpy(), g["grad." + name]) < (1e-4 if kind == "SimpleCNN" else 5e-4), name
    if kind == "ffdnet":
        assert np.array_equal(solver.noise_sigma.cpu().numpy(), g["sigma_after"])


def test_device_implicit_backward_falls_back_for_train_mode_batchnorm():
    def run(mode):
        torch.manual_seed(0)
        net = DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").to(DEV).train()
        solver = deqsci_amd.EquilibriumProxGradSCI(deqsci_amd.A_torch_, deqsci_amd.At_torch_, net, eta=0.2)
        deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=6, tol=1e-9)
        deq.implicit_backward = mode
        gen = torch.Generator().manual_seed(1)
        Phi = (torch.rand(1, 16, 16, 4, generator=gen) < 0.5).float().to(DEV)
        gt = torch.rand(1, 16, 16, 4, generator=gen).to(DEV)
        y = (gt * Phi).sum(-1)
        Ps = deqsci_amd.phi_sum(Phi)
        rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None))
        torch.nn.functional.mse_loss(rec, gt).backward()
        return deq, [p.grad.clone() for p in solver.parameters()]
    d_dev, g_dev = run("device")
    d_ref, g_ref = run("autograd")
    assert d_dev.last_backward_path == "autograd" and d_ref.last_backward_path == "autograd"
    assert "BatchNorm2d" in d_dev.backward_fallback_reason and d_ref.backward_fallback_reason is None
    for a, b in zip(g_dev, g_ref):
        assert _rel(a, b) < 1e-6
