"""GPU: the denoiser's weight gradients on the HIP kernels (csrc/wgrad.hip) - W0 (64 -> 64) and both forms of W1 (the edge layers) exactly on
integer data and within the fp32 chain bound on normal data, DenoiserParamGrads against float64 autograd under the device's own masks, and
DEQFixedPoint(parameter_backward="device") against the reference's own training run (tests/golden/backward.npz) with its fallbacks.

The shapes: an all-border image, ragged rows and columns, image seams, more tiles than one workgroup's share - and, per kernel, one shape at
which a workgroup holds more than WGRAD_CHAIN pixels and so flushes its partial more than once (W0 runs at most 256 workgroups, W1 at most
512).  No shape has an idle workgroup: the launch asks for ceil(tiles / ceil(tiles / cap)) workgroups, so each owns at least one tile."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint, vjp
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.networks import DnCNN

DEV = "cuda"
SHAPES = [(1, 1, 1), (1, 3, 3), (3, 37, 29), (2, 5, 70), (2, 64, 65), (8, 64, 64)]
W0_SHAPES = SHAPES + [(17, 256, 256)]          # 17 * 256 * 8 tiles / 256 workgroups = 136 tiles = 4352 pixels each > WGRAD_CHAIN
W1_SHAPES = SHAPES + [(33, 256, 256)]          # 33 * 256 * 8 tiles / 512 workgroups = 132 tiles = 4224 pixels each > WGRAD_CHAIN
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def test_flush_shapes_hold_more_than_a_chain_per_workgroup():
    assert _hip.WGRAD_CHAIN == 4096
    for (n, H, W), cap in ((W0_SHAPES[-1], 256), (W1_SHAPES[-1], 512)):
        tiles = n * H * -(-W // 32)
        assert -(-tiles // cap) * 32 > _hip.WGRAD_CHAIN


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _window(H, W, ky, kx):
    """The pixels p = (h, w) whose tap p + (ky-1, kx-1) lies inside the image: slices of p and of the tap."""
    dy, dx = ky - 1, kx - 1
    h0, h1, w0, w1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if h0 >= h1 or w0 >= w1:
        return None
    return (slice(h0, h1), slice(w0, w1)), (slice(h0 + dy, h1 + dy), slice(w0 + dx, w1 + dx))


def _ref_w0(x, g):
    """float64 dw[co,ci,ky,kx] = sum g[:,co,p] x[:,ci,p + tap], only the products that exist (a tap outside the image is not multiplied)."""
    x, g = x.double(), g.double()
    H, W = x.shape[2:]
    out = torch.zeros(64, 64, 3, 3, dtype=torch.float64, device=x.device)
    for ky, kx in TAPS:
        win = _window(H, W, ky, kx)
        if win is not None:
            (ph, pw), (th, tw) = win
            out[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", g[:, :, ph, pw], x[:, :, th, tw])
    return out


def _ref_w1(s, t, flip):
    s, t = s.double()[:, 0], t.double()
    H, W = s.shape[1:]
    out = torch.zeros(64, 3, 3, dtype=torch.float64, device=s.device)
    for ky, kx in TAPS:
        win = _window(H, W, ky, kx)
        if win is not None:
            (ph, pw), (th, tw) = win
            if flip:
                out[:, ky, kx] = torch.einsum("nhw,nchw->c", s[:, ph, pw], t[:, :, th, tw])
            else:
                out[:, ky, kx] = torch.einsum("nchw,nhw->c", t[:, :, ph, pw], s[:, th, tw])
    return out.view(1, 64, 3, 3) if flip else out.view(64, 1, 3, 3)


def _gamma(n, H, W):
    c = min(_hip.WGRAD_CHAIN, n * H * W) + 2
    u = c * 2.0 ** -24
    return u / (1.0 - u)


def _ints(shape, gen):
    return torch.randint(-3, 4, shape, device=DEV, generator=gen).float()


@pytest.mark.parametrize("n,H,W", W0_SHAPES)
def test_w0_is_exact_on_integer_data(n, H, W):
    gen = torch.Generator(device=DEV).manual_seed(100 * n + H + W)
    x, g = _cl(_ints((n, 64, H, W), gen)), _cl(_ints((n, 64, H, W), gen))
    got = _hip.wgrad_c64_c64(x, g)
    assert got.shape == (64, 64, 3, 3) and got.dtype == torch.float32
    assert torch.equal(got, _ref_w0(x, g).float())


@pytest.mark.parametrize("n,H,W", W1_SHAPES)
def test_w1_is_exact_on_integer_data_in_both_forms(n, H, W):
    gen = torch.Generator(device=DEV).manual_seed(7 * n + 3 * H + W)
    s, t = _ints((n, 1, H, W), gen), _cl(_ints((n, 64, H, W), gen))
    for flip in (0, 1):
        got = _hip.wgrad_c1_c64(s, t, flip)
        assert got.shape == ((1, 64, 3, 3) if flip else (64, 1, 3, 3)) and got.dtype == torch.float32
        assert torch.equal(got, _ref_w1(s, t, flip).float()), flip


@pytest.mark.parametrize("n,H,W", W0_SHAPES)
def test_w0_rounding_determinism_and_nan(n, H, W):
    gen = torch.Generator(device=DEV).manual_seed(n + 10 * H + W)
    x, g = _cl(torch.randn(n, 64, H, W, device=DEV, generator=gen)), _cl(torch.randn(n, 64, H, W, device=DEV, generator=gen))
    ws = _hip.wgrad_workspace(n, H, W, DEV)
    ws.fill_(float("nan"))                                     # the workspace needs no initialisation
    got = _hip.wgrad_c64_c64(x, g, ws)
    want, S = _ref_w0(x, g), _ref_w0(x.abs(), g.abs())
    err = (got.double() - want).abs()
    print(f"W0 {(n, H, W)}: max |err| / (gamma S) = {float((err / (_gamma(n, H, W) * S).clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= _gamma(n, H, W) * S).all())
    assert torch.equal(_hip.wgrad_c64_c64(x, g), got)
    # a NaN reaches exactly the entries whose sum holds one of its products: x[.., ci, p] every tap that lands on p, g[.., co, p] every tap of p
    x[n - 1, 5, H - 1, W - 1] = float("nan")
    g[0, 9, 0, 0] = float("nan")
    got = _hip.wgrad_c64_c64(x, g, ws)
    want = _ref_w0(x, g)
    assert bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    assert bool(((got.double() - want).abs()[ok] <= (_gamma(n, H, W) * S)[ok]).all())


@pytest.mark.parametrize("n,H,W", W1_SHAPES)
def test_w1_rounding_determinism_and_nan(n, H, W):
    gen = torch.Generator(device=DEV).manual_seed(3 * n + H + 10 * W)
    s, t = torch.randn(n, 1, H, W, device=DEV, generator=gen), _cl(torch.randn(n, 64, H, W, device=DEV, generator=gen))
    ws = _hip.wgrad_workspace(n, H, W, DEV)
    ws.fill_(float("nan"))
    for flip in (0, 1):
        got = _hip.wgrad_c1_c64(s, t, flip, ws)
        want, S = _ref_w1(s, t, flip), _ref_w1(s.abs(), t.abs(), flip)
        err = (got.double() - want).abs()
        print(f"W1 flip={flip} {(n, H, W)}: max |err| / (gamma S) = {float((err / (_gamma(n, H, W) * S).clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= _gamma(n, H, W) * S).all()), flip
        assert torch.equal(_hip.wgrad_c1_c64(s, t, flip), got)
    s2, t2 = s.clone(), t.clone()
    s2[0, 0, 0, W - 1] = float("nan")
    t2[n - 1, 11, H - 1, 0] = float("nan")
    for flip in (0, 1):
        got, want = _hip.wgrad_c1_c64(s2, t2, flip, ws), _ref_w1(s2, t2, flip)
        assert bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan()), flip


def test_wgrad_bindings_refuse_bad_arguments():
    x = _cl(torch.zeros(1, 64, 4, 4, device=DEV))
    with pytest.raises(_hip.DeqsciHipError, match="channels_last"):
        _hip.wgrad_c64_c64(torch.zeros(1, 64, 4, 4, device=DEV), x)
    with pytest.raises(_hip.DeqsciHipError, match="one shape"):
        _hip.wgrad_c64_c64(x, _cl(torch.zeros(1, 64, 4, 5, device=DEV)))
    with pytest.raises(_hip.DeqsciHipError, match="workspace"):
        _hip.wgrad_c64_c64(x, x.clone(), torch.empty(16, device=DEV, dtype=torch.float64))
    with pytest.raises(_hip.DeqsciHipError, match="flip"):
        _hip.wgrad_c1_c64(torch.zeros(1, 1, 4, 4, device=DEV), x, 2)
    with pytest.raises(_hip.DeqsciHipError, match="image"):
        _hip.wgrad_c1_c64(torch.zeros(1, 1, 4, 5, device=DEV), x, 0)


# ----------------------------------------------------------------------------- DenoiserParamGrads
def _net(kind):
    if kind == "SimpleCNN":
        return build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4)[0].nonlinear_op
    gen = torch.Generator().manual_seed(5)
    net = DnCNN(1, num_of_layers=6, lip=0.0, no_bn=True, tag="denoiser")
    for mod in net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.weight.data = torch.randn(mod.weight.shape, generator=gen) * (2.0 / (9 * mod.weight.shape[1])) ** 0.5
    return net.eval().to(DEV)


class _FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, h):
        return h * self.mask


def _masked_module(net, masks):
    """A float64 copy of the module with every ReLU replaced by `h * mask` (the device forward's decisions): its autograd gives the weight
    gradients under those masks.  (A float64 forward decides the units within rounding of 0 differently from any fp32 forward.)"""
    m64 = copy.deepcopy(net).double()
    seq, k = m64.dncnn, 0
    for i, mod in enumerate(list(seq)):
        if isinstance(mod, torch.nn.ReLU):
            seq[i] = _FixedMask(vjp.unpack_masks(masks[k]).double())
            k += 1
    assert k == len(masks)
    return m64


def _chain_sums(m64, x64, v64):
    """S per conv weight: the wgrad sum over |gradient behind the layer| |input of the layer|, from the float64 masked module."""
    convs = [m for m in m64.dncnn if isinstance(m, torch.nn.Conv2d)]
    inputs, outs = [], []
    def keep(mod, inp, out):
        inputs.append(inp[0].detach())
        outs.append(out)
    hooks = [c.register_forward_hook(keep) for c in convs]
    y = m64(x64)
    for h in hooks:
        h.remove()
    gs = torch.autograd.grad(y, outs, v64)
    return [torch.nn.grad.conv2d_weight(i.abs(), c.weight.shape, g.abs(), padding=1) for i, c, g in zip(inputs, convs, gs)]


@pytest.mark.parametrize("kind", ["SimpleCNN", "DnCNN6"])
@pytest.mark.parametrize("n,H,W", [(3, 24, 20), (8, 64, 64)])
def test_denoiser_param_grads_vs_float64_autograd(kind, n, H, W):
    net = _net(kind)
    gen = torch.Generator(device=DEV).manual_seed(n + H)
    x = torch.rand(n, 1, H, W, device=DEV, generator=gen)
    v = torch.randn(n, 1, H, W, device=DEV, generator=gen)
    pg = vjp.DenoiserParamGrads(net, x)
    assert pg.shape == (n, 1, H, W) and len(pg.masks) == len(vjp.conv_weights(net)) - 1
    # .noise is what _MaskedStack's kernels give
    layers, _ = vjp.host_plan(net)
    h = _hip.conv3x3_c1_to_64(x, _hip.pack_c1_to_64_weights(layers[0][0]), relu=True)
    for w, _, _ in layers[1:-1]:
        h = _hip.conv3x3_c64_winograd(h, _hip.pack_winograd_weights(w), None, True)
    assert torch.equal(pg.noise, _hip.conv3x3_c64_to_1(h, _hip.pack_c64_to_1_weights(layers[-1][0])))
    assert torch.equal(pg.masks[-1], _hip.relu_mask_pack(h))
    got = pg.grads(v)
    m64 = _masked_module(net, pg.masks)
    want = torch.autograd.grad(m64(x.double()), vjp.conv_weights(m64), v.double())
    S = _chain_sums(m64, x.double(), v.double())
    assert len(got) == len(want) == len(S)
    for i, (a, b, s) in enumerate(zip(got, want, S)):
        assert a.shape == b.shape and a.dtype == torch.float32
        rel = float((a.double() - b).norm() / b.norm())
        bound = 1e-5 + float((_gamma(n, H, W) * s).norm() / b.norm())
        print(f"{kind} {(n, H, W)} dW_{i}: rel L2 {rel:.3e} (bound {bound:.3e})")
        assert rel <= bound, (i, rel, bound)
    # the host statement under the same masks says the same
    host, _ = vjp.plan_param_grads([(w.double(), None, r) for w, _, r in layers], x.double(), v.double(),
                                   masks=[vjp.unpack_masks(m) for m in pg.masks])
    for a, b in zip(host, want):
        assert float((a - b).norm() / b.norm()) <= 1e-12
    # the input product is DenoiserVJP's, a subset of the weights stops the walk early, and the same call again is bit-equal
    assert torch.equal(pg.vjp(v), vjp.DenoiserVJP(net, x)(v))
    k = len(got)
    part = pg.grads(v, need=[False] * (k - 2) + [True, False])
    assert all(p is None for p in part[:k - 2]) and part[k - 1] is None and torch.equal(part[k - 2], got[k - 2])
    assert all(torch.equal(a, b) for a, b in zip(pg.grads(v), got))
    pg.release()
    with pytest.raises(RuntimeError, match="released"):
        pg.grads(v)


def test_denoiser_noise_function_routes_gradients_and_frees():
    from deqsci_amd import autograd as ag
    net = _net("SimpleCNN")
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(2, 1, 12, 10, device=DEV, generator=gen, requires_grad=True)
    v = torch.randn(2, 1, 12, 10, device=DEV, generator=gen)
    weights = vjp.conv_weights(net)
    weights[1].requires_grad_(False)
    try:
        noise = ag.denoiser_noise(net, x)
        pg = vjp.DenoiserParamGrads(net, x)
        assert torch.equal(noise, pg.noise)
        got = torch.autograd.grad(noise, [x, weights[0], weights[2], weights[3]], v, retain_graph=True)
        ref = pg.grads(v)
        assert torch.equal(got[0], pg.vjp(v)) and torch.equal(got[1], ref[0]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
        with pytest.raises(RuntimeError, match="freed"):
            torch.autograd.grad(noise, [weights[0]], v)
    finally:
        weights[1].requires_grad_(True)


# ----------------------------------------------------------------------------- DEQFixedPoint(parameter_backward="device")
def _golden_run(kind, parameter, implicit):
    g = np.load(os.path.join(GOLDEN, "backward.npz" if kind == "SimpleCNN" else "backward_ffdnet.npz"))
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    solver, _ = build_pipeline(kind, checkpoint.shipped("cnn" if kind == "SimpleCNN" else "ffdnet_gray"), 12)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=12, tol=1e-9)
    if parameter is not None:
        deq.parameter_backward = parameter
    deq.implicit_backward = implicit
    calls = []
    hook = solver.nonlinear_op.register_forward_hook(lambda *a: calls.append(torch.is_grad_enabled()))
    Phi, y, Ps, gt = G(g["Phi"]), G(g["y"]), G(g["Phi_sum"]), G(g["gt"])
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt))
    hook.remove()
    loss = torch.nn.functional.mse_loss(rec, gt)
    solver.zero_grad()
    loss.backward()
    return g, solver, deq, rec, loss, sum(calls)


@pytest.mark.parametrize("implicit", ["autograd", "device"])
def test_device_parameter_backward_vs_reference_golden(implicit):
    g, solver, deq, rec, loss, taped_module_calls = _golden_run("SimpleCNN", "device", implicit)
    assert deq.last_parameter_path == "device" and deq.parameter_fallback_reason is None
    assert deq.last_backward_path == implicit
    assert taped_module_calls == 1, "the torch module ran on the tape for more than f0"
    assert rel_l2(rec.detach().cpu().numpy(), g["rec"]) < 1e-4
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * float(g["loss"])
    assert abs(deq.forward_res - float(g["forward_res"])) < 1e-2 * float(g["forward_res"])
    assert abs(deq.backward_res - float(g["backward_res"])) < 1e-2 * float(g["backward_res"])
    names = [name for name, _ in solver.named_parameters()]
    assert sorted("grad." + name for name in names) == sorted(k for k in g.files if k.startswith("grad."))
    for name, p in solver.named_parameters():
        r = rel_l2(p.grad.cpu().numpy(), g["grad." + name])
        print(f"implicit={implicit} {name}: rel L2 vs the reference {r:.3e}")
        assert r < 1e-4, name


def test_default_parameter_backward_is_autograd():
    g, solver, deq, rec, loss, taped_module_calls = _golden_run("SimpleCNN", None, "autograd")
    assert deq.parameter_backward == "autograd" and deq.last_parameter_path == "autograd" and deq.parameter_fallback_reason is None
    assert taped_module_calls == 2


def test_device_parameter_backward_falls_back_for_ffdnet():
    _, s_dev, d_dev, _, _, _ = _golden_run("ffdnet", "device", "autograd")
    _, s_ref, d_ref, _, _, _ = _golden_run("ffdnet", "autograd", "autograd")
    assert d_dev.last_parameter_path == "autograd" and "FFDNet" in d_dev.parameter_fallback_reason
    assert d_ref.last_parameter_path == "autograd" and d_ref.parameter_fallback_reason is None
    for (name, a), (_, b) in zip(s_dev.named_parameters(), s_ref.named_parameters()):
        assert float((a.grad.double() - b.grad.double()).norm() / b.grad.double().norm()) < 1e-6, name


def test_device_parameter_backward_falls_back_for_train_mode_batchnorm():
    def run(mode):
        torch.manual_seed(0)
        net = DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").to(DEV).train()
        solver = deqsci_amd.EquilibriumProxGradSCI(deqsci_amd.A_torch_, deqsci_amd.At_torch_, net, eta=0.2)
        deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=6, tol=1e-9)
        deq.parameter_backward = mode
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
    assert d_dev.last_parameter_path == "autograd" and d_ref.last_parameter_path == "autograd"
    assert "BatchNorm2d" in d_dev.parameter_fallback_reason and d_ref.parameter_fallback_reason is None
    for a, b in zip(g_dev, g_ref):
        assert float((a.double() - b.double()).norm() / b.double().norm()) < 1e-6
