"""CPU: the implicit backward's host-side plan (deqsci_amd/vjp.py) - transposed, flipped, BN-folded layers with explicit ReLU masks -
equals torch.autograd.grad of the module in float64, and the eligibility rules say why a net is refused."""
import pytest
import torch

from deqsci_amd import vjp
from deqsci_amd.cli import build_denoiser
from deqsci_amd.networks import DnCNN, FFDNet


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(m.weight.shape, generator=g)
            m.bias.data = 0.1 * torch.randn(m.bias.shape, generator=g)
            m.running_mean = 0.1 * torch.randn(m.running_mean.shape, generator=g)
            m.running_var = 0.5 + torch.rand(m.running_var.shape, generator=g)
    for name, buf in net.named_buffers():
        if name.endswith(".weight"):                       # RealSNConv2d's stored, normalised weight
            buf.copy_(torch.randn(buf.shape, generator=g) * (2.0 / (9 * buf.shape[1])) ** 0.5)
    return net


def _nets():
    return {"SimpleCNN": build_denoiser("SimpleCNN").eval(),
            "RealSN_SimpleCNN": _randomise(build_denoiser("RealSN_SimpleCNN"), 1).eval(),
            "DnCNN17_bn": _randomise(DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag="denoiser"), 2).eval()}


@pytest.mark.parametrize("kind", ["SimpleCNN", "RealSN_SimpleCNN", "DnCNN17_bn"])
def test_host_plan_equals_float64_autograd(kind):
    net = _nets()[kind].double()
    ok, why = vjp.eligibility(net)
    assert ok, why
    layers, why = vjp.host_plan(net)
    assert layers is not None, why
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 1, 13, 11, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(2, 1, 13, 11, generator=g, dtype=torch.float64)
    want = torch.autograd.grad(net(x), x, v)[0]
    got, masks = vjp.plan_vjp(layers, x.detach(), v)
    assert len(masks) == len(layers) - 1 and all(m is not None for m in masks)
    assert float((got - want).norm() / want.norm()) <= 1e-12


def test_plan_masks_are_relu_prime_zero_at_zero():
    """ReLU'(0) = 0: a unit whose pre-activation is exactly 0 blocks the gradient, as in PyTorch."""
    net = DnCNN(1, num_of_layers=3, lip=0.0, no_bn=True, tag="denoiser").eval().double()
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data.zero_()
    layers, _ = vjp.host_plan(net)
    x = torch.randn(1, 1, 6, 5, dtype=torch.float64, requires_grad=True)
    v = torch.randn(1, 1, 6, 5, dtype=torch.float64)
    net.dncnn[2].weight.data.normal_()
    net.dncnn[4].weight.data.normal_()
    got, masks = vjp.plan_vjp(layers, x.detach(), v)
    assert not any(bool(m.any()) for m in masks)
    assert torch.equal(got, torch.zeros_like(got)) and torch.equal(torch.autograd.grad(net(x), x, v)[0], torch.zeros_like(got))


def test_eligibility_rules_and_reasons():
    ok, why = vjp.eligibility(build_denoiser("SimpleCNN").eval())
    assert ok and "stack" in why
    ok, why = vjp.eligibility(build_denoiser("RealSN_SimpleCNN").eval())
    assert ok
    ok, why = vjp.eligibility(build_denoiser("RealSN_SimpleCNN").train())
    assert not ok and "RealSN" in why and "train" in why
    ok, why = vjp.eligibility(DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag="denoiser").train())
    assert not ok and "BatchNorm2d" in why and "train" in why
    ok, why = vjp.eligibility(DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag="denoiser").eval())
    assert ok
    ok, why = vjp.eligibility(FFDNet(1, tag="ffdnet").eval())
    assert ok and "detach" in why
    ok, why = vjp.eligibility(FFDNet(3, tag="ffdnet").eval())
    assert not ok and "3 channels" in why
    ok, why = vjp.eligibility(FFDNet(1, tag="ffdnet").train())
    assert not ok and "train" in why

    odd = DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="denoiser").eval()
    odd.dncnn[3] = torch.nn.Tanh()
    ok, why = vjp.eligibility(odd)
    assert not ok and "unknown module Tanh" in why

    class Plugin(torch.nn.Module):
        tag = "denoiser"

        def forward(self, x):
            return x
    ok, why = vjp.eligibility(Plugin())
    assert not ok and "Plugin" in why
    ok, why = vjp.eligibility(DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="conv2d").eval())
    assert not ok and "conv2d" in why
    wide = DnCNN(2, num_of_layers=4, lip=0.0, no_bn=True, tag="denoiser").eval()
    ok, why = vjp.eligibility(wide)
    assert not ok and "shapes" in why


def test_deq_implicit_backward_attribute_defaults_and_validation():
    from deqsci_amd import DEQFixedPoint, andersonexp
    from deqsci_amd.solvers import EquilibriumProxGradSCI
    from deqsci_amd.operators import A_torch_, At_torch_
    solver = EquilibriumProxGradSCI(A_torch_, At_torch_, build_denoiser("SimpleCNN").eval(), eta=0.2)
    deq = DEQFixedPoint(solver, andersonexp, m=5)
    assert deq.implicit_backward == "autograd" and deq.last_backward_path is None
    deq.implicit_backward = "sideways"
    with pytest.raises(ValueError, match="implicit_backward"):
        deq._device_map(None, None)
    deq.implicit_backward = "device"
    solver.nonlinear_op.train()
    solver.nonlinear_op = DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser").train()
    assert deq._device_map(None, None) is None and "BatchNorm2d" in deq.backward_fallback_reason
    assert solver.device_vjp_eligibility()[0] is False


@pytest.mark.parametrize("kind", ["SimpleCNN", "RealSN_SimpleCNN", "DnCNN17_bn", "ffdnet"])
def test_engine_and_plans_walk_the_layers_alike(kind):
    """The f-call's layers (engine._Denoiser.fast) and the plan the backward and the diagnostics differentiate are one walk
    (layers.conv_stack): equal weights (the engine's may be channels_last), equal biases or both None, equal ReLU flags."""
    from deqsci_amd.engine import _Denoiser
    net = _randomise(FFDNet(1, tag="ffdnet"), 3).eval() if kind == "ffdnet" else _nets()[kind]
    plan = vjp.ffdnet_plan(net) if kind == "ffdnet" else vjp.host_plan(net)[0]
    den = _Denoiser(net)
    assert den.fast is not None and len(den.fast) == len(plan) == {"SimpleCNN": 4, "RealSN_SimpleCNN": 4, "DnCNN17_bn": 17, "ffdnet": 15}[kind]
    assert any(b is not None for _, b, _ in plan) == (kind in ("DnCNN17_bn", "ffdnet"))
    for (w, b, relu), (pw, pb, prelu) in zip(den.fast, plan):
        assert torch.equal(w, pw) and relu == prelu
        assert (b is None and pb is None) or torch.equal(b, pb)
        assert not w.requires_grad and (b is None or not b.requires_grad)


@pytest.mark.parametrize("what", ["bias", "5x5", "bn_train"])
def test_engine_leaves_a_stack_the_walk_refuses_to_the_module(what):
    """A plugin the walk refuses runs its own forward: fast stays None, the route is "module", the f-call is the module's output."""
    from deqsci_amd.engine import _Denoiser
    net = _randomise(DnCNN(1, num_of_layers=4, lip=0.0, no_bn=False, tag="denoiser"), 4).eval()
    if what == "bias":
        net.dncnn[2] = torch.nn.Conv2d(64, 64, 3, padding=1, bias=True)
    elif what == "5x5":
        net.dncnn[2] = torch.nn.Conv2d(64, 64, 5, padding=2, bias=False)
    else:
        net.dncnn[3].train()
    assert not net.training and vjp.host_plan(net)[0] is None
    den = _Denoiser(net)
    assert den.fast is None
    assert den._route(6, 9, 7, "cpu", den.conv64, False) == "module"
    z1 = torch.randn(2, 3, 9, 7, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        out, is_noise = den.run(z1, 0)
        want = net(z1.view(6, 1, 9, 7)).reshape(2, 3, 9, 7)
    assert is_noise and torch.equal(out, want)
