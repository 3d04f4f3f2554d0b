"""CPU: the host side of the frozen-BatchNorm weight gradients (deqsci_amd/vjp.py: param_eligibility(frozen_bn=True), grad_parameters,
plan_param_grads_frozen_bn), the "device+bn" switch, and the argument validation of csrc/wgrad_bn.hip's entry points, which happens before
any launch."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from deqsci_amd import _hip, checkpoint, vjp
from deqsci_amd.cli import build_denoiser, build_pipeline
from deqsci_amd.networks import DnCNN, FFDNet


def seeded_bn_dncnn(layers, seed):
    """conv + BN + ReLU DnCNN in eval mode: He-scaled weights, non-trivial running statistics, gamma with an exact 0 and negative entries."""
    g = torch.Generator().manual_seed(seed)
    net = DnCNN(1, num_of_layers=layers, lip=0.0, no_bn=False, tag="denoiser")
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.weight.shape[1])) ** 0.5
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(64, generator=g)
            m.weight.data[3] = 0.0
            m.weight.data[[7, 20, 41]] *= -1.0
            m.bias.data = 0.2 * torch.randn(64, generator=g)
            m.bias.data[3] = 0.3                                        # (the gamma = 0 unit is y = beta: positive, so its ReLU passes the gradient)
            m.running_mean.copy_(0.3 * torch.randn(64, generator=g))
            m.running_var.copy_(0.5 + torch.rand(64, generator=g))
    return net.eval()


def seeded_ffdnet(seed):
    g = torch.Generator().manual_seed(seed)
    net = FFDNet(1, tag="ffdnet")
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.weight.shape[1])) ** 0.5
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(64, generator=g)
            m.weight.data[5] = 0.0
            m.weight.data[[1, 33]] *= -1.0
            m.bias.data = 0.2 * torch.randn(64, generator=g)
            m.bias.data[5] = 0.3
            m.running_mean.copy_(0.3 * torch.randn(64, generator=g))
            m.running_var.copy_(0.5 + torch.rand(64, generator=g))
    return net.eval()


def test_defaults_refuse_ffdnet_and_batchnorm_as_before():
    ok, why = vjp.param_eligibility(FFDNet(1, tag="ffdnet").eval())
    assert not ok and why == "FFDNet: its 5 -> 64 / 64 -> 4 edge layers and BatchNorm2d parameters have no device weight gradient"
    for net in (seeded_bn_dncnn(5, 1), seeded_bn_dncnn(5, 1).train()):
        for answer in (vjp.param_eligibility(net), vjp.param_eligibility(net, frozen_bn=False)):
            assert answer == (False, "BatchNorm2d (its gamma / beta gradients, and the batch statistics in train mode, have no device kernel)")
    assert vjp.param_eligibility(build_denoiser("SimpleCNN").eval()) == (True, "bias-free conv + ReLU stack")


def test_frozen_bn_accepts_eval_ffdnet_and_bn_dncnn():
    ok, why = vjp.param_eligibility(FFDNet(1, tag="ffdnet").eval(), frozen_bn=True)
    assert ok, why
    ok, why = vjp.param_eligibility(build_denoiser("ffdnet").eval(), frozen_bn=True)
    assert ok, why
    for depth in (3, 5, 17):
        ok, why = vjp.param_eligibility(seeded_bn_dncnn(depth, 2), frozen_bn=True)
        assert ok, (depth, why)
    # what "device" serves, "device+bn" serves
    ok, why = vjp.param_eligibility(build_denoiser("SimpleCNN").eval(), frozen_bn=True)
    assert ok, why


def test_frozen_bn_refusals_name_the_cause():
    ok, why = vjp.param_eligibility(seeded_bn_dncnn(5, 1).train(), frozen_bn=True)
    assert not ok and "train mode" in why
    ok, why = vjp.param_eligibility(FFDNet(1, tag="ffdnet").train(), frozen_bn=True)
    assert not ok and "train mode" in why and "FFDNet" in why
    net = seeded_bn_dncnn(5, 1)
    net.dncnn[3] = torch.nn.BatchNorm2d(64, affine=False).eval()
    ok, why = vjp.param_eligibility(net, frozen_bn=True)
    assert not ok and "affine" in why
    net = seeded_bn_dncnn(5, 1)
    net.dncnn[3] = torch.nn.BatchNorm2d(64, track_running_stats=False).eval()
    ok, why = vjp.param_eligibility(net, frozen_bn=True)
    assert not ok and "running statistics" in why
    ok, why = vjp.param_eligibility(build_denoiser("RealSN_SimpleCNN").eval(), frozen_bn=True)
    assert not ok and "RealSNConv2d" in why
    ok, why = vjp.param_eligibility(FFDNet(3, tag="ffdnet").eval(), frozen_bn=True)
    assert not ok and "3 channels" in why
    ok, why = vjp.param_eligibility(DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="conv2d").eval(), frozen_bn=True)
    assert not ok and "'conv2d'" in why
    biased = seeded_bn_dncnn(5, 1)
    biased.dncnn[2] = torch.nn.Conv2d(64, 64, kernel_size=3, padding=1, bias=True)
    ok, why = vjp.param_eligibility(biased, frozen_bn=True)
    assert not ok and "bias" in why
    with pytest.raises(ValueError, match="train mode"):
        vjp.grad_parameters(seeded_bn_dncnn(5, 1).train())


def test_grad_parameters_of_ffdnet_are_the_goldens_in_order():
    g = np.load(os.path.join(GOLDEN, "backward_ffdnet.npz"))
    keys = [k for k in g.files if k.startswith("grad.")]
    assert len(keys) == 41
    net = build_denoiser("ffdnet").eval()
    params = vjp.grad_parameters(net)
    names = {id(p): name for name, p in net.named_parameters()}
    assert ["grad.nonlinear_op." + names[id(p)] for p in params] == keys
    assert [tuple(p.shape) for p in params] == [g[k].shape for k in keys]
    # a BN DnCNN: conv weight, then its BatchNorm's weight and bias, in module order; a plain stack: conv_weights
    net = seeded_bn_dncnn(4, 1)
    assert [name for name, _ in net.named_parameters()] == ["dncnn.0.weight", "dncnn.2.weight", "dncnn.3.weight", "dncnn.3.bias",
                                                              "dncnn.5.weight", "dncnn.6.weight", "dncnn.6.bias", "dncnn.8.weight"]
    assert all(a is b for a, b in zip(vjp.grad_parameters(net), net.parameters())) and len(vjp.grad_parameters(net)) == 8
    plain = build_denoiser("SimpleCNN").eval()
    assert all(a is b for a, b in zip(vjp.grad_parameters(plain), vjp.conv_weights(plain)))


def _check_against_autograd(net, x, v, sigma):
    params = vjp.grad_parameters(net)
    want = torch.autograd.grad(net(x) if sigma is None else net(x, sigma), params, v)
    got, masks = vjp.plan_param_grads_frozen_bn(net, x, v, sigma)
    assert len(got) == len(want) == len(params)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == torch.float64
        assert float((a - b).norm() / b.norm()) <= 1e-10, i
    again, _ = vjp.plan_param_grads_frozen_bn(net, x, v, sigma, masks=masks)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    return got


@pytest.mark.parametrize("H,W", [(6, 6), (10, 14)])
def test_plan_param_grads_frozen_bn_equals_float64_autograd_ffdnet(H, W):
    net = seeded_ffdnet(4).double()
    g = torch.Generator().manual_seed(H)
    x = torch.rand(3, 1, H, W, generator=g, dtype=torch.float64)
    v = torch.randn(3, 1, H, W, generator=g, dtype=torch.float64)
    sigma = torch.tensor([0.1, 0.235, 0.02], dtype=torch.float64)                # per image
    got = _check_against_autograd(net, x, v, sigma)
    assert len(got) == 41 and got[0].shape == (64, 5, 3, 3) and got[-1].shape == (4, 64, 3, 3)
    assert float(got[0][:, 0].abs().max()) > 0                                   # sigma's channel of the first weight has a gradient
    with pytest.raises(ValueError, match="sigma"):
        vjp.plan_param_grads_frozen_bn(net, x, v)
    with pytest.raises(ValueError, match="even"):
        vjp.plan_param_grads_frozen_bn(net, x[:, :, :5], v[:, :, :5], sigma)


def test_plan_param_grads_frozen_bn_equals_float64_autograd_bn_dncnn():
    net = seeded_bn_dncnn(5, 6).double()
    gammas = [m.weight for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert all(bool((w == 0).any()) and bool((w < 0).any()) for w in gammas)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 1, 13, 11, generator=g, dtype=torch.float64)
    v = torch.randn(3, 1, 13, 11, generator=g, dtype=torch.float64)
    got = _check_against_autograd(net, x, v, None)
    assert len(got) == 2 + 3 * 3
    # the gradient of a gamma that is exactly 0 is not 0: nothing divides by it
    assert float(got[2][3].abs()) > 0
    # without a BatchNorm it is plan_param_grads
    plain = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4, device="cpu")[0].nonlinear_op.double()
    a, _ = vjp.plan_param_grads_frozen_bn(plain, x, v)
    b, _ = vjp.plan_param_grads(vjp.host_plan(plain)[0], x, v)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def mixed_bn_dncnn():
    """seeded_bn_dncnn(5, 6) without its second BatchNorm: 64 -> 64 layers with and without one in the same stack (eval mode)."""
    net = seeded_bn_dncnn(5, 6)
    del net.dncnn[[i for i, m in enumerate(net.dncnn) if isinstance(m, torch.nn.BatchNorm2d)][1]]
    return net


def test_plan_param_grads_frozen_bn_equals_float64_autograd_mixed_net():
    net = mixed_bn_dncnn().double()
    assert vjp.param_eligibility(net, frozen_bn=True) == (True, "bias-free conv [+ frozen BN] + ReLU stack")
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 1, 12, 20, generator=g, dtype=torch.float64)
    v = torch.randn(2, 1, 12, 20, generator=g, dtype=torch.float64)
    assert len(_check_against_autograd(net, x, v, None)) == 2 + 3 + 1 + 3


def test_a_plain_net_gets_the_same_gradients_from_all_three_host_statements():
    """One walk: without a BatchNorm the three statements run the same rule in the same order, so their gradients are bit-equal."""
    net = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4, device="cpu")[0].nonlinear_op.double()
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 1, 12, 20, generator=g, dtype=torch.float64)
    v = torch.randn(2, 1, 12, 20, generator=g, dtype=torch.float64)
    plain, masks = vjp.plan_param_grads(vjp.host_plan(net)[0], x, v)
    frozen, _ = vjp.plan_param_grads_frozen_bn(net.eval(), x, v)
    train, masks_train, gx = vjp.plan_param_grads_train_bn(net.train(), x, v, input_grad=True)
    assert len(plain) == len(frozen) == len(train) == len(vjp.conv_weights(net))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(plain, frozen, train))
    assert all(torch.equal(a, b) for a, b in zip(masks, masks_train)) and torch.equal(gx, vjp.plan_vjp(vjp.host_plan(net)[0], x, v)[0])


# ----------------------------------------------------------------------------- one structure check behind every entry point
def _convs(seq):
    return [i for i, m in enumerate(seq) if isinstance(m, torch.nn.Conv2d)]


def _wrong_middle_shape(seq):
    seq[_convs(seq)[1]] = torch.nn.Conv2d(32, 64, kernel_size=3, padding=1, bias=False)


def _missing_relu(seq):
    del seq[[i for i, m in enumerate(seq) if isinstance(m, torch.nn.ReLU)][1]]


def _relu_behind_the_last(seq):
    seq.append(torch.nn.ReLU())


def _bn_behind_the_first(seq):
    seq.insert(1, torch.nn.BatchNorm2d(64))


def _bn_behind_the_last(seq):
    seq.append(torch.nn.BatchNorm2d(seq[_convs(seq)[-1]].out_channels))


def _too_few_layers(seq):
    del seq[2:]


def _weight_no_parameter(seq):
    conv = seq[_convs(seq)[1]]
    w = conv.weight.detach().clone()
    del conv.weight
    conv.register_buffer("weight", w)


# malformation -> (the cause every entry point names, the entry points that look at weights as nn.Parameters only)
MALFORMED = {_wrong_middle_shape: ("layer shapes", False), _missing_relu: ("ReLU pattern", False), _relu_behind_the_last: ("ReLU pattern", False),
             _bn_behind_the_first: ("BatchNorm2d behind the first or the last layer", False),
             _bn_behind_the_last: ("BatchNorm2d behind the first or the last layer", False), _too_few_layers: ("layer shapes", False),
             _weight_no_parameter: ("not an nn.Parameter", True)}
FAMILIES = {"plain": lambda: DnCNN(1, num_of_layers=5, lip=0.0, no_bn=True, tag="denoiser"), "bn-dncnn": lambda: seeded_bn_dncnn(5, 1),
            "ffdnet": lambda: seeded_ffdnet(1)}


def _raised(fn, *args, **kw):
    with pytest.raises(ValueError) as info:
        fn(*args, **kw)
    return False, str(info.value)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("malform", list(MALFORMED), ids=lambda f: f.__name__.strip("_"))
def test_every_entry_point_refuses_a_malformed_stack_with_the_same_cause(malform, family):
    """eligibility, jacobian_eligibility, param_eligibility in its three modes, grad_parameters and ffdnet_plan all ask vjp._structure_refusal
    (the parameter entry points through vjp.bn_stack): a malformed stack is refused everywhere, for the same cause."""
    cause, parameters_only = MALFORMED[malform]
    net = FAMILIES[family]()
    seq = net.intermediate_dncnn.itermediate_dncnn if family == "ffdnet" else net.dncnn
    assert vjp.param_eligibility(net.eval(), frozen_bn=True)[0] and vjp.param_eligibility(net.train(), train_bn=True)[0]
    malform(seq)
    answers = {}
    net.eval()
    if not parameters_only:
        if family == "ffdnet":
            answers["ffdnet_plan"] = _raised(vjp.ffdnet_plan, net)
        else:
            answers["eligibility"], answers["jacobian_eligibility"] = vjp.eligibility(net), vjp.jacobian_eligibility(net)
    elif family == "ffdnet":
        assert len(vjp.ffdnet_plan(net)) == 15                                  # (the input product needs no nn.Parameter)
    else:
        assert vjp.eligibility(net)[0] and vjp.jacobian_eligibility(net)[0]
    if family == "plain" and "BatchNorm2d" not in cause:                       # (the default mode refuses any BatchNorm2d before it looks further)
        answers["param_eligibility"] = vjp.param_eligibility(net)
    answers["param_eligibility frozen"] = vjp.param_eligibility(net, frozen_bn=True)
    answers["grad_parameters"] = _raised(vjp.grad_parameters, net)
    net.train()
    answers["param_eligibility train"] = vjp.param_eligibility(net, train_bn=True)
    answers["grad_parameters train"] = _raised(vjp.grad_parameters, net, train_bn=True)
    for who, (ok, why) in answers.items():
        assert not ok and cause in why, (who, why)
    if family == "plain" and "BatchNorm2d" in cause:
        ok, why = vjp.param_eligibility(net)
        assert not ok and "BatchNorm2d" in why


def test_deq_switch_accepts_device_bn_and_refuses_a_misspelling():
    import deqsci_amd
    solver, deq = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), 4, device="cpu")
    assert deq.parameter_backward == "autograd"
    ok, why = solver.device_param_eligibility()
    assert not ok and "FFDNet" in why
    assert solver.device_param_eligibility(frozen_bn=False) == (ok, why)
    ok, why = solver.device_param_eligibility(frozen_bn=True)
    assert ok, why
    other = deqsci_amd.EquilibriumProxGradSCI(lambda x, Phi: x, lambda y, Phi: y, solver.nonlinear_op, eta=0.2)
    ok, why = other.device_param_eligibility(frozen_bn=True)
    assert not ok and "custom A / At" in why
    solver.nonlinear_op.train()
    ok, why = solver.device_param_eligibility(frozen_bn=True)
    assert not ok and "train mode" in why
    with pytest.raises(ValueError, match="train mode"):
        solver.forward_param_device(None, None, None, None, frozen_bn=True)
    solver.nonlinear_op.eval()
    deq.parameter_backward = "device-bn"
    with pytest.raises(ValueError, match=r"'autograd', 'device' or 'device\+bn'"):
        deq._taped_call(None, None, None, None)
    # an accepted value passes the check and goes on to the call itself
    deq.parameter_backward = "device+bn"
    with pytest.raises(Exception) as info:
        deq._taped_call(None, None, None, None)
    assert "parameter_backward" not in str(info.value)


def test_wgrad_bn_entry_points_validate_before_any_launch():
    lib = _hip.load()
    wsb, old = lib.deqsci_wgrad_bn_workspace_bytes, lib.deqsci_wgrad_workspace_bytes
    assert wsb(0, 4, 4) == 0 and wsb(1, 0, 4) == 0 and wsb(1, 4, -1) == 0 and wsb(1, 1 << 21, 4) == 0 and wsb(1 << 20, 1 << 20, 64) == 0
    assert wsb(1, 1, 1) == (9 * 64 * 64 + 64) * 8                                       # one workgroup: W0's entries and the 64 sums of g
    assert wsb(64, 256, 256) == 256 * (9 * 64 * 64 + 64) * 8                            # bounded: it does not grow with the batch
    assert old(1, 1, 1) == 9 * 64 * 64 * 8 and old(64, 256, 256) == 256 * 9 * 64 * 64 * 8   # the existing query is what it was
    far = 1 << 40                                                                       # addresses only: validation dereferences nothing
    bn, w2 = lib.deqsci_wgrad3x3_c64_c64_bn_f32, lib.deqsci_wgrad3x3_shuffle_f32
    x, g, w, sc, dw, ds, dd, ws = (far + (i << 24) for i in range(8))
    good = [x, g, w, sc, dw, ds, dd]
    # NULL -> -1
    for i in range(7):
        args = list(good)
        args[i] = None
        assert bn(*args, 1, 4, 4, ws, None) == -1, i
    assert bn(*good, 1, 4, 4, None, None) == -1
    assert w2(None, sc, 0, g, dw, 0, 1, 4, 4, ws, None) == -1 and w2(x, sc, 0, None, dw, 0, 1, 4, 4, ws, None) == -1
    assert w2(x, sc, 0, g, None, 1, 1, 4, 4, ws, None) == -1 and w2(x, sc, 0, g, dw, 1, 1, 4, 4, None, None) == -1
    assert w2(x, None, 0, g, dw, 0, 1, 4, 4, ws, None) == -1                             # which = 0 reads sigma ...
    # sizes -> -2; W2's H, W are the image's: its first layer is a 2x2 pixel-unshuffle
    assert bn(*good, 0, 4, 4, ws, None) == -2 and bn(*good, 1, 0, 4, ws, None) == -2 and bn(*good, 1, 4, -4, ws, None) == -2
    assert w2(x, sc, 0, g, dw, 0, 0, 4, 4, ws, None) == -2 and w2(x, sc, 0, g, dw, 0, 1, 4, 0, ws, None) == -2
    assert w2(x, sc, 0, g, dw, 0, 1, 5, 4, ws, None) == -2 and w2(x, sc, 0, g, dw, 1, 1, 4, 7, ws, None) == -2
    assert w2(x, None, 0, g, dw, 1, 1, 5, 4, ws, None) == -2                             # ... which = 1 does not: the odd side is what is wrong
    # alignment -> -3
    assert bn(x + 4, g, w, sc, dw, ds, dd, 1, 4, 4, ws, None) == -3 and bn(x, g + 8, w, sc, dw, ds, dd, 1, 4, 4, ws, None) == -3
    assert bn(x, g, w + 2, sc, dw, ds, dd, 1, 4, 4, ws, None) == -3 and bn(x, g, w, sc + 1, dw, ds, dd, 1, 4, 4, ws, None) == -3
    assert bn(x, g, w, sc, dw + 2, ds, dd, 1, 4, 4, ws, None) == -3 and bn(x, g, w, sc, dw, ds + 2, dd, 1, 4, 4, ws, None) == -3
    assert bn(x, g, w, sc, dw, ds, dd + 1, 1, 4, 4, ws, None) == -3 and bn(*good, 1, 4, 4, ws + 4, None) == -3
    assert w2(x + 2, sc, 0, g, dw, 0, 1, 4, 4, ws, None) == -3 and w2(x, sc + 1, 0, g, dw, 0, 1, 4, 4, ws, None) == -3
    assert w2(x, sc, 0, g + 1, dw, 0, 1, 4, 4, ws, None) == -3 and w2(x, sc, 0, g, dw + 2, 1, 1, 4, 4, ws, None) == -3
    assert w2(x, sc, 0, g, dw, 0, 1, 4, 4, ws + 4, None) == -3
    # overlap / unsupported -> -4
    assert bn(x, g, w, sc, x, ds, dd, 1, 4, 4, ws, None) == -4 and bn(x, g, w, sc, w, ds, dd, 1, 4, 4, ws, None) == -4     # dw over an input
    assert bn(x, g, w, sc, dw, sc, dd, 1, 4, 4, ws, None) == -4 and bn(x, g, w, sc, dw, ds, g + 64, 1, 4, 4, ws, None) == -4
    assert bn(x, g, w, sc, dw, ds, ds + 32, 1, 4, 4, ws, None) == -4 and bn(x, g, w, sc, dw, dw + 64, dd, 1, 4, 4, ws, None) == -4  # outputs over one another
    assert bn(*good, 1, 4, 4, x, None) == -4 and bn(*good, 1, 4, 4, dw + 8, None) == -4 and bn(*good, 1, 4, 4, dd, None) == -4
    assert bn(*good, 1, 1 << 21, 4, ws, None) == -4 and bn(*good, 1 << 20, 1 << 20, 64, ws, None) == -4
    assert w2(x, sc, 0, g, dw, 2, 1, 4, 4, ws, None) == -4 and w2(x, sc, 0, g, dw, -1, 1, 4, 4, ws, None) == -4            # which is 0 or 1
    assert w2(x, sc, 2, g, dw, 0, 1, 4, 4, ws, None) == -4                                                                # sigma_stride is 0 or 1
    assert w2(x, sc, 0, g, x, 0, 1, 4, 4, ws, None) == -4 and w2(x, sc, 0, g, g + 64, 1, 1, 4, 4, ws, None) == -4
    assert w2(x, sc, 0, g, sc, 0, 1, 4, 4, ws, None) == -4 and w2(x, sc, 0, g, dw, 0, 1, 4, 4, x, None) == -4
    assert w2(x, sc, 0, g, dw, 1, 1, 4, 4, g, None) == -4 and w2(x, sc, 0, g, dw, 0, 1, 4, 4, dw + 8, None) == -4
    assert w2(x, sc, 0, g, dw, 0, 1, 4, 1 << 22, ws, None) == -4


def test_wgrad_bn_kernels_compile_without_spills(tmp_path):
    """csrc/wgrad_bn.hip's W0-BN is W0's body with one more accumulator per lane, at the same register budget (9 x 16 accumulators beside the
    next tile's loads), and W2 holds 45 accumulators per lane: every kernel of the file compiles for gfx950 with no spill and no per-lane
    stack, and W0-BN's code is the matrix instructions.  (Cross-compiles without a GPU, ~10 s.)"""
    import re
    import subprocess
    from conftest import ROOT
    src = os.path.join(ROOT, "deqsci_amd", "csrc", "wgrad_bn.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deqsci_amd", "csrc"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage",
           "-save-temps=obj"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    found = re.findall(r"Function Name: (\S*wgrad\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+)"
                       r".*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", out.stderr, flags=re.S)
    assert len(found) == 5, out.stderr[-2000:]      # wgrad_c64_kernel<true>, wgrad_bn_sum_kernel, wgrad_shuffle_kernel<0 / 1>, wgrad_shuffle_sum_kernel
    for name, vgprs, agprs, stack, sspill, vspill, lds in found:
        assert int(vgprs) + int(agprs) <= 512 and (int(stack), int(sspill), int(vspill)) == (0, 0, 0), (name, vgprs, agprs, stack, sspill, vspill)
        assert int(lds) <= 64 << 10, (name, lds)
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(tmp_path)
    assert open(tmp_path / asm[0]).read().count("v_mfma_f32_32x32x2_f32") >= 9
