"""No GPU, no library: vjp.GRAD_MODES held to its users.  The parameter_backward strings DEQFixedPoint._taped_call accepts are "autograd" and
the table's switches, nothing else; training.configure_training tries the table's modes in the table's order and takes the first that
serves; and for a seeded net of each family the parameters a mode answers for (vjp.grad_parameters) are as many as its device rules
count (the .count of the mode's device rule where a layer has a BatchNorm, of _Conv64 where it has none) and as the host walk returns
gradients for (the mode's host rules on vjp._net_param_grads)."""
import pytest
import torch

import deqsci_amd
from deqsci_amd import training, vjp
from deqsci_amd.networks import DnCNN, FFDNet
from deqsci_amd.operators import A_torch_, At_torch_
from deqsci_amd.solvers import EquilibriumProxGradSCI
from test_wgrad_bn_host import seeded_bn_dncnn, seeded_ffdnet


class _Echo(torch.nn.Module):
    """An f that is not this package's map: every device switch falls back to calling it."""

    def forward(self, z, x, Phi, Phi_sum):
        return z


def test_taped_call_accepts_autograd_and_the_tables_switches_only():
    deq = deqsci_amd.DEQFixedPoint(_Echo(), deqsci_amd.andersonexp, max_iter=2)
    z = torch.zeros(1)
    switches = [m.switch for m in vjp.GRAD_MODES]
    assert len(set(switches)) == len(switches) == 4 and "autograd" not in switches
    for switch in ["autograd"] + switches:
        deq.parameter_backward = switch
        assert deq._taped_call(z, None, None, None) is z and deq.last_parameter_path == "autograd"
        assert (deq.parameter_fallback_reason is None) == (switch == "autograd")
        assert switch == "autograd" or vjp.switch_modes(switch)[-1].switch == switch
    others = [m.name for m in vjp.GRAD_MODES] + ["", "Device", "device ", "device+", "device+rsn", "device+bn+train", "device+bn-train+realsn", None, True]
    for switch in others:
        deq.parameter_backward = switch
        assert vjp.switch_modes(switch) is None
        with pytest.raises(ValueError, match="parameter_backward=") as err:
            deq._taped_call(z, None, None, None)
        for known in ["autograd"] + switches:                         # the message names every switch there is
            assert repr(known) in str(err.value), known


def test_every_switch_serves_its_own_mode_last_and_plain_first():
    for m in vjp.GRAD_MODES:
        assert m.serves[0] == "plain" and m.serves[-1] == m.name and set(m.serves) <= set(vjp.GRAD_MODE)
        assert vjp.grad_mode("test", **({} if m.name == "plain" else {m.name: True})) is m
    with pytest.raises(ValueError, match="test: frozen_bn and train_bn exclude one another"):
        vjp.grad_mode("test", frozen_bn=True, train_bn=True)
    for kw in ({"frozen_bn": True}, {"train_bn": True}, {"frozen_bn": True, "train_bn": True}):
        with pytest.raises(ValueError, match="test: train_realsn excludes frozen_bn and train_bn"):
            vjp.grad_mode("test", train_realsn=True, **kw)


def test_configure_training_tries_the_table_in_its_order(monkeypatch):
    net = DnCNN(1, 4, lip=0.0, no_bn=True)
    f = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2)
    names = [m.name for m in vjp.GRAD_MODES]
    assert names == ["plain", "train_realsn", "frozen_bn", "train_bn"]
    for first in range(len(names) + 1):                                 # the modes from `first` on serve the net; len(names): none does
        tried = []

        def eligibility(mode, asked):
            assert asked is net
            tried.append(mode.name)
            return (True, "served") if names.index(mode.name) >= first else (False, f"{mode.name} refuses")
        monkeypatch.setattr(vjp.GradMode, "eligibility", eligibility)
        deq = deqsci_amd.DEQFixedPoint(f, deqsci_amd.andersonexp, max_iter=2)
        deq.engine_options = {"conv64": "fast32", "train_bn": "device", "train_realsn": "device"}
        cfg = training.configure_training(deq, "device")
        assert tried == names[:first + 1]
        options = {"conv64": "fast32"}
        if first < len(names):
            mode = vjp.GRAD_MODES[first]
            options.update([mode.engine_option] if mode.engine_option else [])
            assert cfg.parameter_backward == deq.parameter_backward == mode.switch and "parameter_backward" not in cfg.reasons
        else:
            assert cfg.parameter_backward == "autograd" and cfg.reasons["parameter_backward"] == f"{names[-1]} refuses"
        assert cfg.engine_options == deq.engine_options == options


def _realsn_net():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        return DnCNN(1, 4, lip=1.0, no_bn=True).train()


def _plain_net():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4)
        return DnCNN(1, 5, lip=0.0, no_bn=True).eval()


# family -> (the mode, grad_parameters' keywords - None: conv_weights -, the net, the parameters it has)
FAMILIES = {
    "plain": ("plain", None, _plain_net, 5),
    "plain-under-frozen": ("frozen_bn", {}, _plain_net, 5),
    "realsn": ("train_realsn", {"train_realsn": True}, _realsn_net, 4),
    "frozen-dncnn": ("frozen_bn", {}, lambda: seeded_bn_dncnn(5, 6).eval(), 2 + 3 * 3),
    "train-dncnn": ("train_bn", {"train_bn": True}, lambda: seeded_bn_dncnn(5, 6).train(), 2 + 3 * 3),
    "frozen-ffdnet": ("frozen_bn", {}, lambda: seeded_ffdnet(4).eval(), 2 + 13 * 3),
    "train-ffdnet": ("train_bn", {"train_bn": True}, lambda: seeded_ffdnet(4).train(), 2 + 13 * 3),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_parameters_device_counts_and_host_gradients_agree(family):
    name, kw, make, n_params = FAMILIES[family]
    mode, net = vjp.GRAD_MODE[name], make().double()
    if name == "train_realsn":
        net = net.float()                                               # (realsn_stack asks for fp32)
    ok, why = mode.eligibility(net)
    assert ok, why
    stack, ffdnet, _ = mode.stack(net)
    assert ffdnet == isinstance(net, FFDNet)
    params = vjp.conv_weights(net) if kw is None else vjp.grad_parameters(net, **kw)
    counts = [1] + [(vjp._Conv64 if bn is None else mode.device_rule).count for _, bn, _ in stack[1:-1]] + [1]
    assert len(params) == n_params == sum(counts) and all(isinstance(p, torch.nn.Parameter) for p in params)
    assert all(a is b for a, b in zip(params, mode.parameters(net)))
    dtype = params[0].dtype
    g = torch.Generator().manual_seed(9)
    x, v = torch.rand(2, 1, 8, 8, generator=g).to(dtype), torch.randn(2, 1, 8, 8, generator=g).to(dtype)
    sigma = torch.tensor([0.1, 0.2], dtype=dtype) if ffdnet else None
    with torch.no_grad():
        grads, masks, _ = vjp._net_param_grads("test", net, mode, x, v, sigma, None)
    assert len(grads) == n_params and len(masks) == len(stack) - 1
    assert all(tuple(a.shape) == tuple(p.shape) and bool(torch.isfinite(a).all()) for a, p in zip(grads, params))
