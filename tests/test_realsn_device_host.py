"""No GPU: R3 of csrc/realsn.hip (deqsci_realsn_pack_f32) as the C ABI exports, declares and refuses it; which nets the train-mode RealSN
device paths accept (vjp.param_eligibility(net, train_realsn=True)); the host statement of the weight gradients
(vjp.plan_param_grads_realsn) against torch.autograd through the module's own train-mode forward; the switches' error messages; and
tests/realsn_pack_ref.py, the numpy restatement the GPU tests hold R3 to, against the host packers."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import realsn_cases as rc
import realsn_pack_ref as ref


# ----------------------------------------------------------------------------- the C ABI
def test_entry_is_exported_declared_and_listed():
    from deqsci_amd import _hip
    lib = _hip.load()
    assert hasattr(lib, "deqsci_realsn_pack_f32")
    src = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(deqsci_realsn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    assert len(protos["deqsci_realsn_pack_f32"].split(",")) == 7 == len(_hip.SIGNATURES["deqsci_realsn_pack_f32"])
    hip = open(os.path.join(ROOT, "deqsci_amd", "csrc", "realsn.hip")).read()
    assert re.search(r"\bint\s+deqsci_realsn_pack_f32\s*\(", hip)
    assert callable(_hip.realsn_pack)


def test_arguments_are_refused_before_any_launch():
    """NULL weight or no output -> -1, alignment -> -3, another layer shape, a 4x4 pack of an edge layer and aliasing -> -4: on host
    buffers, with no GPU."""
    from deqsci_amd import _hip
    f = _hip.load().deqsci_realsn_pack_f32
    sizes = {"w": 4 * 64 * 64 * 9, "a": 4 * 64 * 64 * 16, "b": 4 * 64 * 64 * 36, "c": 4 * 64 * 64 * 16}
    buf = (ctypes.c_char * (sum(sizes.values()) + 16 * len(sizes) + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = {}
    for name, nb in sizes.items():
        p[name] = base
        base += nb + 16
    w, a, b, c = p["w"], p["a"], p["b"], p["c"]
    assert f(None, a, b, c, 64, 64, None) == -1 and f(w, None, None, None, 64, 64, None) == -1 and f(w, None, None, None, 1, 64, None) == -1
    for dims in ((64, 32), (2, 64), (1, 1), (3, 3), (0, 64), (64, -1), (32, 32)):
        assert f(w, a, b, c, *dims, None) == -4, dims
    assert f(w, a, b, None, 1, 64, None) == -4 and f(w, a, b, c, 64, 1, None) == -4          # an edge layer has no F(4x4,3x3) pack
    for args in ((w + 4, a, b, c), (w, a + 8, b, c), (w, a, b + 4, c), (w, a, b, c + 12), (w, None, None, c + 4)):
        assert f(*args, 64, 64, None) == -3, args
    assert f(w + 4, a, None, c, 1, 64, None) == -3 and f(w, a, None, c + 8, 64, 1, None) == -3
    # an output on the weight, two outputs on one another, a partial overlap
    assert f(w, w, None, None, 64, 64, None) == -4 and f(w, a, a, None, 64, 64, None) == -4 and f(w, a, None, a, 64, 64, None) == -4
    assert f(w, a, a + sizes["a"] - 16, None, 64, 64, None) == -4 and f(w, w + sizes["w"] - 16, None, None, 64, 64, None) == -4
    assert f(w, a, None, a, 1, 64, None) == -4 and f(w, a, None, a + 4 * 576 - 16, 64, 1, None) == -4 and f(w, None, None, w, 1, 64, None) == -4
    # (an edge layer's packs are 576 floats: buffers that far apart do not overlap)
    assert f(w, None, None, None, 64, 64, None) == -1


# ----------------------------------------------------------------------------- the restatement against the host packers
@pytest.mark.parametrize("kind", ["normal", "integer"])
def test_restatement_has_the_host_packers_layouts(kind):
    from deqsci_amd import _hip, vjp
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.1 if kind == "normal" else torch.randint(-4, 5, (64, 64, 3, 3), generator=g).float() * 24.0
    got, tol = ref.packs(w.numpy()), ref.bound(w.numpy())
    hosts = {"pack": _hip.pack_winograd_weights(w), "pack44": _hip.pack_winograd44_weights(w), "pack_t": _hip.pack_winograd_weights(vjp._transposed(w))}
    for name, host in hosts.items():
        a, h = got[name], host.numpy()
        assert a.shape == h.shape and a.dtype == np.float32
        d = np.abs(a.astype(np.float64) - h.astype(np.float64))
        assert bool((d <= ref.ulp32(np.maximum(np.abs(a), np.abs(h))) + tol[name]).all()), name
    if kind == "integer":                                   # multiples of 24: G g G^T of F(2x2,3x3) is an integer, every evaluation exact
        assert np.array_equal(got["pack"], hosts["pack"].numpy()) and np.array_equal(got["pack_t"], hosts["pack_t"].numpy())
    for cin, cout in ((1, 64), (64, 1)):
        w = torch.randn(cout, cin, 3, 3, generator=g)
        got = ref.packs(w.numpy())
        own, other = (_hip.pack_c1_to_64_weights, _hip.pack_c64_to_1_weights) if cin == 1 else (_hip.pack_c64_to_1_weights, _hip.pack_c1_to_64_weights)
        assert got["pack44"] is None
        assert torch.equal(torch.from_numpy(got["pack"]), own(w)) and torch.equal(torch.from_numpy(got["pack_t"]), other(vjp._transposed(w)))
        assert tuple(got["pack"].shape) == _hip.realsn_pack_shapes(cin, cout)["pack"] and tuple(got["pack_t"].shape) == _hip.realsn_pack_shapes(cin, cout)["pack_t"]


# ----------------------------------------------------------------------------- eligibility
def _net(layers=4, **kw):
    from deqsci_amd.networks import DnCNN
    return DnCNN(1, layers, **{"lip": 1.0, "no_bn": True, **kw})


def test_eligibility_accepts_the_train_mode_realsn_stacks():
    from deqsci_amd import vjp
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    for net in (_net().train(), _net(6, adaptive=True).train(), _net(4, lip=0.0).train()):
        ok, why = vjp.param_eligibility(net, train_realsn=True)
        assert ok and "RealSN" in why, why
        params = vjp.grad_parameters(net, train_realsn=True)
        convs = [m for m in net.dncnn if isinstance(m, (RealSNConv2d, torch.nn.Conv2d))]
        assert len(params) == len(convs)
        for p, m in zip(params, convs):
            assert p is (m.weight_orig if isinstance(m, RealSNConv2d) else m.weight)
    assert vjp.eligibility(_net().train(), train_realsn=True) == (True, vjp._REALSN_OK)
    # what "device" refuses it keeps refusing, in its own words
    assert vjp.param_eligibility(_net().train())[1] == "RealSNConv2d (its parameter is weight_orig behind the spectral normalisation)"
    assert vjp.eligibility(_net().train())[1] == "RealSNConv2d in train mode (its weight is renormalised by the power iteration)"


def test_eligibility_refuses_with_a_reason():
    from deqsci_amd import vjp
    from deqsci_amd.networks import DnCNN, FFDNet
    bn = DnCNN(1, 5, lip=1.0, no_bn=False).train()
    ok, why = vjp.param_eligibility(bn, train_realsn=True)
    assert not ok and "BatchNorm" in why
    assert "BatchNorm" in vjp.eligibility(bn, train_realsn=True)[1]
    biased = _net(4, lip=0.0)
    biased.dncnn[2] = torch.nn.Conv2d(64, 64, 3, padding=1, bias=True)
    ok, why = vjp.param_eligibility(biased.train(), train_realsn=True)
    assert not ok and "bias" in why
    ok, why = vjp.param_eligibility(FFDNet(1, "ffdnet").train(), train_realsn=True)
    assert not ok and "FFDNet" in why
    ok, why = vjp.param_eligibility(_net().eval(), train_realsn=True)
    assert not ok and "eval mode" in why
    ok, why = vjp.param_eligibility(_net().train().double(), train_realsn=True)
    assert not ok and "fp32" in why
    with pytest.raises(ValueError, match="excludes"):
        vjp.param_eligibility(_net().train(), train_bn=True, train_realsn=True)
    with pytest.raises(ValueError, match="BatchNorm"):
        vjp.grad_parameters(bn, train_realsn=True)


# ----------------------------------------------------------------------------- the host statement
@pytest.mark.parametrize("kind", ["simplecnn", "adaptive6", "mixed"])
def test_plan_param_grads_realsn_against_autograd(kind):
    """The yardstick: torch.autograd through the module's own train-mode forward (RealSNConv2d's CPU path is differentiable), 2x1x19x23,
    float32.  1e-5 relative L2: what the CPU weight_grad restatement is held to."""
    from deqsci_amd import vjp
    torch.manual_seed(11)
    net = {"simplecnn": lambda: _net(), "adaptive6": lambda: _net(6, adaptive=True), "mixed": lambda: _net()}[kind]().train()
    if kind == "mixed":
        net.dncnn[2] = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False)
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 1, 19, 23, generator=g)
    v = torch.randn(2, 1, 19, 23, generator=g)
    theirs, mine, untouched = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(net)
    xr = x.clone().requires_grad_(True)
    theirs(xr).backward(v)
    want = [p.grad for p in vjp.grad_parameters(theirs, train_realsn=True)]
    grads, masks = vjp.plan_param_grads_realsn(untouched, x, v)
    for a, b in zip(untouched.state_dict().values(), net.state_dict().values()):
        assert torch.equal(a, b)                                        # the module is left alone unless asked
    grads, masks, gx = vjp.plan_param_grads_realsn(mine, x, v, input_grad=True, update=True)
    assert len(grads) == len(want) == len(masks) + 1
    figures = [rc.rel_l2(a, b) for a, b in zip(grads, want)] + [rc.rel_l2(gx, xr.grad)]
    print(kind, "relative L2 per parameter, then the input:", " ".join(f"{f:.2e}" for f in figures))
    assert max(figures) <= 1e-5
    for (name, a), b in zip(mine.state_dict().items(), theirs.state_dict().values()):
        assert torch.equal(a, b), name                                  # weight_u and weight as the module's own forward leaves them
    assert not torch.equal(mine.dncnn[0].weight_u, net.dncnn[0].weight_u)


# ----------------------------------------------------------------------------- the switches
def test_switches_reject_unknown_values_and_name_the_new_ones():
    import deqsci_amd
    from deqsci_amd.engine import _Denoiser
    from deqsci_amd.solvers import EquilibriumProxGradSCI
    from deqsci_amd.operators import A_torch_, At_torch_
    net = _net().train()
    f = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    deq = deqsci_amd.DEQFixedPoint(f, deqsci_amd.andersonexp, max_iter=2)
    deq.implicit_backward = "device+rsn"
    with pytest.raises(ValueError, match=r"device\+realsn"):
        deq._device_map(None, None)
    deq.parameter_backward = "realsn"
    with pytest.raises(ValueError, match=r"device\+realsn"):
        deq._taped_call(None, None, None, None)
    with pytest.raises(ValueError, match="train_realsn"):
        _Denoiser(net, train_realsn="gpu")
    assert f.device_param_eligibility(train_realsn=True) == (True, "train-mode RealSN conv + ReLU stack")
    assert f.device_vjp_eligibility(train_realsn=True)[0] and not f.device_vjp_eligibility()[0] and not f.device_param_eligibility()[0]
