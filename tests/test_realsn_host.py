"""Host: RealSN in train mode without a GPU - the C ABI's exports and argument checks (they run before any launch), the CPU restatement
(deqsci_amd.realsn) against the reference's own numbers (tests/golden/realsn_train.npz, tests/golden/make_realsn_golden.py), the gradient
formula against autograd, RealSNConv2d's train-mode forward, and operator_norm against a dense singular value.

Tolerances.  The reference's fp32 results sit within 1.4e-7 (cur_sigma), 5.4e-7 (u) and 1.8e-7 (weight, gradient) of float64 on these cases
(the generator prints the figures); two fp32 orders of the same sums differ by that much, so the fp32 restatement is held to 1e-6 against
the reference's tensors.  Float64 against float64: 1e-12.  Against the reference's tensors of a whole training step: 1e-4, the
project's standing tolerance.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
import realsn_cases as rc


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "realsn_train.npz")))


def _ids(case):
    return rc.case_tag(*case)[2:]


# ----------------------------------------------------------------------------- the C ABI
def test_exports_and_argument_counts():
    from deqsci_amd import _hip
    lib = _hip.load()
    for name in ("deqsci_realsn_power_f32", "deqsci_realsn_grad_f32", "deqsci_realsn_workspace_bytes"):
        assert hasattr(lib, name), name
    assert "deqsci_realsn_workspace_bytes" in _hip.OTHER_EXPORTS
    src = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\b(?:int|size_t)\s+(deqsci_realsn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    assert len(protos["deqsci_realsn_power_f32"].split(",")) == 14 == len(_hip.SIGNATURES["deqsci_realsn_power_f32"])
    assert len(protos["deqsci_realsn_grad_f32"].split(",")) == 13 == len(_hip.SIGNATURES["deqsci_realsn_grad_f32"])
    assert len(protos["deqsci_realsn_workspace_bytes"].split(",")) == 4 == len(lib.deqsci_realsn_workspace_bytes.argtypes)
    assert "deqsci_amd/csrc/realsn.hip" in open(os.path.join(ROOT, "Makefile")).read()


def test_workspace_query():
    from deqsci_amd import _hip
    lib = _hip.load()
    for cin, cout in rc.LAYERS:
        for h, w in rc.MAPS + ((1, 1 << 20), (1024, 1024)):
            nb = lib.deqsci_realsn_workspace_bytes(cin, cout, h, w)
            # at least t1, t2 and C in fp32, and a float64 partial; a whole number of 16-byte pieces
            assert nb % 16 == 0 and nb >= 4 * ((cin + cout) * h * w + 9 * cin * cout) + 8, (cin, cout, h, w, nb)
    for bad in ((2, 64, 4, 4), (64, 32, 4, 4), (1, 1, 4, 4), (64, 64, 0, 4), (64, 64, 4, -1), (0, 64, 4, 4), (64, 64, 1025, 1024),
                (64, 64, 1 << 21, 1)):
        assert lib.deqsci_realsn_workspace_bytes(*bad) == 0, bad


def test_arguments_are_refused_before_any_launch():
    """NULL -> -1, sizes -> -2, alignment -> -3, unsupported layers, oversized maps and aliasing -> -4: on host buffers, with no GPU."""
    from deqsci_amd import _hip
    lib = _hip.load()
    cin, cout, h, w = 1, 64, 2, 3
    nws = lib.deqsci_realsn_workspace_bytes(cin, cout, h, w)
    sizes = {"W": 4 * 576, "u": 4 * cout * h * w, "v": 4 * cin * h * w, "weight": 4 * 576, "record": 24, "ws": nws, "G": 4 * 576, "dW": 4 * 576}
    buf = (ctypes.c_char * (sum(sizes.values()) + 16 * len(sizes) + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = {}
    for name, nb in sizes.items():
        p[name] = base
        base += (nb + 15) // 16 * 16 + 16

    def power(W="W", u="u", v="v", weight="weight", record="record", ws="ws", n=1, dims=(cin, cout, h, w), off=None):
        a = {k: (None if val is None else p[val] + ((off or {}).get(k, 0))) for k, val in dict(W=W, u=u, v=v, weight=weight, record=record, ws=ws).items()}
        return lib.deqsci_realsn_power_f32(a["W"], a["u"], a["v"], a["weight"], a["record"], n, 0.84, 1e-12, *dims, a["ws"], None)

    def grad(G="G", W="W", u="u", v="v", record="record", dW="dW", ws="ws", dims=(cin, cout, h, w), off=None):
        a = {k: (None if val is None else p[val] + ((off or {}).get(k, 0))) for k, val in dict(G=G, W=W, u=u, v=v, record=record, dW=dW, ws=ws).items()}
        return lib.deqsci_realsn_grad_f32(a["G"], a["W"], a["u"], a["v"], a["record"], a["dW"], 0.84, *dims, a["ws"], None)

    for name in ("W", "u", "v", "weight", "record", "ws"):
        assert power(**{name: None}) == -1, name
    for name in ("G", "W", "u", "v", "record", "dW", "ws"):
        assert grad(**{name: None}) == -1, name
    assert power(n=0) == -2 and power(n=-3) == -2
    for dims in ((cin, cout, 0, w), (cin, cout, h, -2), (0, cout, h, w), (cin, -64, h, w)):
        assert power(dims=dims) == -2 and grad(dims=dims) == -2, dims
    for dims in ((2, 64, h, w), (64, 32, h, w), (1, 1, h, w), (3, 3, h, w), (cin, cout, 1 << 11, 1 << 10), (cin, cout, 1, (1 << 20) + 1)):
        assert power(dims=dims) == -4 and grad(dims=dims) == -4, dims
    for name in ("W", "u", "v", "weight", "ws"):
        assert power(off={name: 4}) == -3, name
    assert power(off={"record": 4}) == -3 and grad(off={"record": 4}) == -3
    for name in ("G", "W", "u", "v", "dW", "ws"):
        assert grad(off={name: 8}) == -3, name
    # an output on an input, two outputs on one another, the workspace on anything (u is in and out by design)
    assert power(weight="W") == -4 and power(v="u") == -4 and power(v="weight") == -4 and power(ws="W") == -4 and power(ws="u") == -4
    assert power(u="W") == -4 and power(weight="W", off={"weight": 16}) == -4              # a partial overlap
    assert grad(dW="G") == -4 and grad(dW="W") == -4 and grad(ws="G") == -4 and grad(ws="dW") == -4 and grad(dW="u") == -4


# ----------------------------------------------------------------------------- the restatements against the reference
@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
def test_cpu_restatement_matches_the_reference(golden, case):
    from deqsci_amd import realsn
    cin, cout, h, w, n = case
    tag = rc.case_tag(*case)
    W, u, R = rc.inputs(*case)
    assert rc.sha16(W) + rc.sha16(u) + rc.sha16(R) == str(golden[tag + ".hash"]), "the seeded inputs are not the golden's"
    u_in = u.clone()
    weight, u_new, v, cur_sigma = realsn.power_iteration(W, u, rc.SIGMA, n, rc.EPS)
    assert torch.equal(u, u_in) and weight.dtype == u_new.dtype == v.dtype == torch.float32 and cur_sigma.dtype == torch.float64
    want_cs = float(golden[tag + ".cur_sigma"])
    assert 2.0 < want_cs < 13.0                                    # (a missing division cannot pass)
    grad = realsn.weight_grad(R, W, u_new, v, cur_sigma, rc.SIGMA)
    figures = {"u": rc.deviation(golden, tag + ".u", u_new), "weight": rc.deviation(golden, tag + ".weight", weight),
               "cur_sigma": abs(float(cur_sigma) - want_cs) / want_cs, "grad": rc.deviation(golden, tag + ".grad", grad)}
    print(tag, figures)
    for name, value in figures.items():
        assert value <= 1e-6, (name, value)


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
def test_float64_restatement_and_gradient_formula(golden, case):
    """power_iteration_float64 reproduces the golden's float64 values, and the closed-form gradient equals autograd through the last
    two lines of the step, both to 1e-12."""
    from deqsci_amd import realsn
    cin, cout, h, w, n = case
    tag = rc.case_tag(*case)
    W, u, R = rc.inputs(*case)
    weight, u_new, v, cur_sigma = realsn.power_iteration_float64(W, u, rc.SIGMA, n, rc.EPS)
    assert weight.dtype == torch.float64
    assert abs(float(cur_sigma) - float(golden[tag + ".f64.cur_sigma"])) <= 1e-12 * abs(float(cur_sigma))
    for name, t in (("u", u_new), ("v", v), ("weight", weight)):
        assert rc.deviation(golden, f"{tag}.f64.{name}", t) <= 1e-12, name
    W64 = W.double().requires_grad_(True)
    taped = W64 / (u_new * F.conv2d(v, W64, padding=1)).sum() * rc.SIGMA
    (want,) = torch.autograd.grad((taped * R.double()).sum(), W64)
    got = realsn.weight_grad(R.double(), W64, u_new, v, cur_sigma, rc.SIGMA)
    assert float((got - want).norm() / want.norm()) <= 1e-12
    assert rc.deviation(golden, tag + ".f64.grad", got) <= 1e-12
    # C is d cur_sigma / dW
    (C,) = torch.autograd.grad((u_new * F.conv2d(v, W64, padding=1)).sum(), W64)
    assert float((realsn.sigma_jacobian(u_new, v) - C).norm() / C.norm()) <= 1e-12


@pytest.mark.parametrize("layer", rc.LAYERS, ids=lambda l: "%dx%d" % l)
def test_zero_u_gives_zero_sigma_and_the_references_nonfinite_weight(layer):
    from deqsci_amd import realsn
    cin, cout = layer
    W, u, _ = rc.inputs(cin, cout, 7, 9, 1)
    W.view(-1)[5] = 0.0
    weight, u_new, v, cur_sigma = realsn.power_iteration(W, torch.zeros_like(u), rc.SIGMA, 1, rc.EPS)
    assert float(cur_sigma) == 0.0 and not u_new.any() and not v.any()
    want = W / torch.zeros((), dtype=torch.float32) * rc.SIGMA
    assert int(torch.isnan(want).sum()) == 1 and int(torch.isinf(want).sum()) == W.numel() - 1
    assert torch.equal(torch.isnan(weight), torch.isnan(want)) and torch.equal(weight[~torch.isnan(want)], want[~torch.isnan(want)])


def test_power_iteration_refuses_what_it_cannot_run():
    from deqsci_amd import realsn
    W, u, _ = rc.inputs(1, 64, 2, 3, 1)
    with pytest.raises(TypeError):
        realsn.power_iteration(W.double(), u)
    with pytest.raises(ValueError):
        realsn.power_iteration(W, u, n_power_iterations=0)
    with pytest.raises(ValueError):
        realsn.power_iteration(W, u[:, :3])


# ----------------------------------------------------------------------------- the module
def _module(case):
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    cin, cout, h, w, n = case
    W, u, R = rc.inputs(*case)
    m = RealSNConv2d(cin, cout, sigma=rc.SIGMA)
    m.n_power_iterations = n
    with torch.no_grad():
        m.weight_orig.copy_(W)
    m.weight_u = u.clone()                                          # (the buffer's shape decides the map)
    return m, W, u, R


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[2:4] in ((40, 40), (2, 3))], ids=_ids)
def test_module_train_forward_matches_the_reference(golden, case):
    """Fails on the parent commit: its train-mode forward raises NotImplementedError."""
    cin, cout, h, w, n = case
    tag = rc.case_tag(*case)
    m, W, u, R = _module(case)
    m.train()
    u_buf, w_buf = m.weight_u, m.weight
    x = torch.randn(2, cin, 6, 5, generator=torch.Generator().manual_seed(3))
    y = m(x)
    assert m.weight_u is u_buf and m.weight is w_buf                # updated in place
    assert rc.deviation(golden, tag + ".u", m.weight_u) <= 1e-6 and rc.deviation(golden, tag + ".weight", m.weight) <= 1e-6
    assert not m.weight.requires_grad
    assert torch.equal(y, F.conv2d(x, m.weight, padding=1))
    # the gradient of sum(weight * R) through the module: y = conv(x, weight) is linear in weight, so pick the loss through weight itself
    from deqsci_amd import autograd as ag
    m2, _, _, _ = _module(case)
    weight, u_new = ag.realsn_weight(m2.weight_orig, m2.weight_u, rc.SIGMA, n, rc.EPS)
    assert not u_new.requires_grad and weight.requires_grad
    (weight * R).sum().backward()
    assert rc.deviation(golden, tag + ".grad", m2.weight_orig.grad) <= 1e-6
    # eval mode afterwards: the last train-mode weight, bit for bit, and no further step
    m.eval()
    u_after = m.weight_u.clone()
    assert torch.equal(m(x), F.conv2d(x, m.weight, padding=1)) and torch.equal(m.weight_u, u_after)
    assert "weight" in m.state_dict() and torch.equal(m.state_dict()["weight"], m.weight)


def test_module_backward_reaches_weight_orig_and_the_input():
    from deqsci_amd import realsn
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    torch.manual_seed(11)
    m = RealSNConv2d(64, 64, sigma=0.9).train()
    u0 = m.weight_u.clone()
    x = torch.randn(1, 64, 5, 4, requires_grad=True)
    m(x).square().sum().backward()
    assert m.weight_orig.grad is not None and x.grad is not None
    # the same in float64 by autograd through the composed operations, from the same weight_u
    W64 = m.weight_orig.detach().double().requires_grad_(True)
    _, u64, v64, _ = realsn.power_iteration_float64(W64, u0, 0.9, 1, 1e-12)
    taped = W64 / (u64 * F.conv2d(v64, W64, padding=1)).sum() * 0.9
    F.conv2d(x.detach().double(), taped, padding=1).square().sum().backward()
    assert float((m.weight_orig.grad.double() - W64.grad).norm() / W64.grad.norm()) <= 1e-5
    # weight_orig that asks for no gradient gets none, the input still does
    m.weight_orig.requires_grad_(False)
    m.weight_orig.grad = None
    x.grad = None
    m(x).square().sum().backward()
    assert m.weight_orig.grad is None and x.grad is not None


def test_double_backward_raises():
    from deqsci_amd import autograd as ag
    W, u, R = rc.inputs(1, 64, 2, 3, 1)
    W.requires_grad_(True)
    weight, _ = ag.realsn_weight(W, u, rc.SIGMA, 1, rc.EPS)
    (g,) = torch.autograd.grad((weight * R).sum(), W, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.parametrize("layer", rc.LAYERS, ids=lambda l: "%dx%d" % l)
def test_fresh_module_has_a_unit_u_and_leaves_the_global_stream_alone(layer):
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    cin, cout = layer
    torch.manual_seed(5)
    m = RealSNConv2d(cin, cout)
    after = torch.random.get_rng_state()
    torch.manual_seed(5)
    w = torch.empty(cout, cin, 3, 3)
    torch.nn.init.kaiming_uniform_(w, a=5 ** 0.5)                   # all the parent commit's constructor draws
    assert torch.equal(torch.random.get_rng_state(), after) and torch.equal(m.weight_orig.detach(), w)
    assert tuple(m.weight_u.shape) == (1, 1 if cout == 1 else 64, 40, 40)
    assert abs(float(m.weight_u.double().norm()) - 1.0) <= 1e-6
    assert torch.equal(RealSNConv2d(cin, cout).weight_u, m.weight_u)   # its own generator: the same draw again


def test_fresh_net_trains_and_its_layers_draw_different_vectors():
    from deqsci_amd.networks.simplecnn import DnCNN, RealSNConv2d
    net = DnCNN(1, num_of_layers=4, lip=1.0, no_bn=True).train()
    convs = [m for m in net.modules() if isinstance(m, RealSNConv2d)]
    assert len(convs) == 4 and not torch.equal(convs[1].weight_u, convs[2].weight_u)
    out = net(torch.rand(2, 1, 8, 8))
    assert torch.isfinite(out).all()


# ----------------------------------------------------------------------------- a training step, denoiser-level half
def _golden_net(golden):
    """RealSN_SimpleCNN from the shipped checkpoint as (b) modifies it, in train mode; asserts the golden's hash of the starting state."""
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import build_denoiser
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    from deqsci_amd.solvers import EquilibriumProxGradSCI
    from deqsci_amd.operators import A_torch_, At_torch_
    net = build_denoiser("RealSN_SimpleCNN")
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    checkpoint.load_solver(solver, checkpoint.shipped("rsn_cnn"))
    convs = [m for m in net.modules() if isinstance(m, RealSNConv2d)]
    with torch.no_grad():
        for i, (m, s) in enumerate(zip(convs, rc.SCALES)):
            # the reference's module keeps weight_orig and the weight buffer in ONE storage until its first train-mode call, so its
            # load_state_dict leaves the checkpoint's `weight` in both: that, scaled, is the golden's starting weight_orig
            m.weight_orig.copy_(m.weight * s)
            m.weight_u.copy_(rc.unit_u(m.weight_u.shape, rc.U_SEED + i))
    assert "".join(rc.sha16(m.weight_orig) for m in convs) + "".join(rc.sha16(m.weight_u) for m in convs) == str(golden["b.hash"])
    net.train()
    for p in solver.parameters():
        p.requires_grad_(True)
    return solver, net, convs


def test_training_step_of_the_denoiser_matches_the_reference(golden):
    """The GAP operators have no CPU form, so this is the denoiser-level half of golden (b): one taped net(x) of the train-mode net
    and its backward against the reference's, 1e-4."""
    solver, net, convs = _golden_net(golden)
    noise = net(rc.denoiser_input())
    loss = (noise ** 2).mean()
    loss.backward()
    assert rc.rel_l2(noise.detach().numpy(), golden["b.net.noise"]) <= 1e-4
    assert abs(float(loss.detach()) - float(golden["b.net.loss"])) <= 1e-4 * float(golden["b.net.loss"])
    for i, m in enumerate(convs):
        assert rc.deviation(golden, f"b.net.grad.{i}", m.weight_orig.grad) <= 1e-4, i
        assert rc.deviation(golden, f"b.net.weight_u.{i}", m.weight_u) <= 1e-4, i


# ----------------------------------------------------------------------------- operator_norm
def test_operator_norm_against_the_dense_singular_value():
    """float64, map (5,6), layer (1,64): the 1920 x 30 matrix of x -> conv2d(x, W, padding=1) column by column, its largest singular
    value, and the power iteration's estimates |W v|: non-decreasing from the second step on, never above sigma_max (1 + 1e-12), and at
    least 0.999 sigma_max at the iteration count the float64 restatement needs (found by running it first; at most 200)."""
    from deqsci_amd import realsn
    h, w = 5, 6
    W = rc.inputs(1, 64, h, w, 1)[0].double()
    cols = []
    for j in range(h * w):
        e = torch.zeros(1, 1, h, w, dtype=torch.float64)
        e.view(-1)[j] = 1.0
        cols.append(F.conv2d(e, W, padding=1).reshape(-1))
    A = torch.stack(cols, dim=1)
    assert tuple(A.shape) == (1920, 30)
    sigma_max = float(torch.linalg.svdvals(A)[0])
    # the count, from the restatement itself: the step repeated from operator_norm's seeded start
    g = torch.Generator().manual_seed(0)
    u = torch.randn(1, 64, h, w, generator=g, dtype=torch.float64)
    u = u / u.norm()
    count = None
    for k in range(1, 201):
        _, u, v, _ = realsn.power_iteration_float64(W, u, 1.0, 1, 1e-12)
        if float(F.conv2d(v, W, padding=1).norm()) >= 0.999 * sigma_max:
            count = k
            break
    assert count is not None and count <= 200
    norm, trace = realsn.operator_norm(W, size=(h, w), n_iters=count, seed=0, return_trace=True)
    assert len(trace) == count and norm == trace[-1]
    assert all(b >= a for a, b in zip(trace[1:], trace[2:]))
    assert max(trace) <= sigma_max * (1 + 1e-12)
    assert norm >= 0.999 * sigma_max
    assert realsn.operator_norm(W, size=(h, w), n_iters=count, seed=0) == norm


def test_layer_sigmas_reports_every_layer_and_leaves_the_global_stream_alone(golden):
    from deqsci_amd import realsn
    solver, net, convs = _golden_net(golden)
    state = torch.random.get_rng_state()
    rows = realsn.layer_sigmas(net, size=(6, 6), n_iters=30)
    assert torch.equal(torch.random.get_rng_state(), state)
    assert [r["layer"] for r in rows] == ["dncnn.0", "dncnn.2", "dncnn.4", "dncnn.6"]
    assert all(r["sigma"] == 1.0 and 0.0 < r["norm"] < 1.1 for r in rows)      # the shipped, already normalised weights: at most their sigma
