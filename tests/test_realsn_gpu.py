"""GPU: RealSN in train mode on the device (csrc/realsn.hip) - R1 stage by stage and end to end against float64, R2 against float64, run
to run, the non-finite weight of u = 0, RealSNConv2d and DEQFixedPoint against the reference's numbers (tests/golden/realsn_train.npz),
no host synchronisation, and the engine's no-tape path.

Bounds.  u32 = 2^-24.  An fp32 fmaf chain of K products is within K u32 sum|terms| of its exact value, element by element (first order);
what follows a chain adds a constant number c of further roundings of a value no larger than sum|terms|:
  stage 1: v * |W^T u| against W^T u_in in float64.  K = 9 C_out; c = 4: the norm's rounding to fp32 and the division, and two spare for the
           second-order terms of the first-order bound.
  stage 2: u * |W v| against W v_dev in float64.  K = 9 C_in; c = 4 likewise.
  norms:   the record holds them in float64, summed in float64 (csrc/rows.hpp: below 2^-53 N of the sum), from the device's own chain
           results: | |t_dev| - |t_64| | <= |t_dev - t_64|_2 <= the 2-norm of the chain bounds (c = 0), plus N 2^-53 of the norm.
  cur_sigma = sum u_dev t2_dev in float64: within sum |u_dev| * (stage 2's chain bound, c = 0) + N 2^-53 sum |u_dev t2| of sum u_dev t2_64.
  weight = W / (float) cur_sigma * sigma_t: three fp32 roundings, c = 4 u32 relative.
  R2:      C's chain has K = h w products (a wave's 64 partial chains and its butterfly: no more roundings per element than one chain),
           sum(G W) has K = 9 C_in C_out products in float64; s = (float)(sum(G W) / cur_sigma) and a = sigma_t / (float) cur_sigma carry
           one and two fp32 roundings, s C, G - s C and a (.) one each.
End to end against the float64 restatement: 2e-6 for u, weight and cur_sigma - 5 times the reference's own worst fp32 deviation from
float64, the device's summation order being a third order.  Against the reference's tensors: 1e-4.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
import realsn_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
U32 = 2.0 ** -24
U64 = 2.0 ** -53
C_EXTRA = 4
LAYER_MAPS = [(cin, cout, h, w) for cin, cout in rc.LAYERS for h, w in rc.MAPS]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "realsn_train.npz")))


def _ids(case):
    return rc.case_tag(*case)[2:]


def _power(W, u, n):
    """R1 on the device from CPU inputs -> CPU tensors (weight, u, v, record)."""
    from deqsci_amd import _hip
    weight, u_new, v, record = _hip.realsn_power(W.to(DEV), u.to(DEV).clone(), n, rc.SIGMA, rc.EPS)
    return weight.cpu(), u_new.cpu(), v.cpu(), record.cpu()


def _ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 = 0)."""
    err = (got.double() - want.double()).abs()
    ok = bound > 0
    assert bool((err[~ok] == 0).all())
    return float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0


@pytest.mark.parametrize("case", LAYER_MAPS, ids=lambda c: "%dx%d.%dx%d" % c)
def test_r1_stage_by_stage_against_float64(case):
    cin, cout, h, w = case
    W, u_in, _ = rc.inputs(cin, cout, h, w, 1)
    weight, u, v, record = _power(W, u_in, 1)
    n1, n2, cs = (float(x) for x in record)
    W64, N1, N2 = W.double(), cin * h * w, cout * h * w
    # stage 1
    t1 = F.conv_transpose2d(u_in.double(), W64, padding=1)
    abs1 = F.conv_transpose2d(u_in.double().abs(), W64.abs(), padding=1)
    r1 = _ratio(v.double() * n1, t1, (9 * cout + C_EXTRA) * U32 * abs1)
    rn1 = abs(n1 - float(t1.norm())) / (float((9 * cout * U32 * abs1).norm()) + N1 * U64 * n1)
    # stage 2, on the device's v
    t2 = F.conv2d(v.double(), W64, padding=1)
    abs2 = F.conv2d(v.double().abs(), W64.abs(), padding=1)
    r2 = _ratio(u.double() * n2, t2, (9 * cin + C_EXTRA) * U32 * abs2)
    rn2 = abs(n2 - float(t2.norm())) / (float((9 * cin * U32 * abs2).norm()) + N2 * U64 * n2)
    # cur_sigma, on the device's u
    bound_cs = float((u.double().abs() * (9 * cin * U32 * abs2)).sum()) + N2 * U64 * float((u.double() * t2).abs().sum())
    rcs = abs(cs - float((u.double() * t2).sum())) / bound_cs
    # the weight, on the device's cur_sigma
    want = W64 / cs * rc.SIGMA
    rw = _ratio(weight, want, C_EXTRA * U32 * want.abs())
    print(f"{case}: ratios to the bounds: v {r1:.3f} |W^T u| {rn1:.3f} u {r2:.3f} |W v| {rn2:.3f} cur_sigma {rcs:.3f} weight {rw:.3f}")
    assert max(r1, rn1, r2, rn2, rcs, rw) <= 1.0
    assert abs(float(v.double().norm()) - 1.0) <= 1e-6 and abs(float(u.double().norm()) - 1.0) <= 1e-6


@pytest.mark.parametrize("case", rc.CASES, ids=_ids)
def test_r1_end_to_end_against_the_float64_restatement(golden, case):
    from deqsci_amd import realsn
    cin, cout, h, w, n = case
    tag = rc.case_tag(*case)
    W, u_in, _ = rc.inputs(*case)
    assert rc.sha16(W) + rc.sha16(u_in) == str(golden[tag + ".hash"])[:32]
    weight, u, v, record = _power(W, u_in, n)
    w64, u64, v64, cs64 = realsn.power_iteration_float64(W, u_in, rc.SIGMA, n, rc.EPS)
    figures = {"u": rc.rel_l2(u, u64), "weight": rc.rel_l2(weight, w64), "cur_sigma": abs(float(record[2]) - float(cs64)) / float(cs64)}
    assert rc.deviation(golden, tag + ".f64.u", u64) <= 1e-12           # the yardstick is the golden's
    print(f"{tag}: against float64 " + ", ".join(f"{k} {x:.3e} ({x / 2e-6:.3f} of the bound)" for k, x in figures.items()))
    for name, value in figures.items():
        assert value <= 2e-6, (name, value)
    # the functional front end is the same launch sequence, and leaves its input alone
    ud = u_in.to(DEV)
    got = realsn.power_iteration(W.to(DEV), ud, rc.SIGMA, n, rc.EPS)
    assert torch.equal(ud.cpu(), u_in) and torch.equal(got[0].cpu(), weight) and torch.equal(got[1].cpu(), u) and float(got[3]) == float(record[2])


@pytest.mark.parametrize("case", LAYER_MAPS, ids=lambda c: "%dx%d.%dx%d" % c)
def test_r2_against_float64(case):
    """dW on the device's u, v and cur_sigma against the formula in float64 on the same; at (1,1) and (2,3) most taps of C fall outside
    the map."""
    from deqsci_amd import _hip, realsn
    cin, cout, h, w = case
    W, u_in, R = rc.inputs(cin, cout, h, w, 1)
    Wd, Rd = W.to(DEV), R.to(DEV)
    weight, u, v, record = _hip.realsn_power(Wd, u_in.to(DEV), 1, rc.SIGMA, rc.EPS)
    dW = _hip.realsn_grad(Rd, Wd, u, v, record, rc.SIGMA).cpu()
    u, v, cs = u.cpu().double(), v.cpu().double(), float(record.cpu()[2])
    G, W64 = R.double(), W.double()
    C = realsn.sigma_jacobian(u, v)
    Cabs = realsn.sigma_jacobian(u.abs(), v.abs())
    gw = float((G * W64).sum())
    s, a = gw / cs, rc.SIGMA / cs
    want = a * (G - s * C)
    bound = U32 * (abs(a) * abs(s) * (h * w + C_EXTRA) * Cabs            # C's chain, and s's rounding
                   + abs(a) * (2 * (s * C).abs() + (G - s * C).abs())     # s C, G - s C
                   + C_EXTRA * want.abs())                               # a's two roundings, the product's
    bound = bound + abs(a) * C.abs() * (9 * cin * cout * U64 * float((G * W64).abs().sum()) / abs(cs))
    r = _ratio(dW, want, bound)
    print(f"{case}: dW ratio to the bound {r:.3f}, relative L2 {rc.rel_l2(dW, want):.3e}")
    assert r <= 1.0
    if h * w == 1:                                                       # a 1 x 1 map: only the centre tap of C is inside
        centre = torch.zeros(3, 3, dtype=torch.bool)
        centre[1, 1] = True
        assert bool((C[:, :, ~centre] == 0).all())
        assert torch.equal(dW[:, :, ~centre].double(), (torch.tensor(rc.SIGMA, dtype=torch.float32) / torch.tensor(cs).float() * R)[:, :, ~centre].double())


@pytest.mark.parametrize("layer", rc.LAYERS, ids=lambda l: "%dx%d" % l)
def test_r1_and_r2_are_bit_equal_run_to_run(layer):
    from deqsci_amd import _hip
    cin, cout = layer
    W, u_in, R = rc.inputs(cin, cout, 40, 40, 3)
    Wd, Rd = W.to(DEV), R.to(DEV)
    runs = []
    for _ in range(2):
        weight, u, v, record = _hip.realsn_power(Wd, u_in.to(DEV), 3, rc.SIGMA, rc.EPS)
        runs.append([t.clone() for t in (weight, u, v, record, _hip.realsn_grad(Rd, Wd, u, v, record, rc.SIGMA))])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(runs[0][4]).all())


@pytest.mark.parametrize("layer", rc.LAYERS, ids=lambda l: "%dx%d" % l)
def test_zero_u_gives_zero_sigma_and_the_references_nonfinite_weight(layer):
    """R1 only: no backward is started on the non-finite weight."""
    cin, cout = layer
    W, u_in, _ = rc.inputs(cin, cout, 7, 9, 1)
    W.view(-1)[5] = 0.0
    weight, u, v, record = _power(W, torch.zeros_like(u_in), 1)
    assert [float(x) for x in record] == [0.0, 0.0, 0.0] and not u.any() and not v.any()
    want = W / torch.zeros((), dtype=torch.float32) * rc.SIGMA
    assert int(torch.isnan(want).sum()) == 1 and int(torch.isinf(want).sum()) == W.numel() - 1
    assert torch.equal(torch.isnan(weight), torch.isnan(want)) and torch.equal(weight[~torch.isnan(want)], want[~torch.isnan(want)])


def test_wrappers_refuse_what_the_kernels_do_not_cover():
    from deqsci_amd import _hip
    with pytest.raises(_hip.DeqsciHipError, match=r"\(1,64\), \(64,64\)"):
        _hip.realsn_power(torch.zeros(32, 64, 3, 3, device=DEV), torch.zeros(1, 32, 4, 4, device=DEV))
    with pytest.raises(_hip.DeqsciHipError, match="n_iters"):
        _hip.realsn_power(torch.zeros(64, 64, 3, 3, device=DEV), torch.zeros(1, 64, 4, 4, device=DEV), 0)
    with pytest.raises(_hip.DeqsciHipError):
        _hip.realsn_power(torch.zeros(64, 64, 3, 3, device=DEV), torch.zeros(1, 1, 4, 4, device=DEV))


# ----------------------------------------------------------------------------- the module
def _module(case):
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    cin, cout, h, w, n = case
    W, u, R = rc.inputs(*case)
    m = RealSNConv2d(cin, cout, sigma=rc.SIGMA)
    m.n_power_iterations = n
    with torch.no_grad():
        m.weight_orig.copy_(W)
    m.weight_u = u.clone()
    return m.to(DEV).train(), R.to(DEV)


@pytest.mark.parametrize("case", [c for c in rc.CASES if c[2:4] in ((40, 40), (2, 3))], ids=_ids)
def test_module_forward_and_backward_against_the_reference(golden, case):
    cin, cout, h, w, n = case
    tag = rc.case_tag(*case)
    m, R = _module(case)
    u_buf, w_buf = m.weight_u, m.weight
    x = torch.randn(2, cin, 6, 5, device=DEV, generator=torch.Generator(DEV).manual_seed(3), requires_grad=True)
    y = m(x)
    assert m.weight_u is u_buf and m.weight is w_buf
    assert rc.deviation(golden, tag + ".u", m.weight_u) <= 1e-4 and rc.deviation(golden, tag + ".weight", m.weight) <= 1e-4
    assert torch.equal(y.detach(), F.conv2d(x.detach(), m.weight, padding=1))
    # the reference's gradient is that of sum(weight * R): the same loss through the taped weight
    from deqsci_amd import autograd as ag
    m2, _ = _module(case)
    weight, u_new = ag.realsn_weight(m2.weight_orig, m2.weight_u, rc.SIGMA, n, rc.EPS)
    (weight * R).sum().backward()
    assert rc.deviation(golden, tag + ".grad", m2.weight_orig.grad) <= 1e-4
    # ... and through the convolution: the module's backward against the float64 restatement's autograd
    y.square().sum().backward()
    from deqsci_amd import realsn
    W, u0, _ = rc.inputs(*case)
    W64 = W.double().requires_grad_(True)
    _, u64, v64, _ = realsn.power_iteration_float64(W64, u0, rc.SIGMA, n, rc.EPS)
    taped = W64 / (u64 * F.conv2d(v64, W64, padding=1)).sum() * rc.SIGMA
    x64 = x.detach().cpu().double().requires_grad_(True)
    F.conv2d(x64, taped, padding=1).square().sum().backward()
    assert rc.rel_l2(m.weight_orig.grad.cpu(), W64.grad) <= 1e-4 and rc.rel_l2(x.grad.cpu(), x64.grad) <= 1e-4
    m.eval()
    assert torch.equal(m(x.detach()), F.conv2d(x.detach(), m.weight, padding=1))


def test_train_mode_forward_and_backward_do_not_synchronise(monkeypatch):
    m, _ = _module((64, 64, 40, 40, 1))
    x = torch.randn(2, 64, 8, 8, device=DEV, requires_grad=True)
    m(x).sum().backward()                                            # (the library and every kernel loaded)
    m.weight_orig.grad = None
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host synchronisation")
    for name in ("item", "cpu", "tolist", "__float__"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(torch.cuda, "synchronize", refuse)
    y = m(x)
    y.sum().backward()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.weight_orig.grad).all()) and float(m.weight_orig.grad.norm()) > 0


# ----------------------------------------------------------------------------- a training step against the reference
def _golden_solver(golden):
    """RealSN_SimpleCNN from the shipped checkpoint as golden (b) modifies it, in train mode, on the device."""
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
            # (the reference's load_state_dict leaves the checkpoint's `weight` in weight_orig too: tests/test_realsn_host.py)
            m.weight_orig.copy_(m.weight * s)
            m.weight_u.copy_(rc.unit_u(m.weight_u.shape, rc.U_SEED + i))
    assert "".join(rc.sha16(m.weight_orig) for m in convs) + "".join(rc.sha16(m.weight_u) for m in convs) == str(golden["b.hash"])
    start = [(m.weight_orig.detach().clone(), m.weight_u.detach().clone()) for m in convs]
    net.train()
    for p in solver.parameters():
        p.requires_grad_(True)
    return solver.to(DEV), convs, start


def _training_step(golden, implicit):
    import deqsci_amd
    solver, convs, start = _golden_solver(golden)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(golden["b.iters"]), tol=1e-9)
    deq.implicit_backward = implicit
    Phi, gt = (t.to(DEV) for t in rc.problem())
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt).detach())
    loss = F.mse_loss(rec, gt)
    solver.zero_grad()
    loss.backward()
    return deq, convs, start, rec.detach(), loss.detach()


@pytest.mark.parametrize("implicit", ["autograd", "device"])
def test_training_step_against_the_reference(golden, implicit):
    from deqsci_amd import realsn
    assert float(golden["b.conditioning"]) < 1e-5
    deq, convs, start, rec, loss = _training_step(golden, implicit)
    figures = {"rec": rc.rel_l2(rec.cpu(), golden["b.rec"]), "loss": abs(float(loss) - float(golden["b.loss"])) / float(golden["b.loss"])}
    for i, m in enumerate(convs):
        figures[f"grad.{i}"] = rc.deviation(golden, f"b.grad.{i}", m.weight_orig.grad)
        figures[f"weight.{i}"] = rc.deviation(golden, f"b.weight.{i}", m.weight)
        figures[f"weight_u.{i}"] = rc.deviation(golden, f"b.weight_u.{i}", m.weight_u)
    print(f"implicit_backward={implicit}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()),
          f"forward_res {deq.forward_res:.4e} backward_res {deq.backward_res:.4e}")
    for name, value in figures.items():
        assert value <= 1e-4, (name, value)
    assert abs(deq.forward_res - float(golden["b.forward_res"])) < 1e-2 * float(golden["b.forward_res"])
    assert abs(deq.backward_res - float(golden["b.backward_res"])) < 1e-2 * float(golden["b.backward_res"])
    # weight_u after the max_iter + 2 = 14 f-calls of a training forward, against 14 steps of the float64 restatement
    steps = int(golden["b.iters"]) + 2
    for i, (m, (W0, u0)) in enumerate(zip(convs, start)):
        u64 = realsn.power_iteration_float64(W0, u0, m.sigma, steps, 1e-12)[1]
        assert rc.rel_l2(m.weight_u.cpu(), u64) <= steps * 2e-6, i
    # RealSN stays off the device VJP and weight-gradient paths: autograd, with the reason
    assert deq.last_backward_path == "autograd" and deq.last_parameter_path == "autograd"
    if implicit == "device":
        assert "RealSN" in deq.backward_fallback_reason and "train mode" in deq.backward_fallback_reason
    else:
        assert deq.backward_fallback_reason is None


# ----------------------------------------------------------------------------- the engine's no-tape path
def _engine_run(use_engine, options=None):
    import deqsci_amd
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 6)
    solver.nonlinear_op.train()
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=6, tol=1e-9)
    deq.use_engine = use_engine
    deq.engine_options = dict(options or {})
    g = torch.Generator().manual_seed(8)
    Phi = (torch.rand(1, 32, 32, 8, generator=g) < 0.5).float().to(DEV)
    gt = torch.rand(1, 32, 32, 8, generator=g).to(DEV)
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    convs = [m for m in solver.nonlinear_op.modules() if isinstance(m, RealSNConv2d)]
    start = [(m.weight_orig.detach().clone(), m.weight_u.detach().clone()) for m in convs]
    with torch.no_grad():
        rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None))
    return deq, convs, start, rec


def test_engine_runs_a_train_mode_net_eagerly():
    from deqsci_amd import realsn
    deq, convs, start, rec = _engine_run(True)
    eng = deq._engine[1]
    assert eng.last_info["f_calls"] == 8 and eng.last_info["graph"] is False and eng._graph is None
    for m, (W0, u0) in zip(convs, start):
        u = u0
        for _ in range(8):                                           # the power step does not depend on the iterate: exact
            weight, u, _, _ = realsn.power_iteration(W0, u, m.sigma, 1, 1e-12)
        assert torch.equal(m.weight_u, u) and torch.equal(m.weight, weight)
    plain, convs2, _, _ = _engine_run(False)
    assert plain._engine is None
    for m, m2 in zip(convs, convs2):
        assert torch.equal(m.weight_u, m2.weight_u) and torch.equal(m.weight, m2.weight)
    with pytest.raises(ValueError, match="train-mode RealSNConv2d"):
        _engine_run(True, {"use_graph": True})
