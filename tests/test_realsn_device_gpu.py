"""GPU: RealSN_SimpleCNN in TRAIN mode on the device - R3 of csrc/realsn.hip (weight -> packs) bit for bit against its numpy restatement
(tests/realsn_pack_ref.py) and within the last rounding of the host packers; the engine's f-calls under train_realsn="device"; a training
step of DEQFixedPoint under each of the three switches against the reference's own numbers (tests/golden/realsn_train.npz); determinism,
no host synchronisation, and the refusals at run time.

Bounds.  (b): two float64 evaluations of the 9-term form U = G g G^T, each rounded to fp32 once, differ by at most one fp32 spacing plus
16 * 2^-53 * (|G| |g| |G^T|) (realsn_pack_ref.bound).  (c): the float64 chain on the SAME weights; per layer the rounding count c that
profiles/denoiser_exact.md counts for the kernel that ran (denoiser_exact_ref.c_of: first layer 9, F(2x2,3x3) 135, F(4x4,3x3) 139, last
layer 576) times 2^-24 times the layer's absolute-value sum S, and the error of the layer's input carried through |W| (a ReLU does not
enlarge it): e_l = conv(e_{l-1}, |W_l|) + c_l 2^-24 S_l over the four layers.  (d): 1e-4, the bound the autograd path is held to."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
import denoiser_exact_ref as der
import realsn_cases as rc
import realsn_pack_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024                           # floats of NaN on each side of every output (a multiple of 4: the views stay 16-byte aligned)
NAMES = ("pack", "pack44", "pack_t")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "realsn_train.npz")))


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- (a), (b): R3
_SHIPPED = {}


def _shipped():
    if not _SHIPPED:
        from deqsci_amd import checkpoint
        from deqsci_amd.cli import build_pipeline
        from deqsci_amd.networks.simplecnn import RealSNConv2d
        solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 6)
        convs = [m for m in solver.nonlinear_op.modules() if isinstance(m, RealSNConv2d)]
        for layer, i in zip(ref.LAYERS, (0, 1, 3)):
            _SHIPPED[layer] = convs[i].weight.detach().cpu().clone()
    return _SHIPPED


def _weight(layer, kind):
    cin, cout = layer
    g = torch.Generator().manual_seed(1000 * cin + cout)
    if kind == "shipped":
        return _shipped()[layer]
    if kind == "normal":
        return torch.randn(cout, cin, 3, 3, generator=g)
    if kind == "integer":
        return torch.randint(-9, 10, (cout, cin, 3, 3), generator=g).float()
    w = torch.randn(cout, cin, 3, 3, generator=g)
    w[torch.rand(w.shape, generator=g) < 0.3] = 0.0
    w.view(-1)[7] = -0.0
    w[-1, -1] = 0.0                                                       # a whole filter of zeros ...
    w[-1, -1, 1, 1] = -0.0                                                # ... around a negative one
    return w


def _guarded(shape):
    """(the NaN-filled buffer, its view of `shape` between two guard bands)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _run(w, want=NAMES):
    """R3 on the device into guarded buffers -> {name: (buffer, view) or None}."""
    from deqsci_amd import _hip
    cout, cin = w.shape[:2]
    shapes = _hip.realsn_pack_shapes(cin, cout)
    out = {k: _guarded(shapes[k]) if (k in want and shapes[k] is not None) else None for k in NAMES}
    wd = w.to(DEV)
    _hip.realsn_pack(wd, *(None if out[k] is None else out[k][1] for k in NAMES))
    torch.cuda.synchronize()
    assert torch.equal(wd.cpu(), w)
    return out


@pytest.mark.parametrize("kind", ["shipped", "normal", "integer", "zeros"])
@pytest.mark.parametrize("layer", ref.LAYERS, ids=lambda l: "%dx%d" % l)
def test_r3_is_the_restatement_bit_for_bit(layer, kind):
    w = _weight(layer, kind)
    if kind == "zeros":
        assert int((w == 0).sum()) > 50 and bool(torch.signbit(w.view(-1)[7]))
    want = ref.packs(w.numpy())
    got, again = _run(w), _run(w)
    for name in NAMES:
        if want[name] is None:
            assert got[name] is None
            continue
        buf, view = got[name]
        assert tuple(view.shape) == want[name].shape
        assert np.array_equal(_bits(view), _bits(want[name])), (name, int((_bits(view) != _bits(want[name])).sum()))
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), name       # the guard bands are untouched
        assert np.array_equal(_bits(view), _bits(again[name][1])), name                                    # bit-equal run to run
    # a NULL output is skipped: each pack alone gives the same bits
    for name in NAMES:
        if want[name] is not None:
            alone = _run(w, want=(name,))
            assert [k for k in NAMES if alone[k] is not None] == [name]
            assert np.array_equal(_bits(alone[name][1]), _bits(want[name])) and bool(torch.isnan(alone[name][0][:GUARD]).all())


@pytest.mark.parametrize("kind", ["shipped", "normal"])
@pytest.mark.parametrize("layer", ref.LAYERS, ids=lambda l: "%dx%d" % l)
def test_r3_against_the_host_packers(layer, kind):
    from deqsci_amd import _hip, vjp
    w = _weight(layer, kind)
    got = _run(w)
    wd = w.to(DEV)
    if layer == (64, 64):
        hosts = {"pack": _hip.pack_winograd_weights(wd), "pack44": _hip.pack_winograd44_weights(wd), "pack_t": _hip.pack_winograd_weights(vjp._transposed(wd))}
        tol = ref.bound(w.numpy())
        for name, host in hosts.items():
            a, h = got[name][1].cpu().numpy().astype(np.float64), host.cpu().numpy().astype(np.float64)
            assert a.shape == h.shape
            unequal = int((a != h).sum())
            print(f"R3 against the host packer, {kind} {name}: {unequal} of {a.size} elements unequal, worst |a - b| / bound "
                  f"{float((np.abs(a - h) / (ref.ulp32(np.maximum(np.abs(a), np.abs(h))) + tol[name])).max()):.3f}")
            assert bool((np.abs(a - h) <= ref.ulp32(np.maximum(np.abs(a), np.abs(h))) + tol[name]).all()), name
    else:
        own, other = ((_hip.pack_c1_to_64_weights, _hip.pack_c64_to_1_weights) if layer == (1, 64)
                      else (_hip.pack_c64_to_1_weights, _hip.pack_c1_to_64_weights))
        assert got["pack44"] is None
        assert torch.equal(got["pack"][1], own(wd)) and torch.equal(got["pack_t"][1], other(vjp._transposed(wd)))


def test_wrapper_refuses_what_the_kernel_does_not_cover():
    from deqsci_amd import _hip
    with pytest.raises(_hip.DeqsciHipError, match=r"\(1,64\), \(64,64\)"):
        _hip.realsn_pack(torch.zeros(32, 64, 3, 3, device=DEV), torch.zeros(8, device=DEV))
    with pytest.raises(_hip.DeqsciHipError, match="pack44"):
        _hip.realsn_pack(torch.zeros(64, 1, 3, 3, device=DEV), None, torch.zeros(64 * 64 * 36, device=DEV))
    with pytest.raises(_hip.DeqsciHipError, match="pack must hold"):
        _hip.realsn_pack(torch.zeros(64, 64, 3, 3, device=DEV), torch.zeros(576, device=DEV))
    with pytest.raises(_hip.DeqsciHipError):
        _hip.realsn_pack(torch.zeros(64, 64, 3, 3, device=DEV))


# ----------------------------------------------------------------------------- (c): the engine's f-calls
def _engine_run(options=None, train=True, use_engine=True):
    """tests/test_realsn_gpu.py's _engine_run: the shipped RealSN_SimpleCNN, 6 Anderson iterations on a 1 x 32 x 32 x 8 problem, no tape."""
    import deqsci_amd
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 6)
    solver.nonlinear_op.train(train)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=6, tol=1e-9)
    deq.use_engine = use_engine
    deq.engine_options = dict(options or {})
    g = torch.Generator().manual_seed(8)
    Phi = (torch.rand(1, 32, 32, 8, generator=g) < 0.5).float().to(DEV)
    gt = torch.rand(1, 32, 32, 8, generator=g).to(DEV)
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    convs = [m for m in solver.nonlinear_op.modules() if isinstance(m, RealSNConv2d)]
    with torch.no_grad():
        rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None))
    return deq, convs, rec


def test_engine_f_calls_move_the_module_as_its_own_forward_does():
    dev, convs, rec = _engine_run({"train_realsn": "device"})
    info = dev._engine[1].last_info
    assert info["denoiser_path"] == "train realsn per layer" and info["f_calls"] == 8 and info["graph"] is False and dev._engine[1]._graph is None
    assert info["train_realsn"] == "device" and info["train_realsn_reason"] is None
    mod, convs2, rec2 = _engine_run()
    assert mod._engine[1].last_info["denoiser_path"] != "train realsn per layer" and mod._engine[1].last_info["f_calls"] == 8
    for i, (m, m2) in enumerate(zip(convs, convs2)):                      # the power step does not depend on the iterate: exact
        assert torch.equal(m.weight_u, m2.weight_u) and torch.equal(m.weight, m2.weight), i
    print(f"reconstruction, device f-calls against the module's: relative L2 {rc.rel_l2(rec.cpu(), rec2.cpu()):.3e}")
    assert rc.rel_l2(rec.cpu(), rec2.cpu()) <= 1e-4
    with pytest.raises(ValueError, match="train-mode RealSNConv2d"):
        _engine_run({"train_realsn": "device", "use_graph": True})


def test_engine_option_changes_nothing_in_eval_mode():
    a, _, rec_a = _engine_run({"train_realsn": "device"}, train=False)
    b, _, rec_b = _engine_run(train=False)
    ia, ib = a._engine[1].last_info, b._engine[1].last_info
    assert ia["denoiser_path"] == ib["denoiser_path"] != "train realsn per layer" and ia["f_calls"] == ib["f_calls"] and ia["graph"] == ib["graph"]
    assert ia["train_realsn"] == "module" and "train mode" in ia["train_realsn_reason"]
    assert torch.equal(rec_a, rec_b)


def test_one_f_call_against_the_float64_chain_on_the_same_weights():
    """2 x 19 x 23: ragged against the 16-pixel tiles, a batch of more than one.  The yardstick is conv2d in float64 on the weights the
    call left in the module's `weight` buffers - the ones its kernels' packs were made from."""
    from deqsci_amd import _hip, checkpoint
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.engine import _Denoiser
    from deqsci_amd.networks.simplecnn import RealSNConv2d
    solver, _ = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 6)
    net = solver.nonlinear_op.train()
    twin = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 6)[0].nonlinear_op.train()
    den = _Denoiser(net, train_realsn="device")
    assert den.rsn is not None and den.train_why is None
    x = torch.rand(1, 2, 19, 23, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    den.prepare(4, x.device)
    with torch.no_grad():
        out, is_noise = den.run(x, 0)
        want_module = twin(x.view(2, 1, 19, 23))
    assert is_noise and den.last_path == "train realsn per layer" and tuple(out.shape) == (1, 2, 19, 23)
    convs = [m for m in net.modules() if isinstance(m, RealSNConv2d)]
    for m, m2 in zip(convs, (m for m in twin.modules() if isinstance(m, RealSNConv2d))):
        assert torch.equal(m.weight, m2.weight) and torch.equal(m.weight_u, m2.weight_u)       # bit-equal weights: the module's own kernels
    kind = _hip.conv64_kernel_for(2, 19, 23, x.device, "fast32")
    cs = [der.c_of("c1_to_64")] + [der.c_of(kind)] * (len(convs) - 2) + [der.c_of("tail_valu")]
    h, e = x.view(2, 1, 19, 23).double().cpu(), torch.zeros(2, 1, 19, 23, dtype=torch.float64)
    for i, (m, c) in enumerate(zip(convs, cs)):
        w = m.weight.detach().double().cpu()
        mid = 0 < i < len(convs) - 1
        S = der.s_wino(h.abs(), w.abs(), {"f22": (2, 2), "f44": (4, 4)}[kind]) if mid else der.s_plain(h.abs(), w.abs())
        e = F.conv2d(e, w.abs(), padding=1) + c * der.U * S
        h = F.conv2d(h, w, padding=1)
        if i < len(convs) - 1:
            h = torch.relu(h)
    err = (out.view(2, 1, 19, 23).double().cpu() - h).abs()
    worst, ratio = float(err.max()), float((err / e).max())
    print(f"one train-mode f-call at 2x19x23 on the {kind} kernel against the float64 chain: worst element {worst:.3e} "
          f"(largest |noise| {float(h.abs().max()):.3e}), worst err / bound {ratio:.4f}; against the module's own forward "
          f"{float((out.view(2, 1, 19, 23) - want_module).abs().max()):.3e}")
    assert bool((err <= e).all())


# ----------------------------------------------------------------------------- (d): a training step against the reference
MODES = {"defaults": ({}, "autograd", "autograd"),
         "engine": ({"train_realsn": "device"}, "autograd", "autograd"),
         "parameter": ({}, "autograd", "device+realsn"),
         "implicit": ({}, "device+realsn", "autograd"),
         "all": ({"train_realsn": "device"}, "device+realsn", "device+realsn")}
_STEPS = {}


def _golden_solver(golden):
    """tests/test_realsn_gpu.py's: RealSN_SimpleCNN from the shipped checkpoint as golden (b) modifies it, in train mode, on the device."""
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
            m.weight_orig.copy_(m.weight * s)
            m.weight_u.copy_(rc.unit_u(m.weight_u.shape, rc.U_SEED + i))
    assert "".join(rc.sha16(m.weight_orig) for m in convs) + "".join(rc.sha16(m.weight_u) for m in convs) == str(golden["b.hash"])
    net.train()
    for p in solver.parameters():
        p.requires_grad_(True)
    return solver.to(DEV), convs


def _training_step(golden, mode):
    import deqsci_amd
    options, implicit, parameter = MODES[mode]
    solver, convs = _golden_solver(golden)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(golden["b.iters"]), tol=1e-9)
    deq.engine_options = dict(options)
    deq.implicit_backward, deq.parameter_backward = implicit, parameter
    Phi, gt = (t.to(DEV) for t in rc.problem())
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt).detach())
    loss = F.mse_loss(rec, gt)
    solver.zero_grad()
    loss.backward()
    return {"deq": deq, "rec": rec.detach(), "loss": loss.detach(), "grads": [m.weight_orig.grad.clone() for m in convs],
            "weight": [m.weight.clone() for m in convs], "weight_u": [m.weight_u.clone() for m in convs]}


def _step(golden, mode):
    if mode not in _STEPS:
        _STEPS[mode] = _training_step(golden, mode)
    return _STEPS[mode]


@pytest.mark.parametrize("mode", ["engine", "parameter", "implicit", "all"])
def test_training_step_against_the_reference(golden, mode):
    s = _step(golden, mode)
    deq = s["deq"]
    figures = {"rec": rc.rel_l2(s["rec"].cpu(), golden["b.rec"]), "loss": abs(float(s["loss"]) - float(golden["b.loss"])) / float(golden["b.loss"])}
    for i in range(len(s["grads"])):
        figures[f"grad.{i}"] = rc.deviation(golden, f"b.grad.{i}", s["grads"][i])
        figures[f"weight.{i}"] = rc.deviation(golden, f"b.weight.{i}", s["weight"][i])
        figures[f"weight_u.{i}"] = rc.deviation(golden, f"b.weight_u.{i}", s["weight_u"][i])
    print(f"{mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()),
          f"forward_res {deq.forward_res:.4e} backward_res {deq.backward_res:.4e}")
    for name, value in figures.items():
        assert value <= 1e-4, (name, value)
    assert abs(deq.forward_res - float(golden["b.forward_res"])) < 1e-2 * float(golden["b.forward_res"])
    assert abs(deq.backward_res - float(golden["b.backward_res"])) < 1e-2 * float(golden["b.backward_res"])
    _, implicit, parameter = MODES[mode]
    assert deq.last_backward_path == ("device" if implicit == "device+realsn" else "autograd")
    assert deq.last_parameter_path == ("device" if parameter == "device+realsn" else "autograd")
    assert deq.backward_fallback_reason is None and deq.parameter_fallback_reason is None
    if MODES[mode][0]:
        info = deq._engine[1].last_info
        assert info["denoiser_path"] == "train realsn per layer" and info["train_realsn"] == "device" and info["graph"] is False
    # the power step does not depend on the iterate, and every path runs it on the same kernels: max_iter + 2 steps, the same bits
    base = _step(golden, "defaults")
    for i, (a, b) in enumerate(zip(s["weight_u"], base["weight_u"])):
        assert torch.equal(a, b), i
    for i, (a, b) in enumerate(zip(s["weight"], base["weight"])):
        assert torch.equal(a, b), i


# ----------------------------------------------------------------------------- (e): determinism, no synchronisation
def test_two_identical_steps_give_the_same_bits(golden):
    a, b = _step(golden, "all"), _training_step(golden, "all")
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(x, y), i
    assert torch.equal(a["rec"], b["rec"]) and bool(all(torch.isfinite(g).all() for g in a["grads"]))


def test_taped_call_and_backward_do_not_synchronise(golden, monkeypatch):
    """The taped call, f0 = f(z0), the device map and its products, and the backward through the taped call, under "device+realsn" for
    both - everything between the taped call and the end of backward but the solver's own per-iteration residual read-back."""
    import deqsci_amd
    solver, convs = _golden_solver(golden)
    Phi, gt = (t.to(DEV) for t in rc.problem())
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    z_in = deqsci_amd.initial_point(y, Phi, Ps, gt).detach()
    grad = torch.randn(z_in.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2))

    def step():
        z = solver.forward_param_device(z_in, y, Phi, Ps, train_realsn=True)
        z0 = z.clone().detach().requires_grad_()
        solver(z0, y, Phi, Ps)
        jmap = solver.device_vjp(Phi, Ps, train_realsn=True)
        g = jmap(jmap(grad) + grad) + grad
        solver.zero_grad()
        z.backward(g)
        return [m.weight_orig.grad for m in convs]

    step()                                                            # (the library and every kernel loaded)
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError("host synchronisation")
    for name in ("item", "cpu", "tolist", "__float__"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    monkeypatch.setattr(torch.cuda, "synchronize", refuse)
    grads = step()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) and float(g.norm()) > 0 for g in grads)


# ----------------------------------------------------------------------------- (f): refusals at run time
def test_realsn_with_batchnorm_stays_on_the_old_paths():
    import deqsci_amd
    from deqsci_amd.networks import DnCNN
    from deqsci_amd.solvers import EquilibriumProxGradSCI
    from deqsci_amd.operators import A_torch_, At_torch_
    torch.manual_seed(3)
    net = DnCNN(1, 5, lip=1.0, no_bn=False).train()
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1).to(DEV)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=3, beta=1.0, lam=1e-2, max_iter=3, tol=1e-9)
    deq.engine_options = {"train_realsn": "device"}
    deq.implicit_backward = deq.parameter_backward = "device+realsn"
    g = torch.Generator().manual_seed(9)
    Phi = (torch.rand(1, 16, 16, 2, generator=g) < 0.5).float().to(DEV)
    gt = torch.rand(1, 16, 16, 2, generator=g).to(DEV)
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None).detach())
    F.mse_loss(rec, gt).backward()
    assert deq.last_backward_path == "autograd" and deq.last_parameter_path == "autograd"
    assert "BatchNorm" in deq.backward_fallback_reason and "BatchNorm" in deq.parameter_fallback_reason
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with torch.no_grad():
        deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None))
    info = deq._engine[1].last_info
    assert info["train_realsn"] == "module" and "BatchNorm" in info["train_realsn_reason"] and info["denoiser_path"] != "train realsn per layer"
