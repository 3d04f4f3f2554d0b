"""GPU: the mask gradient through the public interface.
  * operator level - A_torch_, At_torch_, phi_sum, gap_update and a learnable SCIOperator with Phi.requires_grad, against the float64
    references of tests/sci_grad_ref.py (themselves held to float64 CPU autograd by tests/test_sci_grad_host.py) within its bounds, for a
    mask per sample, a shared (1,H,W,B) mask and a shared 3-D (H,W,B) mask; the gradient has Phi's own shape;
  * end to end - every case of tests/golden/mask_grad.npz (the reference's own DEQFixedPoint runs, tests/golden/make_mask_grad_golden.py)
    through DEQFixedPoint under implicit_backward "autograd" / "device" and parameter_backward "autograd" / "device" (SimpleCNN) or
    "device+bn" (FFDNet): grad.Phi within 1e-4 (SimpleCNN) / 5e-4 (FFDNet) relative L2 - the gates of backward.npz and
    backward_ffdnet.npz, against a measured conditioning of 1.1e-6 - the parameter gradients within the same gates, sigma_after equal;
  * no regression - a mask that asks for no gradient takes none of the new launches and gives the bits of a run on a detached copy."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sci_grad_ref as sg
from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint
    from deqsci_amd.cli import build_pipeline

DEV = "cuda"
BSZ = sg.BSZ
H, W, B = 37, 53, 8
GRAD_TOL = {"SimpleCNN": 1e-4, "ffdnet": 5e-4}
MASK_SHAPES = ("persample", "shared4d", "shared3d")


@functools.lru_cache(maxsize=None)
def data(shared):
    return sg.case_data(H, W, B, "uniform", shared)


def dev(t, requires_grad=False):
    return t.reshape(t.shape[0], H, W, *t.shape[2:]).contiguous().to(DEV).requires_grad_(requires_grad)


def mask_leaf(Phi, kind):
    p = dev(Phi)
    return (p[0].contiguous() if kind == "shared3d" else p).requires_grad_(True)


def logical(t, like):
    return t.detach().reshape(like.shape).cpu()


# ----------------------------------------------------------------------------- operator level
@pytest.mark.parametrize("kind", MASK_SHAPES)
def test_operators_give_the_mask_gradient(kind):
    shared = kind != "persample"
    Phi, z, g, y, s, a, gs_in = data(shared)
    # y = A(x, Phi): grad_Phi = grad_y x, grad_x = At(grad_y, Phi)
    P, x = mask_leaf(Phi, kind), dev(z, True)
    out = deqsci_amd.A_torch_(x, P)
    out.backward(dev(a))
    assert P.grad.shape == P.shape and sg.ratio(logical(P.grad, Phi), *sg.ref_mask_grad(a, z, shared)) <= 1
    assert torch.equal(x.grad, _hip.sci_adjoint(dev(a), P.detach()))
    # only the mask asks
    P2 = mask_leaf(Phi, kind)
    deqsci_amd.A_torch_(dev(z), P2).backward(dev(a))
    assert torch.equal(P2.grad, P.grad)
    # x = At(y, Phi): grad_Phi = y grad_x
    P, yy = mask_leaf(Phi, kind), dev(a, True)
    deqsci_amd.At_torch_(yy, P).backward(dev(g))
    assert P.grad.shape == P.shape and sg.ratio(logical(P.grad, Phi), *sg.ref_mask_grad(a, g, shared)) <= 1
    assert torch.equal(yy.grad, _hip.sci_forward(dev(g), P.detach()))
    # phi_sum
    P = mask_leaf(Phi, kind)
    S = deqsci_amd.phi_sum(P)
    assert S.requires_grad and torch.equal(S.detach(), _hip.phi_sum(P.detach()))
    S.backward(dev(gs_in)[0] if kind == "shared3d" else dev(gs_in))
    assert P.grad.shape == P.shape and torch.equal(logical(P.grad, Phi), sg.ref_phi_sum_grad(Phi, gs_in))
    # gap_update, all four inputs
    P, zz, yy = mask_leaf(Phi, kind), dev(z, True), dev(y, True)
    ss = (dev(s)[0].contiguous() if kind == "shared3d" else dev(s)).requires_grad_(True)
    z1 = deqsci_amd.operators.gap_update(zz, yy, P, ss)
    assert torch.equal(z1.detach(), _hip.gap_update(zz.detach(), P.detach(), yy.detach(), ss.detach()))
    z1.backward(dev(g))
    ref = sg.ref_gap_grad(z, Phi, g, y, s)
    assert P.grad.shape == P.shape and ss.grad.shape == ss.shape
    for name, t, like in (("gphi", P.grad, Phi), ("gs", ss.grad, s), ("gz", zz.grad, z), ("gy", yy.grad, y)):
        r = sg.ratio(logical(t, like), *ref[name])
        print(f"gap_update {kind} {name}: err / bound {r:.3f}")
        assert r <= 1, name
    # the mask alone: the same bits, nothing else produced
    P2 = mask_leaf(Phi, kind)
    deqsci_amd.operators.gap_update(dev(z), dev(y), P2, ss.detach()).backward(dev(g))
    assert torch.equal(P2.grad, P.grad)


def test_learnable_sci_operator():
    Phi, z, g, y, s, a, _ = data(True)
    fixed = deqsci_amd.SCIOperator(dev(Phi))
    assert list(fixed.parameters()) == [] and "Phi" in dict(fixed.named_buffers())
    op = deqsci_amd.SCIOperator(dev(Phi), learnable=True)
    assert [n for n, _ in op.named_parameters()] == ["Phi"] and op.Phi.requires_grad and op.Phi.shape == (1, H, W, B)
    meas = op(dev(z))
    assert meas.requires_grad and torch.equal(meas.detach(), fixed(dev(z)))
    back = op.adjoint(dev(a))
    (meas * dev(a)).sum().backward()
    assert sg.ratio(logical(op.Phi.grad, Phi), *sg.ref_mask_grad(a, z, True)) <= 1
    op.Phi.grad = None
    (back * dev(g)).sum().backward()
    assert sg.ratio(logical(op.Phi.grad, Phi), *sg.ref_mask_grad(a, g, True)) <= 1


def test_admm_variant_refuses_a_mask_gradient():
    Phi, z, g, y, s, _, _ = data(False)
    f = deqsci_amd.solvers.EquilibriumADMMSCI(deqsci_amd.A_torch_, deqsci_amd.At_torch_, torch.nn.Identity(), eta=0.2)
    with pytest.raises(NotImplementedError, match="mask gradient"):
        f(dev(z), dev(g), dev(y), dev(Phi, True), dev(s))
    with pytest.raises(NotImplementedError, match="mask gradient"):
        f(dev(z), dev(g), dev(y), dev(Phi), dev(s, True))


# ----------------------------------------------------------------------------- end to end against the reference
def _G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _solver(kind):
    return build_pipeline(kind, checkpoint.shipped("cnn" if kind == "SimpleCNN" else "ffdnet_gray"), 12)[0]


def _run(g, kind, mask, trainable, implicit="autograd", parameter="autograd", mask_grad=True):
    """The training forward and backward of make_mask_grad_golden.py: y and Phi_sum formed from Phi under the tape when mask_grad."""
    solver = _solver(kind)
    for p in solver.parameters():
        p.requires_grad_(trainable)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(g["iters"]), tol=1e-9)
    deq.implicit_backward, deq.parameter_backward = implicit, parameter
    Phi, gt = _G(g["Phi." + mask]).requires_grad_(mask_grad), _G(g["gt"])
    y = deqsci_amd.A_torch_(gt, Phi)
    Ps = deqsci_amd.phi_sum(Phi)
    assert y.requires_grad == Ps.requires_grad == mask_grad
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt).detach())
    loss = F.mse_loss(rec, gt)
    solver.zero_grad()
    if rec.requires_grad:
        loss.backward()
    return solver, deq, rec.detach(), loss.detach(), Phi


E2E = [(kind, mask, params, implicit, parameter) for kind in ("SimpleCNN", "ffdnet") for mask in ("ps", "sh") for params in ("train", "frozen")
       for implicit in ("autograd", "device") for parameter in ("autograd", "device" if kind == "SimpleCNN" else "device+bn")]


@pytest.mark.parametrize("kind,mask,params,implicit,parameter", E2E, ids=["-".join(c) for c in E2E])
def test_phi_grad_vs_reference_golden(kind, mask, params, implicit, parameter):
    g = np.load(os.path.join(GOLDEN, "mask_grad.npz"))
    tag = f"{kind}.{mask}.{params}"
    assert float(g["conditioning"].max()) < 1e-5
    solver, deq, rec, loss, Phi = _run(g, kind, mask, params == "train", implicit, parameter)
    assert deq.last_backward_path == implicit
    assert Phi.grad is not None and Phi.grad.shape == Phi.shape
    r = rel_l2(Phi.grad.cpu().numpy(), g[tag + ".grad.Phi"])
    print(f"{tag} implicit={implicit} parameter={parameter}: grad.Phi rel L2 vs the reference {r:.3e}")
    assert r < GRAD_TOL[kind]
    assert (Phi.grad[:, 0, :2] == 0).all() and (g[tag + ".grad.Phi"][:, 0, :2] == 0).all()   # an all-zero pixel measures nothing: y = fb = q = 0 there, and Phi_sum is cut
    assert rel_l2(rec.cpu().numpy(), g[tag + ".rec"]) <= 1e-4
    assert abs(float(loss) - float(g[tag + ".loss"])) < 1e-5 * float(g[tag + ".loss"])
    assert abs(deq.forward_res - float(g[tag + ".forward_res"])) < 1e-2 * float(g[tag + ".forward_res"])
    assert abs(deq.backward_res - float(g[tag + ".backward_res"])) < 1e-2 * float(g[tag + ".backward_res"])
    if kind == "ffdnet":
        assert np.array_equal(solver.noise_sigma.cpu().numpy(), g[tag + ".sigma_after"])
    seen = 0
    for name, p in solver.named_parameters():
        if params == "frozen":
            assert p.grad is None
            continue
        if tag + ".grad." + name in g.files:
            rp = rel_l2(p.grad.cpu().numpy(), g[tag + ".grad." + name])
        else:
            rp = rel_l2(p.grad[:2].cpu().numpy(), g[tag + ".gradslice." + name])
        seen += 1
        assert rp < GRAD_TOL[kind], (name, rp)
    assert seen == (len([k for k in g.files if k.startswith(tag + ".grad") and not k.endswith("grad.Phi")]) if params == "train" else 0)


# ----------------------------------------------------------------------------- no regression
@pytest.mark.parametrize("kind,parameter", [("SimpleCNN", "device"), ("ffdnet", "device+bn")])
def test_a_mask_without_gradient_is_data(kind, parameter, monkeypatch):
    """A mask that asks for no gradient: none of the new launches is made, and the reconstruction and the parameter gradients have the
    bits of a run on a detached copy of a mask that does.  With the gradient on, the reconstruction keeps those bits (the forward is
    the same kernels) and so do the parameter gradients: G1's gz is bit-equal to the GAP launch it replaces (tests/test_sci_grad_gpu.py
    (c)), and the backward solve runs on a graph the mask is not on."""
    g = np.load(os.path.join(GOLDEN, "mask_grad.npz"))
    on = _run(g, kind, "ps", True, "device", parameter, mask_grad=True)

    def refuse(*a, **k):
        raise AssertionError("a mask-gradient launch without a mask gradient")
    for name in ("gap_update_grad", "sci_mask_grad", "phi_sum_grad"):
        monkeypatch.setattr(_hip, name, refuse)
    off = _run(g, kind, "ps", True, "device", parameter, mask_grad=False)
    assert off[4].grad is None
    solver = _solver(kind)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(g["iters"]), tol=1e-9)
    deq.implicit_backward, deq.parameter_backward = "device", parameter
    Phi = _G(g["Phi.ps"]).requires_grad_(True).detach()
    gt = _G(g["gt"])
    y, Ps = deqsci_amd.A_torch_(gt, Phi), deqsci_amd.phi_sum(Phi)
    rec = deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, gt))
    solver.zero_grad()
    F.mse_loss(rec, gt).backward()
    for other in (off, on):
        assert torch.equal(other[2], rec.detach())
        for p, q in zip(other[0].parameters(), solver.parameters()):
            assert torch.equal(p.grad, q.grad)
