"""CPU: the host side of train-mode BatchNorm (deqsci_amd/vjp.py: param_eligibility(train_bn=True), plan_forward_train_bn,
plan_param_grads_train_bn), what stays as it was without the keyword, the reference's one f-call (tests/golden/bn_train.npz, case b.)
through the host plan, the "device+bn-train" switch and the engine option, and the argument validation of csrc/bn_train.hip's entry
points, which happens before any launch."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from deqsci_amd import _hip, checkpoint, vjp
from deqsci_amd.cli import build_denoiser, build_pipeline
from deqsci_amd.layers import conv_bn_stack, conv_stack
from deqsci_amd.networks import DnCNN, FFDNet
from test_wgrad_bn_host import mixed_bn_dncnn, seeded_bn_dncnn, seeded_ffdnet

OLD_REFUSAL = "BatchNorm2d in train mode (batch statistics have no device kernel)"


def load_golden():
    """tests/golden/bn_train.npz and its parts (make_bn_train_golden.py splits the arrays over archives below the size limit), merged."""
    out = {}
    for fn in [os.path.join(GOLDEN, "bn_train.npz")] + sorted(glob.glob(os.path.join(GOLDEN, "bn_train.part*.npz"))):
        with np.load(fn) as z:
            out.update({k: z[k] for k in z.files})
    return out


def golden_b_net(g):
    """Case b.'s seeded conv + BN + ReLU DnCNN in the state before its one train-mode f-call."""
    net = DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser")
    net.load_state_dict({k[len("b.state."):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("b.state.")})
    return net.train()


def test_train_bn_accepts_both_families_in_train_mode():
    assert vjp.param_eligibility(build_denoiser("ffdnet").train(), train_bn=True) == (True, "FFDNet with its BatchNorm in train mode")
    for depth in (3, 5, 17):
        assert vjp.param_eligibility(seeded_bn_dncnn(depth, 2).train(), train_bn=True) == (True, "bias-free conv [+ train-mode BN] + ReLU stack")
    # a stack without a BatchNorm has nothing to normalise: served in either mode
    assert vjp.param_eligibility(build_denoiser("SimpleCNN").train(), train_bn=True)[0]
    net = seeded_bn_dncnn(4, 1).train()
    assert all(a is b for a, b in zip(vjp.grad_parameters(net, train_bn=True), net.parameters())) and len(vjp.grad_parameters(net, train_bn=True)) == 8
    assert len(vjp.grad_parameters(build_denoiser("ffdnet").train(), train_bn=True)) == 41


def test_train_bn_refusals_name_the_cause():
    ok, why = vjp.param_eligibility(seeded_bn_dncnn(5, 1), train_bn=True)                  # eval mode: "device+bn"'s job
    assert not ok and "eval mode" in why and "device+bn" in why
    ok, why = vjp.param_eligibility(build_denoiser("ffdnet").eval(), train_bn=True)
    assert not ok and "eval mode" in why and "FFDNet" in why
    for kw, word in ((dict(momentum=None), "momentum=None"), (dict(affine=False), "affine"), (dict(track_running_stats=False), "running statistics")):
        net = seeded_bn_dncnn(5, 1)
        net.dncnn[3] = torch.nn.BatchNorm2d(64, **kw)
        ok, why = vjp.param_eligibility(net.train(), train_bn=True)
        assert not ok and word in why, (kw, why)
    net = seeded_bn_dncnn(5, 1).train()
    net.dncnn[3].momentum = 1                                                                # an int is not torch's float momentum
    assert not vjp.param_eligibility(net, train_bn=True)[0]
    ok, why = vjp.param_eligibility(build_denoiser("RealSN_SimpleCNN").train(), train_bn=True)
    assert not ok and "RealSNConv2d" in why
    ok, why = vjp.param_eligibility(FFDNet(3, tag="ffdnet").train(), train_bn=True)
    assert not ok and "3 channels" in why
    ok, why = vjp.param_eligibility(DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="conv2d").train(), train_bn=True)
    assert not ok and "'conv2d'" in why
    biased = seeded_bn_dncnn(5, 1)
    biased.dncnn[2] = torch.nn.Conv2d(64, 64, kernel_size=3, padding=1, bias=True)
    ok, why = vjp.param_eligibility(biased.train(), train_bn=True)
    assert not ok and "bias" in why
    with pytest.raises(ValueError, match="exclude"):
        vjp.param_eligibility(seeded_bn_dncnn(5, 1).train(), frozen_bn=True, train_bn=True)
    with pytest.raises(ValueError, match="eval mode"):
        vjp.grad_parameters(seeded_bn_dncnn(5, 1), train_bn=True)
    with pytest.raises(ValueError, match="eval mode"):
        vjp.plan_forward_train_bn(seeded_bn_dncnn(5, 1), torch.zeros(1, 1, 4, 4))


def test_answers_without_the_keyword_are_what_they_were():
    for net in (seeded_bn_dncnn(5, 1).train(), build_denoiser("ffdnet").train()):
        ok, why = vjp.param_eligibility(net, frozen_bn=True)
        assert not ok and why.endswith(OLD_REFUSAL)
        assert not vjp.param_eligibility(net)[0] and not vjp.eligibility(net)[0]
        with pytest.raises(ValueError, match="train mode"):
            vjp.grad_parameters(net)
    mods = seeded_bn_dncnn(5, 1).train().dncnn
    assert conv_stack(mods) == conv_bn_stack(mods) == (None, "BatchNorm2d in train mode (batch statistics: its Jacobian is not a fixed scale)")
    assert conv_bn_stack(mods, train_bn=True)[0] is not None
    assert vjp.param_eligibility(seeded_bn_dncnn(5, 1), frozen_bn=True) == (True, "bias-free conv [+ frozen BN] + ReLU stack")
    assert vjp.param_eligibility(build_denoiser("ffdnet").eval(), frozen_bn=True) == (True, "FFDNet with its BatchNorm frozen")


def _set_bn(net, eps, momentum):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps, m.momentum = eps, momentum
    return net


def _buffers_equal(a, b, tol):
    for (name, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(p) == int(q), name
        else:
            assert p.dtype == q.dtype and float((p - q).abs().max()) <= tol * float(q.abs().max()), name


@pytest.mark.parametrize("eps,momentum", [(1e-5, 0.1), (1e-3, 0.3)], ids=("torch-defaults", "other"))
def test_plan_forward_train_bn_is_the_module_in_float64(eps, momentum):
    """Both families keep torch's defaults (eps 1e-5, momentum 0.1: FFDNet's and the DnCNN's nn.BatchNorm2d(64)); another pair shows that the
    plan reads them from the module."""
    g = torch.Generator().manual_seed(5)
    for net, sigma, (H, W) in ((_set_bn(seeded_bn_dncnn(5, 6).double().train(), eps, momentum), None, (13, 11)),
                               (_set_bn(seeded_ffdnet(4).double().train(), eps, momentum), torch.tensor([0.1, 0.235, 0.02], dtype=torch.float64), (10, 14))):
        x = torch.rand(3, 1, H, W, generator=g, dtype=torch.float64)
        module, frozen = copy.deepcopy(net), copy.deepcopy(net)
        for step in range(2):                                                    # two calls: the buffers move twice
            want = (module(x) if sigma is None else module(x, sigma)).detach()
            got, masks = vjp.plan_forward_train_bn(net, x, sigma)
            assert got.dtype == torch.float64 and float((got - want).norm() / want.norm()) <= 1e-12
            _buffers_equal(net, module, 1e-13)
        assert all(int(m.num_batches_tracked) == 2 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
        assert len(masks) == len(vjp.grad_parameters(net, train_bn=True)) // 3 + 1 and all(m.dtype == torch.bool for m in masks)
        pristine = copy.deepcopy(frozen)
        again, _ = vjp.plan_forward_train_bn(frozen, x, sigma, update=False)     # update=False: the same answer from the first state, no buffer moves
        _buffers_equal(frozen, pristine, 0.0)
        assert all(int(m.num_batches_tracked) == 0 for m in frozen.modules() if isinstance(m, torch.nn.BatchNorm2d))
        assert float((again - got).norm() / got.norm()) <= 1e-12                 # batch statistics do not read the buffers


def _check_against_autograd(net, x, v, sigma):
    params = vjp.grad_parameters(net, train_bn=True)
    before = copy.deepcopy(net.state_dict())
    xr = x.clone().requires_grad_(True)
    module = copy.deepcopy(net)
    want = torch.autograd.grad(module(xr) if sigma is None else module(xr, sigma), vjp.grad_parameters(module, train_bn=True) + ([xr] if sigma is None else []), v)
    got, masks, gx = vjp.plan_param_grads_train_bn(net, x, v, sigma, input_grad=True)
    assert len(got) == len(params)
    for i, (a, b) in enumerate(zip(got + ([gx] if sigma is None else []), want)):
        assert a.shape == b.shape and a.dtype == torch.float64
        assert float((a - b).norm() / b.norm()) <= 1e-10, i
    assert (gx is None) == (sigma is not None)                                   # FFDNet detaches its input
    assert all(torch.equal(t, before[k]) for k, t in net.state_dict().items())   # the backward statement moves no buffer
    again, _ = vjp.plan_param_grads_train_bn(net, x, v, sigma, masks=masks)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    return got


def test_plan_param_grads_train_bn_equals_float64_autograd():
    g = torch.Generator().manual_seed(3)
    net = seeded_bn_dncnn(5, 6).double().train()
    x = torch.rand(3, 1, 13, 11, generator=g, dtype=torch.float64)
    v = torch.randn(3, 1, 13, 11, generator=g, dtype=torch.float64)
    got = _check_against_autograd(net, x, v, None)
    assert len(got) == 2 + 3 * 3 and float(got[2][3].abs()) > 0                  # the gradient of a gamma that is exactly 0 is not 0
    ffd = seeded_ffdnet(4).double().train()
    x = torch.rand(3, 1, 10, 14, generator=g, dtype=torch.float64)
    v = torch.randn(3, 1, 10, 14, generator=g, dtype=torch.float64)
    got = _check_against_autograd(ffd, x, v, torch.tensor([0.1, 0.235, 0.02], dtype=torch.float64))
    assert len(got) == 41 and got[0].shape == (64, 5, 3, 3) and got[-1].shape == (4, 64, 3, 3)
    with pytest.raises(ValueError, match="sigma"):
        vjp.plan_param_grads_train_bn(ffd, x, v)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        vjp.plan_forward_train_bn(seeded_bn_dncnn(3, 1).train(), torch.zeros(1, 1, 1, 1))


def test_plan_param_grads_train_bn_equals_float64_autograd_mixed_net():
    """64 -> 64 layers with and without a BatchNorm in one stack: the walk takes a rule per layer."""
    net = mixed_bn_dncnn().double().train()
    assert vjp.param_eligibility(net, train_bn=True) == (True, "bias-free conv [+ train-mode BN] + ReLU stack")
    g = torch.Generator().manual_seed(8)
    x = torch.rand(2, 1, 12, 20, generator=g, dtype=torch.float64)
    v = torch.randn(2, 1, 12, 20, generator=g, dtype=torch.float64)
    assert len(_check_against_autograd(net, x, v, None)) == 2 + 3 + 1 + 3


def test_golden_one_fcall_through_the_host_plan():
    """Case b.: the reference's own train-mode f-call in fp32 against the float64 statement - the project's parity bar, 1e-4."""
    g = load_golden()
    net = golden_b_net(g)
    gammas = [m.weight for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(gammas) == 3 and all(bool((w == 0).any()) and bool((w < 0).any()) for w in gammas)
    x, v = torch.from_numpy(g["b.x"]).double(), torch.from_numpy(g["b.v"]).double()
    net64 = net.double()
    noise, _ = vjp.plan_forward_train_bn(net64, x)
    grads, _, gx = vjp.plan_param_grads_train_bn(net64, x, v, input_grad=True)
    worst = {"noise": rel_l2(noise, g["b.noise"]), "grad_input": rel_l2(gx, g["b.grad_input"])}
    names = [name for name, _ in net.named_parameters()]
    assert [id(p) for p in vjp.grad_parameters(net64, train_bn=True)] == [id(p) for p in net64.parameters()]
    for name, got in zip(names, grads):
        worst["grad." + name] = rel_l2(got, g["b.grad." + name])
    for name, b in net64.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g["b.buffer." + name]) == 1
        else:
            worst["buffer." + name] = rel_l2(b, g["b.buffer." + name])
    print({k: f"{e:.2e}" for k, e in worst.items()})
    assert max(worst.values()) <= 1e-4, worst


def test_golden_training_step_is_stored_with_its_conditioning():
    g = load_golden()
    cond = {k: float(v) for k, v in g.items() if k.startswith("a.conditioning.")}
    grads = [k for k in g if k.startswith("a.grad.")]
    bufs = [k for k in g if k.startswith("a.buffer.")]
    assert len(grads) == 41 and len(bufs) == 39 and len(cond) == 1 + 41 + 26 and max(cond.values()) < 1e-5
    assert all(int(g[k]) == int(g["a.iters"]) + 2 == 14 for k in bufs if k.endswith("num_batches_tracked"))
    net = build_denoiser("ffdnet")
    names = {id(p): name for name, p in net.named_parameters()}
    assert ["a.grad." + names[id(p)] for p in vjp.grad_parameters(net.train(), train_bn=True)] == grads
    for fn in glob.glob(os.path.join(GOLDEN, "bn_train*.npz")):
        assert os.path.getsize(fn) < 1 << 20, fn


def test_switch_and_engine_option_take_the_new_values():
    import deqsci_amd
    solver, deq = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), 4, device="cpu")
    solver.nonlinear_op.train()
    ok, why = solver.device_param_eligibility(frozen_bn=True)
    assert not ok and why.endswith(OLD_REFUSAL)                                  # "device+bn" refuses what it refused
    assert solver.device_param_eligibility(train_bn=True) == (True, "FFDNet with its BatchNorm in train mode")
    solver.nonlinear_op.eval()
    assert solver.device_param_eligibility(train_bn=True) == solver.device_param_eligibility(frozen_bn=True) == (True, "FFDNet with its BatchNorm frozen")
    plain = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 4, device="cpu")[0]
    assert plain.device_param_eligibility(train_bn=True) == plain.device_param_eligibility() == (True, "bias-free conv + ReLU stack")
    rsn = build_pipeline("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), 4, device="cpu")[0]
    assert rsn.device_param_eligibility(train_bn=True) == rsn.device_param_eligibility(frozen_bn=True)
    other = deqsci_amd.EquilibriumProxGradSCI(lambda x, Phi: x, lambda y, Phi: y, solver.nonlinear_op, eta=0.2)
    assert "custom A / At" in other.device_param_eligibility(train_bn=True)[1]
    deq.parameter_backward = "device+bn_train"
    with pytest.raises(ValueError, match=r"'device\+bn-train'"):
        deq._taped_call(None, None, None, None)
    deq.parameter_backward = "device+bn-train"
    with pytest.raises(Exception) as info:                                        # an accepted value goes on to the call itself
        deq._taped_call(None, None, None, None)
    assert "parameter_backward" not in str(info.value)
    # the engine option: "module" by default, "device" accepted, anything else refused; on the CPU nothing is served
    from deqsci_amd.engine import DEQSCIEngine
    net = build_denoiser("ffdnet").train()
    assert DEQSCIEngine(net).train_bn == "module" and DEQSCIEngine(net).den.train is None
    with pytest.raises(ValueError, match="'module' or 'device'"):
        DEQSCIEngine(net, train_bn="hip")
    eng = DEQSCIEngine(net, train_bn="device")
    assert eng.den.train is None and "GPU" in eng.den.train_why and eng.den._route(8, 24, 20, "cpu", "fast", False) == "module"
    eng = DEQSCIEngine(seeded_bn_dncnn(5, 1), train_bn="device")                 # eval mode: the folded kernels' business, no reason to give
    assert eng.den.train is None and eng.den.train_why is None and eng.den.fast is not None
    deq.engine_options = {"train_bn": "device"}
    assert deq._train_solve_engine() is None                                         # not served here: the solve takes the solver as it always did


def test_bn_train_entry_points_validate_before_any_launch():
    lib = _hip.load()
    wsb = lib.deqsci_bn_train_workspace_bytes
    assert wsb(-1) == 0 and wsb(0) == 0 and wsb(1) == 0 and wsb(1 << 31) == 0
    assert wsb(2) == wsb(128) == 128 * 8 and wsb(129) == 2 * 128 * 8 and wsb(128 * 1024) == 1024 * 128 * 8
    assert wsb(128 * 1024 + 1) == 911 * 128 * 8 and wsb(64 * 256 * 256) < 1024 * 128 * 8 + 1       # bounded: it does not grow with the batch
    far = 1 << 40                                                                # addresses only: validation dereferences nothing
    t1, t2, t3, t4 = (lib.deqsci_bn_train_stats_f32, lib.deqsci_bn_train_apply_f32, lib.deqsci_bn_train_grad_stats_f32,
                      lib.deqsci_bn_train_grad_apply_f32)
    c, gy, y, rec, grec, rm, rv, nbt, ga, be, dg, db, mask, ws = (far + (i << 28) for i in range(14))
    P = 105
    # NULL -> -1 (T1's three buffers: all or none; T2's mask may be NULL)
    assert t1(None, rec, rm, rv, nbt, 0.1, P, ws, None) == -1 and t1(c, None, rm, rv, nbt, 0.1, P, ws, None) == -1
    assert t1(c, rec, rm, rv, nbt, 0.1, P, None, None) == -1
    assert t1(c, rec, None, rv, nbt, 0.1, P, ws, None) == -1 and t1(c, rec, rm, None, nbt, 0.1, P, ws, None) == -1
    assert t1(c, rec, rm, rv, None, 0.1, P, ws, None) == -1 and t1(c, rec, rm, None, None, 0.1, P, ws, None) == -1
    for i in range(5):
        args = [c, rec, ga, be, 1e-5, y]
        args[i if i < 4 else 5] = None
        assert t2(*args, mask, 1, P, None) == -1, i
    for i in (0, 1, 2, 4, 5, 6):
        args = [gy, c, rec, 1e-5, grec, dg, db]
        args[i] = None
        assert t3(*args, P, ws, None) == -1, i
    assert t3(gy, c, rec, 1e-5, grec, dg, db, P, None, None) == -1
    for i in (0, 1, 2, 3, 4, 6):
        args = [gy, c, rec, grec, ga, 1e-5, y]
        args[i] = None
        assert t4(*args, P, None) == -1, i
    # sizes -> -2: a negative count, one value per channel, more than the index range; P = 0 launches nothing
    for bad in (-1, 1, 1 << 31):
        assert t1(c, rec, rm, rv, nbt, 0.1, bad, ws, None) == -2 and t2(c, rec, ga, be, 1e-5, y, mask, 1, bad, None) == -2
        assert t3(gy, c, rec, 1e-5, grec, dg, db, bad, ws, None) == -2 and t4(gy, c, rec, grec, ga, 1e-5, y, bad, None) == -2
    assert t1(c, rec, rm, rv, nbt, 0.1, 0, ws, None) == 0 and t2(c, rec, ga, be, 1e-5, y, mask, 1, 0, None) == 0
    assert t3(gy, c, rec, 1e-5, grec, dg, db, 0, ws, None) == 0 and t4(gy, c, rec, grec, ga, 1e-5, y, 0, None) == 0
    # alignment -> -3
    assert t1(c + 4, rec, rm, rv, nbt, 0.1, P, ws, None) == -3 and t1(c, rec + 4, rm, rv, nbt, 0.1, P, ws, None) == -3
    assert t1(c, rec, rm + 2, rv, nbt, 0.1, P, ws, None) == -3 and t1(c, rec, rm, rv + 1, nbt, 0.1, P, ws, None) == -3
    assert t1(c, rec, rm, rv, nbt + 4, 0.1, P, ws, None) == -3 and t1(c, rec, rm, rv, nbt, 0.1, P, ws + 4, None) == -3
    assert t2(c + 8, rec, ga, be, 1e-5, y, mask, 1, P, None) == -3 and t2(c, rec, ga, be, 1e-5, y + 4, mask, 1, P, None) == -3
    assert t2(c, rec + 2, ga, be, 1e-5, y, mask, 1, P, None) == -3 and t2(c, rec, ga + 1, be, 1e-5, y, mask, 1, P, None) == -3
    assert t2(c, rec, ga, be + 2, 1e-5, y, mask, 1, P, None) == -3 and t2(c, rec, ga, be, 1e-5, y, mask + 4, 1, P, None) == -3
    assert t3(gy + 4, c, rec, 1e-5, grec, dg, db, P, ws, None) == -3 and t3(gy, c + 12, rec, 1e-5, grec, dg, db, P, ws, None) == -3
    assert t3(gy, c, rec, 1e-5, grec + 4, dg, db, P, ws, None) == -3 and t3(gy, c, rec, 1e-5, grec, dg + 2, db, P, ws, None) == -3
    assert t3(gy, c, rec, 1e-5, grec, dg, db + 1, P, ws, None) == -3 and t3(gy, c, rec, 1e-5, grec, dg, db, P, ws + 4, None) == -3
    assert t4(gy + 4, c, rec, grec, ga, 1e-5, y, P, None) == -3 and t4(gy, c, rec, grec, ga, 1e-5, y + 8, P, None) == -3
    assert t4(gy, c, rec, grec + 4, ga, 1e-5, y, P, None) == -3 and t4(gy, c, rec, grec, ga + 2, 1e-5, y, P, None) == -3
    # overlap / unsupported -> -4; y == c and dc == gy are the two aliases that are served
    assert t1(c, c + 64, rm, rv, nbt, 0.1, P, ws, None) == -4 and t1(c, rec, rm, rm + 32, nbt, 0.1, P, ws, None) == -4
    assert t1(c, rec, rm, rv, nbt, 0.1, P, c, None) == -4 and t1(c, rec, rm, rv, rec + 8, 0.1, P, ws, None) == -4
    assert t2(c, rec, ga, be, 1e-5, c + 256, mask, 1, P, None) == -4 and t2(c, rec, ga, be, 1e-5, y, c + 8, 1, P, None) == -4
    assert t2(c, rec, ga, be, 1e-5, y, y + 64, 1, P, None) == -4 and t2(c, rec, ga, be, 1e-5, ga - 64, None, 1, P, None) == -4
    assert t2(c, rec, ga, be, 1e-5, y, mask, 2, P, None) == -4 and t2(c, rec, ga, be, 1e-5, y, mask, -1, P, None) == -4
    assert t3(gy, c, rec, 1e-5, rec, dg, db, P, ws, None) == -4 and t3(gy, c, rec, 1e-5, grec, dg, dg + 32, P, ws, None) == -4
    assert t3(gy, c, rec, 1e-5, grec, dg, db, P, gy, None) == -4 and t3(gy, c, rec, 1e-5, grec, c + 64, db, P, ws, None) == -4
    assert t4(gy, c, rec, grec, ga, 1e-5, c, P, None) == -4 and t4(gy, c, rec, grec, ga, 1e-5, gy + 256, P, None) == -4
    assert t4(gy, c, rec, grec, ga, 1e-5, ga - 64, P, None) == -4


def test_bn_train_kernels_compile_without_spills(tmp_path):
    """Streaming kernels with a handful of float64 accumulators per lane: none may spill or keep a per-lane stack, and the two reducing
    kernels hold one 8 KiB fold buffer in LDS.  (Cross-compiles without a GPU, a few seconds.)"""
    import re
    import subprocess
    from conftest import ROOT
    src = os.path.join(ROOT, "deqsci_amd", "csrc", "bn_train.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deqsci_amd", "csrc"), "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    found = re.findall(r"Function Name: (\S*bn_train\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+)"
                       r".*?VGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", out.stderr, flags=re.S)
    assert len(found) == 11, out.stderr[-2000:]      # stats<0/1>, mean, var, apply<relu, mask> x 4, grad_stats, grad_sum, grad_apply
    for name, vgprs, stack, sspill, vspill, lds in found:
        assert int(vgprs) <= 128 and (int(stack), int(sspill), int(vspill)) == (0, 0, 0), (name, vgprs, stack, sspill, vspill)
        assert int(lds) <= 8 << 10, (name, lds)
