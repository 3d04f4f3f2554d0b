"""GPU: BatchNorm2d in train mode on the HIP kernels (csrc/bn_train.hip).  T1 .. T4 one by one against the float64 restatements of
tests/bn_train_ref.py, within bounds counted from the order of operations include/deqsci_hip.h states (statistics: P 2^-52 relative to
mean |c| and to the variance ITSELF, on c = 1000 + 1e-2 randn too, where a one-pass E[c^2] - mean^2 is four orders of magnitude off);
NaN, sentinels, aliasing, determinism.  Then the paths: DenoiserParamGrads(train_bn=True) on one f-call of the seeded conv + BN + ReLU DnCNN
against the reference (tests/golden/bn_train.npz, case b.) and the float64 host statement under the device's own masks;
DEQFixedPoint(parameter_backward="device+bn-train", engine_options={"train_bn": "device"}) on a training step of FFDNet in train mode
against the reference's (case a.); the engine's no-tape path; and what stays as it was.

The shapes (bn_train_ref.SHAPES, BIG) are stated from the kernels' own chunk size there."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
import bn_train_ref as ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint, vjp
    from deqsci_amd import autograd as ag
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.networks import DnCNN

DEV = "cuda"
PAD, SENTINEL = 64, 12345.0                 # elements in front of and behind every output, and what they hold
KERNEL_CASES = [(s, c) for s in ref.SHAPES for c in ref.CASES] + [(ref.BIG, "signed"), (ref.BIG, "offset")]
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v       # noqa: E731


def _act(a, shape):
    """(P, 64) numpy -> the channels_last (n,64,H,W) GPU activation the kernels read."""
    n, H, W = shape
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV).view(n, H, W, 64).permute(0, 3, 1, 2)


def _flat(t):
    """channels_last (n,64,H,W) -> (P, 64) float64 numpy."""
    return t.permute(0, 2, 3, 1).reshape(-1, 64).double().cpu().numpy()


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


class Guarded:
    """An output in the middle of a larger buffer of sentinels: .t is what the kernel writes, .intact() whether it wrote nothing else."""

    def __init__(self, numel, dtype, like=None):
        self.buf = torch.full((numel + 2 * PAD,), SENTINEL if dtype.is_floating_point else 12345, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + numel]
        if like is not None:
            self.t.copy_(like.reshape(-1))

    def act(self, shape):
        n, H, W = shape
        return self.t.view(n, H, W, 64).permute(0, 3, 1, 2)

    def intact(self):
        want = SENTINEL if self.buf.dtype.is_floating_point else 12345
        return bool((self.buf[:PAD] == want).all()) and bool((self.buf[-PAD:] == want).all())


def _record(shape, case):
    """T1's reference record as the float64 device vector T2 .. T4 read."""
    mean, var, _ = ref.stats(shape, case)
    return np.concatenate([np.asarray(mean, np.float64), np.asarray(var, np.float64)])


def test_library_limits_are_the_ones_the_shapes_were_stated_from():
    lib = _hip.load()
    assert (_hip.BN_TRAIN_CHUNK, _hip.BN_TRAIN_MAX_WG) == (ref.CHUNK, ref.MAX_WG)
    for shape in ref.SHAPES + (ref.BIG,):
        P = shape[0] * shape[1] * shape[2]
        assert lib.deqsci_bn_train_workspace_bytes(P) == ref.split(P)[1] * 128 * 8


# ----------------------------------------------------------------------------- T1
@pytest.mark.parametrize("shape,case", KERNEL_CASES, ids=_id)
def test_t1_statistics_and_buffers_against_float64(shape, case):
    c, _, _, _, rm, rv = ref.data(shape, case)
    P = c.shape[0]
    mean, var, mean_abs = ref.stats(shape, case)
    x = _act(c, shape)
    rec, g_rm, g_rv, nbt = Guarded(128, torch.float64), Guarded(64, torch.float32, _dev(rm)), Guarded(64, torch.float32, _dev(rv)), Guarded(1, torch.int64)
    nbt.t.fill_(41)
    ws = _hip.bn_train_workspace(P, DEV)
    ws.fill_(float("nan"))                                      # the workspace needs no initialisation
    _hip.bn_train_stats(x, g_rm.t, g_rv.t, nbt.t, ref.MOMENTUM, record=rec.t, workspace=ws)
    got = rec.t.cpu().numpy()
    b_mean, b_var = ref.stats_bounds(P, var, mean_abs)
    e_mean, e_var = np.abs(got[:64] - mean), np.abs(got[64:] - var)
    print(f"T1 {shape} {case}: mean err / bound {float(np.max(e_mean / np.maximum(b_mean, 1e-300))):.3f}, var err / bound "
          f"{float(np.max(e_var / np.maximum(b_var, 1e-300))):.3f}, var range {float(var.min()):.3e} .. {float(var.max()):.3e}")
    assert np.all(e_mean <= b_mean) and np.all(e_var <= b_var)
    if case == "constant":
        assert got[64 + 7] == 0.0 and got[7] == 0.75 and got[9] == 0.0 and got[64 + 9] == 0.0
    want_rm, want_rv = ref.running(rm, rv, mean, var, P)
    assert np.all(np.abs(g_rm.t.double().cpu().numpy() - want_rm) <= ref.one_rounding(want_rm))
    assert np.all(np.abs(g_rv.t.double().cpu().numpy() - want_rv) <= ref.one_rounding(want_rv))
    assert int(nbt.t) == 42
    assert rec.intact() and g_rm.intact() and g_rv.intact() and nbt.intact() and torch.equal(x, _act(c, shape))
    # no buffers: the same record, nothing else; and twice the same bits
    rec2 = _hip.bn_train_stats(x, workspace=ws)
    assert torch.equal(rec2, rec.t)


def test_t1_one_pass_variance_would_miss_the_offset_bound():
    """The bound is not one a one-pass E[c^2] - mean^2 in float64 meets: the reason T1 centres."""
    shape = ref.SHAPES[-1]
    c = ref.data(shape, "offset")[0].astype(np.float64)
    _, var, mean_abs = ref.stats(shape, "offset")
    one_pass = (c * c).mean(0) - c.mean(0) ** 2
    assert np.max(np.abs(one_pass - var) / ref.stats_bounds(c.shape[0], var, mean_abs)[1]) > 10.0


# ----------------------------------------------------------------------------- T2
@pytest.mark.parametrize("shape,case", KERNEL_CASES, ids=_id)
@pytest.mark.parametrize("relu", (True, False), ids=("relu", "linear"))
def test_t2_apply_and_mask_against_float64(shape, case, relu):
    c, _, gamma, beta, _, _ = ref.data(shape, case)
    P = c.shape[0]
    record = _record(shape, case)
    want, bound = ref.apply(c, record, gamma, beta, relu=relu)
    x, rec, g, b = _act(c, shape), _dev(record), _dev(gamma), _dev(beta)
    y, mask = Guarded(P * 64, torch.float32), Guarded(P, torch.int64)
    _hip.bn_train_apply(x, rec, g, b, ref.EPS, relu=relu, out=y.act(shape), mask=mask.t.view(shape))
    got = _flat(y.act(shape))
    print(f"T2 {shape} {case} relu={relu}: worst err / bound {float(np.max(np.abs(got - want) / bound)):.3f}")
    assert np.all(np.abs(got - want) <= bound)
    assert y.intact() and mask.intact() and torch.equal(x, _act(c, shape))
    # the mask is V0's of the kernel's own output, in the same pass
    assert torch.equal(mask.t.view(shape), _hip.relu_mask_pack(y.act(shape).contiguous(memory_format=torch.channels_last)))
    assert np.array_equal(mask.t.cpu().numpy(), ref.mask_words(y.t.view(P, 64).cpu().numpy()))
    assert got[:, 3].min() == got[:, 3].max() == (max(float(beta[3]), 0.0) if relu else float(beta[3]))       # gamma = 0: beta alone
    # without the mask, and in place: the same bits
    plain = _hip.bn_train_apply(x, rec, g, b, ref.EPS, relu=relu)
    assert torch.equal(plain, y.act(shape))
    inplace = x.clone(memory_format=torch.channels_last)
    assert _hip.bn_train_apply(inplace, rec, g, b, ref.EPS, relu=relu, out=inplace) is inplace and torch.equal(inplace, plain)


# ----------------------------------------------------------------------------- T3, T4
@pytest.mark.parametrize("shape,case", KERNEL_CASES, ids=_id)
def test_t3_gradient_sums_against_float64(shape, case):
    c, gy, _, _, _, _ = ref.data(shape, case)
    P = c.shape[0]
    record = _record(shape, case)
    dbeta, dgamma, b_beta, b_gamma = ref.grad_stats(gy, c, record)
    out = Guarded(64, torch.float32), Guarded(64, torch.float32), Guarded(128, torch.float64)
    ws = _hip.bn_train_workspace(P, DEV)
    ws.fill_(float("nan"))
    g, x = _act(gy, shape), _act(c, shape)
    _hip.bn_train_grad_stats(g, x, _dev(record), ref.EPS, workspace=ws, out=tuple(o.t for o in out))
    grec = out[2].t.cpu().numpy()
    print(f"T3 {shape} {case}: dbeta err / bound {float(np.max(np.abs(grec[:64] - dbeta) / np.maximum(b_beta, 1e-300))):.3f}, dgamma "
          f"{float(np.max(np.abs(grec[64:] - dgamma) / np.maximum(b_gamma, 1e-300))):.3f}")
    assert np.all(np.abs(grec[:64] - dbeta) <= b_beta) and np.all(np.abs(grec[64:] - dgamma) <= b_gamma)
    # the fp32 outputs: the float64 sums rounded once
    assert np.all(np.abs(out[1].t.double().cpu().numpy() - grec[:64]) <= ref.V * np.abs(grec[:64]) + ref.TINY)
    assert np.all(np.abs(out[0].t.double().cpu().numpy() - grec[64:]) <= ref.V * np.abs(grec[64:]) + ref.TINY)
    assert all(o.intact() for o in out) and torch.equal(g, _act(gy, shape)) and torch.equal(x, _act(c, shape))
    again = _hip.bn_train_grad_stats(g, x, _dev(record), ref.EPS)
    assert all(torch.equal(a, o.t) for a, o in zip(again, out))


@pytest.mark.parametrize("shape,case", KERNEL_CASES, ids=_id)
def test_t4_gradient_behind_the_convolution_against_float64(shape, case):
    c, gy, gamma, _, _, _ = ref.data(shape, case)
    P = c.shape[0]
    record = _record(shape, case)
    dbeta, dgamma, _, _ = ref.grad_stats(gy, c, record)
    grec = np.concatenate([dbeta, dgamma])
    want, bound = ref.grad_apply(gy, c, record, grec, gamma)
    g, x = _act(gy, shape), _act(c, shape)
    dc = Guarded(P * 64, torch.float32)
    _hip.bn_train_grad_apply(g, x, _dev(record), _dev(grec), _dev(gamma), ref.EPS, out=dc.act(shape))
    got = _flat(dc.act(shape))
    print(f"T4 {shape} {case}: worst err / bound {float(np.max(np.abs(got - want) / bound)):.3f}")
    assert np.all(np.abs(got - want) <= bound)
    assert dc.intact() and torch.equal(g, _act(gy, shape)) and torch.equal(x, _act(c, shape))
    assert not got[:, 3].any()                                    # gamma = 0: nothing goes down
    # a pixel the ReLU masked (gy = 0) still receives the statistic terms
    masked = (gy == 0) & (np.abs(want) > 0)
    assert masked.any() and np.all(got[masked] != 0)
    fresh = _hip.bn_train_grad_apply(g, x, _dev(record), _dev(grec), _dev(gamma), ref.EPS)
    inplace = g.clone(memory_format=torch.channels_last)
    assert _hip.bn_train_grad_apply(inplace, x, _dev(record), _dev(grec), _dev(gamma), ref.EPS, out=inplace) is inplace
    assert torch.equal(fresh, dc.act(shape)) and torch.equal(inplace, fresh)


@pytest.mark.parametrize("shape", ref.SHAPES[1:], ids=_id)
def test_a_nan_stays_in_its_channel(shape):
    """One NaN in one pixel of channel 5 (of c, then of gy): that channel's statistics, buffers and outputs are NaN, the other 63 finite."""
    c, gy, gamma, beta, rm, rv = ref.data(shape, "signed")
    P = c.shape[0]
    cn, gn = c.copy(), gy.copy()
    cn[P // 2, 5] = np.nan
    gn[P // 3, 5] = np.nan
    others = torch.arange(64) != 5
    x = _act(cn, shape)
    d_rm, d_rv, nbt = _dev(rm), _dev(rv), torch.zeros((), dtype=torch.int64, device=DEV)
    rec = _hip.bn_train_stats(x, d_rm, d_rv, nbt, ref.MOMENTUM)
    for t in (rec[:64], rec[64:], d_rm, d_rv):
        assert bool(torch.isnan(t[5])) and bool(torch.isfinite(t.cpu()[others]).all())
    y, mask = _hip.bn_train_apply(x, rec, _dev(gamma), _dev(beta), ref.EPS, relu=True, want_mask=True)
    yf = _flat(y)
    assert np.isnan(yf[:, 5]).all() and np.isfinite(yf[:, others.numpy()]).all()
    assert not bool(((mask >> 5) & 1).any())                      # NaN > 0 is false: V0's rule
    # a NaN in the gradient, clean statistics
    clean = _dev(_record(shape, "signed"))
    dgamma, dbeta, grec = _hip.bn_train_grad_stats(_act(gn, shape), _act(c, shape), clean, ref.EPS)
    for t in (dgamma, dbeta, grec[:64], grec[64:]):
        assert bool(torch.isnan(t[5])) and bool(torch.isfinite(t.cpu()[others]).all())
    dc = _flat(_hip.bn_train_grad_apply(_act(gn, shape), _act(c, shape), clean, grec, _dev(gamma), ref.EPS))
    assert np.isnan(dc[:, 5]).all() and np.isfinite(dc[:, others.numpy()]).all()


def test_wrappers_and_library_refuse_what_the_kernels_do_not_cover():
    lib, stream = _hip.load(), torch.cuda.current_stream().cuda_stream
    one = torch.zeros(1, 64, 1, 1, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_hip.DeqsciHipError, match="more than 1 value per channel"):
        _hip.bn_train_stats(one)
    x = _act(ref.data(ref.SHAPES[1], "signed")[0], ref.SHAPES[1])
    rec, ws = torch.zeros(128, dtype=torch.float64, device=DEV), _hip.bn_train_workspace(105, DEV)
    f64 = torch.zeros(64, device=DEV)
    with pytest.raises(_hip.DeqsciHipError, match="all three or none"):
        _hip.bn_train_stats(x, f64, None, None)
    assert lib.deqsci_bn_train_stats_f32(x.data_ptr(), rec.data_ptr(), None, None, None, 0.1, 1, ws.data_ptr(), stream) == -2
    assert lib.deqsci_bn_train_stats_f32(x.data_ptr(), rec.data_ptr(), None, None, None, 0.1, 0, ws.data_ptr(), stream) == 0       # launches nothing
    assert lib.deqsci_bn_train_stats_f32(x.data_ptr(), rec.data_ptr(), f64.data_ptr(), None, None, 0.1, 105, ws.data_ptr(), stream) == -1
    assert lib.deqsci_bn_train_stats_f32(x.data_ptr() + 4, rec.data_ptr(), None, None, None, 0.1, 16, ws.data_ptr(), stream) == -3
    assert lib.deqsci_bn_train_stats_f32(x.data_ptr(), x.data_ptr(), None, None, None, 0.1, 105, ws.data_ptr(), stream) == -4
    y = torch.empty_like(x)
    assert lib.deqsci_bn_train_apply_f32(x.data_ptr(), rec.data_ptr(), f64.data_ptr(), f64.data_ptr(), 1e-5, x.data_ptr() + 256, None, 1, 100, stream) == -4
    assert lib.deqsci_bn_train_apply_f32(x.data_ptr(), rec.data_ptr(), f64.data_ptr(), f64.data_ptr(), 1e-5, y.data_ptr(), None, 2, 105, stream) == -4
    torch.cuda.synchronize()
    assert not bool(rec.any()) and not bool(f64.any())           # nothing ran


# ----------------------------------------------------------------------------- DenoiserParamGrads(train_bn=True): one f-call of the reference
import test_bn_train_host as host            # noqa: E402  (the golden's loader and case b.'s net)


@pytest.fixture(scope="module")
def golden():
    return host.load_golden()


def _G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bn_layers(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def test_param_grads_train_bn_on_the_references_fcall(golden):
    """Case b.: noise, every gradient, the input product and the buffers against the reference's own train-mode f-call at the project's
    parity bar 1e-4 (one f-call: no DEQ amplification), and within 1e-5 of the float64 host statement under the device's own masks."""
    g = golden
    net = host.golden_b_net(g).to(DEV)
    x, v = _G(g["b.x"]), _G(g["b.v"])
    with pytest.raises(ValueError, match="BatchNorm2d"):
        vjp.DenoiserParamGrads(net, x)                                                   # not without the keyword
    with pytest.raises(ValueError, match="train mode"):
        vjp.DenoiserParamGrads(net, x, frozen_bn=True)
    assert all(int(m.num_batches_tracked) == 0 for m in _bn_layers(net))                 # a refusal moves nothing
    before = copy.deepcopy(net)
    pg = vjp.DenoiserParamGrads(net, x, train_bn=True)
    assert pg.shape == tuple(x.shape) and len(pg.masks) == 4 and not pg.ffdnet
    worst = {"noise": rel_l2(pg.noise.cpu().numpy(), g["b.noise"])}
    for name, b in net.named_buffers():                                                 # moved in place, exactly once
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g["b.buffer." + name]) == 1
        else:
            worst["buffer." + name] = rel_l2(b.cpu().numpy(), g["b.buffer." + name])
    got = pg.grads(v)
    params = vjp.grad_parameters(net, train_bn=True)
    names = [name for name, _ in net.named_parameters()]
    assert len(got) == len(params) == 11 and all(a.shape == p.shape and a.dtype == torch.float32 for a, p in zip(got, params))
    for name, a in zip(names, got):
        worst["grad." + name] = rel_l2(a.cpu().numpy(), g["b.grad." + name])
    gx = pg.vjp(v)
    worst["grad_input"] = rel_l2(gx.cpu().numpy(), g["b.grad_input"])
    print("vs the reference:", {k: f"{e:.2e}" for k, e in worst.items()})
    assert max(worst.values()) <= 1e-4, worst
    assert all(int(m.num_batches_tracked) == 1 for m in _bn_layers(net))                 # the walks back move nothing
    # the float64 host statement under the device's own ReLU decisions
    masks = [vjp.unpack_masks(m) for m in pg.masks]
    want, _, wx = vjp.plan_param_grads_train_bn(copy.deepcopy(before).double(), x.double(), v.double(), masks=masks, input_grad=True)
    host_err = {name: float((a.double() - b).norm() / b.norm()) for name, a, b in zip(names + ["input"], got + [gx], want + [wx])}
    print("vs float64 under the device's masks:", {k: f"{e:.2e}" for k, e in host_err.items()})
    assert max(host_err.values()) <= 1e-5, host_err
    assert float(got[2].abs()[3]) > 0                                                    # the gamma = 0 unit has a gradient of its own
    # a subset stops the walk early and leaves the others None; the same call again is bit-equal; release frees the activations
    need = [False] * 11
    need[8] = True                                                                       # the last BatchNorm's gamma alone
    part = pg.grads(v, need=need)
    assert all(t is None for j, t in enumerate(part) if j != 8) and torch.equal(part[8], got[8])
    assert all(torch.equal(a, b) for a, b in zip(pg.grads(v), got)) and torch.equal(pg.vjp(v), gx)
    pg.release()
    with pytest.raises(RuntimeError, match="released"):
        pg.grads(v)


@pytest.mark.parametrize("kind", ["ffdnet", "dncnn_bn5"])
def test_denoiser_noise_train_bn_routes_gradients_and_frees(kind):
    net = (host.seeded_ffdnet(4) if kind == "ffdnet" else host.seeded_bn_dncnn(5, 6)).to(DEV).train()
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(2, 1, 12, 10, device=DEV, generator=gen, requires_grad=True)
    v = torch.randn(2, 1, 12, 10, device=DEV, generator=gen)
    sigma = torch.full((2,), 0.1, device=DEV) if kind == "ffdnet" else None
    params = vjp.grad_parameters(net, train_bn=True)
    params[1].requires_grad_(False)
    asked = [p for p in params if p.requires_grad]
    noise = ag.denoiser_noise(net, x, sigma, train_bn=True)
    assert all(int(m.num_batches_tracked) == 1 for m in _bn_layers(net))
    pg = vjp.DenoiserParamGrads(net, x, sigma, train_bn=True)                            # (batch statistics do not read the buffers it moves)
    assert torch.equal(noise, pg.noise) and all(int(m.num_batches_tracked) == 2 for m in _bn_layers(net))
    got = torch.autograd.grad(noise, [x] + asked, v, retain_graph=True, allow_unused=True)
    want = [t for t, p in zip(pg.grads(v), params) if p.requires_grad]
    assert len(got) == 1 + len(want) and all(torch.equal(a, b) for a, b in zip(got[1:], want))
    if kind == "ffdnet":
        assert got[0] is None and not bool(pg.vjp(v).any())                              # networks/ffdnet.py detaches its input
        m64 = copy.deepcopy(net).double().requires_grad_(True)
        auto = torch.autograd.grad(m64(x.detach().double(), sigma.double()), vjp.grad_parameters(m64, train_bn=True), v.double())
        for i, (a, b) in enumerate(zip(pg.grads(v), auto)):
            assert float((a.double() - b).norm() / b.norm()) < 1e-4, i                   # (ReLU decisions at fp32 and float64 activations can differ)
    else:
        assert torch.equal(got[0], pg.vjp(v))
    with pytest.raises(RuntimeError, match="freed"):
        torch.autograd.grad(noise, [asked[0]], v)


# ----------------------------------------------------------------------------- a training step of FFDNet in train mode (golden case a.)
def _problem(g):
    Phi, y, Ps, gt = _G(g["a.Phi"]), _G(g["a.y"]), _G(g["a.Phi_sum"]), _G(g["a.gt"])
    return Phi, y, Ps, gt, deqsci_amd.initial_point(y, Phi, Ps, gt)


def _training_step(g, engine, parameter):
    solver, _ = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), int(g["a.iters"]))
    solver.nonlinear_op.train()
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(g["a.iters"]), tol=1e-9)
    deq.parameter_backward = parameter
    if engine:
        deq.engine_options = {"train_bn": "device"}
    calls = []
    hook = solver.nonlinear_op.register_forward_hook(lambda *a: calls.append(torch.is_grad_enabled()))
    Phi, y, Ps, gt, x0 = _problem(g)
    rec = deq(y, Phi, Ps, initial_point=x0)
    hook.remove()
    loss = torch.nn.functional.mse_loss(rec, gt)
    solver.zero_grad()
    loss.backward()
    return solver, deq, rec, loss, len(calls)


@pytest.mark.parametrize("engine,parameter,module_calls", [(True, "device+bn-train", 1), (True, "autograd", 2), (False, "device+bn-train", 13)],
                         ids=("both", "engine-option-alone", "backward-value-alone"))
def test_training_step_in_train_mode_vs_reference_golden(golden, engine, parameter, module_calls):
    """rec, loss, the 41 gradients and the 39 buffers within 1e-4 - the project's bar, 10 x over the stored conditioning bound of 1e-5, a
    margin for the fp32 convolutions' 1e-7 .. 1e-6 per layer; num_batches_tracked and sigma exact.  The torch module runs only what the
    options leave it: the closing f0 = f(z0), and the taped call or the 12 calls of the solve where that side stays on it."""
    g = golden
    assert max(float(v) for k, v in g.items() if k.startswith("a.conditioning.")) < 1e-5
    solver, deq, rec, loss, calls = _training_step(g, engine, parameter)
    assert calls == module_calls
    if parameter == "autograd":
        assert deq.last_parameter_path == "autograd"
    else:
        assert deq.last_parameter_path == "device" and deq.parameter_fallback_reason is None
    assert deq.last_backward_path == "autograd"
    if engine:
        info = deq._engine[1].last_info
        assert info["denoiser_path"] == "train bn per layer" and info["train_bn"] == "device" and info["train_bn_reason"] is None
        assert info["f_calls"] == int(g["a.iters"]) and not info["graph"]                # the solve alone: the taped call is the caller's
    else:
        assert deq._engine is None
    worst = {"rec": rel_l2(rec.detach().cpu().numpy(), g["a.rec"])}
    assert abs(float(loss.detach()) - float(g["a.loss"])) <= 1e-4 * float(g["a.loss"])
    net = solver.nonlinear_op
    names = [name for name, _ in net.named_parameters()]
    assert ["a.grad." + name for name in names] == [k for k in g if k.startswith("a.grad.")] and len(names) == 41
    for name, p in net.named_parameters():
        worst["grad." + name] = rel_l2(p.grad.cpu().numpy(), g["a.grad." + name])
    n_buf = 0
    for name, b in net.named_buffers():
        n_buf += 1
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g["a.buffer." + name]) == 14, name
        else:
            worst["buffer." + name] = rel_l2(b.cpu().numpy(), g["a.buffer." + name])
    assert n_buf == 39
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"engine={engine} parameter={parameter}: worst rel L2 vs the reference", [(k, f"{e:.2e}") for k, e in top],
          f"| forward res {deq.forward_res:.4e} (reference {float(g['a.forward_res']):.4e}), backward res {deq.backward_res:.4e} "
          f"({float(g['a.backward_res']):.4e})")
    assert max(worst.values()) <= 1e-4, top
    assert np.array_equal(solver.noise_sigma.cpu().numpy(), g["a.sigma_after"])


def _reconstruct(g, options, train=True):
    solver, _ = build_pipeline("ffdnet", checkpoint.shipped("ffdnet_gray"), int(g["a.iters"]))
    solver.nonlinear_op.train(train)
    deq = deqsci_amd.DEQFixedPoint(solver, deqsci_amd.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=int(g["a.iters"]), tol=1e-9)
    deq.engine_options = dict(options)
    Phi, y, Ps, _, x0 = _problem(g)
    with torch.no_grad():
        rec = deq(y, Phi, Ps, initial_point=x0, train_flag=False)
    return solver.nonlinear_op, deq._engine[1], rec


def test_no_tape_reconstruction_in_train_mode_makes_every_f_call(golden):
    """Every f-call moves the buffers, the reference's closing f0 = f(z) too: max_iter + 2 calls on the device path, as the module path
    makes them with extra_call=True - and the two agree within 1e-4 at 12 iterations."""
    iters = int(golden["a.iters"])
    net_d, eng_d, rec_d = _reconstruct(golden, {"train_bn": "device"})
    assert eng_d.last_info["denoiser_path"] == "train bn per layer" and eng_d.last_info["f_calls"] == iters + 2 and not eng_d.last_info["graph"]
    net_m, eng_m, rec_m = _reconstruct(golden, {"extra_call": True})
    assert eng_m.den.train is None and "train_bn" not in eng_m.last_info and eng_m.last_info["f_calls"] == iters + 2
    worst = {"rec": rel_l2(rec_d.cpu().numpy(), rec_m.cpu().numpy())}
    for (name, a), (_, b) in zip(net_d.named_buffers(), net_m.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(a) == int(b) == iters + 2, name
        else:
            worst[name] = rel_l2(a.cpu().numpy(), b.cpu().numpy())
    print("device path vs module path:", sorted(((k, f"{e:.2e}") for k, e in worst.items()), key=lambda kv: kv[1])[-3:])
    assert max(worst.values()) <= 1e-4, worst
    with pytest.raises(ValueError, match="use_graph=True"):
        _reconstruct(golden, {"train_bn": "device", "use_graph": True})


def test_defaults_and_unserved_nets_stay_where_they_were(golden):
    iters = int(golden["a.iters"])
    # train_bn="module" is the default, bit for bit: the module runs, the dead closing call stays skipped
    net_a, eng_a, rec_a = _reconstruct(golden, {})
    net_b, eng_b, rec_b = _reconstruct(golden, {"train_bn": "module"})
    assert torch.equal(rec_a, rec_b) and eng_b.den.train is None and "train_bn" not in eng_b.last_info
    assert all(int(m.num_batches_tracked) == iters + 1 for m in _bn_layers(net_a) + _bn_layers(net_b))
    assert eng_b.den._route(8, 24, 20, DEV, "fast", False) == "module"
    # a net the option does not serve keeps its path, and last_info says why: eval mode is the folded kernels' business
    _, eng_c, rec_c = _reconstruct(golden, {"train_bn": "device"}, train=False)
    _, eng_d, rec_d = _reconstruct(golden, {}, train=False)
    assert torch.equal(rec_c, rec_d) and eng_c.last_info["train_bn"] == "module" and "not in train mode" in eng_c.last_info["train_bn_reason"]
    assert eng_c.last_info["denoiser_path"] == eng_d.last_info["denoiser_path"] != "train bn per layer"
    # "device+bn" refuses a train-mode BatchNorm as it did, and an unknown value names the new one
    solver, deq, _, _, calls = _training_step(golden, False, "device+bn")
    assert deq.last_parameter_path == "autograd" and "train mode" in deq.parameter_fallback_reason and calls == iters + 2
    deq.parameter_backward = "device-bn-train"
    with pytest.raises(ValueError, match=r"'device\+bn-train'"):
        deq._taped_call(None, None, None, None)
