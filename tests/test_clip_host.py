"""CPU: gradient clipping by global norm - the host paths of deqsci_amd.optim against tests/clip_ref.py bit for bit and against torch's
clip_grad_norm_ in float64, the skipped step, the state_dict, the refusals, the loop, the command line and the C ABI (no GPU, no launch)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import clip_ref as cr
import train_cases as tc
import train_ref as tr
from conftest import ROOT

from deqsci_amd import _hip, optim, training
from deqsci_amd.optim import DeviceAdam, clip_grad_norm_

BETAS, EPS = (0.9, 0.999), 1e-8
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193, 257 * 4096 + 3]         # the last: more chunks than a workgroup has threads (stage 2 takes a second trip)


def _grads(sizes=SIZES, seed=0, lo=-6, hi=3):
    rng = np.random.RandomState(seed)
    return [(rng.randn(n) * 10.0 ** rng.uniform(lo, hi, size=n)).astype(np.float32) for n in sizes]


def _params(grads):
    params = [torch.nn.Parameter(torch.from_numpy(np.random.RandomState(100 + i).randn(g.size).astype(np.float32))) for i, g in enumerate(grads)]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    return params


# ----------------------------------------------------------------------------- (a) the CPU paths are the restated order
@pytest.mark.parametrize("max_norm", [1.0, 1e30, 0.0])
def test_cpu_clip_grad_norm_equals_the_restated_order(max_norm):
    grads = _grads()
    want = cr.grad_stats(grads, max_norm)
    params = _params(grads)
    stats = clip_grad_norm_(params, max_norm, return_stats=True)
    assert stats.dtype == torch.float64 and np.array_equal(stats.numpy(), want), (stats.numpy()[:3], want[:3])
    assert want[2] == 0.0 and (want[1] == 1.0) == (max_norm == 1e30) and (max_norm != 0.0 or want[1] == 0.0)
    for p, g in zip(params, cr.clipped(grads, want[1])):
        assert np.array_equal(p.grad.numpy(), g)
    params = _params(grads)
    norm = clip_grad_norm_(params, max_norm)
    assert norm.dim() == 0 and norm.dtype == torch.float64 and float(norm) == want[0]
    # one tensor, not a list; no gradients at all
    assert float(clip_grad_norm_(_params(grads[3:4])[0], 1.0)) == cr.grad_stats(grads[3:4], 1.0)[0]
    assert float(clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0


def test_zero_gradients_give_coef_one():
    params = _params([np.zeros(n, np.float32) for n in (5, 4097)])
    stats = clip_grad_norm_(params, 0.5, return_stats=True).numpy()
    assert np.array_equal(stats, np.array([0.0, 1.0, 0.0, 0.0, 0.0])) and np.array_equal(stats, cr.grad_stats([np.zeros(5, np.float32), np.zeros(4097, np.float32)], 0.5))


def test_sum_of_squares_and_coef_against_torch_in_float64():
    """Any order of a float64 sum of n non-negative terms lies within n 2^-53 relative of the exact sum; coef is ONE fp32 rounding of the
    float64 quotient, so it lies within 2^-24 (+ the norm's error) of torch's coefficient on the float64 casts."""
    grads = _grads(seed=3)
    n = sum(g.size for g in grads)
    for max_norm in (1e-3, 1.0, 250.0):
        stats = cr.grad_stats(grads, max_norm)
        got = clip_grad_norm_(_params(grads), max_norm, return_stats=True).numpy()
        assert np.array_equal(got, stats)
        exact = cr.exact_sum_of_squares(grads)
        sums, _ = cr.tensor_sums(grads)
        total = 0.0
        for s in sums:
            total += s
        assert abs(total - exact) <= n * 2.0 ** -53 * exact and stats[0] == math.sqrt(total)
        for g, s, t in zip(grads, sums, stats[3:]):
            assert abs(s - cr.exact_sum_of_squares([g])) <= g.size * 2.0 ** -53 * s and t == math.sqrt(s)
        assert stats[1] == float(np.float32(min(1.0, max_norm / (stats[0] + 1e-6))))              # the fp32 rounding of the float64 value
        p64 = [torch.nn.Parameter(torch.zeros(g.size, dtype=torch.float64)) for g in grads]
        for p, g in zip(p64, grads):
            p.grad = torch.from_numpy(g.astype(np.float64))
        t_norm = float(torch.nn.utils.clip_grad_norm_(p64, max_norm))
        assert abs(stats[0] - t_norm) <= n * 2.0 ** -53 * t_norm
        t_coef = min(1.0, max_norm / (t_norm + 1e-6))
        assert abs(stats[1] - t_coef) <= (2.0 ** -24 + n * 2.0 ** -52) * t_coef
        for p, g in zip(p64, grads):                                                                # torch's clipped float64 gradients
            assert np.allclose(p.grad.numpy(), g.astype(np.float64) * stats[1], rtol=2.0 ** -23, atol=0)


def test_device_adam_cpu_path_with_clipping_is_the_restated_order():
    sizes = [5, 4097, 300]
    rng = np.random.RandomState(7)
    p0 = [rng.randn(n).astype(np.float32) for n in sizes]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    opt = DeviceAdam([{"params": params[:1]}, {"params": params[1:], "lr": 5e-4}], lr=1e-3, betas=BETAS, eps=EPS, max_grad_norm=0.75)
    host = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in p0]
    coefs = []
    for t in (1, 2, 3):
        grads = _grads(sizes, seed=20 + t, lo=-3, hi=1 if t < 3 else -5)
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        want = cr.grad_stats(grads, 0.75)                                                           # every group's gradients, one norm
        coefs.append(want[1])
        assert np.array_equal(opt.last_grad_stats.numpy(), want) and opt.grad_norm() == want[0] and opt.last_launches == 0
        for i, g in enumerate(cr.clipped(grads, want[1])):
            host[i] = tr.adam_f32_step(host[i][0], g, host[i][1], host[i][2], t, 1e-3 if i == 0 else 5e-4, BETAS, EPS)
            st = opt.state[params[i]]
            assert np.array_equal(params[i].detach().numpy(), host[i][0]) and np.array_equal(st["exp_avg"].numpy(), host[i][1])
            assert np.array_equal(st["exp_avg_sq"].numpy(), host[i][2]) and float(st["step"]) == t
            assert np.array_equal(params[i].grad.numpy(), grads[i])                                 # p.grad is not written
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0
    # a norm below max_norm: the bits of DeviceAdam without clipping
    a, b = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0], [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    oa, ob = DeviceAdam(a, lr=1e-3, max_grad_norm=1e30), DeviceAdam(b, lr=1e-3)
    for x, y, g in zip(a, b, _grads(sizes, seed=1)):
        x.grad, y.grad = torch.from_numpy(g.copy()), torch.from_numpy(g.copy())
    oa.step()
    ob.step()
    assert all(torch.equal(x, y) and torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]) for x, y in zip(a, b))
    assert ob.last_grad_stats is None and ob.grad_norm() is None and ob.max_grad_norm is None


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_one_non_finite_gradient_changes_nothing_but_step(value):
    sizes = [5, 4097, 300]
    grads = _grads(sizes, seed=2, lo=-2, hi=1)
    params = _params(grads)
    opt = DeviceAdam(params, lr=1e-3, max_grad_norm=1.0)
    opt.step()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    params[1].grad[4096] = value
    kept = [p.grad.clone() for p in params]
    opt.step()
    assert float(opt.last_grad_stats[2]) == 1.0 and not math.isfinite(opt.grad_norm())
    for p, (p0, m0, v0), g in zip(params, before, kept):
        st = opt.state[p]
        assert torch.equal(p.detach(), p0) and torch.equal(st["exp_avg"], m0) and torch.equal(st["exp_avg_sq"], v0)
        assert float(st["step"]) == 2.0                                                             # the one deviation: the host cannot know
        assert np.array_equal(p.grad.numpy(), g.numpy(), equal_nan=True)
    # clip_grad_norm_ scales nothing either, and raises on request
    stats = clip_grad_norm_(params, 1e-3, return_stats=True)
    assert float(stats[2]) == 1.0 and all(np.array_equal(p.grad.numpy(), g.numpy(), equal_nan=True) for p, g in zip(params, kept))
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(params, 1e-3, error_if_nonfinite=True)
    assert np.array_equal(stats.numpy()[1:3], cr.grad_stats([g.numpy() for g in kept], 1e-3)[1:3], equal_nan=True)
    # the next finite step goes on from the untouched state, with the bias corrections of step 3
    params[1].grad[4096] = 0.5
    want = cr.grad_stats([p.grad.numpy() for p in params], 1.0)
    new = [tr.adam_f32_step(p0.numpy(), g, m0.numpy(), v0.numpy(), 3, 1e-3, BETAS, EPS)
           for (p0, m0, v0), g in zip(before, cr.clipped([p.grad.numpy() for p in params], want[1]))]
    opt.step()
    assert all(np.array_equal(p.detach().numpy(), n[0]) for p, n in zip(params, new))


def test_state_dict_still_swaps_with_torch_adam():
    grads = _grads([64, 5], seed=5, lo=-2, hi=1)
    pa, pb = _params(grads), _params(grads)
    a, b = DeviceAdam(pa, lr=1e-3, max_grad_norm=0.5), torch.optim.Adam(pb, lr=1e-3, foreach=False)
    a.step()
    b.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and sorted(sa["param_groups"][0]) == sorted(sb["param_groups"][0]) and "max_grad_norm" not in sa["param_groups"][0]
    assert sorted(sa["state"][0]) == sorted(sb["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    a2, b2 = DeviceAdam(pa, lr=1e-3, max_grad_norm=0.5), torch.optim.Adam(pb, lr=1e-3, foreach=False)
    a2.load_state_dict(sb)
    b2.load_state_dict(sa)
    assert a2.max_grad_norm == 0.5 and torch.equal(a2.state[pa[0]]["exp_avg"], b.state[pb[0]]["exp_avg"])
    a2.step()
    b2.step()
    assert float(a2.state[pa[0]]["step"]) == 2.0 == float(b2.state[pb[0]]["step"])


def test_refusals():
    p = [torch.nn.Parameter(torch.zeros(4))]
    p[0].grad = torch.ones(4)
    for norm_type in (1.0, float("inf"), 3):
        with pytest.raises(NotImplementedError, match="norm_type"):
            clip_grad_norm_(p, 1.0, norm_type=norm_type)
    assert torch.equal(p[0].grad, torch.ones(4))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            clip_grad_norm_(p, bad)
        with pytest.raises(ValueError, match="max_norm"):
            DeviceAdam(p, lr=1e-3, max_grad_norm=bad)
    with pytest.raises(NotImplementedError, match="weight decay"):
        DeviceAdam(p, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        DeviceAdam(p, lr=1e-3, amsgrad=True, max_grad_norm=1.0)
    opt = DeviceAdam(p, lr=1e-3, max_grad_norm=1.0)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    assert opt.state[p[0]] == {} and torch.equal(p[0], torch.zeros(4))
    # parameters on more than one device
    q = torch.nn.Parameter(torch.zeros(3, device="meta"))
    q.grad = torch.zeros(3, device="meta")
    opt = DeviceAdam(p + [q], lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="2 devices"):
        opt.step()
    with pytest.raises(NotImplementedError, match="2 devices"):
        clip_grad_norm_(p + [q], 1.0)
    assert opt.state[p[0]] == {} and torch.equal(p[0].grad, torch.ones(4))
    h = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    h.grad = torch.ones(4, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="float32"):
        clip_grad_norm_([h], 1.0)
    with pytest.raises(_hip.DeqsciHipError, match="no CPU path"):
        _hip.grad_norm([torch.ones(4)], 1.0)
    with pytest.raises(_hip.DeqsciHipError, match="no CPU path"):
        _hip.grad_scale_([torch.ones(4)], torch.zeros(3, dtype=torch.float64))


# ----------------------------------------------------------------------------- (b) the loop and the command line
class _Stub(torch.nn.Module):
    """tests/test_train_host.py's stub: a solver and a DEQ module in one"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(11)
        self.nonlinear_op = torch.nn.Conv2d(tc.B, tc.B, 3, padding=1)

    def forward(self, y, Phi, Phi_sum, initial_point=None, train_flag=True):
        return initial_point + 0.1 * self.nonlinear_op(initial_point.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


def _loop(tmp_path, opt_cls, poison_at=None, **kw):
    d = tc.write(tmp_path / "data")
    ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
    loader = torch.utils.data.DataLoader(ds, batch_size=tc.BATCH, shuffle=False, drop_last=True)
    stub = _Stub()
    calls = [0]

    def hook(g):                                                                     # poisons one element of the weight's gradient of one step
        calls[0] += 1
        if calls[0] - 1 == poison_at:
            g = g.contiguous().clone()
            g.view(-1)[3] = float("nan")
        return g
    stub.nonlinear_op.weight.register_hook(hook)
    opt = opt_cls(stub.parameters(), lr=1e-3)
    model = str(tmp_path / "model") + "/"
    os.makedirs(model, exist_ok=True)
    weights = [stub.nonlinear_op.weight.detach().clone()]
    steps = training.train_solver_sci(stub, loader, opt, model, "device" if opt_cls is DeviceAdam else torch.nn.MSELoss(), 2, stub,
                                      print_every_n_steps=1, tflog_path=model, on_step=lambda s: weights.append(stub.nonlinear_op.weight.detach().clone()), **kw)
    rows = [json.loads(ln) for ln in open(model + "scalars.jsonl")]
    return stub, opt, steps, rows, weights


@pytest.mark.parametrize("opt_cls", [DeviceAdam, torch.optim.Adam], ids=["DeviceAdam", "torch.Adam"])
def test_loop_skips_a_poisoned_step_logs_it_and_goes_on(tmp_path, opt_cls, capsys):
    stub, opt, steps, rows, weights = _loop(tmp_path, opt_cls, poison_at=1, clip_grad_norm=0.05)
    assert [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1), (1, 0), (1, 1)] and steps[0]._fields == ("epoch", "step", "loss", "psnr", "lr", "nonfinite")
    assert all(math.isfinite(s.loss) for s in steps)                                 # the loss never saw it: the reference's reset rule stays quiet
    assert [r["main/skipped"] for r in rows] == [0, 1, 0, 0]
    assert all(math.isfinite(r["main/grad_norm"]) and r["main/grad_norm"] > 0 for i, r in enumerate(rows) if i != 1) and math.isnan(rows[1]["main/grad_norm"])
    assert set(rows[0]) == {"global_step", "walltime", "main/PSNR", "main/loss", "config/lr", "main/best_PSNR", "main/grad_norm", "main/skipped"}
    assert torch.equal(weights[2], weights[1]) and not torch.equal(weights[1], weights[0]) and not torch.equal(weights[3], weights[2])
    assert bool(torch.isfinite(stub.nonlinear_op.weight).all())
    st = opt.state[stub.nonlinear_op.weight]
    assert float(st["step"]) == (4.0 if opt_cls is DeviceAdam else 3.0) and bool(torch.isfinite(st["exp_avg"]).all())
    out = capsys.readouterr().out
    assert "skipped steps (gradient not finite) in epoch 0: 1" in out and "skipped steps (gradient not finite) in epoch 1: 0" in out
    assert out.count("(not finite: step skipped)") == 1 and "grad norm: %.4e" % rows[0]["main/grad_norm"] in out
    assert sorted(f for f in os.listdir(tmp_path / "model") if f.endswith(".ckpt")) == ["epoch_0.ckpt", "epoch_1.ckpt"]
    if opt_cls is DeviceAdam:
        assert opt.max_grad_norm == 0.05


@pytest.mark.parametrize("opt_cls", [DeviceAdam, torch.optim.Adam], ids=["DeviceAdam", "torch.Adam"])
def test_loop_with_a_huge_clip_is_the_loop_without(tmp_path, opt_cls):
    a = _loop(tmp_path / "a", opt_cls, clip_grad_norm=1e30)
    b = _loop(tmp_path / "b", opt_cls)
    assert [s.loss for s in a[2]] == [s.loss for s in b[2]] and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))
    assert "main/grad_norm" not in b[3][0] and all(r["main/skipped"] == 0 for r in a[3])


def test_loop_clips_the_update_as_restated(tmp_path):
    stub, opt, steps, rows, weights = _loop(tmp_path, DeviceAdam, clip_grad_norm=1e-4)
    assert float(opt.last_grad_stats[1]) < 1.0 and rows[0]["main/grad_norm"] > 1e-4


def test_cli_flag_parses():
    from deqsci_amd.cli import parser
    assert parser().parse_args([]).clip_grad_norm is None
    a = parser().parse_args(["--inference", "False", "--clip_grad_norm", "0.5"])
    assert a.clip_grad_norm == 0.5 and type(a.clip_grad_norm) is float
    helps = {x.dest: x.help for x in parser()._actions}
    assert "(this build)" in helps["clip_grad_norm"]
    with pytest.raises(SystemExit):
        parser().parse_args(["--clip_grad_norm", "tight"])
    import deqsci_amd
    assert deqsci_amd.clip_grad_norm_ is optim.clip_grad_norm_


# ----------------------------------------------------------------------------- (c) the C ABI
def test_header_binding_and_library_agree_on_the_clipping_entry_points():
    src = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(deqsci_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    for name, n in (("deqsci_grad_norm_f32", 6), ("deqsci_grad_scale_f32", 4), ("deqsci_adam_step_clipped_f32", 9)):
        params = [p for p in protos[name].split(",") if p.strip()]
        assert len(params) == len(_hip.SIGNATURES[name]) == n, name
    assert "deqsci_grad_norm_workspace_bytes" in _hip.OTHER_EXPORTS and re.search(r"size_t\s+deqsci_grad_norm_workspace_bytes\s*\(", src)
    body = re.search(r"typedef struct \{([^{}]*)\} deqsci_grad_entry;", src).group(1)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in _hip.GradEntry._fields_] and ctypes.sizeof(_hip.GradEntry) == 16
    assert _hip.grad_norm_launches(1) == 3 == _hip.grad_norm_launches(64) and _hip.grad_norm_launches(65) == 5 and _hip.grad_norm_launches(130) == 7
    lib = _hip.load()
    buf = (ctypes.c_float * 256)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    table = (_hip.GradEntry * 2)()
    table[0].grad, table[0].numel, table[1].grad, table[1].numel = p16, 4, p16 + 16, _hip.TRAIN_CHUNK + 1
    ptr = ctypes.cast(table, ctypes.c_void_p)
    assert lib.deqsci_grad_norm_workspace_bytes(ptr, 2) == (1 + 2 + 2) * 16 and lib.deqsci_grad_norm_workspace_bytes(ptr, 1) == 2 * 16
    assert lib.deqsci_grad_norm_workspace_bytes(None, 0) == 0 and lib.deqsci_grad_norm_workspace_bytes(None, 2) == 0 and lib.deqsci_grad_norm_workspace_bytes(ptr, -1) == 0
    # argument validation happens before any launch
    table[1].numel = 4
    stats, ws = p16 + 256, p16 + 512
    assert lib.deqsci_grad_norm_f32(None, 2, 1.0, stats, ws, None) == -1 and lib.deqsci_grad_norm_f32(ptr, 2, 1.0, None, ws, None) == -1
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, None, None) == -1
    assert lib.deqsci_grad_norm_f32(ptr, -1, 1.0, stats, ws, None) == -2
    assert lib.deqsci_grad_norm_f32(ptr, 2, -1.0, stats, ws, None) == -4 and lib.deqsci_grad_norm_f32(ptr, 2, float("nan"), stats, ws, None) == -4
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats + 4, ws, None) == -3 and lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, ws + 4, None) == -3
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, stats + 32, None) == -4                    # stats (5 words) overlaps the workspace
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, p16 + 24, ws, None) == -4                          # stats overlaps a gradient
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, p16, None) == -4                            # the workspace overlaps a gradient
    assert lib.deqsci_grad_scale_f32(ptr, 0, stats, None) == 0 and lib.deqsci_grad_scale_f32(None, 2, stats, None) == -1
    assert lib.deqsci_grad_scale_f32(ptr, 2, None, None) == -1 and lib.deqsci_grad_scale_f32(ptr, 2, stats + 4, None) == -3
    assert lib.deqsci_grad_scale_f32(ptr, 2, p16 + 8, None) == -4
    table[1].numel = 0
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, ws, None) == -2 and lib.deqsci_grad_scale_f32(ptr, 2, stats, None) == -2
    table[1].numel, table[1].grad = 4, p16 + 18
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, ws, None) == -3 and lib.deqsci_grad_scale_f32(ptr, 2, stats, None) == -3
    table[1].grad = None
    assert lib.deqsci_grad_norm_f32(ptr, 2, 1.0, stats, ws, None) == -1 and lib.deqsci_grad_scale_f32(ptr, 2, stats, None) == -1
    # L2c: L2's checks, and the statistics
    adam = (_hip.AdamEntry * 1)()
    adam[0].param, adam[0].grad, adam[0].exp_avg, adam[0].exp_avg_sq, adam[0].numel = p16, p16 + 16, p16 + 32, p16 + 48, 4
    aptr = ctypes.cast(adam, ctypes.c_void_p)
    k = (0.9, 0.1, 0.999, 0.001, 1e-8)
    assert lib.deqsci_adam_step_clipped_f32(aptr, 0, *k, stats, None) == 0 and lib.deqsci_adam_step_clipped_f32(None, 1, *k, stats, None) == -1
    assert lib.deqsci_adam_step_clipped_f32(aptr, 1, *k, None, None) == -1 and lib.deqsci_adam_step_clipped_f32(aptr, 1, *k, stats + 4, None) == -3
    assert lib.deqsci_adam_step_clipped_f32(aptr, 1, *k, p16 + 40, None) == -4                      # stats inside exp_avg
    assert lib.deqsci_adam_step_clipped_f32(aptr, _hip.ADAM_MAX_TENSORS + 1, *k, stats, None) == -4
    adam[0].grad = p16 + 8
    assert lib.deqsci_adam_step_clipped_f32(aptr, 1, *k, stats, None) == -4                         # grad overlaps param, as L2
    adam[0].grad, adam[0].numel = p16 + 16, 0
    assert lib.deqsci_adam_step_clipped_f32(aptr, 1, *k, stats, None) == -2
