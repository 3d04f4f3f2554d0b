"""CPU: the training loop's host side - the data set, the Adam restatement and its counted bound, DeviceAdam on CPU parameters,
train_solver_sci with a stub DEQ module, the command line, and the C ABI of csrc/train.hip (no GPU, no launch)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import train_cases as tc
import train_ref as tr
from conftest import ROOT

from deqsci_amd import checkpoint, harness, training
from deqsci_amd.autograd import mse_loss_stats
from deqsci_amd.optim import DeviceAdam

BETAS, EPS = (0.9, 0.999), 1e-8


# ----------------------------------------------------------------------------- (a) the data set
def test_training_dataset_reads_the_reference_layout(tmp_path):
    d = tc.write(tmp_path)
    ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
    mask, gt, meas = tc.samples()
    assert len(ds) == tc.N_SAMPLES
    assert [os.path.basename(f) for f in ds.full_gt_filelist] == sorted(tc.NAMES) == [os.path.basename(f) for f in ds.full_meas_filelist]
    assert tc.SORTED == (1, 0, 3, 2)                                             # "10.mat" < "9.mat" < "a.mat" < "b.mat"
    for j, i in enumerate(tc.SORTED):
        item = ds[j]
        assert sorted(item) == ["gt", "mask", "meas"]
        assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in item.values())
        assert item["gt"].shape == (tc.H, tc.W, tc.B) and item["meas"].shape == (tc.H, tc.W) and item["mask"].shape == (tc.H, tc.W, tc.B)
        assert np.array_equal(item["gt"], np.float32(gt[i] / 255))               # every one of the four keys, / 255 in double, then fp32
        assert np.array_equal(item["meas"], np.float32(meas[i] / 255)) and np.array_equal(item["mask"], np.float32(mask))
    assert float(ds[0]["mask"][0, :2].sum()) == 0.0
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))
    assert tuple(batch["gt"].shape) == (2, tc.H, tc.W, tc.B) and tuple(batch["mask"].shape) == (2, tc.H, tc.W, tc.B)
    with pytest.raises(ValueError, match="unknown key"):
        training.load_mat(d + "mask.mat", "orig")
    with pytest.raises(KeyError, match="patch_save"):
        training.load_mat(d + "mask.mat", "gt")


def test_matlab_v73_files_are_refused_as_the_test_loader_refuses_them(tmp_path, monkeypatch):
    import sys
    path = str(tmp_path / "v73.mat")
    with open(path, "wb") as fh:                                                   # the 128-byte header of a v7.3 file: version 0x0200
        fh.write(b"MATLAB 7.3 MAT-file, Platform: GLNXA64".ljust(116) + b"\x00" * 8 + b"\x00\x02" + b"IM" + b"\x00" * 64)
    monkeypatch.setitem(sys.modules, "h5py", None)                                 # (not installed here; absent for this test wherever it runs)
    with pytest.raises(NotImplementedError, match="h5py") as a:
        training.load_mat(path, "mask")
    with pytest.raises(NotImplementedError, match="h5py") as b:
        harness.load_test_data(path)
    assert str(a.value) == str(b.value)


# ----------------------------------------------------------------------------- (b) the fp32 order against float64
def _adam_inputs(n=4096, steps=5, seed=5):
    """p0 and one gradient per step: normal draws over six decades, with runs of 0, 1e-12 and 1e4 (kept, or met on one step only)."""
    rng = np.random.RandomState(seed)
    p0 = rng.randn(n).astype(np.float32)
    grads = []
    for s in range(steps):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-4, 2, size=n)).astype(np.float32)
        g[0:64] = 0.0
        g[64:128] = 1e-12
        g[128:192] = 1e4
        g[192:256] = -1e4
        if s == 2:
            g[256:320], g[320:384], g[384:448] = 0.0, 1e-12, 1e4
        grads.append(g)
    return p0, grads


def _trajectories(p0, grads, lr, step=tr.adam_f32_step, state=None, t0=0):
    """-> the step function's fp32 states, the float64 states, and the bounds, step by step"""
    z = np.zeros_like(p0)
    s32 = (p0, z, z) if state is None else state
    s64 = tuple(a.astype(np.float64) for a in s32)
    e = (np.zeros(p0.shape),) * 3
    out = []
    for k, g in enumerate(grads):
        t = t0 + k + 1
        s32 = step(s32[0], g, s32[1], s32[2], t, lr, BETAS, EPS)
        new64 = tr.adam_f64_step(s64[0], g, s64[1], s64[2], t, lr, BETAS, EPS)
        e = tr.adam_bound_step(e, s64, new64, g, t, lr, BETAS, EPS)
        s64 = new64
        out.append((s32, s64, e))
    return out


def _within(s32, s64, e, what):
    worst = 0.0
    for name, a, b, bound in zip("pmv", s32, s64, e):
        err = np.abs(a.astype(np.float64) - b)
        over = err > tr.SECOND_ORDER * bound
        assert not over.any(), (what, name, int(over.sum()), float(err[over].max()), float(bound[over].min()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def test_fp32_adam_order_is_within_its_counted_roundings_of_float64():
    """20 roundings per element and step (train_ref.ADAM_ROUNDINGS), each bounded by 2^-24 of the magnitude its stage sums, carried
    through five steps first order in 2^-24 (x 1.01 for the rest): the bound is counted, the worst use of it is printed."""
    p0, grads = _adam_inputs()
    for lr in (1e-3, 1e-4):
        steps = _trajectories(p0, grads, lr)
        used = [_within(*s, f"lr {lr} step {k + 1}") for k, s in enumerate(steps)]
        print(f"lr {lr}: largest |fp32 - float64| / bound per step", ["%.3f" % u for u in used])
        assert steps[-1][0][0].dtype == np.float32 and np.isfinite(steps[-1][0][0]).all()
        assert float(np.abs(steps[-1][0][0] - p0).max()) > lr                      # (the parameters moved)


def _torch_adam_step_fn(lr, cls=torch.optim.Adam, **kw):
    def step(p, g, m, v, t, lr_, betas, eps):
        param = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = cls([param], lr=lr_, betas=betas, eps=eps, **kw)
        if t > 1:
            opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[param]
        assert int(st["step"]) == t
        return param.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    return step


def test_installed_torch_adam_is_within_the_same_bound():
    """torch.optim.Adam(foreach=False) on the CPU forms m by lerp - m + (1 - b1)(g - m): other roundings, no more of them per stage."""
    p0, grads = _adam_inputs()
    steps = _trajectories(p0, grads, 1e-3, step=_torch_adam_step_fn(1e-3, foreach=False))
    used = [_within(*s, f"torch step {k + 1}") for k, s in enumerate(steps)]
    print("torch.optim.Adam: largest |fp32 - float64| / bound per step", ["%.3f" % u for u in used])


# ----------------------------------------------------------------------------- (c) DeviceAdam on CPU parameters
def test_device_adam_cpu_path_is_the_restated_order_bit_for_bit():
    p0, grads = _adam_inputs(n=1000)
    steps = _trajectories(p0, grads, 1e-3, step=_torch_adam_step_fn(1e-3, cls=DeviceAdam))
    want = _trajectories(p0, grads, 1e-3)
    for (a, _, _), (b, _, _) in zip(steps, want):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_device_adam_state_dict_swaps_with_torch_adam():
    p0, grads = _adam_inputs(n=512, steps=4)
    g = [torch.from_numpy(x) for x in grads]

    def params():
        return [torch.nn.Parameter(torch.from_numpy(p0.copy())), torch.nn.Parameter(torch.ones(3))]
    pa, pb = params(), params()
    a, b = DeviceAdam(pa, lr=1e-3, betas=BETAS, eps=EPS), torch.optim.Adam(pb, lr=1e-3, betas=BETAS, eps=EPS, foreach=False)
    for k in range(2):
        pa[0].grad, pb[0].grad = g[k].clone(), g[k].clone()                       # the second parameter never gets a gradient
        a.step()
        b.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa["state"]) == list(sb["state"]) == [0] and sorted(sa["state"][0]) == sorted(sb["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert sorted(sa["param_groups"][0]) == sorted(sb["param_groups"][0])
    assert type(sa["state"][0]["step"]) is type(sb["state"][0]["step"]) and sa["state"][0]["step"].dtype == sb["state"][0]["step"].dtype
    assert float(sa["state"][0]["step"]) == 2.0 and pa[1] not in a.state and torch.equal(pa[1], torch.ones(3))    # skipped: no step, no state
    # swap: each continues from the other's state, on its own parameters
    before = {"a": [pa[0].detach().numpy().copy(), sa["state"][0]["exp_avg"].numpy().copy(), sa["state"][0]["exp_avg_sq"].numpy().copy()],
              "b": [pb[0].detach().numpy().copy(), sb["state"][0]["exp_avg"].numpy().copy(), sb["state"][0]["exp_avg_sq"].numpy().copy()]}
    a2, b2 = DeviceAdam(pa, lr=1e-3, betas=BETAS, eps=EPS), torch.optim.Adam(pb, lr=1e-3, betas=BETAS, eps=EPS, foreach=False)
    a2.load_state_dict(sb)
    b2.load_state_dict(sa)
    pa[0].grad, pb[0].grad = g[2].clone(), g[2].clone()
    a2.step()
    b2.step()
    for opt, p, start in ((a2, pa[0], [before["a"][0], before["b"][1], before["b"][2]]), (b2, pb[0], [before["b"][0], before["a"][1], before["a"][2]])):
        st = opt.state[p]
        assert int(st["step"]) == 3
        s64 = tuple(x.astype(np.float64) for x in start)
        new64 = tr.adam_f64_step(s64[0], grads[2], s64[1], s64[2], 3, 1e-3, BETAS, EPS)
        e = tr.adam_bound_step((np.zeros(512),) * 3, s64, new64, grads[2], 3, 1e-3, BETAS, EPS)
        _within((p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), new64, e, type(opt).__name__)
    # a checkpoint of the reference's torch 1.9 holds an integer step
    sd = a2.state_dict()
    sd["state"][0]["step"] = 3
    a3 = DeviceAdam(pa, lr=1e-3)
    a3.load_state_dict(sd)
    pa[0].grad = g[3].clone()
    a3.step()
    assert float(a3.state[pa[0]]["step"]) == 4.0 and isinstance(a3.state[pa[0]]["step"], torch.Tensor)


def test_device_adam_refuses_what_it_does_not_implement():
    p = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(NotImplementedError, match="weight decay"):
        DeviceAdam(p, lr=1e-3, weight_decay=1e-2)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        DeviceAdam(p, lr=1e-3, amsgrad=True)
    with pytest.raises(ValueError):
        DeviceAdam(p, lr=-1.0)                                                     # torch.optim.Adam's own checks
    opt = DeviceAdam(p, lr=1e-3)
    p[0].grad = torch.ones(2)
    for key in ("weight_decay", "amsgrad", "maximize"):
        opt.param_groups[0][key] = 0.1 if key == "weight_decay" else True         # (a loaded state_dict can bring them)
        with pytest.raises(NotImplementedError, match=key):
            opt.step()
        opt.param_groups[0][key] = 0 if key == "weight_decay" else False
    opt.step()
    assert float(opt.state[p[0]]["step"]) == 1.0


def test_mse_loss_stats_on_the_host_is_mse_loss():
    g = torch.Generator().manual_seed(3)
    rec = (torch.rand(2, 6, 5, 4, generator=g, dtype=torch.float64) * 1.6 - 0.3).requires_grad_(True)
    gt = torch.rand(2, 6, 5, 4, generator=g, dtype=torch.float64)
    loss, stats = mse_loss_stats(rec, gt)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and not stats.requires_grad and stats.dtype == torch.float64
    want = torch.nn.functional.mse_loss(rec, gt)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-15
    (ga,) = torch.autograd.grad(loss * 3.0, rec)
    (gb,) = torch.autograd.grad(want * 3.0, rec)
    assert float((ga - gb).abs().max()) <= 1e-15
    total = rec.numel()
    assert abs(10 * math.log10(total / float(stats[1])) - harness.psnr(rec.detach().clip(0, 1).float().numpy(), gt.float().numpy())) < 1e-5
    assert float(stats[2]) == 0.0 and float(stats[1]) < float(stats[0])          # the clamp mattered
    bad = rec.detach().clone()
    bad[0, 0, 0, 0], bad[1, 2, 3, 0] = float("nan"), float("inf")
    loss, stats = mse_loss_stats(bad, gt)
    assert float(stats[2]) == 2.0 and not math.isfinite(float(loss))
    # fp32, as the loop uses it on CPU tensors: train_ref's terms, torch's float64 sum
    r32, g32 = rec.detach().float(), gt.float()
    loss, stats = mse_loss_stats(r32, g32)
    grad, want_stats = tr.mse_stats(r32.numpy().ravel(), g32.numpy().ravel())
    assert loss.dtype == torch.float32 and np.allclose(stats.numpy(), want_stats, rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="differ"):
        mse_loss_stats(r32, g32[:1])


# ----------------------------------------------------------------------------- (d) the loop, with a stub DEQ module
class _Stub(torch.nn.Module):
    """A solver and a DEQ module in one: `nonlinear_op` is a 3x3 conv over the frames of the initial point; forward has DEQFixedPoint's
    signature.  nan_at: the calls (counted from 0) that return NaN."""

    def __init__(self, nan_at=()):
        super().__init__()
        torch.manual_seed(11)
        self.nonlinear_op = torch.nn.Conv2d(tc.B, tc.B, 3, padding=1)
        self.calls, self.nan_at, self.recs = 0, set(nan_at), []

    def forward(self, y, Phi, Phi_sum, initial_point=None, train_flag=True):
        assert float(Phi_sum.min()) == 1.0 and initial_point is not None and not initial_point.requires_grad
        assert torch.equal(initial_point, y.unsqueeze(3) * Phi)
        out = initial_point + 0.1 * self.nonlinear_op(initial_point.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        if self.calls in self.nan_at:
            out = out * float("nan")
        self.calls += 1
        self.recs.append(out.detach().clone())
        return out


def _loop(tmp_path, loss_function, n_epochs=2, nan_at=(), opt_cls=torch.optim.Adam, **kw):
    d = tc.write(tmp_path / "data")
    ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
    loader = torch.utils.data.DataLoader(ds, batch_size=tc.BATCH, shuffle=False, drop_last=True)
    stub = _Stub(nan_at)
    opt = opt_cls(stub.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    model = str(tmp_path / "model") + "/"
    os.makedirs(model, exist_ok=True)
    steps = []
    hist = training.train_solver_sci(stub, loader, opt, model, loss_function, n_epochs, stub, scheduler=sched, print_every_n_steps=1,
                                     save_every_n_steps=1000, tflog_path=model, on_step=steps.append, **kw)
    assert hist == steps
    return stub, opt, sched, model, steps, ds


@pytest.mark.parametrize("loss", ["mse", "device"])
def test_loop_writes_the_reference_checkpoints_and_reports_its_psnr(tmp_path, loss, capsys):
    stub, opt, sched, model, steps, ds = _loop(tmp_path, torch.nn.MSELoss(reduction="mean") if loss == "mse" else "device",
                                               opt_cls=torch.optim.Adam if loss == "mse" else DeviceAdam)
    assert sorted(os.listdir(model)) == ["epoch_0.ckpt", "epoch_1.ckpt", "scalars.jsonl"]
    for e in (0, 1):
        obj = torch.load(model + f"epoch_{e}.ckpt", weights_only=False)
        assert sorted(obj) == ["epoch", "optimizer_state_dict", "scheduler_state_dict", "solver_state_dict"] and obj["epoch"] == e
        assert sorted(obj["solver_state_dict"]) == ["nonlinear_op.bias", "nonlinear_op.weight"]
        assert float(obj["optimizer_state_dict"]["state"][0]["step"]) == 2.0 * (e + 1)
    fresh = _Stub()
    assert checkpoint.load_solver(fresh, model + "epoch_1.ckpt") == 1 and torch.equal(fresh.nonlinear_op.weight, stub.nonlinear_op.weight)
    assert not torch.equal(_Stub().nonlinear_op.weight, stub.nonlinear_op.weight)
    assert sched.last_epoch == 2 and math.isclose(opt.param_groups[0]["lr"], 1e-3 * 0.25)            # one scheduler step per epoch
    assert [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1), (1, 0), (1, 1)] and [s.lr for s in steps] == [1e-3, 1e-3, 5e-4, 5e-4]
    for k, s in enumerate(steps):
        items = [ds[j]["gt"] for j in ((0, 1), (2, 3))[k % 2]]
        want = harness.psnr(stub.recs[k].clip(0, 1).numpy(), np.stack(items))                       # the reference's batch PSNR
        assert abs(s.psnr - want) <= (0.0 if loss == "mse" else 1e-9), (k, s.psnr, want)
        assert abs(s.loss - float(torch.nn.functional.mse_loss(stub.recs[k], torch.from_numpy(np.stack(items))))) <= 1e-6 * s.loss
        assert s.nonfinite == (None if loss == "mse" else 0)
    out = capsys.readouterr().out
    assert out.count("dict saved!") == 2 and "avg PSNR in epoch 1: %.2f dB" % ((steps[2].psnr + steps[3].psnr) / 2) in out
    assert "Epoch: 0 Step: 1 Loss: " + str(np.float32(steps[1].loss)) + " PSNR: %2.2f dB" % steps[1].psnr + " best PSNR (test): 0.00 dB lr: 0.00100000" in out
    import json
    rows = [json.loads(ln) for ln in open(model + "scalars.jsonl")]
    assert len(rows) == 4 and [r["global_step"] for r in rows] == [2, 4, 6, 8]
    assert all(set(r) == {"global_step", "walltime", "main/PSNR", "main/loss", "config/lr", "main/best_PSNR"} for r in rows)
    # resume: optimizer and scheduler come back
    opt2 = type(opt)(fresh.parameters(), lr=1e-3)
    sched2 = torch.optim.lr_scheduler.StepLR(opt2, step_size=1, gamma=0.5)
    assert checkpoint.load_training(model + "epoch_1.ckpt", fresh, opt2, sched2) == 1
    assert sched2.last_epoch == 2 and float(opt2.state[fresh.nonlinear_op.weight]["step"]) == 4.0


def test_max_steps_stops_the_loop(tmp_path):
    stub, opt, sched, model, steps, _ = _loop(tmp_path, torch.nn.MSELoss(), n_epochs=5, max_steps=3)
    assert len(steps) == 3 and stub.calls == 3 and [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1), (1, 0)]
    assert sorted(f for f in os.listdir(model) if f.endswith(".ckpt")) == ["epoch_0.ckpt", "epoch_1.ckpt"]


@pytest.mark.parametrize("loss", ["mse", "device"])
def test_nan_loss_breaks_the_epoch_and_reloads(tmp_path, loss, monkeypatch, capsys):
    loaded = []
    real = checkpoint.load_training
    monkeypatch.setattr(checkpoint, "load_training", lambda path, *a, **k: (loaded.append(path), real(path, *a, **k))[1])
    stepped = []
    cls = torch.optim.Adam if loss == "mse" else DeviceAdam

    class Counting(cls):
        def step(self, closure=None):
            stepped.append(1)
            return super().step(closure)
    stub, opt, sched, model, steps, _ = _loop(tmp_path, torch.nn.MSELoss() if loss == "mse" else "device", n_epochs=3, nan_at=(2,), opt_cls=Counting)
    # epoch 0: two steps; epoch 1: NaN at its first step - no optimizer step, the epoch ends, no checkpoint; epoch 2: reload, two steps
    assert stub.calls == 5 and len(stepped) == 4 and [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1), (2, 0), (2, 1)]
    assert loaded == [model + "epoch_0.ckpt"]
    assert sorted(f for f in os.listdir(model) if f.endswith(".ckpt")) == ["epoch_0.ckpt", "epoch_2.ckpt"]
    assert sched.last_epoch == 3 and "Loss is nan!" in capsys.readouterr().out
    assert float(opt.state[stub.nonlinear_op.weight]["step"]) == 4.0


def test_loop_refuses_what_it_does_not_do(tmp_path):
    stub = _Stub()
    with pytest.raises(NotImplementedError, match="single-device"):
        training.train_solver_sci(stub, [], None, "", torch.nn.MSELoss(), 1, stub, use_dataparallel=True)
    with pytest.raises(ValueError, match="'device'"):
        training.train_solver_sci(stub, [], None, "", "mse", 1, stub)


def test_configure_training_picks_the_modes_from_the_eligibility_tables():
    import deqsci_amd
    from deqsci_amd.cli import build_pipeline
    want = {("SimpleCNN", True): ("device", "device", {}), ("SimpleCNN", False): ("device", "device", {}),
            ("RealSN_SimpleCNN", True): ("device+realsn", "device+realsn", {"train_realsn": "device"}),
            ("ffdnet", False): ("device", "device+bn", {}), ("ffdnet", True): ("autograd", "device+bn-train", {"train_bn": "device"})}
    for (name, train), (implicit, parameter, options) in want.items():
        solver, deq = build_pipeline(name, None, 3, device="cpu")
        solver.nonlinear_op.train(train)
        deq.engine_options = {"conv64": "fast32", "train_bn": "module"}
        cfg = training.configure_training(deq, "device")
        assert (cfg.implicit_backward, cfg.parameter_backward) == (implicit, parameter) == (deq.implicit_backward, deq.parameter_backward), (name, train, cfg)
        assert cfg.engine_options == {"conv64": "fast32", **options} == deq.engine_options
        assert sorted(cfg.reasons) == (["implicit_backward"] if implicit == "autograd" else []), cfg.reasons
        if implicit == "autograd":
            assert "BatchNorm2d in train mode" in cfg.reasons["implicit_backward"]
        cfg = training.configure_training(deq, "autograd")
        assert (deq.implicit_backward, deq.parameter_backward, deq.engine_options, cfg.reasons) == ("autograd", "autograd", {"conv64": "fast32"}, {})
    deq.f.A = lambda x, Phi: x.sum(3)
    cfg = training.configure_training(deq, "device")
    assert cfg.implicit_backward == cfg.parameter_backward == "autograd" and all("custom A / At" in v for v in cfg.reasons.values()) and len(cfg.reasons) == 2
    with pytest.raises(ValueError, match="backend"):
        training.configure_training(deq, "hip")
    assert deqsci_amd.configure_training is training.configure_training and deqsci_amd.DeviceAdam is DeviceAdam


# ----------------------------------------------------------------------------- (e) the command line
def test_cli_training_flags_and_refusals(capsys):
    from deqsci_amd.cli import main, parser
    a = parser().parse_args(["--inference", "False", "--n_epochs", "3", "--batch_size", "2", "--lr", "1e-3", "--lr_gamma", "0.5", "--sched_step", "2",
                             "--trainpath", "t/", "--print_every_n_steps", "7", "--save_every_n_steps", "5", "--train_backend", "device",
                             "--seed", "4", "--max_steps", "9"])
    assert (a.n_epochs, a.batch_size, a.lr, a.lr_gamma, a.sched_step, a.trainpath) == (3, 2, 1e-3, 0.5, 2, "t/")
    assert all(type(v) is int for v in (a.n_epochs, a.batch_size, a.sched_step, a.print_every_n_steps, a.save_every_n_steps, a.seed, a.max_steps))
    assert a.train_backend == "device"
    d = parser().parse_args([])
    assert (d.n_epochs, d.batch_size, d.lr, d.lr_gamma, d.sched_step, d.trainpath, d.print_every_n_steps, d.save_every_n_steps) == \
        (80, 1, 1e-4, 0.9, 10, "", 1, 50)                                         # the reference's defaults
    assert d.train_backend in ("device", "autograd") and d.seed is None and d.max_steps is None
    groups = {g.title: [x.dest for x in g._group_actions] for g in parser()._action_groups}
    assert all("n_epochs" not in dests for title, dests in groups.items() if "unused" in title or "ignored" in title)
    helps = {x.dest: x.help for x in parser()._actions}
    assert all("(this build)" in helps[k] for k in ("train_backend", "seed", "max_steps"))
    with pytest.raises(SystemExit) as e:
        main(["--inference", "False"])
    assert "--trainpath" in str(e.value)
    with pytest.raises(SystemExit) as e:
        main(["--inference", "False", "--trainpath", "t/", "--gpu_ids", "0,1"])
    assert "single-device" in str(e.value) and "--gpu_ids" in str(e.value)
    with pytest.raises(SystemExit) as e:
        main(["--inference", "False", "--trainpath", "t/", "--loadpath", "no/such.ckpt"])
    assert "--loadpath" in str(e.value) and "no such file" in str(e.value)
    with pytest.raises(SystemExit):
        parser().parse_args(["--train_backend", "hip"])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit) as e:
            main(["--inference", "False", "--trainpath", "t/"])
        assert "MI355X" in str(e.value)


# ----------------------------------------------------------------------------- (f) the C ABI
def test_header_binding_and_library_agree_on_the_training_entry_points():
    import ctypes
    from deqsci_amd import _hip
    src = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\bint\s+(deqsci_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    for name, n in (("deqsci_mse_stats_grad_f32", 8), ("deqsci_adam_step_f32", 8)):
        params = [p for p in protos[name].split(",") if p.strip()]
        assert len(params) == len(_hip.SIGNATURES[name]) == n, name
    assert "deqsci_mse_workspace_bytes" in _hip.OTHER_EXPORTS and re.search(r"size_t\s+deqsci_mse_workspace_bytes\s*\(\s*int64_t\s+total\s*\)", src)
    assert f"#define DEQSCI_ADAM_MAX_TENSORS {_hip.ADAM_MAX_TENSORS}" in src and f"#define DEQSCI_TRAIN_CHUNK {_hip.TRAIN_CHUNK}" in src
    assert _hip.ADAM_MAX_TENSORS == tr.ADAM_MAX_TENSORS and _hip.TRAIN_CHUNK == tr.CHUNK
    # the struct of the header, field by field, and the size the kernel-argument table is built from
    body = re.search(r"typedef struct \{(.*?)\} deqsci_adam_entry;", src, flags=re.S).group(1)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in _hip.AdamEntry._fields_] and ctypes.sizeof(_hip.AdamEntry) == 48
    assert 64 * 48 + 65 * 4 + 6 * 4 <= 4096
    lib = _hip.load()
    chunk = _hip.TRAIN_CHUNK
    assert lib.deqsci_mse_workspace_bytes(1) == 24 and lib.deqsci_mse_workspace_bytes(chunk) == 24 and lib.deqsci_mse_workspace_bytes(chunk + 1) == 48
    assert lib.deqsci_mse_workspace_bytes(-1) == 0 and lib.deqsci_mse_workspace_bytes(0) == 0
    # argument validation happens before any launch
    buf = (ctypes.c_float * 64)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    s = ctypes.c_float(0.5)
    assert lib.deqsci_mse_stats_grad_f32(None, p16, p16 + 64, p16 + 128, 4, s, p16 + 160, None) == -1
    assert lib.deqsci_mse_stats_grad_f32(p16, p16 + 16, p16 + 64, p16 + 128, 0, s, p16 + 160, None) == -2
    assert lib.deqsci_mse_stats_grad_f32(p16 + 2, p16 + 16, p16 + 64, p16 + 128, 4, s, p16 + 160, None) == -3
    assert lib.deqsci_mse_stats_grad_f32(p16, p16 + 16, p16 + 64, p16 + 132, 4, s, p16 + 160, None) == -3           # stats: 8-byte aligned
    assert lib.deqsci_mse_stats_grad_f32(p16, p16 + 16, p16 + 8, p16 + 128, 4, s, p16 + 160, None) == -4            # grad overlaps rec
    table = (_hip.AdamEntry * 2)()
    for i in range(2):
        table[i].param, table[i].grad, table[i].exp_avg, table[i].exp_avg_sq, table[i].numel = p16 + 64 * i, p16 + 64 * i + 16, p16 + 64 * i + 32, p16 + 64 * i + 48, 4
    ptr = ctypes.cast(table, ctypes.c_void_p)
    assert lib.deqsci_adam_step_f32(ptr, 0, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == 0                                # nothing to do, nothing launched
    assert lib.deqsci_adam_step_f32(None, 1, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert lib.deqsci_adam_step_f32(ptr, _hip.ADAM_MAX_TENSORS + 1, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -4
    assert lib.deqsci_adam_step_f32(ptr, -1, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -4
    table[1].numel = 0
    assert lib.deqsci_adam_step_f32(ptr, 2, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -2
    table[1].numel, table[1].grad = 4, p16 + 64 + 2
    assert lib.deqsci_adam_step_f32(ptr, 2, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -3
    table[1].grad = p16 + 64 + 8
    assert lib.deqsci_adam_step_f32(ptr, 2, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -4                               # grad overlaps param
    table[1].grad, table[1].exp_avg = p16 + 64 + 16, None
    assert lib.deqsci_adam_step_f32(ptr, 2, 0.9, 0.1, 0.999, 0.001, 1e-8, None) == -1
