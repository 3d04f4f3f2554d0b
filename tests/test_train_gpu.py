"""GPU: the training loop - csrc/train.hip's two kernels against tests/train_ref.py BIT FOR BIT, mse_loss_stats, DeviceAdam, and
train_solver_sci against the reference's own training run (tests/golden/train_simplecnn.npz, made by tests/golden/make_train_golden.py
on the tiny training set of tests/train_cases.py), its resume, the stale-weight guard and the two train-mode denoiser families."""
import math
import os

import numpy as np
import pytest
import torch

import train_cases as tc
import train_ref as tr
from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint, training
    from deqsci_amd.autograd import mse_loss_stats
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.optim import DeviceAdam

DEV = "cuda"
SENT = 7.25                                                    # the sentinel around every buffer a kernel writes
CHUNK = tr.CHUNK
BETAS, EPS = (0.9, 0.999), 1e-8


def _view(a, offset, sentinel=SENT):
    """numpy fp32 array -> (a device buffer filled with the sentinel, its view `offset` floats past a 16-byte boundary holding a)"""
    buf = torch.full((a.size + 8,), sentinel, device=DEV, dtype=torch.float32)
    v = buf[offset:offset + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * (offset % 4)
    return buf, v


def _intact(buf, offset, n, sentinel=SENT):
    b = buf.cpu().numpy()
    return bool((b[:offset] == sentinel).all() and (b[offset + n:] == sentinel).all())


# ----------------------------------------------------------------------------- (a) L1
L1_TOTALS = [1, 3, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * tc.H * tc.W * tc.B, 3 * CHUNK + 5]


def _l1_inputs(total):
    rng = np.random.RandomState(total)
    rec = (rng.randn(total) * 0.8 + 0.5).astype(np.float32)                       # values below 0 and above 1: the clamp matters
    if total >= 3:
        rec[0], rec[-1] = -0.25, 1.5
    return rec, rng.rand(total).astype(np.float32)


def _run_l1(rec, gt, off):
    total = rec.size
    _, drec = _view(rec, off)
    _, dgt = _view(gt, 0)
    gbuf, dgrad = _view(np.zeros(total, np.float32), off)
    sbuf = torch.full((5,), SENT, device=DEV, dtype=torch.float64)
    grad, stats = _hip.mse_stats_grad(drec, dgt, grad=dgrad, stats=sbuf[1:4])
    assert grad is dgrad
    s = sbuf.cpu().numpy()
    assert s[0] == SENT and s[4] == SENT and _intact(gbuf, off, total)
    return dgrad.cpu().numpy(), s[1:4]


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("total", L1_TOTALS)
def test_mse_stats_grad_equals_the_restated_order(total, off):
    assert _hip.load().deqsci_mse_workspace_bytes(CHUNK + 1) == 48                 # the chunk this file assumes
    rec, gt = _l1_inputs(total)
    want_grad, want = tr.mse_stats(rec, gt)
    grad, stats = _run_l1(rec, gt, off)
    assert np.array_equal(grad, want_grad)
    assert np.array_equal(stats, want), (stats, want)                              # float64, bit for bit
    assert stats[2] == 0.0 and (total < 3 or stats[1] < stats[0])
    _, sq, sqc, _ = tr.mse_terms(rec, gt)
    exact = tr.mse_stats_f64(rec, gt)
    for k, t in enumerate((sq, sqc)):                                              # any float64 summation order: N 2^-53 sum |t| of the exact sum
        assert abs(stats[k] - exact[k]) <= total * 2.0 ** -53 * math.fsum(np.abs(t.astype(np.float64)))
    again_grad, again = _run_l1(rec, gt, off)
    assert np.array_equal(again, stats) and np.array_equal(again_grad, grad)
    # the wrapper's own buffers, and the loss / PSNR the host forms from the three words
    _, drec = _view(rec, off)
    g2, s2 = _hip.mse_stats_grad(drec, torch.from_numpy(gt).to(DEV))
    assert np.array_equal(g2.cpu().numpy(), grad) and np.array_equal(s2.cpu().numpy(), stats)
    assert abs(stats[0] / total - float(np.mean((rec - gt).astype(np.float64) ** 2))) <= 1e-6 * stats[0] / total


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_mse_stats_grad_counts_nan_and_inf_and_still_writes_the_gradient(off):
    total = 2 * tc.H * tc.W * tc.B
    rec, gt = _l1_inputs(total)
    rec[5], rec[700] = np.nan, np.inf
    want_grad, want = tr.mse_stats(rec, gt)
    grad, stats = _run_l1(rec, gt, off)                                            # (sentinels around grad and stats checked there)
    assert stats[2] == 2.0 == want[2] and not math.isfinite(stats[0] / total) and math.isnan(want[0])
    assert math.isnan(stats[1]) and math.isnan(want[1])                            # the clamp turns Inf into 1; NaN stays NaN
    assert math.isnan(grad[5]) and math.isinf(grad[700])
    keep = np.ones(total, bool)
    keep[[5, 700]] = False
    assert np.array_equal(grad[keep], want_grad[keep]) and np.isfinite(grad[keep]).all()
    again_grad, again = _run_l1(rec, gt, off)
    assert np.array_equal(again_grad, grad, equal_nan=True) and np.array_equal(again, stats, equal_nan=True)


def test_mse_stats_grad_wrapper_refusals():
    a = torch.zeros(2, 3, device=DEV)
    with pytest.raises(_hip.DeqsciHipError, match="one shape"):
        _hip.mse_stats_grad(a, torch.zeros(3, 2, device=DEV))
    with pytest.raises(_hip.DeqsciHipError, match="HIP device"):
        _hip.mse_stats_grad(a, torch.zeros(2, 3))
    with pytest.raises(_hip.DeqsciHipError, match="empty"):
        _hip.mse_stats_grad(a[:0], a[:0])
    with pytest.raises(_hip.DeqsciHipError, match="workspace too small"):
        _hip.mse_stats_grad(torch.zeros(CHUNK + 1, device=DEV), torch.zeros(CHUNK + 1, device=DEV), workspace=torch.zeros(3, device=DEV, dtype=torch.float64))


# ----------------------------------------------------------------------------- (b) L2
L2_SIZES = [1, 5, 576, 36864, CHUNK + 3]


def _adam_layout(n_tensors, rng):
    """-> sizes and start offsets of n_tensors tensors in one flat buffer: one sentinel at least behind every tensor, the starts at every
    residue mod 4 (most tensors: 4-byte aligned only)"""
    sizes = L2_SIZES + [1 + (7 * i) % 41 for i in range(n_tensors - len(L2_SIZES))]
    starts, o = [], 0
    for i, n in enumerate(sizes):
        o += 1 + (i % 3)
        starts.append(o)
        o += n
    return sizes, starts, o + 4


def test_adam_step_equals_the_restated_order_over_three_steps(monkeypatch):
    n_tensors = tr.ADAM_MAX_TENSORS + 3
    rng = np.random.RandomState(9)
    sizes, starts, flat_n = _adam_layout(n_tensors, rng)
    assert len({s % 4 for s in starts}) == 4
    host = {k: np.full(flat_n, SENT, np.float32) for k in "pgmv"}
    for n, s in zip(sizes, starts):
        host["p"][s:s + n] = rng.randn(n)
        host["m"][s:s + n] = 0.0
        host["v"][s:s + n] = 0.0
    dev = {k: torch.from_numpy(host[k].copy()).to(DEV) for k in "pgmv"}
    views = {k: [dev[k][s:s + n] for n, s in zip(sizes, starts)] for k in "pgmv"}
    assert any(v.data_ptr() % 16 for v in views["p"])
    lib = _hip.load()
    calls = []
    real = lib.deqsci_adam_step_f32
    monkeypatch.setattr(lib, "deqsci_adam_step_f32", lambda *a: (calls.append(a[1]), real(*a))[1])
    for t, lr in ((1, 1e-3), (2, 1e-3), (3, 2.5e-4)):                               # lr changed between steps
        for n, s in zip(sizes, starts):
            g = (rng.randn(n) * 10.0 ** rng.uniform(-4, 2, size=n)).astype(np.float32)
            if n >= 576:
                g[:8], g[8:16], g[16:24] = 0.0, 1e-12, 1e4
            host["g"][s:s + n] = g
        dev["g"].copy_(torch.from_numpy(host["g"]))
        del calls[:]
        launches = _hip.adam_step(views["p"], views["g"], views["m"], views["v"], t, lr, BETAS, EPS)
        assert launches == 2 == -(-n_tensors // tr.ADAM_MAX_TENSORS) and calls == [tr.ADAM_MAX_TENSORS, 3]
        for n, s in zip(sizes, starts):
            sl = slice(s, s + n)
            host["p"][sl], host["m"][sl], host["v"][sl] = tr.adam_f32_step(host["p"][sl], host["g"][sl], host["m"][sl], host["v"][sl], t, lr, BETAS, EPS)
        for k in "pmvg":                                                            # the whole buffers: every tensor, every sentinel
            got = dev[k].cpu().numpy()
            assert np.array_equal(got, host[k]), (t, k, int((got != host[k]).sum()))
    assert float(np.abs(host["p"][starts[3]:starts[3] + 8]).max()) > 0


def test_adam_step_wrapper_refusals():
    p = [torch.zeros(4, device=DEV)]
    assert _hip.adam_step([], [], [], [], 1, 1e-3, BETAS, EPS) == 0
    with pytest.raises(_hip.DeqsciHipError, match="one length"):
        _hip.adam_step(p, [], p, p, 1, 1e-3, BETAS, EPS)
    with pytest.raises(_hip.DeqsciHipError, match="step must be"):
        _hip.adam_step(p, p, p, p, 0, 1e-3, BETAS, EPS)
    with pytest.raises(_hip.DeqsciHipError, match="grad 0"):
        _hip.adam_step(p, [torch.zeros(4)], p, p, 1, 1e-3, BETAS, EPS)
    with pytest.raises(_hip.DeqsciHipError, match="code -4"):                       # the four ranges of an entry must not overlap
        _hip.adam_step(p, p, [torch.zeros(4, device=DEV)], [torch.zeros(4, device=DEV)], 1, 1e-3, BETAS, EPS)


def test_device_adam_steps_tables_of_tensors_and_bumps_versions(monkeypatch):
    n_tensors = tr.ADAM_MAX_TENSORS + 3
    rng = np.random.RandomState(4)
    sizes, starts, flat_n = _adam_layout(n_tensors, rng)
    flat = torch.full((flat_n,), SENT, device=DEV)
    params, host_p = [], []
    for n, s in zip(sizes, starts):
        p0 = rng.randn(n).astype(np.float32)
        flat[s:s + n] = torch.from_numpy(p0).to(DEV)
        params.append(flat[s:s + n].requires_grad_())                              # views into a flat buffer: 4-byte aligned only
        host_p.append(p0)
    skipped = 2                                                                     # this one never gets a gradient
    opt = DeviceAdam(params, lr=1e-3, betas=BETAS, eps=EPS)
    lib = _hip.load()
    calls = []
    real = lib.deqsci_adam_step_f32
    monkeypatch.setattr(lib, "deqsci_adam_step_f32", lambda *a: (calls.append(a[1]), real(*a))[1])
    host_m = [np.zeros(n, np.float32) for n in sizes]
    host_v = [np.zeros(n, np.float32) for n in sizes]
    for t, lr in ((1, 1e-3), (2, 5e-4), (3, 5e-4)):
        opt.param_groups[0]["lr"] = lr
        versions = [p._version for p in params]
        grads = []
        for i, n in enumerate(sizes):
            g = (rng.randn(n) * 10.0 ** rng.uniform(-3, 1, size=n)).astype(np.float32)
            grads.append(g)
            params[i].grad = None if i == skipped else torch.from_numpy(g).to(DEV)
        del calls[:]
        opt.step()
        assert calls == [tr.ADAM_MAX_TENSORS, 2] and opt.last_launches == 2         # 66 tensors with a gradient: ceil(66 / 64) launches
        for i, n in enumerate(sizes):
            if i == skipped:
                assert params[i] not in opt.state                                   # (views of one buffer share its version counter)
                continue
            assert params[i]._version > versions[i], i                              # the engine's staleness test reads this
            host_p[i], host_m[i], host_v[i] = tr.adam_f32_step(host_p[i], grads[i], host_m[i], host_v[i], t, lr, BETAS, EPS)
            st = opt.state[params[i]]
            assert float(st["step"]) == t and not st["step"].is_cuda
            assert np.array_equal(params[i].detach().cpu().numpy(), host_p[i]), (t, i)
            assert np.array_equal(st["exp_avg"].cpu().numpy(), host_m[i]) and np.array_equal(st["exp_avg_sq"].cpu().numpy(), host_v[i]), (t, i)
    want = np.full(flat_n, SENT, np.float32)
    for p, s in zip(host_p, starts):
        want[s:s + p.size] = p
    assert np.array_equal(flat.detach().cpu().numpy(), want)                        # nothing written between the tensors
    # the state loads into torch.optim.Adam, which continues from it
    ref = torch.optim.Adam(params, lr=5e-4, betas=BETAS, eps=EPS)
    ref.load_state_dict(opt.state_dict())
    assert float(ref.state[params[0]]["step"]) == 3.0 and torch.equal(ref.state[params[3]]["exp_avg"], opt.state[params[3]]["exp_avg"])


# ----------------------------------------------------------------------------- (c) mse_loss_stats
def test_mse_loss_stats_gradient_and_loss_on_the_device():
    g = torch.Generator().manual_seed(6)
    rec_h = torch.rand(2, tc.H, tc.W, tc.B, generator=g) * 1.6 - 0.3
    gt_h = torch.rand(2, tc.H, tc.W, tc.B, generator=g)
    rec = rec_h.to(DEV).requires_grad_(True)
    loss, stats = mse_loss_stats(rec, gt_h.to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad and not stats.requires_grad and stats.dtype == torch.float64
    total = rec.numel()
    want_grad, want = tr.mse_stats(rec_h.numpy().ravel(), gt_h.numpy().ravel())
    assert np.array_equal(stats.cpu().numpy(), want)
    assert float(loss.detach()) == float(np.float32(want[0] / total))
    ref = torch.nn.functional.mse_loss(rec.detach(), gt_h.to(DEV))
    assert abs(float(loss.detach()) - float(ref)) <= 1e-6 * float(ref)
    loss.backward()
    assert np.array_equal(rec.grad.cpu().numpy().ravel(), want_grad)               # 2 (rec - gt) / total, bit for bit
    assert np.array_equal(want_grad, (rec_h.numpy().ravel() - gt_h.numpy().ravel()) * np.float32(2.0 / total))
    rec2 = rec_h.to(DEV).requires_grad_(True)
    (mse_loss_stats(rec2, gt_h.to(DEV))[0] * 0.5).backward()
    assert np.array_equal(rec2.grad.cpu().numpy().ravel(), want_grad * np.float32(0.5))
    # the host restatement is the same function of rec (tests/test_train_host.py compares it with F.mse_loss in float64)
    loss_h, stats_h = mse_loss_stats(rec_h.clone().requires_grad_(True), gt_h)
    assert abs(float(loss_h.detach()) - float(loss.detach())) <= 1e-6 * float(loss.detach()) and np.allclose(stats_h.numpy(), want, rtol=1e-12)


# ----------------------------------------------------------------------------- the loop on the tiny training set
WEIGHTS = {"SimpleCNN": "cnn", "ffdnet": "ffdnet_gray", "RealSN_SimpleCNN": "rsn_cnn"}


class _Watched:
    """An optimizer class that keeps the gradients of its first step"""

    @staticmethod
    def of(cls):
        class Watched(cls):
            first_grads = None

            def step(self, closure=None):
                if self.first_grads is None:
                    self.first_grads = [p.grad.detach().clone() for g in self.param_groups for p in g["params"] if p.grad is not None]
                return super().step(closure)
        return Watched


def _pipeline(kind, backend, lr=tc.LR):
    solver, deq = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), tc.ITERS)
    solver.nonlinear_op.train()
    cfg = training.configure_training(deq, backend)
    opt = _Watched.of(DeviceAdam if backend == "device" else torch.optim.Adam)(solver.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.9)
    return solver, deq, cfg, opt, sched


def _loader(directory, start=0):
    ds = training.SCITrainingDatasetSubset(directory + "gt/", directory + "measurement/", directory + "mask.mat")
    return torch.utils.data.DataLoader(ds, batch_size=tc.BATCH, sampler=tc.RecordedSampler(start=start), drop_last=True)


def _train(kind, backend, tmp, n_epochs=tc.EPOCHS, pipeline=None, start_epoch=0, **kw):
    directory = tc.write(tmp / "data")
    model = str(tmp / f"model_{kind}_{backend}_{start_epoch}") + "/"
    os.makedirs(model, exist_ok=True)
    solver, deq, cfg, opt, sched = pipeline or _pipeline(kind, backend)
    steps = training.train_solver_sci(solver, _loader(directory, start_epoch), opt, model, "device" if backend == "device" else torch.nn.MSELoss(reduction="mean"),
                                      n_epochs, deq, scheduler=sched, print_every_n_steps=1, save_every_n_steps=1000, start_epoch=start_epoch, **kw)
    return {"solver": solver, "deq": deq, "cfg": cfg, "opt": opt, "sched": sched, "steps": steps, "model": model}


_RUNS = {}


def _run(kind, backend, tmp_path_factory):
    if (kind, backend) not in _RUNS:
        _RUNS[kind, backend] = _train(kind, backend, tmp_path_factory.mktemp(f"train_{kind}_{backend}"))
    return _RUNS[kind, backend]


# ----------------------------------------------------------------------------- (d) no synchronisation beyond the solver's and the one read-back
def test_a_step_reads_back_once_between_the_loss_and_the_end_of_the_optimizer_step(tmp_path, monkeypatch):
    pipe = _pipeline("SimpleCNN", "device")
    _train("SimpleCNN", "device", tmp_path / "warm", n_epochs=1, pipeline=pipe, max_steps=1)      # the library and every kernel loaded
    torch.cuda.synchronize()
    solver, deq, cfg, opt, sched = pipe
    state = {"in_solver": 0, "phase": "before"}
    events = []
    real_solver, real_forward = deq.solver, deq.forward

    def solver_fn(*a, **k):                                                          # the solver's own per-iteration residual reads are its business
        state["in_solver"] += 1
        try:
            return real_solver(*a, **k)
        finally:
            state["in_solver"] -= 1

    def forward(*a, **k):
        out = real_forward(*a, **k)
        state["phase"] = "step"                                                      # from here: the loss, backward, optimizer.step()
        return out
    deq.solver, deq.forward = solver_fn, forward
    for name in ("item", "cpu", "tolist", "__float__"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _name=name, _orig=orig, **k):
            if self.is_cuda and state["phase"] == "step" and not state["in_solver"]:
                events.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (events.append("synchronize") if state["phase"] == "step" else None, real_sync(*a, **k))[1])

    def on_step(step):
        state["phase"] = "after"
    out = _train("SimpleCNN", "device", tmp_path / "spied", n_epochs=1, pipeline=pipe, max_steps=1, on_step=on_step)
    monkeypatch.undo()
    deq.solver, deq.forward = real_solver, real_forward
    assert len(out["steps"]) == 1 and math.isfinite(out["steps"][0].loss) and out["steps"][0].nonfinite == 0
    assert deq.last_backward_path == "device" and deq.last_parameter_path == "device"
    assert events == ["cpu"], events                                                 # the ONE read-back of stats


# ----------------------------------------------------------------------------- (e) against the reference's own training run
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "train_simplecnn.npz"))


@pytest.mark.parametrize("backend", ["autograd", "device"])
def test_training_run_against_the_reference(golden, backend, tmp_path_factory):
    """Step-1 loss and gradients within 1e-4 (the project's bound for one training step against the reference), every step's loss within
    1e-4 relative, and the update w_4 - w_0 within 4 x update_spread: Adam's first steps move every weight by about lr whatever the
    gradient's size, so the golden's generator measured how far the update moves under 1e-4 gradient noise (3 seeds; x 4 for that
    estimate).  The PSNR is 10 log10 of a mean squared error held to 1e-4 relative like the loss: 10 log10(1 + 1e-4) dB."""
    g = golden
    assert np.array_equal(g["order"], np.array(tc.ORDER)) and int(g["iters"]) == tc.ITERS and float(g["lr"]) == tc.LR
    assert float(g["spreads"].max()) <= 2 * float(g["spreads"].mean()) and float(g["update_spread"]) == float(g["spreads"].max())
    shipped = checkpoint.read_state_dict(checkpoint.shipped("cnn"))[0]
    r = _run("SimpleCNN", backend, tmp_path_factory)
    steps, solver = r["steps"], r["solver"]
    assert [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    names = [n for n, _ in solver.named_parameters()]
    assert names == [str(n) for n in g["names"]] and len(names) == 4
    figures = {}
    for k, s in enumerate(steps):
        figures[f"loss.{k}"] = abs(s.loss - float(g["loss"][k])) / float(g["loss"][k])
        figures[f"psnr.{k}"] = abs(s.psnr - float(g["psnr"][k]))
    for i, got in enumerate(r["opt"].first_grads):
        figures[f"grad.{i}"] = rel_l2(got.cpu().numpy(), g[f"grad.{i}"])
    updates = {}
    for i, (name, p) in enumerate(solver.named_parameters()):
        start = shipped[name]
        want = g[f"weight.{i}"].astype(np.float64) - start.numpy().astype(np.float64)
        updates[f"update.{i}"] = rel_l2(p.detach().cpu().numpy().astype(np.float64) - start.numpy().astype(np.float64), want)
        assert 0.5 * tc.LR < float(np.abs(want).max()) <= 4.5 * tc.LR                # four Adam steps of lr each, at most
    print(f"{backend}: " + ", ".join(f"{k} {v:.3e}" for k, v in {**figures, **updates}.items()), f"| update_spread {float(g['update_spread']):.3e}")
    for name, value in figures.items():
        assert value <= (10 * math.log10(1 + 1e-4) if name.startswith("psnr") else 1e-4), (name, value)
    for name, value in updates.items():
        assert value <= 4 * float(g["update_spread"]), (name, value)
    deq, cfg = r["deq"], r["cfg"]
    if backend == "device":
        assert (cfg.implicit_backward, cfg.parameter_backward, cfg.reasons) == ("device", "device", {})
        assert deq.last_backward_path == "device" and deq.last_parameter_path == "device"
        assert deq.backward_fallback_reason is None and deq.parameter_fallback_reason is None
        assert all(s.nonfinite == 0 for s in steps) and r["opt"].last_launches == 1
    else:
        assert (cfg.implicit_backward, cfg.parameter_backward, cfg.reasons) == ("autograd", "autograd", {})
        assert deq.last_backward_path == "autograd" and deq.last_parameter_path == "autograd"
    assert sorted(f for f in os.listdir(r["model"])) == ["epoch_0.ckpt", "epoch_1.ckpt"]


# ----------------------------------------------------------------------------- (f) resume
def test_resumed_training_gives_the_same_bits(tmp_path, tmp_path_factory):
    whole = _run("SimpleCNN", "device", tmp_path_factory)
    first = _train("SimpleCNN", "device", tmp_path / "first", n_epochs=1)
    assert [s.loss for s in first["steps"]] == [s.loss for s in whole["steps"][:2]]
    pipe = _pipeline("SimpleCNN", "device")
    solver, deq, cfg, opt, sched = pipe
    assert checkpoint.load_training(first["model"] + "epoch_0.ckpt", solver, opt, sched) == 0
    rest = _train("SimpleCNN", "device", tmp_path / "rest", n_epochs=2, pipeline=pipe, start_epoch=1)
    assert [(s.epoch, s.step) for s in rest["steps"]] == [(1, 0), (1, 1)]
    assert [(s.loss, s.psnr) for s in rest["steps"]] == [(s.loss, s.psnr) for s in whole["steps"][2:]]
    for a, b in zip(solver.parameters(), whole["solver"].parameters()):
        assert torch.equal(a, b)
    for a, b in zip(opt.state_dict()["state"].values(), whole["opt"].state_dict()["state"].values()):
        assert float(a["step"]) == float(b["step"]) == 4.0 and torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    obj = torch.load(first["model"] + "epoch_0.ckpt", map_location="cpu", weights_only=False)
    ref = torch.optim.Adam(solver.parameters(), lr=tc.LR)
    ref.load_state_dict(obj["optimizer_state_dict"])
    assert all(float(s["step"]) == 2.0 for s in ref.state.values()) and len(ref.state) == 4


# ----------------------------------------------------------------------------- the command line
def test_cli_trains_resumes_and_writes_the_reference_checkpoints(tmp_path, capsys):
    from deqsci_amd.cli import main
    d = tc.write(tmp_path / "data")
    save = str(tmp_path / "save") + "/"
    # a test clip of two measurements (the reference evaluates --testpath every save_every_n_steps steps and after every epoch)
    import scipy.io as sio
    mask, gt, meas = tc.samples()
    clips = tmp_path / "clips"
    os.makedirs(clips)
    sio.savemat(str(clips / "tiny_cacti.mat"), {"mask": mask, "meas": np.stack([meas[0], meas[1]], axis=2),
                                                "orig": np.concatenate([gt[0], gt[1]], axis=2).astype(np.float64)})
    first = checkpoint.read_state_dict(checkpoint.shipped("cnn"))[1] + 1          # the shipped archive carries its epoch: training continues behind it, as the reference
    base = ["--inference", "False", "--denoiser", "SimpleCNN", "--trainpath", d, "--savepath", save, "--and_maxiters", "6", "--batch_size", "2",
            "--lr", "1e-4", "--seed", "3"]
    steps = main(base + ["--loadpath", checkpoint.shipped("cnn"), "--n_epochs", str(first + 2), "--max_steps", "3", "--train_backend", "device",
                         "--testpath", str(clips) + "/", "--save_every_n_steps", "2"])
    assert [(s.epoch, s.step) for s in steps] == [(first, 0), (first, 1), (first + 1, 0)] and all(math.isfinite(s.loss) and s.nonfinite == 0 for s in steps)
    assert sorted(os.listdir(save + "model/")) == ["best.ckpt", f"epoch_{first}.ckpt", f"epoch_{first + 1}.ckpt"] and os.path.exists(save + "scalars.jsonl")
    out = capsys.readouterr().out
    assert "train backend device: implicit_backward=device parameter_backward=device" in out and "loaded dict!" in out
    assert out.count("saving best model") == 1 and out.count("Total Average PSNR") == 2          # after step 2 of epoch 0; after each epoch
    base += ["--testpath", str(tmp_path / "no_clips")]
    obj = torch.load(save + f"model/epoch_{first + 1}.ckpt", map_location="cpu", weights_only=False)
    assert obj["epoch"] == first + 1 and float(obj["optimizer_state_dict"]["state"][0]["step"]) == 3.0
    # --loadpath of a training checkpoint resumes at the epoch after it (the solver alone, as the reference), on the other backend here
    steps = main(base + ["--loadpath", save + f"model/epoch_{first + 1}.ckpt", "--n_epochs", str(first + 3), "--train_backend", "autograd"])
    assert [(s.epoch, s.step) for s in steps] == [(first + 2, 0), (first + 2, 1)] and all(s.nonfinite is None for s in steps)
    assert "train backend autograd: implicit_backward=autograd parameter_backward=autograd" in capsys.readouterr().out
    sd = torch.load(save + f"model/epoch_{first + 2}.ckpt", map_location="cpu", weights_only=False)["solver_state_dict"]
    assert all(not torch.equal(sd[k], obj["solver_state_dict"][k]) for k in sd)


# ----------------------------------------------------------------------------- (g) stale weights
@pytest.mark.parametrize("bsz", [1, 2])
def test_the_engine_sees_the_weights_device_adam_wrote(bsz):
    """The kernel writes the parameters through raw pointers; the engine rebuilds its packed weights when (data_ptr, _version) of a
    parameter changes.  Without the version bump in DeviceAdam.step the cached engine would reconstruct with the old weights."""
    mask, gt, meas = tc.samples()
    Phi = torch.from_numpy(np.float32(mask)).to(DEV)[None].repeat(bsz, 1, 1, 1).contiguous()
    y = torch.from_numpy(np.float32(meas[:bsz] / 255)).to(DEV)
    Ps = deqsci_amd.phi_sum(Phi)

    def reconstruct(deq):
        with torch.no_grad():
            return deq(y, Phi, Ps, initial_point=deqsci_amd.initial_point(y, Phi, Ps, None)).clone()
    solver, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 6)
    before = reconstruct(deq)
    assert torch.equal(reconstruct(deq), before)                                    # (batch 1: the second call replays the captured graph)
    engine = deq._engine[1]
    opt = DeviceAdam(solver.parameters(), lr=1e-2)
    gen = torch.Generator(DEV).manual_seed(1)
    for p in solver.parameters():
        p.grad = torch.randn(p.shape, device=DEV, generator=gen)
    opt.step()
    after = reconstruct(deq)
    assert deq._engine[1] is engine                                                 # the cached engine, not a new one
    fresh_solver, fresh = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 6)
    fresh_solver.load_state_dict(solver.state_dict())
    want = reconstruct(fresh)
    assert not torch.equal(after, before) and rel_l2(after.cpu().numpy(), before.cpu().numpy()) > 1e-3
    assert torch.equal(after, want)
    assert torch.equal(reconstruct(deq), want)                                      # and the replay after the rebuild


# ----------------------------------------------------------------------------- (h) the train-mode families
@pytest.mark.parametrize("kind", ["ffdnet", "RealSN_SimpleCNN"])
def test_train_mode_denoisers_on_the_device_backend(kind, tmp_path):
    """Two steps at the same shapes: finite losses within 1e-4 of the same steps under backend="autograd"; the paths configure_training
    reports are the ones that ran; the checkpoint carries the buffers the f-calls moved.  FFDNet's implicit backward stays on autograd:
    vjp.eligibility refuses a train-mode BatchNorm2d (the backward kernels are not this feature's to change), and the report says so."""
    runs = {b: _train(kind, b, tmp_path / b, n_epochs=1) for b in ("autograd", "device")}
    dev, ref = runs["device"], runs["autograd"]
    for a, b in zip(dev["steps"], ref["steps"]):
        print(f"{kind} step {a.step}: loss device {a.loss:.6e} autograd {b.loss:.6e} rel {abs(a.loss - b.loss) / b.loss:.2e}; PSNR {a.psnr:.4f} / {b.psnr:.4f}")
    assert len(dev["steps"]) == len(ref["steps"]) == 2
    for a, b in zip(dev["steps"], ref["steps"]):
        assert math.isfinite(a.loss) and a.nonfinite == 0 and abs(a.loss - b.loss) <= 1e-4 * b.loss, (a, b)
    deq, cfg = dev["deq"], dev["cfg"]
    assert deq.last_parameter_path == "device" and deq.parameter_fallback_reason is None
    info = deq._engine[1].last_info
    if kind == "ffdnet":
        assert (cfg.implicit_backward, cfg.parameter_backward, cfg.engine_options) == ("autograd", "device+bn-train", {"train_bn": "device"})
        assert list(cfg.reasons) == ["implicit_backward"] and "BatchNorm2d in train mode" in cfg.reasons["implicit_backward"]
        assert deq.last_backward_path == "autograd" and info["denoiser_path"] == "train bn per layer" and info["train_bn"] == "device"
        moved = [n for n, _ in dev["solver"].named_buffers() if "running_" in n or "num_batches_tracked" in n]
        assert len(moved) == 39
    else:
        assert (cfg.implicit_backward, cfg.parameter_backward, cfg.engine_options) == ("device+realsn", "device+realsn", {"train_realsn": "device"})
        assert cfg.reasons == {} and deq.last_backward_path == "device" and deq.backward_fallback_reason is None
        assert info["denoiser_path"] == "train realsn per layer" and info["train_realsn"] == "device"
        moved = [n for n, _ in dev["solver"].named_buffers() if n.endswith("weight_u")]
        assert len(moved) == 4
    assert ref["deq"].last_parameter_path == "autograd" and ref["deq"].last_backward_path == "autograd"
    # the checkpoint carries the moved buffers, and load_training puts them back
    sd = dev["solver"].state_dict()
    fresh_solver, fresh_deq, _, fresh_opt, fresh_sched = _pipeline(kind, "device")
    shipped = {k: v.clone() for k, v in fresh_solver.state_dict().items()}
    for n in moved:
        assert not torch.equal(sd[n], shipped[n]), n
    assert checkpoint.load_training(dev["model"] + "epoch_0.ckpt", fresh_solver, fresh_opt, fresh_sched) == 0
    for (n, a), (_, b) in zip(fresh_solver.state_dict().items(), sd.items()):
        assert torch.equal(a, b), n
    assert all(float(s["step"]) == 2.0 for s in fresh_opt.state_dict()["state"].values())
