"""GPU: gradient clipping by global norm - csrc/train.hip's L3 (norm), L3s (scale) and L2c (the clipped Adam step) against
tests/clip_ref.py BIT FOR BIT, the skipped step, the step's read-backs and train_solver_sci(clip_grad_norm=...) on the tiny training set."""
import math
import os

import numpy as np
import pytest
import torch

import clip_ref as cr
import train_cases as tc
import train_ref as tr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip, checkpoint, training
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.optim import DeviceAdam, adam_reference_step_, clip_grad_norm_

DEV = "cuda"
SENT = 7.25                                                    # the sentinel around every buffer a kernel writes
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193]                   # below a float4, the chunk's edges, more than one workgroup, a ragged third chunk
BETAS, EPS = (0.9, 0.999), 1e-8
MAX_NORM = 1.0


def _values(n, rng):
    return (rng.randn(n) * 10.0 ** rng.uniform(-6, 3, size=n)).astype(np.float32)


def _layout(sizes, off):
    """-> the starts of the tensors in one flat buffer and its length: every start `off` floats past a 16-byte boundary, sentinels between"""
    starts, o = [], 4
    for n in sizes:
        starts.append(o + off)
        o += -(-(n + off + 1) // 4) * 4
    return starts, o + 4


def _flat(arrays, off):
    """numpy fp32 arrays -> (the flat device buffer, its views, the host copy of the buffer)"""
    starts, total = _layout([a.size for a in arrays], off)
    host = np.full(total, SENT, np.float32)
    for a, s in zip(arrays, starts):
        host[s:s + a.size] = a
    buf = torch.from_numpy(host.copy()).to(DEV)
    views = [buf[s:s + a.size] for a, s in zip(arrays, starts)]
    assert all(v.data_ptr() % 16 == 4 * off for v in views)
    return buf, views, host


def _norm(views, max_norm=MAX_NORM):
    """-> stats (3 + n,) as numpy, the sentinels around it checked"""
    n = len(views)
    sbuf = torch.full((n + 5,), SENT, device=DEV, dtype=torch.float64)
    stats = _hip.grad_norm(views, max_norm, stats=sbuf[1:n + 4])
    assert stats.data_ptr() == sbuf.data_ptr() + 8
    s = sbuf.cpu().numpy()
    assert s[0] == SENT and s[-1] == SENT
    return s[1:n + 4]


_LISTS = {}


def _list(n_tensors):
    """n_tensors gradients over SIZES, their restated statistics and the exact sum of squares: computed once, never modified"""
    if n_tensors not in _LISTS:
        rng = np.random.RandomState(n_tensors)
        grads = [_values(SIZES[(i * 3 + n_tensors) % len(SIZES)], rng) for i in range(n_tensors)]
        for g in grads:
            g.setflags(write=False)
        _LISTS[n_tensors] = (grads, cr.grad_stats(grads, MAX_NORM), cr.exact_sum_of_squares(grads))
    return _LISTS[n_tensors]


# ----------------------------------------------------------------------------- (a) L3
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("size", SIZES)
def test_grad_norm_of_one_tensor_equals_the_restated_order(size, off):
    g = _values(size, np.random.RandomState(size))
    want = cr.grad_stats([g], MAX_NORM)
    buf, views, host = _flat([g], off)
    stats = _norm(views)
    assert np.array_equal(stats, want), (stats, want)                               # float64, bit for bit
    assert stats[0] == stats[3] and stats[2] == 0.0 and stats[1] == float(np.float32(min(1.0, MAX_NORM / (stats[0] + 1e-6))))
    exact = cr.exact_sum_of_squares([g])
    assert abs(cr.tensor_sums([g])[0][0] - exact) <= size * 2.0 ** -53 * exact      # any order of a sum of non-negative float64 terms
    assert np.array_equal(_norm(views), stats) and np.array_equal(buf.cpu().numpy(), host)      # run to run; the gradient is only read


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_grad_norm_of_more_chunks_than_a_workgroup_has_threads(off):
    """257 chunks and three elements: the fold's thread 0 and thread 1 add two partials each (stage 2's second trip)"""
    if "big" not in _LISTS:
        g = _values(257 * tr.CHUNK + 3, np.random.RandomState(257))
        g.setflags(write=False)
        _LISTS["big"] = (g, cr.grad_stats([g], MAX_NORM), cr.exact_sum_of_squares([g]))
    g, want, exact = _LISTS["big"]
    _, views, _ = _flat([g, g[:5]], off)
    stats = _norm(views[:1])
    assert np.array_equal(stats, want), (stats, want)
    assert abs(stats[0] ** 2 - exact) <= (g.size + 2) * 2.0 ** -53 * exact
    assert np.array_equal(_norm(views)[[3, 4]], np.array([want[3], cr.grad_stats([g[:5]], MAX_NORM)[3]]))     # the tensor behind it starts at chunk 258


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n_tensors", [1, 64, 65, 130])
def test_grad_norm_of_a_list_equals_the_restated_order(n_tensors, off):
    grads, want, exact = _list(n_tensors)
    n = sum(g.size for g in grads)
    buf, views, host = _flat(grads, off)
    stats = _norm(views)
    assert np.array_equal(stats, want), (stats[:3], want[:3], int((stats != want).sum()))
    assert stats[2] == 0.0 and 0.0 < stats[1] <= 1.0 and (n_tensors == 1 or stats[1] < 1.0) and _hip.grad_norm_launches(n_tensors) == 2 * -(-n_tensors // tr.ADAM_MAX_TENSORS) + 1
    assert abs(stats[0] ** 2 - exact) <= (n + 2) * 2.0 ** -53 * exact               # (+ the root and its square)
    sums, _ = cr.tensor_sums(grads)
    total = 0.0
    for s in sums:
        total += s
    assert abs(total - exact) <= n * 2.0 ** -53 * exact and stats[0] == math.sqrt(total)
    assert np.array_equal(_norm(views), stats) and np.array_equal(buf.cpu().numpy(), host)
    # the wrapper's own buffers; a caller's workspace
    assert np.array_equal(_hip.grad_norm(views, MAX_NORM).cpu().numpy(), want)
    ws = _hip.grad_norm_workspace(views)
    assert ws.numel() == 2 * (sum(-(-g.size // tr.CHUNK) for g in grads) + n_tensors)
    assert np.array_equal(_hip.grad_norm(views, MAX_NORM, workspace=ws.fill_(float("nan"))).cpu().numpy(), want)      # no initialisation needed
    with pytest.raises(_hip.DeqsciHipError, match="workspace too small"):
        _hip.grad_norm(views, MAX_NORM, workspace=ws[:-1])
    if n_tensors == 65:                                                             # other limits: the same norm, another coefficient
        for max_norm in (1e30, 0.0, float("inf")):
            assert np.array_equal(_norm(views, max_norm), cr.grad_stats(grads, max_norm))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_grad_norm_of_zeros_gives_coef_one(off):
    grads = [np.zeros(n, np.float32) for n in SIZES]
    _, views, _ = _flat(grads, off)
    stats = _norm(views, 0.5)
    assert np.array_equal(stats, np.array([0.0, 1.0, 0.0] + [0.0] * len(SIZES))) and np.array_equal(stats, cr.grad_stats(grads, 0.5))


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("turn", [0, 1, 2])
def test_grad_norm_counts_nan_and_inf(turn, off):
    """NaN, +Inf and -Inf in a first element, a last element and an element of a ragged tail (8193 = two chunks and one element; 4097;
    5 = one float4 and one element), every value in every place over the three turns."""
    rng = np.random.RandomState(40 + turn)
    grads = [_values(n, rng) for n in (8193, 4097, 5, 4096)]
    bad = [float("nan"), float("inf"), -float("inf")]
    bad = bad[turn:] + bad[:turn]
    grads[0][0], grads[1][-1], grads[2][4], grads[0][8192] = bad[0], bad[1], bad[2], bad[0]
    count = sum(int((~np.isfinite(g)).sum()) for g in grads)
    assert count == 4
    _, views, _ = _flat(grads, off)
    stats = _norm(views)
    want = cr.grad_stats(grads, MAX_NORM)
    assert stats[2] == float(count) == want[2] and not math.isfinite(stats[0])
    assert np.array_equal(stats, want, equal_nan=True)
    assert np.isfinite(stats[6]) and stats[6] == want[6]                            # the tensor without one keeps its norm: the first diagnostic


# ----------------------------------------------------------------------------- (b) L3s
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_clip_grad_norm_scales_in_place_and_leaves_a_non_finite_gradient_alone(off):
    grads, want, _ = _list(65)
    buf, views, host = _flat(grads, off)
    params = [torch.nn.Parameter(torch.zeros(g.size, device=DEV)) for g in grads]
    for p, v in zip(params, views):
        p.grad = v
    norm = clip_grad_norm_(params, MAX_NORM)
    assert norm.is_cuda and norm.dim() == 0 and norm.dtype == torch.float64 and float(norm) == want[0]
    starts, _ = _layout([g.size for g in grads], off)
    for g, s in zip(cr.clipped(grads, want[1]), starts):
        host[s:s + g.size] = g
    assert np.array_equal(buf.cpu().numpy(), host)                                  # g * coef, one rounding; every sentinel
    assert float(np.abs(host[starts[0]:starts[0] + grads[0].size] - grads[0]).max()) > 0
    # already within the limit: nothing moves; a NaN: nothing moves either
    stats = clip_grad_norm_(params, 1e30, return_stats=True).cpu().numpy()
    assert stats[1] == 1.0 and np.array_equal(buf.cpu().numpy(), host)
    views[64][0] = float("inf")
    host[starts[64]] = np.inf
    stats = clip_grad_norm_(params, 1e-3, return_stats=True).cpu().numpy()
    assert stats[2] == 1.0 and np.array_equal(buf.cpu().numpy(), host)
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(params, 1e-3, error_if_nonfinite=True)
    with pytest.raises(NotImplementedError, match="norm_type"):
        clip_grad_norm_(params, 1.0, norm_type=1)


# ----------------------------------------------------------------------------- (c) L2c
def _adam_problem(n_tensors, off, seed):
    rng = np.random.RandomState(seed)
    sizes = [SIZES[(i * 5 + 1) % len(SIZES)] for i in range(n_tensors)]
    p0 = [rng.randn(n).astype(np.float32) for n in sizes]
    zeros = [np.zeros(n, np.float32) for n in sizes]
    dev = {k: _flat(a, off) for k, a in (("p", p0), ("g", zeros), ("m", zeros), ("v", zeros))}
    starts, _ = _layout(sizes, off)
    return rng, sizes, starts, p0, dev


def test_clipped_adam_step_equals_the_reference_step_on_the_scaled_gradient():
    n_tensors = tr.ADAM_MAX_TENSORS + 1
    rng, sizes, starts, p0, dev = _adam_problem(n_tensors, 1, seed=12)
    host = {k: [torch.from_numpy(a.copy()) for a in (p0 if k == "p" else [np.zeros(n, np.float32) for n in sizes])] for k in "pmv"}
    coefs = []
    for t, lr, scale in ((1, 1e-3, 1.0), (2, 1e-3, 1.0), (3, 2.5e-4, 1e-9)):
        grads = [_values(n, rng) * np.float32(scale) for n in sizes]
        for view, g in zip(dev["g"][1], grads):
            view.copy_(torch.from_numpy(g))
        g_before = dev["g"][0].cpu().numpy()
        stats = _hip.grad_norm(dev["g"][1], MAX_NORM)
        launches = _hip.adam_step(dev["p"][1], dev["g"][1], dev["m"][1], dev["v"][1], t, lr, BETAS, EPS, stats=stats)
        assert launches == 2
        want = cr.grad_stats(grads, MAX_NORM)
        assert np.array_equal(stats.cpu().numpy(), want)
        coefs.append(want[1])
        for i, g in enumerate(cr.clipped(grads, want[1])):
            adam_reference_step_(host["p"][i], torch.from_numpy(g), host["m"][i], host["v"][i], t, lr, BETAS, EPS)
        for k in "pmv":                                                             # the whole buffers: every tensor, every sentinel
            expect = dev[k][2]
            for a, s in zip(host[k], starts):
                expect[s:s + a.numel()] = a.numpy()
            got = dev[k][0].cpu().numpy()
            assert np.array_equal(got, expect), (t, k, int((got != expect).sum()))
        assert np.array_equal(dev["g"][0].cpu().numpy(), g_before)                  # the gradient is not written
    assert coefs[0] < 1.0 and coefs[1] < 1.0 and coefs[2] == 1.0                    # the third step: within the limit, L2's own arithmetic
    assert float(np.abs(host["p"][0].numpy() - p0[0]).max()) > 0


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
def test_a_non_finite_gradient_leaves_every_word_as_it_was(off):
    rng, sizes, starts, p0, dev = _adam_problem(tr.ADAM_MAX_TENSORS + 1, off, seed=13)
    for view, n in zip(dev["g"][1], sizes):
        view.copy_(torch.from_numpy(_values(n, rng)))
    stats = _hip.grad_norm(dev["g"][1], MAX_NORM)
    _hip.adam_step(dev["p"][1], dev["g"][1], dev["m"][1], dev["v"][1], 1, 1e-3, BETAS, EPS, stats=stats)
    before = {k: dev[k][0].cpu().numpy() for k in "pgmv"}
    assert not np.array_equal(before["p"], dev["p"][2]) and float(np.abs(before["v"]).max()) > 0
    dev["g"][1][64][sizes[64] - 1] = float("nan")                                   # the last element of the second table's only tensor
    before["g"] = dev["g"][0].cpu().numpy()
    stats = _hip.grad_norm(dev["g"][1], MAX_NORM)
    _hip.adam_step(dev["p"][1], dev["g"][1], dev["m"][1], dev["v"][1], 2, 1e-3, BETAS, EPS, stats=stats)
    assert float(stats[2]) == 1.0
    for k in "pgmv":
        assert np.array_equal(dev[k][0].cpu().numpy(), before[k], equal_nan=True), k


def test_device_adam_with_clipping(monkeypatch):
    grads, want, _ = _list(65)
    rng = np.random.RandomState(3)
    p0 = [rng.randn(g.size).astype(np.float32) for g in grads]

    def optimizer(**kw):
        params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(DEV)) for p in p0]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g.copy()).to(DEV)
        return params, DeviceAdam([{"params": params[:3]}, {"params": params[3:], "lr": 5e-4}], lr=1e-3, betas=BETAS, eps=EPS, **kw)
    params, opt = optimizer(max_grad_norm=MAX_NORM)
    calls = []
    lib = _hip.load()
    for name in ("deqsci_adam_step_f32", "deqsci_adam_step_clipped_f32", "deqsci_grad_norm_f32"):
        monkeypatch.setattr(lib, name, lambda *a, _real=getattr(lib, name), _name=name: (calls.append((_name, a[1])), _real(*a))[1])
    versions = [p._version for p in params]
    opt.step()
    # one norm over both groups (5 launches for 65 tensors), then L2c per group and table
    assert calls == [("deqsci_grad_norm_f32", 65), ("deqsci_adam_step_clipped_f32", 3), ("deqsci_adam_step_clipped_f32", 62)] and opt.last_launches == 5 + 2
    assert opt.last_grad_stats.is_cuda and np.array_equal(opt.last_grad_stats.cpu().numpy(), want) and opt.grad_norm() == want[0]
    for i, (p, g) in enumerate(zip(params, cr.clipped(grads, want[1]))):
        hp, hm, hv = tr.adam_f32_step(p0[i], g, np.zeros_like(g), np.zeros_like(g), 1, 1e-3 if i < 3 else 5e-4, BETAS, EPS)
        st = opt.state[p]
        assert np.array_equal(p.detach().cpu().numpy(), hp) and np.array_equal(st["exp_avg"].cpu().numpy(), hm) and np.array_equal(st["exp_avg_sq"].cpu().numpy(), hv)
        assert np.array_equal(p.grad.cpu().numpy(), grads[i]) and p._version > versions[i] and float(st["step"]) == 1.0      # p.grad is not written
    # a norm below max_norm: the bits of DeviceAdam without clipping
    pa, oa = optimizer(max_grad_norm=1e30)
    pb, ob = optimizer()
    del calls[:]
    for _ in range(2):
        oa.step()
        ob.step()
    assert [c[0] for c in calls].count("deqsci_adam_step_f32") == 4 and ob.last_launches == 2 and ob.last_grad_stats is None
    assert float(oa.last_grad_stats[1].cpu()) == 1.0
    for x, y in zip(pa, pb):
        assert torch.equal(x, y) and torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]) and torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
    # one NaN: nothing changes but `step`; the state still loads into torch.optim.Adam
    kept = [(p.detach().clone(), oa.state[p]["exp_avg"].clone(), oa.state[p]["exp_avg_sq"].clone()) for p in pa]
    pa[7].grad.view(-1)[0] = float("nan")
    oa.step()
    assert float(oa.last_grad_stats[2].cpu()) == 1.0 and math.isnan(oa.grad_norm())
    for p, (p_, m_, v_) in zip(pa, kept):
        st = oa.state[p]
        assert torch.equal(p.detach(), p_) and torch.equal(st["exp_avg"], m_) and torch.equal(st["exp_avg_sq"], v_) and float(st["step"]) == 3.0
    ref = torch.optim.Adam([{"params": pa[:3]}, {"params": pa[3:]}], lr=1e-3)
    ref.load_state_dict(oa.state_dict())
    assert float(ref.state[pa[0]]["step"]) == 3.0 and "max_grad_norm" not in oa.state_dict()["param_groups"][0]
    # refused: parameters on the device and on the host under one norm
    mixed = DeviceAdam([pa[0], torch.nn.Parameter(torch.zeros(3))], lr=1e-3, max_grad_norm=1.0)
    mixed.param_groups[0]["params"][1].grad = torch.ones(3)
    with pytest.raises(NotImplementedError, match="2 devices"):
        mixed.step()


# ----------------------------------------------------------------------------- the loop on the tiny training set (tests/test_train_gpu.py's smallest)
def _pipeline(watch=False):
    solver, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), tc.ITERS)
    solver.nonlinear_op.train()
    training.configure_training(deq, "device")

    class Watched(DeviceAdam):
        """keeps the gradients of its first step"""
        first_grads = None

        def step(self, closure=None):
            if self.first_grads is None:
                self.first_grads = [p.grad.detach().clone() for g in self.param_groups for p in g["params"] if p.grad is not None]
            return super().step(closure)
    opt = (Watched if watch else DeviceAdam)(solver.parameters(), lr=tc.LR)
    return solver, deq, opt


def _train(tmp, pipeline=None, max_steps=2, **kw):
    directory = tc.write(tmp / "data")
    model = str(tmp / "model") + "/"
    os.makedirs(model, exist_ok=True)
    solver, deq, opt = pipeline or _pipeline()
    ds = training.SCITrainingDatasetSubset(directory + "gt/", directory + "measurement/", directory + "mask.mat")
    loader = torch.utils.data.DataLoader(ds, batch_size=tc.BATCH, sampler=tc.RecordedSampler(start=0), drop_last=True)
    steps = training.train_solver_sci(solver, loader, opt, model, "device", 1, deq, print_every_n_steps=1, save_every_n_steps=1000, tflog_path=model,
                                      max_steps=max_steps, **kw)
    import json
    rows = [json.loads(ln) for ln in open(model + "scalars.jsonl")]
    return {"solver": solver, "deq": deq, "opt": opt, "steps": steps, "rows": rows}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _train(tmp_path_factory.mktemp("clip_plain"))


def test_a_huge_clip_gives_the_bits_of_a_run_without(plain, tmp_path):
    r = _train(tmp_path, clip_grad_norm=1e30)
    assert len(r["steps"]) == 2 and [s.loss for s in r["steps"]] == [s.loss for s in plain["steps"]] and [s.psnr for s in r["steps"]] == [s.psnr for s in plain["steps"]]
    for a, b in zip(r["solver"].parameters(), plain["solver"].parameters()):
        assert torch.equal(a, b)
    assert r["opt"].max_grad_norm == 1e30 and plain["opt"].max_grad_norm is None and plain["opt"].last_launches == 1
    assert r["opt"].last_launches == 3 + 1                                          # L3 of four tensors, L2c
    assert all(row["main/skipped"] == 0 and math.isfinite(row["main/grad_norm"]) and row["main/grad_norm"] > 0 for row in r["rows"])
    assert "main/grad_norm" not in plain["rows"][0]
    again = _train(tmp_path / "again", clip_grad_norm=1e30)                         # run to run
    assert [row["main/grad_norm"] for row in again["rows"]] == [row["main/grad_norm"] for row in r["rows"]]


def test_a_small_clip_gives_the_restated_update_of_the_unclipped_gradient(tmp_path):
    shipped = checkpoint.read_state_dict(checkpoint.shipped("cnn"))[0]
    pipe = _pipeline(watch=True)
    r = _train(tmp_path, pipeline=pipe, max_steps=1, clip_grad_norm=1e-3)
    grads = [g.cpu().numpy() for g in r["opt"].first_grads]
    names = [n for n, _ in r["solver"].named_parameters()]
    assert len(grads) == len(names) == 4
    want = cr.grad_stats([g.ravel() for g in grads], 1e-3)
    assert want[0] > 1e-3 and want[1] < 1.0 and want[2] == 0.0
    assert np.array_equal(r["opt"].last_grad_stats.cpu().numpy(), want) and r["rows"][0]["main/grad_norm"] == want[0] and r["rows"][0]["main/skipped"] == 0
    for (name, p), g in zip(r["solver"].named_parameters(), grads):
        assert np.array_equal(p.grad.cpu().numpy(), g)                              # read back unclipped: L2c does not write p.grad
        start = shipped[name].numpy()
        hp, _, _ = tr.adam_f32_step(start.ravel(), g.ravel() * np.float32(want[1]), np.zeros(g.size, np.float32), np.zeros(g.size, np.float32), 1, tc.LR, BETAS, EPS)
        assert np.array_equal(p.detach().cpu().numpy().ravel(), hp), name


# ----------------------------------------------------------------------------- no synchronisation beyond the solver's and the two read-backs
def test_a_clipped_step_reads_back_twice_the_second_time_behind_the_adam_launch(tmp_path, monkeypatch):
    """tests/test_train_gpu.py's spying scheme: every device read between the end of deq.forward and on_step, outside the solver."""
    pipe = _pipeline()
    _train(tmp_path / "warm", pipeline=pipe, max_steps=1, clip_grad_norm=1.0)      # the library and every kernel loaded
    torch.cuda.synchronize()
    solver, deq, opt = pipe
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
        state["phase"] = "step"                                                      # from here: the loss, backward, optimizer.step(), the statistics
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
    lib = _hip.load()
    real_adam, real_norm = lib.deqsci_adam_step_clipped_f32, lib.deqsci_grad_norm_f32
    monkeypatch.setattr(lib, "deqsci_adam_step_clipped_f32", lambda *a: (events.append("L2c"), real_adam(*a))[1])
    monkeypatch.setattr(lib, "deqsci_grad_norm_f32", lambda *a: (events.append("L3"), real_norm(*a))[1])
    real_step = opt.step

    def step(*a, **k):
        events.append("step>")
        try:
            return real_step(*a, **k)
        finally:
            events.append("<step")
    opt.step = step

    def on_step(s):
        state["phase"] = "after"
    out = _train(tmp_path / "spied", pipeline=pipe, max_steps=1, on_step=on_step, clip_grad_norm=1.0)
    monkeypatch.undo()
    del opt.step
    deq.solver, deq.forward = real_solver, real_forward
    assert len(out["steps"]) == 1 and math.isfinite(out["steps"][0].loss) and out["steps"][0].nonfinite == 0
    assert deq.last_backward_path == "device" and deq.last_parameter_path == "device"
    assert [e for e in events if e in ("item", "cpu", "tolist", "__float__", "synchronize")] == ["cpu", "cpu"], events
    assert events == ["cpu", "step>", "L3", "L2c", "<step", "cpu"], events          # DeviceAdam.step() itself reads back nothing
