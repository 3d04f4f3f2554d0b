"""GPU: several iteration horizons (snapshots=) and a residual / PSNR trace (trace=) out of ONE DEQ run - the squared-error kernel
against float64, every snapshot against the separate run bit for bit, the reference's own runs at several horizons from one run,
the trace against the snapshots, and the harness / CLI layers.  Tolerances of the golden comparisons are those tests/test_gpu_parity.py
applies to the same files: 1e-4 relative L2, 0.01 dB, 2 % of the residual."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint, harness
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.engine import DEQSCIEngine
    from oracle import deqsci_oracle as orc

DEV = "cuda"


# ----------------------------------------------------------------------------- 1. the kernel
def _sqerr_want(x, gt, clamp):
    d = (x.clamp(0, 1) if clamp else x) - gt
    return (d * d).double().sum(1)


@pytest.mark.parametrize("bsz,N", [(1, 5), (3, 7), (8, 4095), (64, 4097), (3, 65538), (8, 256 * 256 * 8), (64, (1 << 20) + 3), (1, 1 << 22),
                                    (3, (1 << 22) + 1)])
def test_sqerr_rows_against_float64(bsz, N):
    """Both sides sum the same fp32 terms in float64: they differ by summation order only, relative bound N 2^-53 <= 5e-10; gate 1e-9."""
    g = torch.Generator(device=DEV).manual_seed(bsz * 1000003 + N)
    x = torch.rand(bsz, N, device=DEV, generator=g) * 1.6 - 0.3                  # values outside [0,1] on both sides
    gt = torch.rand(bsz, N, device=DEV, generator=g)
    for clamp in (True, False):
        got = _hip.sqerr_rows(x, gt, clamp_x=clamp)
        want = _sqerr_want(x, gt, clamp)
        rel = ((got - want).abs() / want).max().item()
        print(f"sqerr bsz={bsz} N={N} clamp={clamp}: max rel {rel:.3e}")
        assert got.dtype == torch.float64 and rel < 1e-9
        assert torch.equal(got, _hip.sqerr_rows(x, gt, clamp_x=clamp))           # run twice: bit-identical
    # rows of a history slot: m * N apart (whatever that does to their alignment), same values -> same bits as the dense rows
    hist = torch.zeros(bsz, 3, N, device=DEV)
    hist[:, 1] = x
    assert torch.equal(_hip.sqerr_rows(hist[:, 1], gt), _hip.sqerr_rows(x, gt))
    # a NaN makes its own sample NaN, no other
    s = bsz // 2
    x[s, N // 2] = float("nan")
    got = _hip.sqerr_rows(x, gt)
    assert torch.isnan(got[s]) and int(torch.isnan(got).sum()) == 1
    x[s, N // 2] = 0.5
    x[s, N - 1] = float("nan")                                                  # ... in the scalar tail too
    got = _hip.sqerr_rows(x, gt)
    assert torch.isnan(got[s]) and int(torch.isnan(got).sum()) == 1


def test_sqerr_rows_edges():
    e = torch.empty(0, 16, device=DEV)
    assert _hip.sqerr_rows(e, e).shape == (0,)
    z = torch.empty(4, 0, device=DEV)
    assert torch.equal(_hip.sqerr_rows(z, z), torch.zeros(4, dtype=torch.float64, device=DEV))
    x = torch.full((2, 9), 2.0, device=DEV)
    gt = torch.zeros(2, 9, device=DEV)
    assert _hip.sqerr_rows(x, gt).tolist() == [9.0, 9.0] and _hip.sqerr_rows(x, gt, clamp_x=False).tolist() == [36.0, 36.0]
    with pytest.raises(_hip.DeqsciHipError):
        _hip.sqerr_rows(x.cpu(), gt.cpu())
    with pytest.raises(_hip.DeqsciHipError):
        _hip.sqerr_rows(x, gt[:, :8])


# ----------------------------------------------------------------------------- data
def _clip(name):
    d = orc.load_clip(os.path.join(orc.DATA_DIR, name))
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _batch(n):
    """(y (n,H,W), Phi (n,H,W,B), gt (n,H,W,B)) on the device: traffic m0 for n = 1; the eight shipped measurements for n = 8."""
    t = _clip("traffic_cacti.mat")
    if n == 1:
        picks = [(t, 0)]
    else:
        picks = [(_clip("drop8_cacti.mat"), 0), (_clip("runner8_cacti.mat"), 0)] + [(t, i) for i in range(6)]
    y = torch.stack([c["meas"][..., i] for c, i in picks]).contiguous().to(DEV)
    Phi = torch.stack([c["mask"] for c, _ in picks]).contiguous().to(DEV)
    gt = torch.stack([c["gt"][..., 8 * i:8 * i + 8] for c, i in picks]).contiguous().to(DEV)
    return y, Phi, gt


def _net(kind):
    solver, _ = build_pipeline(kind, checkpoint.shipped("ffdnet_gray" if kind == "ffdnet" else "cnn"), 10)
    return solver.nonlinear_op


def _engine(net, iterator, max_iter):
    return DEQSCIEngine(net, iterator=iterator, max_iter=max_iter, lam=1e-2, tol=1e-5)


def _psnr_rows(rec, gt):
    d = rec.clamp(0, 1) - gt
    return 10.0 * np.log10(1.0 / (d * d).double().mean(dim=(1, 2, 3)).cpu().numpy())


# ----------------------------------------------------------------------------- 2. + 4. snapshot = separate run; trace rows
@pytest.mark.parametrize("bsz", [1, 8])
@pytest.mark.parametrize("iterator", ["anderson", "picard"])
@pytest.mark.parametrize("kind", ["SimpleCNN", "ffdnet"])
def test_snapshot_is_the_separate_run_bit_for_bit(kind, iterator, bsz):
    """One run to 40 with snapshots (3, 10, 30) against engines built with max_iter = 3, 10, 30: torch.equal reconstructions, equal residual
    rows; one measurement per call takes the replayed hipGraph from the second call of the shape on (calls 2 and 3 are checked too), eight
    the eager path.  The main result is the result without the options.  The trace's residual row K - 1 (Picard: K) is the residual the
    run to K reports; for SimpleCNN (no sigma: F_{K-1} IS the horizon-K reconstruction) the trace PSNR of f-call K - 1 equals the PSNR of
    snapshot K to 0.01 dB - largest difference measured on an MI355X over all cases: 3.6e-15 dB (float64 rounding; the line printed below)."""
    net = _net(kind)
    y, Phi, gt = _batch(bsz)
    horizons = (3, 10, 30)
    eng = _engine(net, iterator, 40)
    plain = eng.reconstruct(y, Phi)
    assert eng.last_info["snapshots"] is None and eng.last_info["trace"] is None
    res_plain = eng.last_info["res"]
    want = {}
    for K in horizons:
        e = _engine(net, iterator, K)
        want[K] = (e.reconstruct(y, Phi), e.last_info["res"], e.last_info["res_per_sample"])
    worst = 0.0
    for call in range(3):
        rec = eng.reconstruct(y, Phi, snapshots=horizons, trace=True, gt=gt)
        info = eng.last_info
        # (SimpleCNN under Picard leaves fp16's range before iteration 40: conv64="auto" then redoes the WHOLE run eagerly on the fp32 kernels,
        # and the trace is that run's; the runs to 3, 10 and 30 stay finite and keep the split-fp16 kernels - and so must their snapshots)
        fb = info["conv64_fallback"] is not None
        assert fb or info["graph"] is (bsz == 1 and call > 0), (call, info["graph"])
        assert torch.equal(rec, plain) and (info["res"] == res_plain or (fb and not np.isfinite(res_plain)))
        assert sorted(info["snapshots"]) == list(horizons)
        tr = info["trace"]
        n_calls = 40 if iterator == "anderson" else 41
        assert tr["res"].shape == (n_calls,) and tr["res_per_sample"].shape == (n_calls, bsz) and tr["psnr"].shape == (n_calls, bsz)
        assert tr["res"].dtype == np.float64 and tr["psnr"].dtype == np.float64 and (fb or np.isfinite(tr["psnr"]).all())
        assert tr["res"][-1] == res_plain or (fb and not np.isfinite(res_plain))
        for K in horizons:
            s = info["snapshots"][K]
            w_rec, w_res, w_per = want[K]
            assert torch.equal(s["rec"], w_rec), (K, call, float((s["rec"] - w_rec).abs().max()))
            assert s["res"] == w_res and s["res_per_sample"] == w_per, (K, call)
            if fb:
                continue
            row = K - 1 if iterator == "anderson" else K
            assert tr["res"][row] == w_res and tr["res_per_sample"][row].tolist() == w_per
            if kind == "SimpleCNN":
                diff = np.abs(tr["psnr"][row] - _psnr_rows(s["rec"], gt)).max()
                worst = max(worst, float(diff))
                assert diff < 0.01, (K, diff)
    print(f"trace PSNR vs snapshot PSNR ({kind}, {iterator}, bsz {bsz}): largest difference {worst:.3e} dB")
    # and without the options again: the same result, the keys back to None
    assert torch.equal(eng.reconstruct(y, Phi), plain) and eng.last_info["snapshots"] is None and eng.last_info["trace"] is None


def test_trace_without_ground_truth_and_snapshots_alone():
    net = _net("SimpleCNN")
    y, Phi, gt = _batch(1)
    eng = _engine(net, "anderson", 12)
    plain = eng.reconstruct(y, Phi)
    rec = eng.reconstruct(y, Phi, trace=True)
    assert torch.equal(rec, plain) and eng.last_info["trace"]["psnr"] is None and eng.last_info["trace"]["res"].shape == (12,)
    assert eng.last_info["snapshots"] is None
    rec = eng.reconstruct(y, Phi, snapshots=[5])
    assert torch.equal(rec, plain) and eng.last_info["trace"] is None and list(eng.last_info["snapshots"]) == [5]
    assert eng.last_info["f_calls"] == 14
    with pytest.raises(ValueError):
        eng.reconstruct(y, Phi, snapshots=(5, 12))
    with pytest.raises(ValueError):
        eng.reconstruct(y, Phi, trace=True, gt=gt.cpu())


def test_early_stop_hands_the_final_result_to_later_horizons():
    """tol so large that the run stops at the first test: every horizon beyond the stop is the run's own result, as a run with that
    max_iter would have stopped there too (checked against those runs)."""
    net = _net("SimpleCNN")
    y, Phi, _ = _batch(8)
    eng = DEQSCIEngine(net, max_iter=20, lam=1e-2, tol=1e3)
    rec = eng.reconstruct(y, Phi, snapshots=(3, 6, 12), trace=True)
    info = eng.last_info
    assert info["iterations"] < 5 and info["trace"]["res"].shape == (info["iterations"] + 1,)
    for K in (3, 6, 12):
        e = DEQSCIEngine(net, max_iter=K, lam=1e-2, tol=1e3)
        w = e.reconstruct(y, Phi)
        assert torch.equal(info["snapshots"][K]["rec"], w) and info["snapshots"][K]["res"] == e.last_info["res"], K
    assert torch.equal(info["snapshots"][12]["rec"], rec)


# ----------------------------------------------------------------------------- 3. the reference's own runs, several horizons from one run
def _meta(tag):
    with open(os.path.join(GOLDEN, f"e2e_{tag}.json")) as fh:
        return json.load(fh)


def _harness_run(kind, iters, snapshots, trace=False):
    _, deq = build_pipeline(kind, checkpoint.shipped("ffdnet_gray" if kind == "ffdnet" else "cnn"), iters)
    loader = torch.utils.data.DataLoader(dataset=harness.SCITestDataset(orc.DATA_DIR), batch_size=1, shuffle=False, drop_last=True)
    records = []
    avg, _ = harness.test_solver_sci(deq, test_dataloader=loader, save_img_path="", verbose=False, save_image=False, records=records,
                                     snapshots=snapshots, trace=trace)
    return avg, records


def _check_horizon(records, tag, pick):
    meta = _meta(tag)
    assert [r["id"] for r in records] == [m["id"] for m in meta["measurements"]]
    ps = []
    for r, m in zip(records, meta["measurements"]):
        got = pick(r)
        ps.append(got["psnr"])
        assert abs(got["psnr"] - m["psnr"]) < 0.01, (tag, r["id"], got["psnr"], m["psnr"])
        assert abs(got["res"] - m["res"]) < 2e-2 * m["res"], (tag, r["id"], got["res"], m["res"])
    return {r["id"]: pick(r)["rec"].numpy() for r in records}


def test_simplecnn_180_with_snapshots_reproduces_the_reference_at_10_100_180():
    """One run at 180 with snapshots (10, 100) and the trace against the reference's three separate runs (golden JSONs and tensors)."""
    avg, records = _harness_run("SimpleCNN", 180, (10, 100), trace=True)
    final = _check_horizon(records, "SimpleCNN_anderson_180", lambda r: r)
    s10 = _check_horizon(records, "SimpleCNN_anderson_10", lambda r: r["snapshots"][10])
    _check_horizon(records, "SimpleCNN_anderson_100", lambda r: r["snapshots"][100])
    assert abs(avg - _meta("SimpleCNN_anderson_180")["avg_psnr"]) < 0.01
    g180 = np.load(os.path.join(GOLDEN, "e2e_SimpleCNN_anderson_180_rec.npz"))
    for key, rid in (("traffic_m0", "traffic_cacti.mat:0"), ("drop8_m0", "drop8_cacti.mat:0"), ("runner8_m0", "runner8_cacti.mat:0")):
        assert rel_l2(final[rid], g180[key]) < 1e-4, key
    g10 = np.load(os.path.join(GOLDEN, "e2e_SimpleCNN_anderson_10_rec.npz"))
    assert rel_l2(s10["traffic_cacti.mat:3"], g10["traffic_m3"]) < 1e-4
    # the trace's last row (f-call 179 = the horizon-180 reconstruction: SimpleCNN has no sigma) against the golden per-measurement PSNR
    for r, m in zip(records, _meta("SimpleCNN_anderson_180")["measurements"]):
        assert r["trace"]["psnr"].shape == (180,) and r["trace"]["res"].shape == (180,)
        assert abs(r["trace"]["psnr"][-1] - m["psnr"]) < 0.01, r["id"]
        assert abs(r["trace"]["psnr"][9] - r["snapshots"][10]["psnr"]) < 0.01 and r["trace"]["res"][-1] == r["res"]


def test_ffdnet_30_with_a_snapshot_reproduces_the_reference_at_10_and_30():
    _, records = _harness_run("ffdnet", 30, (10,))
    final = _check_horizon(records, "ffdnet_anderson_30", lambda r: r)
    s10 = _check_horizon(records, "ffdnet_anderson_10", lambda r: r["snapshots"][10])
    assert "trace" not in records[0]
    assert rel_l2(final["traffic_cacti.mat:0"], np.load(os.path.join(GOLDEN, "e2e_ffdnet_anderson_30_rec.npz"))["traffic_m0"]) < 1e-4
    g10 = np.load(os.path.join(GOLDEN, "e2e_ffdnet_anderson_10_rec.npz"))
    assert rel_l2(s10["traffic_cacti.mat:0"], g10["traffic_m0"]) < 1e-4 and rel_l2(s10["drop8_cacti.mat:0"], g10["drop8_m0"]) < 1e-4


# ----------------------------------------------------------------------------- 5. harness schedules and the CLI
def test_evaluate_schedules_agree_on_the_snapshots():
    """SimpleCNN, where the three schedules' final PSNRs agree to 1e-3 dB today (test_harness_clip_batched_equals_sequential): so do the
    snapshots'.  Every snapshot is scored as the final result is: it equals the final PSNR of a run to that horizon."""
    _, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 14)
    _, deq10 = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 10)
    clips = list(harness.SCITestDataset(orc.DATA_DIR))
    runs = {b: harness.evaluate(deq, clips, batch=b, snapshots=(10,), trace=True, ssim=True)[1] for b in (False, True, "all")}
    plain = harness.evaluate(deq, clips, batch=False)[1]
    at10 = harness.evaluate(deq10, clips, batch=False, ssim=True)[1]
    assert plain[0].snapshots is None and plain[0].trace is None
    for b, results in runs.items():
        for r, r0, p, q in zip(results, runs[False], plain, at10):
            assert r.name == r0.name and list(r.snapshots) == [10]
            s = r.snapshots[10]
            assert len(s["psnr"]) == len(s["res"]) == len(s["ssim"]) == len(r.psnr) and r.trace["psnr"].shape == (len(r.psnr), 14)
            assert np.abs(np.array(s["psnr"]) - np.array(r0.snapshots[10]["psnr"])).max() < 1e-3, b
            assert np.abs(np.array(r.psnr) - np.array(p.psnr)).max() < 1e-3
            if b is False:
                assert s["psnr"] == q.psnr and s["res"] == q.res and s["ssim"] == q.ssim and torch.equal(r.rec, p.rec)
    means = harness.horizon_means(runs["all"])
    assert abs(means[10][0] - sum(r.mean_psnr for r in at10) / len(at10)) < 1e-3 and means[10][1] is not None


def test_cli_snapshots_and_trace(tmp_path, capsys):
    from deqsci_amd.cli import main as cli_main
    base = ["--denoiser", "SimpleCNN", "--testpath", orc.DATA_DIR + "/", "--and_maxiters", "14", "--inference", "True"]
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    avg0 = cli_main(base + ["--savepath", str(tmp_path / "a") + "/"])
    out0 = capsys.readouterr().out.splitlines()
    tfile = tmp_path / "t.json"
    avg1 = cli_main(base + ["--savepath", str(tmp_path / "b") + "/", "--snapshots", "10", "--trace", str(tfile)])
    out1 = capsys.readouterr().out.splitlines()
    assert avg0 == avg1
    # the unchanged lines first (all but the closing timing line), then one line per horizon, then the timing line
    assert out1[:len(out0) - 1] == out0[:-1] and "frames in" in out0[-1] and "frames in" in out1[-1]
    extra = out1[len(out0) - 1:-1]
    assert len(extra) == 1 and "[and_maxiters 10] Total Average PSNR:" in extra[0]
    want = _meta("SimpleCNN_anderson_10")["avg_psnr"]
    assert abs(float(extra[0].split("PSNR:")[1].split("dB")[0]) - want) < 0.01 + 0.005       # (printed to 2 decimals)
    doc = json.loads(tfile.read_text())
    assert sorted(doc) == ["drop8_cacti.mat", "runner8_cacti.mat", "traffic_cacti.mat"]
    assert sorted(doc["traffic_cacti.mat"]) == [str(i) for i in range(6)] and list(doc["drop8_cacti.mat"]) == ["0"]
    for clip in doc.values():
        for row in clip.values():
            assert sorted(row) == ["psnr", "res"] and len(row["psnr"]) == len(row["res"]) == 14       # one row per issued f-call
            assert all(isinstance(v, float) for v in row["psnr"] + row["res"])
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
