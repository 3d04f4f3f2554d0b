"""GPU: csrc/synth.hip - Y1 against tests/synth_ref.py and against the shipped clips' own measurements BIT FOR BIT, the 64-row chunking,
Y0, determinism, and one training run from two sources that must not differ in a bit.  No tolerance anywhere: with masks of zeros and
ones and B <= 64 every sum is an integer below 2^24 (tests/test_synth_host.py checks the rounding fact exhaustively), and for
real-valued masks the reference restates the kernel's order of operations."""
import math
import os

import numpy as np
import pytest
import torch

import synth_ref as sr
from conftest import ROOT

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip, checkpoint, harness, synth, training
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.optim import DeviceAdam

DEV = "cuda"
SENT = 7.25                                                    # the guard bands around gt and meas
GUARD = 8
CLIPS = os.path.join(ROOT, "data", "test_gray")
# (T,Hv,Wv): the two of the issue, and a third that the patches of 8 and more frames fit in (two tiles each way, two runs of frames)
VIDEOS = ((7, 19, 23), (5, 33, 17), (40, 37, 45))
# (H,W,B) -> how many crop positions per (video, orientation, dt, ds): 10x13x3 (odd width) and 16x16x8 in full; 33x40x20 = two tiles each
# way, float4 accesses, a second run of 4 frames; 35x34x17 = element by element, a second run of one frame
PATCHES = {(10, 13, 3): "all", (16, 16, 8): "all", (33, 40, 20): "diagonal", (35, 34, 17): "diagonal"}
_CACHE = {}


def _pool_host():
    if "pool" not in _CACHE:
        rng = np.random.RandomState(11)
        videos = [rng.randint(0, 256, size=v).astype(np.uint8) for v in VIDEOS]
        videos[0][0, 0, :4] = (0, 255, 1, 254)
        _CACHE["pool"] = videos
    return _CACHE["pool"]


def _pool():
    if "dev" not in _CACHE:
        _CACHE["dev"] = synth.VideoPool(_pool_host(), DEV)
    return _CACHE["dev"]


def _rows(H, W, B, positions):
    """The full product of the eight orientations x dt in {1,-1,2} x ds in {1,2} over the videos, where it fits, the crop pinned to the
    corners of the video ("all": the four corners, at the first and the last admissible t0; "diagonal": two corners, the first t0)."""
    rows, offset = [], 0
    for (T, Hv, Wv) in VIDEOS:
        for flags in sr.ORIENTATIONS:
            Hc, Wc = (W, H) if flags & sr.TRANSPOSE else (H, W)
            for dt in (1, -1, 2):
                for ds in (1, 2):
                    ymax, xmax, span = Hv - 1 - ds * (Hc - 1), Wv - 1 - ds * (Wc - 1), abs(dt) * (B - 1)
                    if ymax < 0 or xmax < 0 or span > T - 1:
                        continue
                    t0s = (0, T - 1 - span) if dt > 0 else (span, T - 1)
                    corners = ((0, 0), (0, xmax), (ymax, 0), (ymax, xmax)) if positions == "all" else ((0, xmax), (ymax, 0))
                    for t0 in (t0s if positions == "all" else t0s[:1]):
                        for y0, x0 in corners:
                            rows.append((offset, T, Hv, Wv, t0, dt, y0, x0, ds, flags))
        offset += T * Hv * Wv
    rows = sorted(set(rows))
    assert all(sr.fits(r, H, W, B) for r in rows)
    return np.asarray(rows, np.int64)


def _case(shape):
    """rows and their source bytes by the reference's loops: once per patch shape, shared by the tests"""
    if shape not in _CACHE:
        rows = _rows(*shape, PATCHES[shape])
        _CACHE[shape] = (rows, sr.patches_u8(np.concatenate([v.reshape(-1) for v in _pool_host()]), rows, *shape))
    return _CACHE[shape]


def _guarded(shape, offset):
    """A flat NaN-filled buffer between two guard bands, as a view of `shape` that starts `offset` floats past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 4,), SENT, device=DEV, dtype=torch.float32)
    lo = GUARD + offset
    buf[lo:lo + n] = float("nan")
    view = buf[lo:lo + n].view(shape)
    assert view.data_ptr() % 16 == 4 * (offset % 4) and view.is_contiguous()
    return buf, view, lo, n


def _intact(buf, lo, n):
    b = buf.cpu().numpy()
    return bool((b[:lo] == SENT).all() and (b[lo + n:] == SENT).all())


def _masks(n, H, W, B):
    rng = np.random.RandomState(H * W + B)
    binary = (rng.rand(H, W, B) < 0.5).astype(np.float32)
    binary[0, :2, :] = 0
    real = (rng.randn(H, W, B) * 0.7).astype(np.float32)
    return {"shared binary": binary, "shared real": real, "per-sample binary": (rng.rand(n, H, W, B) < 0.5).astype(np.float32),
            "per-sample real": (rng.randn(n, H, W, B) * 0.7).astype(np.float32)}


@pytest.mark.parametrize("shape", list(PATCHES), ids=lambda s: "x".join(map(str, s)))
def test_synth_batch_equals_the_reference_loops(shape):
    H, W, B = shape
    rows, u = _case(shape)
    n = len(rows)
    print(f"{shape}: {n} rows from {len(set(rows[:, 0]))} videos")
    assert {int(f) for f in rows[:, 9]} == ({0, 1, 2, 3} if shape == (33, 40, 20) else set(sr.ORIENTATIONS))   # (40x33 is taller than every video)
    assert len(set(rows[:, 0])) == (3 if B == 3 else 1)                            # eight and more frames fit the third video only
    assert {int(np.sign(d)) for d in rows[:, 5]} == {1, -1} and {abs(int(d)) for d in rows[:, 5]} == {1, 2}
    pool = _pool()
    for offset in ((0, 1) if B % 4 == 0 else (0,)):                               # 16-byte aligned: float4 accesses; offset 1: element by element
        for name, mask in _masks(n, H, W, B).items():
            want_gt, want_meas = sr.snapshots(u, mask)
            gbuf, gt, glo, gn = _guarded((n, H, W, B), offset)
            mbuf, meas, mlo, mn = _guarded((n, H, W), offset)
            got = _hip.synth_batch(pool.data, rows, torch.from_numpy(mask).to(DEV), H, W, B, gt=gt, meas=meas)
            assert got[0] is gt and got[1] is meas
            g, m = gt.cpu().numpy(), meas.cpu().numpy()
            assert not np.isnan(g).any() and not np.isnan(m).any(), (name, offset)      # every element written
            assert np.array_equal(g, want_gt), (name, offset, int((g != want_gt).sum()))
            assert np.array_equal(m, want_meas), (name, offset, int((m != want_meas).sum()))
            assert _intact(gbuf, glo, gn) and _intact(mbuf, mlo, mn), (name, offset)
    # through the package: the same rows as PatchSpecs, the wrapper's own buffers
    mask = _masks(n, H, W, B)["shared binary"]
    gt, meas = synth.synthesize(pool, [synth.PatchSpec(*r) for r in rows], mask)
    want_gt, want_meas = sr.snapshots(u, mask)
    assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(meas.cpu().numpy(), want_meas)


def test_a_batch_of_70_crosses_the_chunk_and_equals_two_smaller_calls():
    H, W, B = 10, 13, 3
    rows, u = _case((H, W, B))
    assert len(rows) >= 70 and _hip.SYNTH_MAX_ROWS == 64
    pick = np.linspace(0, len(rows) - 1, 70).astype(int)
    rows, u = rows[pick], u[pick]
    pool = _pool()
    for mask in (_masks(70, H, W, B)["per-sample real"], _masks(70, H, W, B)["shared binary"]):
        dm = torch.from_numpy(mask).to(DEV)
        gt, meas = _hip.synth_batch(pool.data, rows, dm, H, W, B)
        parts = [_hip.synth_batch(pool.data, rows[a:b], dm[a:b].contiguous() if mask.ndim == 4 else dm, H, W, B) for a, b in ((0, 33), (33, 70))]
        assert torch.equal(gt, torch.cat([p[0] for p in parts])) and torch.equal(meas, torch.cat([p[1] for p in parts]))
        want_gt, want_meas = sr.snapshots(u, mask)
        assert np.array_equal(gt.cpu().numpy(), want_gt) and np.array_equal(meas.cpu().numpy(), want_meas)
    bad = rows.copy()
    bad[69, 4] = bad[69, 1]                                                        # the 70th row starts behind its video's last frame
    with pytest.raises(_hip.DeqsciHipError, match="code -2"):
        _hip.synth_batch(pool.data, bad, dm, H, W, B)
    gt0, meas0 = _hip.synth_batch(pool.data, rows[:0], dm, H, W, B)                # a zero-size batch
    assert tuple(gt0.shape) == (0, H, W, B) and tuple(meas0.shape) == (0, H, W)


def test_rgb_to_gray_equals_its_integer_statement():
    rng = np.random.RandomState(6)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    for n in (1, 255, 256, 1000):
        rgb = np.concatenate([corners, rng.randint(0, 256, size=(n, 3)).astype(np.uint8)])[:max(n, 8)]
        buf = torch.full((len(rgb) + 16,), 201, device=DEV, dtype=torch.uint8)
        out = _hip.rgb_to_gray(torch.from_numpy(rgb).to(DEV), out=buf[8:8 + len(rgb)])
        assert np.array_equal(out.cpu().numpy(), sr.gray(rgb))
        assert bool((buf[:8] == 201).all()) and bool((buf[8 + len(rgb):] == 201).all())
    colour = rng.randint(0, 256, size=(3, 9, 7, 3)).astype(np.uint8)
    pool = synth.VideoPool([colour], DEV)                                          # a colour video enters the pool through Y0
    assert np.array_equal(pool.frames(0), synth.rgb_to_gray(colour)) and np.array_equal(pool.frames(0).ravel(), sr.gray(colour))


@pytest.fixture(scope="module")
def clip_pool():
    names = ("traffic", "drop8", "runner8")
    paths = [os.path.join(CLIPS, f"{n}_cacti.mat") for n in names]
    return names, synth.VideoPool(paths, DEV), {n: harness.load_test_data(p) for n, p in zip(names, paths)}


def test_the_shipped_clips_measurements_are_regenerated_on_the_device(clip_pool):
    names, pool, data = clip_pool
    for name, v in zip(names, pool.videos):
        d = data[name]
        ks = range(6) if name == "traffic" else (0,)
        assert (v.H, v.W) == (256, 256) and v.T >= 8 * len(ks) and set(np.unique(d["mask"])) == {0.0, 1.0}
        specs = [synth.PatchSpec(v.offset, v.T, v.H, v.W, 8 * k, 1, 0, 0, 1, 0) for k in ks]
        gt, meas = synth.synthesize(pool, specs, d["mask"])
        gt, meas = gt.cpu().numpy(), meas.cpu().numpy()
        for i, k in enumerate(ks):
            assert np.array_equal(meas[i], d["meas"][:, :, k]), (name, k, int((meas[i] != d["meas"][:, :, k]).sum()))
            assert np.array_equal(gt[i], d["gt"][:, :, 8 * k:8 * k + 8]), (name, k)


def test_two_runs_give_equal_bits(clip_pool):
    names, pool, data = clip_pool
    specs = synth.sample_specs(pool, 16, 64, 64, 8, np.random.default_rng([3, 0]), max_dt=2, max_ds=2)
    mask = np.ascontiguousarray(data["traffic"]["mask"][:64, :64])
    a = synth.synthesize(pool, specs, mask)
    b = synth.synthesize(pool, specs, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].data_ptr() != b[0].data_ptr()
    host = synth.synthesize(synth._host_view(pool), specs, mask)                   # and the restatement on the same pool
    assert np.array_equal(a[0].cpu().numpy(), host[0]) and np.array_equal(a[1].cpu().numpy(), host[1])


def _train(loader, tmp, name):
    solver, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 6)
    solver.nonlinear_op.train()
    cfg = training.configure_training(deq, "device")
    opt = DeviceAdam(solver.parameters(), lr=1e-4)
    model = str(tmp / name) + "/"
    os.makedirs(model, exist_ok=True)
    steps = training.train_solver_sci(solver, loader, opt, model, "device", 1, deq, print_every_n_steps=1, save_every_n_steps=1000)
    assert (cfg.implicit_backward, cfg.parameter_backward) == ("device", "device") and deq.last_parameter_path == "device"
    return steps, solver


def test_one_training_run_from_two_sources_gives_equal_bits(tmp_path):
    """Two steps at 24x20x4, batch 2, and_maxiters 6, SimpleCNN on the device backend: from a SynthTrainLoader, and from a DataLoader over
    the directory write_training_directory made from the same descriptors in the same order.  The batches are equal bits, so the losses
    and the updated weights are EQUAL."""
    rng = np.random.RandomState(3)
    videos = [rng.randint(0, 256, size=(9, 30, 27)).astype(np.uint8), rng.randint(0, 256, size=(6, 25, 40)).astype(np.uint8)]
    mask = (rng.rand(24, 20, 4) < 0.5).astype(np.float32)
    mask[0, :2, :] = 0
    pool = synth.VideoPool(videos, DEV)
    loader = synth.SynthTrainLoader(pool, mask, 2, 4, 24, 20, 4, seed=7, max_dt=2)
    specs = loader.epoch_specs(0)
    d = synth.write_training_directory(tmp_path / "data", pool, mask, specs)
    ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
    files = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, drop_last=True)
    for a, b in zip(loader, files):                                               # the batches themselves (this advances the loader to epoch 1)
        for key in ("gt", "meas", "mask"):
            assert a[key].is_cuda and torch.equal(a[key].cpu(), b[key]), key
    loader.epoch = 0
    steps_a, solver_a = _train(loader, tmp_path, "synth")
    steps_b, solver_b = _train(files, tmp_path, "files")
    print("synth:", [(s.loss, s.psnr) for s in steps_a], "files:", [(s.loss, s.psnr) for s in steps_b])
    assert len(steps_a) == len(steps_b) == 2 and all(math.isfinite(s.loss) and s.nonfinite == 0 for s in steps_a)
    assert [(s.loss, s.psnr) for s in steps_a] == [(s.loss, s.psnr) for s in steps_b]
    shipped = checkpoint.read_state_dict(checkpoint.shipped("cnn"))[0]
    for (name, pa), pb in zip(solver_a.named_parameters(), solver_b.parameters()):
        assert torch.equal(pa, pb), name
        assert not torch.equal(pa.detach().cpu(), shipped[name]), name             # (the weights moved)
