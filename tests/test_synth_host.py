"""CPU: training samples out of raw video - deqsci_amd/synth.py's restatement against the reference's own loader (tests/golden/synth.npz,
made by tests/golden/make_synth_golden.py) and against the shipped clips' measurements, BIT FOR BIT; the rounding fact the equalities
rest on, exhaustively; the sampler; the C entry points' validation (no GPU, no launch); the loader under train_solver_sci; the flags."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import synth_ref as sr
from conftest import GOLDEN, ROOT

from deqsci_amd import _hip, harness, synth, training

CLIPS = os.path.join(ROOT, "data", "test_gray")
ANCHORS = [("traffic", k) for k in range(6)] + [("drop8", 0), ("runner8", 0)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "synth.npz"))


def _golden_pool(g):
    pool = synth.VideoPool([g["video"]], "cpu")
    return pool, [synth.PatchSpec(*row) for row in g["specs"]]


# ----------------------------------------------------------------------------- (a) against the reference's loader
def test_restatement_equals_what_the_reference_loads(golden):
    g = golden
    pool, specs = _golden_pool(g)
    assert len(specs) == 12 and {s.flags for s in specs} == set(range(8)) and {int(np.sign(s.dt)) for s in specs} == {1, -1}
    assert {abs(s.dt) for s in specs} == {1, 2} and {s.ds for s in specs} == {1, 2}
    gt, meas = synth.synthesize(pool, specs, g["mask"])
    assert gt.dtype == np.float32 and meas.dtype == np.float32
    assert np.array_equal(gt, g["gt"]) and np.array_equal(meas, g["meas"]) and np.array_equal(g["ref_mask"], g["mask"])
    # the independent statement (explicit loops) says the same
    rgt, rmeas = sr.batch(g["video"].reshape(-1), g["specs"], g["mask"], 16, 16, 8)
    assert np.array_equal(rgt, g["gt"]) and np.array_equal(rmeas, g["meas"])
    assert len({m.tobytes() for m in meas}) == 12                                 # twelve different samples


def test_written_directory_reads_back_the_same_bits_in_spec_order(golden, tmp_path):
    g = golden
    pool, specs = _golden_pool(g)
    d = synth.write_training_directory(tmp_path / "train", pool, g["mask"], specs)
    assert d.endswith("/") and sorted(os.listdir(d)) == ["gt", "mask.mat", "measurement"]
    assert sorted(os.listdir(d + "gt")) == ["%06d.mat" % k for k in range(12)] == sorted(os.listdir(d + "measurement"))
    import scipy.io as sio
    f = sio.loadmat(d + "gt/000003.mat")
    assert f["patch_save"].dtype == np.uint8 and f["patch_save"].shape == (16, 16, 8)
    assert sio.loadmat(d + "measurement/000003.mat")["meas"].dtype == np.float64
    ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
    assert len(ds) == 12
    for k in range(12):
        item = ds[k]
        assert np.array_equal(item["gt"], g["gt"][k]) and np.array_equal(item["meas"], g["meas"][k]) and np.array_equal(item["mask"], g["mask"])


# ----------------------------------------------------------------------------- (b) the benchmark's own snapshots
@pytest.fixture(scope="module")
def clips():
    return {name: harness.load_test_data(os.path.join(CLIPS, f"{name}_cacti.mat")) for name in ("traffic", "drop8", "runner8")}


@pytest.mark.parametrize("name,k", ANCHORS)
def test_shipped_clips_measurements_are_regenerated(clips, name, k):
    path = os.path.join(CLIPS, f"{name}_cacti.mat")
    d = clips[name]
    video = synth.load_video(path)
    assert video.dtype == np.uint8 and video.shape == (d["gt"].shape[2], 256, 256)
    assert set(np.unique(d["mask"])) == {0.0, 1.0}
    pool = synth.VideoPool([video], "cpu")
    gt, meas = synth.synthesize(pool, [synth.PatchSpec(0, video.shape[0], 256, 256, 8 * k, 1, 0, 0, 1, 0)], d["mask"])
    assert np.array_equal(meas[0], d["meas"][:, :, k])
    assert np.array_equal(gt[0], d["gt"][:, :, 8 * k:8 * k + 8])


def test_one_fp32_division_is_the_float_nearest_the_double_quotient():
    """The condition under which the device batch equals the written file: masks of zeros and ones and B <= 64 make every sum an integer
    S <= 255 x 64, and float32(S) / float32(255) == float32(S / 255.) for every one of them; a multiplication by 1/255 is not."""
    S = np.arange(255 * 64 + 1)
    a = S.astype(np.float32) / np.float32(255)
    b = (S / 255.0).astype(np.float32)
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert int((S.astype(np.float32) * np.float32(1.0 / 255.0) != b).sum()) == 12096


# ----------------------------------------------------------------------------- (c) Y0
def test_rgb_to_gray_formula():
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    want = [0, 29, 149, 178, 77, 106, 226, 255]                                   # e.g. green: (150 x 255 + 128) >> 8 = 38378 >> 8
    assert synth.rgb_to_gray(corners).tolist() == want == sr.gray(corners).tolist()
    rgb = np.random.RandomState(1).randint(0, 256, size=(5, 7, 9, 3)).astype(np.uint8)
    got = synth.rgb_to_gray(rgb)
    assert got.dtype == np.uint8 and got.shape == (5, 7, 9) and np.array_equal(got.ravel(), sr.gray(rgb))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert np.array_equal(synth.rgb_to_gray(grey), np.arange(256))                # 77 + 150 + 29 = 256: grey stays grey
    with pytest.raises(ValueError):
        synth.rgb_to_gray(rgb.astype(np.float32))


def test_load_video_formats(tmp_path):
    rng = np.random.RandomState(2)
    mono = rng.randint(0, 256, size=(3, 5, 4)).astype(np.uint8)
    rgb = rng.randint(0, 256, size=(3, 5, 4, 3)).astype(np.uint8)
    np.save(tmp_path / "a.npy", mono)
    np.save(tmp_path / "b.npy", rgb)
    np.save(tmp_path / "c.npy", mono.astype(np.float32))
    import scipy.io as sio
    sio.savemat(str(tmp_path / "d.mat"), {"orig": mono.transpose(1, 2, 0).astype(np.float64)})
    assert np.array_equal(synth.load_video(tmp_path / "a.npy"), mono)
    assert np.array_equal(synth.load_video(tmp_path / "b.npy"), synth.rgb_to_gray(rgb))
    assert np.array_equal(synth.load_video(tmp_path / "d.mat"), mono)
    with pytest.raises(ValueError, match="uint8"):
        synth.load_video(tmp_path / "c.npy")
    with pytest.raises(ValueError, match="out of scope"):
        synth.load_video(tmp_path / "e.png")
    assert [os.path.basename(p) for p in synth.list_videos(tmp_path)] == ["a.npy", "b.npy", "c.npy", "d.mat"]
    pool = synth.VideoPool([tmp_path / "a.npy", rgb, tmp_path / "d.mat"], "cpu")
    assert [(v.offset, v.T, v.H, v.W) for v in pool.videos] == [(0, 3, 5, 4), (60, 3, 5, 4), (120, 3, 5, 4)] and pool.nbytes == 180
    assert np.array_equal(pool.frames(1), synth.rgb_to_gray(rgb)) and pool.video_at(120).name.endswith("d.mat")


# ----------------------------------------------------------------------------- (d) the sampler
def test_sampler_draws_only_rows_that_fit_at_the_tightest_geometry():
    H, W, B = 6, 5, 4
    # patch-sized, exactly 1 + |dt| (B - 1) frames long, for |dt| = 2 and ds = 2; its transposed twin; and one with room
    videos = [np.zeros((1 + 2 * (B - 1), 1 + 2 * (H - 1), 1 + 2 * (W - 1)), np.uint8),
              np.zeros((1 + 2 * (B - 1), 1 + 2 * (W - 1), 1 + 2 * (H - 1)), np.uint8), np.zeros((9, 14, 13), np.uint8)]
    pool = synth.VideoPool(videos, "cpu")
    specs = synth.sample_specs(pool, 10000, H, W, B, np.random.default_rng(5), max_dt=2, max_ds=2)
    assert len(specs) == 10000
    for s in specs:
        assert sr.fits(s, H, W, B), s
        synth.check_spec(pool, s, H, W, B)
    by_video = {v.offset: [s for s in specs if s.video_offset == v.offset] for v in pool.videos}
    assert all(len(v) > 50 for v in by_video.values())
    tight = by_video[0]
    twin = by_video[pool.videos[1].offset]
    assert {s.flags & 4 for s in tight if s.ds == 2} == {0} and {s.flags & 4 for s in twin if s.ds == 2} == {4}    # at ds = 2 one orientation each
    assert {s.flags & 4 for s in tight if s.ds == 1} == {0, 4}
    assert {(abs(s.dt), s.ds) for s in tight} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert any(abs(s.dt) == 2 and s.ds == 2 and (s.y0, s.x0) == (0, 0) and s.t0 in (0, 6) for s in tight)
    assert {s.flags & 3 for s in specs} == {0, 1, 2, 3} and {int(np.sign(s.dt)) for s in specs} == {1, -1}
    # in proportion to the admissible crops: counted here from the definition
    def crops(v):
        n = 0
        for tr in (0, 1):
            Hc, Wc = (W, H) if tr else (H, W)
            for dt in (1, 2):
                for ds in (1, 2):
                    n += max(0, v.T - dt * (B - 1)) * max(0, v.H - ds * (Hc - 1)) * max(0, v.W - ds * (Wc - 1))
        return n
    counts = np.array([crops(v) for v in pool.videos], np.float64)
    share = np.array([len(by_video[v.offset]) for v in pool.videos]) / 10000.0
    p = counts / counts.sum()
    assert np.all(np.abs(share - p) <= 5 * np.sqrt(p * (1 - p) / 10000)), (share, p)     # five standard deviations of a binomial share
    plain = synth.sample_specs(pool, 200, H, W, B, np.random.default_rng(5), augment=())
    assert {(s.flags, s.dt, s.ds) for s in plain} == {(0, 1, 1)}


def test_sampler_refuses_a_too_small_video_by_name(tmp_path):
    np.save(tmp_path / "small.npy", np.zeros((3, 8, 8), np.uint8))
    np.save(tmp_path / "fine.npy", np.zeros((4, 8, 8), np.uint8))
    pool = synth.VideoPool(synth.list_videos(tmp_path), "cpu")
    with pytest.raises(ValueError, match=r"small\.npy"):
        synth.sample_specs(pool, 1, 8, 8, 4, np.random.default_rng(0))
    with pytest.raises(ValueError, match=r"small\.npy"):
        synth.SynthTrainLoader(pool, np.ones((8, 8, 4), np.float32), 1, 4, 8, 8, 4, seed=0)
    assert len(synth.sample_specs(pool, 3, 8, 8, 3, np.random.default_rng(0))) == 3
    with pytest.raises(ValueError, match="augment"):
        synth.sample_specs(pool, 1, 8, 8, 3, np.random.default_rng(0), augment=("rotate",))


def _tiny_loader(device="cpu", start_epoch=0, seed=7, patches=4):
    rng = np.random.RandomState(3)
    videos = [rng.randint(0, 256, size=(9, 30, 27)).astype(np.uint8), rng.randint(0, 256, size=(6, 25, 40)).astype(np.uint8)]
    mask = (rng.rand(24, 20, 4) < 0.5).astype(np.float32)
    mask[0, :2, :] = 0
    pool = synth.VideoPool(videos, device)
    return synth.SynthTrainLoader(pool, mask, 2, patches, 24, 20, 4, seed=seed, start_epoch=start_epoch, max_dt=2)


def test_loader_epochs_are_a_function_of_seed_and_epoch():
    a, b = _tiny_loader(), _tiny_loader()
    assert len(a) == 2 and len(_tiny_loader(patches=5)) == 2
    assert a.epoch_specs(0) == b.epoch_specs(0) and a.epoch_specs(1) == b.epoch_specs(1)
    assert a.epoch_specs(0) != a.epoch_specs(1) and a.epoch_specs(0) != _tiny_loader(seed=8).epoch_specs(0)
    first = list(a)
    second = list(a)
    assert a.epoch == 2 and len(first) == len(second) == 2
    for batch in first:
        assert sorted(batch) == ["gt", "mask", "meas"] and all(t.dtype == torch.float32 for t in batch.values())
        assert tuple(batch["gt"].shape) == (2, 24, 20, 4) and tuple(batch["meas"].shape) == (2, 24, 20) and tuple(batch["mask"].shape) == (2, 24, 20, 4)
        assert torch.equal(batch["mask"][0], batch["mask"][1]) and batch["mask"].is_contiguous()
        assert torch.equal(batch["meas"], (batch["mask"] * batch["gt"] * 255).sum(3) / 255)          # integers below 2^24: any order
    assert not torch.equal(first[0]["gt"], second[0]["gt"])
    resumed = list(_tiny_loader(start_epoch=1))                                   # a run resumed at epoch 1 draws the second epoch's batches
    for x, y in zip(resumed, second):
        assert torch.equal(x["gt"], y["gt"]) and torch.equal(x["meas"], y["meas"])
    want_gt, want_meas = sr.batch(a.pool.data, synth.spec_table(a.epoch_specs(1)), a.mask.numpy(), 24, 20, 4)
    assert np.array_equal(torch.cat([b_["gt"] for b_ in second]).numpy(), want_gt)
    assert np.array_equal(torch.cat([b_["meas"] for b_ in second]).numpy(), want_meas)


# ----------------------------------------------------------------------------- (e) the C entry points' validation
class _Host:
    """Host buffers that stand in for device memory: the entry point decides everything below before it would launch."""

    def __init__(self, T=5, Hv=12, Wv=10, H=6, W=4, B=3, bsz=2):
        self.dims = (T, Hv, Wv, H, W, B, bsz)
        self.pool = (ctypes.c_uint8 * (7 + T * Hv * Wv))()
        self.buf = (ctypes.c_float * (4 * bsz * H * W * B + 64))()
        base = (ctypes.addressof(self.buf) + 15) // 16 * 16
        n = H * W * B * 4
        self.mask, self.gt, self.meas = base, base + bsz * n, base + 2 * bsz * n
        self.lib = _hip.load()

    def call(self, rows, null=(), pool_bytes=None, table=None, mask=None, gt=None, meas=None, B=None, H=None, W=None, stride=0, bsz=None):
        """The entry point on these buffers; null: the pointers passed as NULL; every other keyword replaces one argument."""
        T, Hv, Wv, H0, W0, B0, bsz0 = self.dims
        t = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
        ptr = {"pool": ctypes.addressof(self.pool), "table": t.ctypes.data if table is None else table, "mask": self.mask if mask is None else mask,
               "gt": self.gt if gt is None else gt, "meas": self.meas if meas is None else meas}
        ptr.update({k: None for k in null})
        return self.lib.deqsci_synth_batch_u8(ptr["pool"], len(self.pool) if pool_bytes is None else pool_bytes, ptr["table"],
                                              len(t) if bsz is None else bsz, ptr["mask"], stride, ptr["gt"], ptr["meas"],
                                              H0 if H is None else H, W0 if W is None else W, B0 if B is None else B, None)


def test_synth_entry_decides_everything_before_a_launch():
    h = _Host(bsz=3)
    T, Hv, Wv, H, W, B, bsz = h.dims
    off = 7                                                                        # the video starts 7 bytes into the pool and ends with it
    good = [off, T, Hv, Wv, 0, 1, 0, 0, 1, 0]
    # NULLs
    # (every call of this test is refused on the host: a row that passed would be launched on these host buffers)
    for name in ("pool", "table", "mask", "gt", "meas"):
        assert h.call([good], null=(name,)) == -1, name
    # B = 0, B = 65, sizes, a mask stride shorter than a sample
    assert h.call([good], B=0) == -2 and h.call([good], B=65) == -2 and h.call([good], H=0) == -2 and h.call([good], W=-1) == -2
    assert h.call([good], bsz=-1) == -2 and h.call([good], stride=H * W * B - 1) == -2 and h.call([good], pool_bytes=-1) == -2
    # a zero-size batch is a no-op, whatever the pointers
    assert h.call([good], bsz=0) == 0 and h.call([good], bsz=0, null=("pool", "table", "gt")) == 0
    # misalignment
    assert h.call([good], gt=h.gt + 2) == -3 and h.call([good], meas=h.meas + 1) == -3 and h.call([good], mask=h.mask + 2) == -3
    t = np.zeros(11, np.int64)
    t[:10] = good
    assert h.call([good], table=t.ctypes.data + 4) == -3
    # aliasing: gt on meas, an output on the mask, an output on the pool
    assert h.call([good], meas=h.gt + 16) == -4 and h.call([good], gt=h.mask + 16) == -4 and h.call([good], meas=h.mask) == -4
    assert h.call([good], gt=ctypes.addressof(h.pool) // 4 * 4 + 8) == -4
    assert h.call([good, good], stride=bsz * H * W * B) == -4                      # per-sample masks: the second sample's lies on gt
    # unknown flag bits
    assert h.call([good[:9] + [8]]) == -4 and h.call([good[:9] + [-1]]) == -4

    def row(t0=0, dt=1, y0=0, x0=0, ds=1, flags=0, off_=off, T_=T, Hv_=Hv, Wv_=Wv):
        return [off_, T_, Hv_, Wv_, t0, dt, y0, x0, ds, flags]
    # rows that fit exactly, at every edge
    fit = [row(t0=T - B), row(t0=B - 1, dt=-1), row(t0=0, dt=2), row(t0=T - 1, dt=-2), row(y0=Hv - H, x0=Wv - W), row(y0=Hv - W, x0=Wv - H, flags=4),
           row(y0=1, x0=3, ds=2, flags=3), row(y0=Hv - W, x0=Wv - H, flags=7)]
    for r in fit:
        assert sr.fits(r, H, W, B), r
    # ... and each way a row can leave its video: every one of them is refused, alone and behind good rows
    bad = [row(t0=T - B + 1), row(t0=T), row(t0=-1), row(t0=B - 2, dt=-1), row(t0=1, dt=2), row(t0=T - 2, dt=-2), row(dt=0),
           row(y0=Hv - H + 1), row(x0=Wv - W + 1), row(y0=-1), row(x0=-1),
           row(y0=Hv - W + 1, flags=4), row(x0=Wv - H + 1, flags=4), row(y0=Hv - H + 1, flags=2), row(x0=Wv - W + 1, flags=1),
           row(y0=Hv - W + 1, flags=7), row(x0=Wv - H + 1, flags=7),
           row(ds=0), row(ds=-1), row(y0=2, ds=2), row(x0=4, ds=2), row(ds=3), row(y0=2, x0=4, ds=2, flags=3),
           row(T_=T + 1), row(off_=off + 1), row(off_=-1), row(off_=len(h.pool) + 1), row(T_=0), row(Hv_=0), row(Wv_=-3), row(Hv_=Hv + 1),
           row(T_=2 ** 62), row(Hv_=2 ** 40), row(t0=2 ** 62, dt=2 ** 40)]
    for flags in sr.ORIENTATIONS:                                                   # each corner under each orientation: one pixel too far, either way
        Hc, Wc = (W, H) if flags & 4 else (H, W)
        ymax, xmax = Hv - Hc, Wv - Wc
        assert all(sr.fits(row(y0=y, x0=x, flags=flags), H, W, B) for y in (0, ymax) for x in (0, xmax))
        bad += [row(y0=ymax + 1, x0=x, flags=flags) for x in (0, xmax)] + [row(y0=y, x0=xmax + 1, flags=flags) for y in (0, ymax)]
        bad += [row(y0=-1, x0=xmax, flags=flags), row(y0=ymax, x0=-1, flags=flags)]
    for r in bad:
        if all(v > 0 for v in r[1:4]) and r[0] == off and r[1:4] == [T, Hv, Wv]:
            assert not sr.fits(r, H, W, B), r
        assert h.call([r]) == -2, r
        assert h.call([fit[0], fit[1], r]) == -2, r
    many = [fit[k % len(fit)] for k in range(70)] + [bad[0]]                        # the 71st row, in the second chunk: still before the first launch
    big = _Host(bsz=71)
    assert big.call(many) == -2


def test_rgb_to_gray_entry_validation():
    lib = _hip.load()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    assert lib.deqsci_rgb_to_gray_u8(None, p, 4, None) == -1 and lib.deqsci_rgb_to_gray_u8(p, None, 4, None) == -1
    assert lib.deqsci_rgb_to_gray_u8(p, p + 32, -1, None) == -2
    assert lib.deqsci_rgb_to_gray_u8(p, p + 8, 4, None) == -4 and lib.deqsci_rgb_to_gray_u8(p, p, 4, None) == -4
    assert lib.deqsci_rgb_to_gray_u8(None, None, 0, None) == 0
    assert (_hip.SYNTH_ROW_WORDS, _hip.SYNTH_MAX_ROWS, _hip.SYNTH_MAX_FRAMES) == (10, 64, 64)
    hdr = open(os.path.join(ROOT, "include", "deqsci_hip.h")).read()
    for name, v in (("ROW_WORDS", 10), ("MAX_ROWS", 64), ("MAX_FRAMES", 64), ("FLIP_H", sr.FLIP_H), ("FLIP_V", sr.FLIP_V), ("TRANSPOSE", sr.TRANSPOSE)):
        assert f"#define DEQSCI_SYNTH_{name} {v}\n" in hdr
    assert (synth.FLIP_H, synth.FLIP_V, synth.TRANSPOSE) == (sr.FLIP_H, sr.FLIP_V, sr.TRANSPOSE)
    assert synth.PatchSpec._fields == ("video_offset", "T", "Hv", "Wv", "t0", "dt", "y0", "x0", "ds", "flags")


# ----------------------------------------------------------------------------- (f) under the training loop
class _Stub(torch.nn.Module):
    """A solver and a DEQ module in one (DEQFixedPoint's forward signature): a 3x3 conv over the frames of the initial point."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(11)
        self.nonlinear_op = torch.nn.Conv2d(4, 4, 3, padding=1)
        self.seen = []

    def forward(self, y, Phi, Phi_sum, initial_point=None, train_flag=True):
        assert float(Phi_sum.min()) == 1.0 and torch.equal(initial_point, y.unsqueeze(3) * Phi)
        self.seen.append(y.clone())
        return initial_point + 0.1 * self.nonlinear_op(initial_point.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)


def test_two_cpu_steps_of_the_training_loop_from_a_synth_loader(tmp_path):
    import deqsci_amd
    assert deqsci_amd.SynthTrainLoader is synth.SynthTrainLoader and deqsci_amd.VideoPool is synth.VideoPool
    assert deqsci_amd.sample_specs is synth.sample_specs and deqsci_amd.write_training_directory is synth.write_training_directory
    assert deqsci_amd.synthesize is synth.synthesize and deqsci_amd.load_video is synth.load_video and deqsci_amd.PatchSpec is synth.PatchSpec
    loader = _tiny_loader()
    stub = _Stub()
    opt = torch.optim.Adam(stub.parameters(), lr=1e-3)
    model = str(tmp_path / "model") + "/"
    os.makedirs(model)
    steps = training.train_solver_sci(stub, loader, opt, model, torch.nn.MSELoss(), 1, stub, print_every_n_steps=1, save_every_n_steps=1000)
    assert [(s.epoch, s.step) for s in steps] == [(0, 0), (0, 1)] and all(math.isfinite(s.loss) and s.loss > 0 for s in steps)
    assert loader.epoch == 1 and os.listdir(model) == ["epoch_0.ckpt"]
    want = list(_tiny_loader())
    assert all(torch.equal(a, b["meas"]) for a, b in zip(stub.seen, want))


# ----------------------------------------------------------------------------- (g) the command line
def test_cli_flags_parse_and_the_two_sources_exclude_one_another(capsys, tmp_path):
    from deqsci_amd.cli import main, parser
    a = parser().parse_args(["--inference", "False", "--trainvideos", "v/", "--trainmask", "m.mat", "--patches_per_epoch", "64", "--patch_size", "128",
                             "--frames", "4", "--augment", "flip,reverse"])
    assert (a.trainvideos, a.trainmask, a.patches_per_epoch, a.patch_size, a.frames, a.augment, a.trainpath) == ("v/", "m.mat", 64, 128, 4, "flip,reverse", "")
    d = parser().parse_args([])
    assert (d.trainvideos, d.trainmask, d.patch_size, d.frames, d.augment) == ("", "", 256, 8, "flip,transpose,reverse")
    helps = {x.dest: x.help for x in parser()._actions}
    assert all("(this build)" in helps[k] for k in ("trainvideos", "trainmask", "patches_per_epoch", "patch_size", "frames", "augment"))
    for argv, word in ((["--trainvideos", "v/", "--trainmask", "m.mat", "--trainpath", "t/"], "exclude"), (["--trainvideos", "v/"], "--trainmask"),
                       (["--trainvideos", "v/", "--trainmask", "m.mat", "--augment", "rotate"], "augment"),
                       (["--trainvideos", "v/", "--trainmask", "m.mat", "--patches_per_epoch", "1", "--batch_size", "2"], "--patches_per_epoch")):
        with pytest.raises(SystemExit) as e:
            main(["--inference", "False"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv         # argparse's own error
    with pytest.raises(SystemExit) as e:
        main(["--inference", "False"])
    assert "--trainpath" in str(e.value) and "--trainvideos" in str(e.value)
    assert synth.parse_augment("none") == () and synth.parse_augment("flip, transpose") == ("flip", "transpose")
    # the shell entry of the writer, on two small videos
    rng = np.random.RandomState(4)
    os.makedirs(tmp_path / "videos")
    np.save(tmp_path / "videos" / "a.npy", rng.randint(0, 256, size=(5, 20, 22)).astype(np.uint8))
    np.save(tmp_path / "videos" / "b.npy", rng.randint(0, 256, size=(4, 18, 18, 3)).astype(np.uint8))
    import scipy.io as sio
    sio.savemat(str(tmp_path / "m.mat"), {"mask": (rng.rand(20, 20, 6) < 0.5).astype(np.float64)})
    argv = ["write", "--videos", str(tmp_path / "videos"), "--mask", str(tmp_path / "m.mat"), "--n", "5", "--seed", "3", "--patch_size", "16", "--frames", "4"]
    out = synth.main(argv + ["--out", str(tmp_path / "out")])
    again = synth.main(argv + ["--out", str(tmp_path / "again")])
    ds, ds2 = (training.SCITrainingDatasetSubset(o + "gt/", o + "measurement/", o + "mask.mat") for o in (out, again))
    assert len(ds) == 5 and ds[0]["gt"].shape == (16, 16, 4) and ds[0]["mask"].shape == (16, 16, 4)
    for k in range(5):
        assert np.array_equal(ds[k]["meas"], np.float32((ds[k]["mask"] * ds[k]["gt"] * 255).sum(2) / 255))
        assert np.array_equal(ds[k]["gt"], ds2[k]["gt"])
    with pytest.raises(ValueError, match="smaller than the patch"):
        synth.load_mask(tmp_path / "m.mat", 16, 16, 8)
