"""CPU: the sensor-noise model's host side - Philox4x32-10 against its known answers, the statistics of the float64 normals,
SensorNoise.apply on CPU arrays against tests/noise_ref.py bit for bit, the three exports' argument validation (no launch), the
sequence-number rules of the loader and the harness, and the command line's refusal.  (The kernels: tests/test_noise_gpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

import noise_ref as nr

N_STAT = 1 << 18
SEED = 1234
_CACHE = {}


def _normals(seq):
    """The float64 normals of (seed 1234, seq), N = 2^18: once per session."""
    if seq not in _CACHE:
        _CACHE[seq] = nr.normals64(nr.words([seq], N_STAT, SEED), N_STAT)[0]
    return _CACHE[seq]


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("counter,key,want", nr.KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    from deqsci_amd import noise
    assert nr.philox_scalar(counter, key) == want
    assert tuple(int(v) for v in noise.philox4x32_10(counter, key)) == want
    got = nr.philox(*(np.asarray([c], np.uint64) for c in counter), *key)
    assert tuple(int(v[0]) for v in got) == want


def test_group_words_follow_the_counter_layout():
    """counter = (g low, g high, seq low, seq high), key = (seed low, seed high): both restatements, against the scalar one; the
    issue's example (group 5 of seq 7, seed 1234) among them; both high words matter."""
    from deqsci_amd import noise
    seqs, seed = [7, (1 << 32) | 5, 5, (1 << 63) + 3], (1 << 32) | SEED
    for s in (SEED, seed):
        w = nr.words(seqs, 255, s)
        assert w.shape == (4, 64, 4) and np.array_equal(w, noise.group_words(4, 255, seqs, s))
        for k, g in ((0, 5), (1, 0), (3, 63)):
            assert tuple(int(v) for v in w[k, g]) == nr.philox_scalar((g, 0, seqs[k] & nr.MASK32, seqs[k] >> 32), (s & nr.MASK32, s >> 32))
    assert tuple(int(v) for v in nr.words([7], 24, SEED)[0, 5]) == (289107249, 2204080987, 1141931367, 543250339)
    assert not np.array_equal(nr.words([(1 << 32) | 5], 64, SEED), nr.words([5], 64, SEED))
    assert not np.array_equal(nr.words([5], 64, seed), nr.words([5], 64, SEED))


@pytest.mark.parametrize("seq", [0, 1])
def test_float64_normals_pass_the_moment_conditions(seq):
    """Each statistic under 4 of its own standard errors (conditions from the issue, not measurements), and |n| <= sqrt(-2 ln 2^-24)."""
    x = _normals(seq)
    stats = nr.moments(x)
    print(seq, stats)
    for name, v in stats.items():
        assert v < 4.0, (name, v)
    assert np.abs(x).max() <= nr.NORMAL_MAX < 5.77


def test_float64_normals_of_two_sequences_are_uncorrelated():
    c = nr.correlation(_normals(0), _normals(1))
    print(c)
    assert c < 4.0


def test_normal_host_is_the_float64_restatement_rounded():
    from deqsci_amd import noise
    got = noise.normal_host(2, 1021, [0, (1 << 40) + 9], SEED)
    want = nr.normals64(nr.words([0, (1 << 40) + 9], 1021, SEED), 1021)
    assert got.dtype == np.float32 and got.shape == (2, 1021)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * 1.0001 * np.abs(want))          # one fp32 rounding: half an ulp


# ----------------------------------------------------------------------------- the model on CPU arrays
@pytest.mark.parametrize("sigma,gain,bits,full_scale", nr.GRID)
def test_apply_on_cpu_arrays_equals_the_reference_bit_for_bit(sigma, gain, bits, full_scale):
    from deqsci_amd import noise
    seqs, y = [4, 5, (1 << 40) + 1], nr.ramp(3, 15 * 17).reshape(3, 15, 17)
    model = noise.SensorNoise(sigma, gain, bits, full_scale, seed=9)
    got = model.apply(y, seqs, frames=8)
    if not model.enabled:
        assert got is y
        return
    nrm = noise.normal_host(3, 255, seqs, 9)
    want = nr.sensor_f32(y.reshape(3, 255), nrm, sigma, gain, bits, full_scale or 8.0).reshape(y.shape)
    assert nr.same_bits(got, want)
    bad = ~np.isfinite(y)
    assert bad.sum() == 3 and nr.same_bits(got[bad], y[bad])                       # NaN, +Inf, -Inf: untouched
    assert not nr.same_bits(got[~bad], y[~bad])
    t = model.apply(torch.from_numpy(y), seqs, frames=8)                           # a CPU tensor: the same values, as a tensor
    assert isinstance(t, torch.Tensor) and nr.same_bits(t.numpy(), want)
    if bits:
        L, fs = 2 ** bits - 1, np.float32(full_scale)
        q = got[~bad].astype(np.float64) / float(fs) * L
        assert np.abs(q - np.rint(q)).max() < 1e-3 and got[~bad].min() >= 0 and got[~bad].max() <= fs


def test_sensor_noise_is_frozen_checked_and_names_its_scale():
    from deqsci_amd import SensorNoise
    m = SensorNoise()
    assert not m.enabled and (m.sigma, m.gain, m.bits, m.full_scale, m.seed) == (0.0, 0.0, 0, None, 0)
    with pytest.raises(Exception):
        m.sigma = 1.0
    assert SensorNoise(bits=8).enabled and SensorNoise(gain=0.01).enabled and SensorNoise(sigma=1e-3).enabled
    assert SensorNoise(bits=8).scale(8) == 8.0 and SensorNoise(bits=8, full_scale=3.5).scale(8) == 3.5
    with pytest.raises(ValueError):
        SensorNoise(bits=8).scale()
    for bad in (dict(sigma=-1.0), dict(gain=float("nan")), dict(bits=17), dict(bits=-1), dict(full_scale=0.0), dict(sigma=float("inf"))):
        with pytest.raises(ValueError):
            SensorNoise(**bad)


# ----------------------------------------------------------------------------- the C ABI, before any launch
def test_exports_validate_their_arguments_before_any_launch():
    from deqsci_amd import _hip
    lib = _hip.load()
    buf = (ctypes.c_float * 256)()
    p16 = (ctypes.addressof(buf) + 15) // 16 * 16
    q16 = p16 + 512
    seq = (ctypes.c_uint64 * 4)(0, 1, 2, 3)
    s = ctypes.addressof(seq)
    for fn in (lib.deqsci_philox_words_u32, lib.deqsci_philox_normal_f32):
        assert fn(None, s, 1, 8, SEED, None) == -1 and fn(p16, None, 1, 8, SEED, None) == -1
        assert fn(p16, s, -1, 8, SEED, None) == -2 and fn(p16, s, 1, 0, SEED, None) == -2 and fn(p16, s, 1, -4, SEED, None) == -2
        assert fn(p16, s, 1 << 30, 1 << 30, SEED, None) == -2                                       # more than 2^40 elements
        assert fn(p16 + 2, s, 1, 8, SEED, None) == -3
        assert fn(p16, s, 0, 8, SEED, None) == 0 and fn(None, None, 0, 8, SEED, None) == 0            # bsz == 0: nothing to do

    def sensor(y=p16, out=q16, sq=s, bsz=1, n=8, sigma=0.02, gain=0.01, bits=8, fs=8.0):
        return lib.deqsci_sensor_noise_f32(y, out, sq, bsz, n, SEED, sigma, gain, bits, fs, None)
    assert sensor(y=None) == -1 and sensor(out=None) == -1 and sensor(sq=None) == -1
    assert sensor(bsz=-1) == -2 and sensor(n=0) == -2
    assert sensor(y=p16 + 2) == -3 and sensor(out=q16 + 1) == -3
    assert sensor(bits=17) == -4 and sensor(bits=-1) == -4
    for bad in (-1.0, float("nan"), float("inf")):
        assert sensor(sigma=bad) == -4 and sensor(gain=bad) == -4
    for bad in (0.0, -8.0, float("nan"), float("inf")):
        assert sensor(fs=bad) == -4
    assert sensor(out=p16 + 4) == -4 and sensor(y=p16 + 16, out=p16, bsz=2) == -4                     # partial overlap, either way round
    assert sensor(bsz=0) == 0
    for name in ("philox_words", "philox_normal", "sensor_noise"):
        assert callable(getattr(_hip, name))
    for name in ("deqsci_philox_words_u32", "deqsci_philox_normal_f32", "deqsci_sensor_noise_f32"):
        assert name in _hip.SIGNATURES


# ----------------------------------------------------------------------------- the loader
H, W, B = 16, 16, 8


def _pool():
    from deqsci_amd import synth
    if "pool" not in _CACHE:
        rng = np.random.RandomState(5)
        _CACHE["pool"] = synth.VideoPool([rng.randint(0, 256, size=s).astype(np.uint8) for s in ((12, 20, 24), (9, 18, 17))], "cpu")
        _CACHE["mask"] = (rng.rand(H, W, B) < 0.5).astype(np.float32)
    return _CACHE["pool"], _CACHE["mask"]


def _epoch(loader):
    batches = list(loader)
    return torch.cat([b["gt"] for b in batches]).numpy(), torch.cat([b["meas"] for b in batches]).numpy()


def test_loader_noise_does_not_depend_on_the_batch_size_or_the_resume_point():
    from deqsci_amd import SensorNoise, synth
    pool, mask = _pool()
    model = SensorNoise(sigma=5 / 255, gain=0.01, bits=10, seed=77)

    def loader(bsz, noise, start_epoch=0):
        return synth.SynthTrainLoader(pool, mask, bsz, 8, H, W, B, seed=3, start_epoch=start_epoch, noise=noise)
    clean2, noisy2, noisy4 = loader(2, None), loader(2, model), loader(4, model)
    epochs = []
    for e in range(2):
        (g0, m0), (g2, m2), (g4, m4) = _epoch(clean2), _epoch(noisy2), _epoch(noisy4)
        assert nr.same_bits(m2, m4) and not nr.same_bits(m2, m0)
        assert nr.same_bits(g2, g0) and nr.same_bits(g4, g0)                          # gt is never changed
        seq = list(range(e * 8, e * 8 + 8))
        assert noisy2.epoch_seq(e) == seq
        assert nr.same_bits(m2, model.apply(m0, seq, frames=B))                       # sample i of epoch e: seq = e * patches_per_epoch + i
        epochs.append(m2)
    assert not nr.same_bits(epochs[0], epochs[1])
    assert nr.same_bits(_epoch(loader(4, model, start_epoch=1))[1], epochs[1])        # a resumed run draws what the uninterrupted run drew


def test_noise_none_and_a_disabled_model_give_todays_bits():
    from deqsci_amd import SensorNoise, synth
    pool, mask = _pool()
    specs = synth.sample_specs(pool, 5, H, W, B, np.random.default_rng(1))
    gt, meas = synth.synthesize(pool, specs, mask)
    for noise, seq in ((None, None), (SensorNoise(), None), (SensorNoise(seed=5), [1, 2, 3, 4, 5])):
        g, m = synth.synthesize(pool, specs, mask, noise, seq)
        assert nr.same_bits(g, gt) and nr.same_bits(m, meas)
    g, m = synth.synthesize(pool, specs, mask, SensorNoise(sigma=0.02), [1, 2, 3, 4, 5])
    assert nr.same_bits(g, gt) and not nr.same_bits(m, meas)
    with pytest.raises(ValueError):
        synth.synthesize(pool, specs, mask, SensorNoise(sigma=0.02))                  # an enabled model needs its sequence numbers
    a = _epoch(synth.SynthTrainLoader(pool, mask, 2, 4, H, W, B, seed=3))
    b = _epoch(synth.SynthTrainLoader(pool, mask, 2, 4, H, W, B, seed=3, noise=SensorNoise()))
    assert nr.same_bits(a[0], b[0]) and nr.same_bits(a[1], b[1])


def test_written_directory_holds_the_host_restatement(tmp_path):
    import scipy.io as sio
    from deqsci_amd import SensorNoise, synth
    pool, mask = _pool()
    specs = synth.sample_specs(pool, 3, H, W, B, np.random.default_rng(2))
    model = SensorNoise(sigma=5 / 255, bits=8, seed=4)
    out = synth.write_training_directory(tmp_path / "noisy", pool, mask, specs, model, [0, 1, 2])
    gt, meas = synth.synthesize(pool, specs, mask, model, [0, 1, 2])
    for k in range(3):
        got = sio.loadmat(out + "measurement/%06d.mat" % k)["meas"]
        assert got.dtype == np.float64 and np.array_equal(got, meas[k].astype(np.float64) * 255.0)
        assert np.array_equal(sio.loadmat(out + "gt/%06d.mat" % k)["patch_save"], np.rint(gt[k] * 255).astype(np.uint8))
    clean = synth.write_training_directory(tmp_path / "clean", pool, mask, specs)
    assert not np.array_equal(sio.loadmat(clean + "measurement/000000.mat")["meas"], sio.loadmat(out + "measurement/000000.mat")["meas"])


# ----------------------------------------------------------------------------- the harness
class _Recorder:
    """A DEQ module's stand-in: forward records y and returns the starting point."""

    def __init__(self):
        self.seen = []
        self.forward_res = None

    def forward(self, y, Phi, Phi_sum, initial_point=None, train_flag=False):
        self.seen.extend(v.clone() for v in y)
        return initial_point


def _clips():
    rng = np.random.RandomState(8)
    out = []
    for name, M in (("alpha.mat", 3), ("beta.mat", 2)):
        gt = rng.rand(12, 10, 4 * M).astype(np.float32)
        mask = (rng.rand(12, 10, 4) < 0.5).astype(np.float32)
        meas = np.stack([(gt[..., 4 * m:4 * m + 4] * mask).sum(-1) for m in range(M)], axis=-1).astype(np.float32)
        out.append({"file": name, "gt": gt, "mask": mask, "meas": meas})
    return out


def test_harness_noise_depends_on_clip_and_measurement_only(monkeypatch):
    from deqsci_amd import SensorNoise, harness, operators
    monkeypatch.setattr(operators, "phi_sum", lambda Phi: torch.where(Phi.sum(-1) == 0, torch.ones(()), Phi.sum(-1)))
    monkeypatch.setattr(operators, "initial_point", lambda y, Phi, Phi_sum=None, gt=None: y[..., None] * Phi)
    model = SensorNoise(sigma=5 / 255, gain=0.01, bits=8, seed=21)
    clips = _clips()
    seen = {}
    for batch in (False, True, "all"):
        rec = _Recorder()
        harness.evaluate(rec, clips, device="cpu", batch=batch, noise=model)
        seen[batch] = torch.stack(rec.seen).numpy()
        assert seen[batch].shape == (5, 12, 10)
    assert nr.same_bits(seen[False], seen[True]) and nr.same_bits(seen[False], seen["all"])
    k = 0
    for c, clip in enumerate(clips):                                                    # seq = (clip << 32) | measurement
        for m in range(clip["meas"].shape[-1]):
            want = model.apply(np.ascontiguousarray(clip["meas"][..., m])[None], [(c << 32) | m], frames=4)[0]
            assert nr.same_bits(seen[False][k], want)
            k += 1
    diff = [seen[False][i] - clips[0 if i < 3 else 1]["meas"][..., i if i < 3 else i - 3] for i in range(5)]
    assert not np.array_equal(diff[0], diff[3]) and not np.array_equal(diff[0], diff[1])   # the two clips, and two measurements of one, differ
    rec = _Recorder()
    harness.evaluate(rec, clips, device="cpu", batch=True)                               # no model: the clean measurements
    assert nr.same_bits(torch.stack(rec.seen).numpy()[:3], np.moveaxis(clips[0]["meas"], -1, 0))
    rec = _Recorder()
    harness.evaluate(rec, clips, device="cpu", batch=True, noise=SensorNoise())          # a disabled model: the same
    assert nr.same_bits(torch.stack(rec.seen).numpy()[3:], np.moveaxis(clips[1]["meas"], -1, 0))


# ----------------------------------------------------------------------------- the command line
def test_cli_refuses_noise_flags_with_trainpath(capsys):
    from deqsci_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--inference", "False", "--denoiser", "SimpleCNN", "--trainpath", "data/train/", "--meas_noise_sigma", "5"])
    assert e.value.code not in (0, None)
    assert "python -m deqsci_amd.synth write" in capsys.readouterr().err


def test_cli_noise_flags_parse_to_the_model():
    from deqsci_amd import cli
    from deqsci_amd.noise import noise_from_arguments
    p = cli.parser()
    a = p.parse_args(["--meas_noise_sigma", "5", "--meas_bits", "8", "--seed", "3"])
    m = noise_from_arguments(a, a.seed)
    assert (m.sigma, m.gain, m.bits, m.full_scale, m.seed) == (5 / 255.0, 0.0, 8, None, 3)
    assert noise_from_arguments(p.parse_args(["--meas_noise_sigma", "5", "--noise_seed", "9", "--seed", "3"]), 3).seed == 9
    assert noise_from_arguments(p.parse_args([]), None) is None and noise_from_arguments(p.parse_args(["--sigma", "5"]), None) is None
    assert "sensor noise (this build)" in p.format_help()
