"""GPU: csrc/noise.hip - N0 against tests/noise_ref.py bit for bit, N1 against the float64 normals of the same words within K ulps,
N2 bit for bit against the fp32 emulation applied to the DEVICE's own normals (so the transcendental tolerance does not enter), every
output between sentinels, and the two consumers on a device pool.

K: no document shipped with the toolchain states the ULP errors of logf / sqrtf / sincospif, so K is measured, by the issue's rule: the
largest |n_dev - n64| / (2^-23 |n64|) over the 2^18 normals of (seed 1234, seq 0) on an MI355X was MEASURED_MAX (profiles/noise.md);
K = ceil(2 x that), and may not exceed 16 - library-grade functions stay under 5, the fast intrinsics miss by hundreds."""
import math

import numpy as np
import pytest
import torch

import noise_ref as nr

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import SensorNoise, _hip, synth

DEV = "cuda"
SEED = 1234
GUARD = 8
SENT = 7.25
SENT_I = 0x5A5A5A5A
MEASURED_MAX = 1.7558                                      # at |n| = 0.265; 1.70 .. 1.82 over three other (seed, seq) pairs, mean 0.34
K = math.ceil(2 * MEASURED_MAX)                            # 4
assert K <= 16
FLOOR = 2.0 ** -149                                        # one fp32 ulp of the smallest normal value
# (bsz, n, offset of the base pointer in floats): scalar path with a partial last group; float4 path; the float4 shape forced onto the
# scalar path; one element; across the 64-samples-per-launch boundary
SHAPES = ((3, 15 * 17, 0), (2, 256, 0), (2, 256, 1), (2, 1, 0), (65, 64, 0))
N_STAT = 1 << 18
_CACHE = {}


def _seqs(bsz):
    return [(k * 0x9E3779B97F4A7C15 + 11) & ((1 << 64) - 1) if k % 3 else k for k in range(bsz)]     # small ones and ones with high words


def _guarded(numel, offset, dtype=torch.float32):
    """A buffer of sentinels and the view of `numel` elements that starts `offset` elements past a 16-byte boundary behind the guard."""
    fill = SENT if dtype == torch.float32 else SENT_I
    buf = torch.full((GUARD + offset + numel + GUARD,), fill, device=DEV, dtype=dtype)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + offset:GUARD + offset + numel]


def _guards_intact(buf, numel, offset):
    lo, hi = buf[:GUARD + offset].cpu().numpy(), buf[GUARD + offset + numel:].cpu().numpy()
    fill = SENT if buf.dtype == torch.float32 else SENT_I
    return bool((lo == fill).all() and (hi == fill).all())


def _words(seqs, n, seed=SEED, offset=0):
    groups = -(-n // 4)
    buf, view = _guarded(len(seqs) * groups * 4, offset, torch.int32)
    _hip.philox_words(seqs, n, seed, out=view.view(len(seqs), groups, 4))
    torch.cuda.synchronize()
    assert _guards_intact(buf, view.numel(), offset)
    return view.cpu().numpy().view(np.uint32).reshape(len(seqs), groups, 4)


def _normals(seqs, n, seed=SEED, offset=0):
    buf, view = _guarded(len(seqs) * n, offset)
    _hip.philox_normal(seqs, n, seed, out=view.view(len(seqs), n))
    torch.cuda.synchronize()
    assert _guards_intact(buf, view.numel(), offset)
    return view.cpu().numpy().reshape(len(seqs), n)


def _ulps(dev, n64):
    """|n_dev - n64| in units of 2^-23 |n64|, after the absolute floor."""
    err = np.maximum(np.abs(dev.astype(np.float64) - n64) - FLOOR, 0.0)
    return err / (2.0 ** -23 * np.abs(n64))


# ----------------------------------------------------------------------------- N0
@pytest.mark.parametrize("bsz,n,offset", SHAPES)
def test_words_equal_the_reference_bit_for_bit(bsz, n, offset):
    seqs = _seqs(bsz)
    got = _words(seqs, n, offset=offset)
    assert np.array_equal(got, nr.words(seqs, n, SEED))
    assert np.array_equal(got, _words(seqs, n, offset=offset))                           # two identical calls
    if bsz == 65:
        assert np.array_equal(got[64:65], _words(seqs[64:], n))                           # sample 64 = a bsz-1 call with its seq


def test_words_depend_on_both_high_words():
    n = 64
    a, b = _words([(1 << 32) | 5], n), _words([5], n)
    assert not np.array_equal(a, b) and np.array_equal(a, nr.words([(1 << 32) | 5], n, SEED))
    c = _words([5], n, seed=(1 << 32) | SEED)
    assert not np.array_equal(c, b) and np.array_equal(c, nr.words([5], n, (1 << 32) | SEED))
    assert tuple(int(v) for v in _words([7], 24)[0, 5]) == (289107249, 2204080987, 1141931367, 543250339)


# ----------------------------------------------------------------------------- N1
@pytest.mark.parametrize("bsz,n,offset", SHAPES)
def test_normals_match_float64_on_the_same_words(bsz, n, offset):
    seqs = _seqs(bsz)
    got = _normals(seqs, n, offset=offset)
    want = nr.normals64(nr.words(seqs, n, SEED), n)
    worst = float(_ulps(got, want).max())
    print(f"N1 {bsz}x{n}+{offset}: max error {worst:.3f} x 2^-23 |n| (K = {K})")
    assert worst <= K
    assert nr.same_bits(got, _normals(seqs, n, offset=offset))
    if offset == 0 and n % 4 == 0:
        assert nr.same_bits(got, _normals(seqs, n, offset=1))                             # float4 and scalar accesses: the same values
    if bsz == 65:
        assert nr.same_bits(got[64:65], _normals(seqs[64:], n))


def _stat_normals():
    if "stat" not in _CACHE:
        _CACHE["stat"] = (_normals([0], N_STAT), nr.normals64(nr.words([0], N_STAT, SEED), N_STAT))
    return _CACHE["stat"]


def test_normal_error_statistics_at_2_to_the_18():
    got, want = _stat_normals()
    u = _ulps(got, want)
    print(f"N1 1x{N_STAT}: max error {u.max():.4f} x 2^-23 |n|, mean {u.mean():.4f}, at |n| = {abs(want.reshape(-1)[u.argmax()]):.3e} (K = {K})")
    assert u.max() <= K
    assert np.abs(got).max() <= np.float32(nr.NORMAL_MAX) * (1 + K * 2.0 ** -23)
    for name, v in nr.moments(got).items():                                               # the device's normals pass the host's conditions
        assert v < 4.0, (name, v)


# ----------------------------------------------------------------------------- N2
def _sensor(y, seqs, model, frames, offset, in_place):
    bsz, n = y.shape
    buf, view = _guarded(bsz * n, offset)
    out = view.view(bsz, n)
    if in_place:
        out.copy_(torch.from_numpy(y))
        src = out
    else:
        sbuf, sview = _guarded(bsz * n, offset)
        src = sview.view(bsz, n)
        src.copy_(torch.from_numpy(y))
    got = _hip.sensor_noise(src, seqs, model.seed, model.sigma, model.gain, model.bits, model.scale(frames), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and _guards_intact(buf, bsz * n, offset)
    if not in_place:
        assert _guards_intact(sbuf, bsz * n, offset) and nr.same_bits(src.cpu().numpy(), y)
    return out.cpu().numpy()


@pytest.mark.parametrize("sigma,gain,bits,full_scale", nr.GRID)
@pytest.mark.parametrize("bsz,n,offset", SHAPES)
def test_sensor_noise_equals_the_emulation_on_the_devices_normals(bsz, n, offset, sigma, gain, bits, full_scale):
    seqs, y = _seqs(bsz), nr.ramp(bsz, n)
    model = SensorNoise(sigma, gain, bits, full_scale, seed=SEED)
    nrm = _normals(seqs, n)
    want = nr.sensor_f32(y, nrm, sigma, gain, bits, full_scale or 8.0)
    got = _sensor(y, seqs, model, 8, offset, in_place=False)
    assert nr.same_bits(got, want)
    assert nr.same_bits(_sensor(y, seqs, model, 8, offset, in_place=True), got)           # in place equals out of place
    bad = ~np.isfinite(y)
    assert nr.same_bits(got[bad], y[bad]) and (bad.sum() == 3 or y.size < 8)              # NaN, +Inf, -Inf come back unchanged
    if not model.enabled:
        assert nr.same_bits(got, y)                                                       # the identity row
    if bsz == 65:
        assert nr.same_bits(got[64:65], _sensor(y[64:65], seqs[64:], model, 8, 0, in_place=False))


def test_sensor_noise_refuses_partial_overlap_and_bad_parameters():
    buf = torch.zeros(64, device=DEV)
    y, out = buf[:32].view(1, 32), buf[4:36].view(1, 32)
    with pytest.raises(_hip.DeqsciHipError, match="-4"):
        _hip.sensor_noise(y, [0], 0, 0.02, 0.0, 0, 1.0, out=out)
    with pytest.raises(_hip.DeqsciHipError, match="-4"):
        _hip.sensor_noise(y, [0], 0, 0.02, 0.0, 17, 1.0)
    with pytest.raises(_hip.DeqsciHipError):
        _hip.sensor_noise(y, [0, 1], 0, 0.02, 0.0, 0, 1.0)                                # two sequence numbers, one sample


# ----------------------------------------------------------------------------- the consumers, on a device pool
H, W, B = 16, 16, 8


def _pool():
    if "pool" not in _CACHE:
        rng = np.random.RandomState(5)
        _CACHE["pool"] = synth.VideoPool([rng.randint(0, 256, size=s).astype(np.uint8) for s in ((12, 20, 24), (9, 18, 17))], DEV)
        _CACHE["mask"] = (rng.rand(H, W, B) < 0.5).astype(np.float32)
    return _CACHE["pool"], _CACHE["mask"]


def test_synthesize_with_noise_changes_meas_only():
    pool, mask = _pool()
    specs = synth.sample_specs(pool, 5, H, W, B, np.random.default_rng(1))
    seq = [3, 1 << 33, 5, 6, 7]
    model = SensorNoise(sigma=5 / 255, gain=0.01, bits=10, seed=77)
    gt, meas = synth.synthesize(pool, specs, mask)
    g, m = synth.synthesize(pool, specs, mask, model, seq)
    assert torch.equal(g, gt) and not torch.equal(m, meas)
    assert nr.same_bits(m.cpu().numpy(), model.apply(meas, seq, frames=B).cpu().numpy())
    assert nr.same_bits(meas.cpu().numpy(), synth.synthesize(pool, specs, mask, SensorNoise(), None)[1].cpu().numpy())
    host = model.apply(meas.cpu().numpy(), seq, frames=B)                                 # the host restatement: equal to within the normals'
    step = B / (2 ** 10 - 1)                                                              # tolerance, i.e. at most one ADC step apart
    assert np.abs(host - m.cpu().numpy()).max() <= step * 1.001


def test_loader_noise_does_not_depend_on_the_batch_size_on_the_device():
    pool, mask = _pool()
    model = SensorNoise(sigma=5 / 255, gain=0.01, bits=10, seed=77)

    def epoch(bsz, noise, start_epoch=0):
        batches = list(synth.SynthTrainLoader(pool, mask, bsz, 8, H, W, B, seed=3, start_epoch=start_epoch, noise=noise))
        return torch.cat([b["gt"] for b in batches]), torch.cat([b["meas"] for b in batches])
    (g0, m0), (g2, m2), (g4, m4) = epoch(2, None), epoch(2, model), epoch(4, model)
    assert torch.equal(m2, m4) and not torch.equal(m2, m0) and torch.equal(g2, g0) and torch.equal(g4, g0)
    assert torch.equal(m2, model.apply(m0, list(range(8)), frames=B))
    assert torch.equal(epoch(4, model, start_epoch=1)[1], model.apply(epoch(4, None, start_epoch=1)[1], list(range(8, 16)), frames=B))
