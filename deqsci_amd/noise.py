"""Sensor noise on a reproducible random source: the host side of csrc/noise.hip (include/deqsci_hip.h states generator, counter layout and
order of operations).

    philox4x32_10(counter, key)        the numpy restatement of the generator (uint64 arithmetic): (..., 4) and (..., 2) uint32 -> (..., 4)
    group_words(bsz, n, seq, seed)     the words kernel N0 writes, (bsz, ceil(n / 4), 4) uint32
    normal_host(bsz, n, seq, seed)     the normals of kernel N1, computed in float64 and rounded to fp32 - equal to the device's to within
                                       the error of its logf / sincospif, NOT bit for bit
    SensorNoise(sigma, gain, bits, full_scale, seed)
        .enabled                       False when sigma, gain and bits are all zero: nothing is drawn, nothing is launched
        .apply(meas, seq, frames)      meas (bsz,H,W) -> the noisy measurement: device tensors through kernel N2, CPU tensors and numpy
                                       arrays through the restatement of N2's fp32 order on normal_host

The model is the usual Gaussian approximation of Poisson-Gaussian noise followed by an ADC: variance gain * y + sigma^2, then `bits` bits
over [0, full_scale].  y is in the loader's units (grey / 255, summed over the frames), sigma in the same units (5 grey levels: 5 / 255).
Element e of a sample is a function of (seed, seq, e): the caller's rule for seq decides what "the same sample" means (synth.py: the
position in the epoch; harness.py: (clip << 32) | measurement), and nothing else - batch size, launch geometry, rank count - enters.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import _hip

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10: counter (..., 4), key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] & _LO for i in range(4))
    k0, k1 = k[..., 0] & _LO, k[..., 1] & _LO
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + np.uint64(W0)) & _LO, (k1 + np.uint64(W1)) & _LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _seq_u64(seq, bsz):
    vals = [int(v) for v in np.asarray(seq, dtype=object).reshape(-1)]
    if len(vals) != bsz or any(v < 0 or v >= 1 << 64 for v in vals):
        raise ValueError(f"seq: {bsz} sequence numbers in 0 .. 2^64 - 1 expected, got {len(vals)}")
    return np.asarray(vals, dtype=np.uint64)


def group_words(bsz, n, seq, seed):
    """(bsz, ceil(n / 4), 4) uint32: counter (g low, g high, seq low, seq high), key (seed low, seed high)."""
    seq, seed = _seq_u64(seq, bsz), int(seed) & ((1 << 64) - 1)
    g = np.arange(-(-int(n) // 4), dtype=np.uint64)
    counter = np.empty((bsz, g.size, 4), np.uint64)
    counter[..., 0], counter[..., 1] = g & _LO, g >> _S32
    counter[..., 2], counter[..., 3] = (seq & _LO)[:, None], (seq >> _S32)[:, None]
    return philox4x32_10(counter, np.asarray([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))


def normals_from_words(words, n):
    """The Box-Muller step of N1 in float64: (bsz, groups, 4) uint32 -> (bsz, n) float64."""
    u = ((np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u[..., 0::2]))                             # (bsz, groups, 2): from x0 and x2
    t = 2.0 * u[..., 1::2]                                               # from x1 and x3; sin(pi t), cos(pi t) by quadrants: the
    q = np.rint(2.0 * t)                                                 # reduction t - q / 2 is exact, so the small values near the
    f = np.pi * (t - 0.5 * q)                                            # zeros keep their relative accuracy
    s0, c0, q = np.sin(f), np.cos(f), q.astype(np.int64) & 3
    s = np.choose(q, [s0, c0, -s0, -c0])
    c = np.choose(q, [c0, -s0, -c0, s0])
    out = np.stack([r * c, r * s], axis=-1)                              # (bsz, groups, pair, {cos, sin}) = elements 4g .. 4g+3
    return out.reshape(out.shape[0], -1)[:, :int(n)]


def normal_host(bsz, n, seq, seed):
    """(bsz, n) fp32: the normals kernel N1 draws, from float64 arithmetic."""
    return normals_from_words(group_words(bsz, n, seq, seed), n).astype(np.float32)


def sensor_f32(y, nrm, sigma, gain, bits, full_scale):
    """N2's order of operations on given normals, every step one fp32 rounding (numpy arrays of float32 in, float32 out)."""
    f = np.float32
    y, nrm = np.asarray(y, dtype=f), np.asarray(nrm, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(y)
        p = np.fmax(np.where(finite, y, f(0)), f(0))
        v = f(gain) * p
        v = v + f(sigma) * f(sigma)
        t = np.sqrt(v) * nrm
        o = y + t
        if bits > 0:
            L = f(2 ** int(bits) - 1)
            c = o / f(full_scale)
            c = np.fmin(np.fmax(c, f(0)), f(1))
            o = (np.rint(c * L) / L) * f(full_scale)
    return np.where(finite, o, y).astype(f)


@dataclass(frozen=True)
class SensorNoise:
    """sigma: read noise, in the measurement's units (grey / 255); gain: shot-noise variance per unit of signal; bits: the ADC's width, 0 for
    none; full_scale: the ADC's top, None for the number of frames B (the largest sum a binary mask can give); seed: Philox' 64-bit key."""
    sigma: float = 0.0
    gain: float = 0.0
    bits: int = 0
    full_scale: float = None
    seed: int = 0

    def __post_init__(self):
        ok = np.isfinite(self.sigma) and self.sigma >= 0 and np.isfinite(self.gain) and self.gain >= 0 and int(self.bits) == self.bits \
            and 0 <= self.bits <= 16 and (self.full_scale is None or (np.isfinite(self.full_scale) and self.full_scale > 0))
        if not ok:
            raise ValueError(f"{self}: sigma, gain >= 0 and finite, bits in 0..16, full_scale > 0 and finite (or None) expected")

    @property
    def enabled(self):
        return bool(self.sigma or self.gain or self.bits)

    def scale(self, frames=None):
        """The ADC's top: full_scale, or the number of frames where none was given."""
        if self.full_scale is not None:
            return float(self.full_scale)
        if not self.bits:
            return 1.0                                                   # (no quantiser: the value is checked, never used)
        if frames is None:
            raise ValueError("SensorNoise: a quantiser without full_scale needs the number of frames")
        return float(frames)

    def describe(self, frames=None):
        top = "the frames per measurement" if self.full_scale is None and frames is None else f"{self.scale(frames):g}"
        adc = f"{self.bits} bits over [0, {top}]" if self.bits else "no quantiser"
        return f"sigma {self.sigma * 255:g}/255, gain {self.gain:g}, {adc}, seed {self.seed}"

    def apply(self, meas, seq, frames=None, out=None):
        """meas (bsz, H, W) -> the noisy measurement, sample k drawn with sequence number seq[k].  frames: B, for full_scale=None.
        A device tensor goes through kernel N2 (out=meas: in place); a CPU tensor or numpy array through the host restatement (fp32 order
        of N2 on normal_host: the device's values to within the tolerance of the normals).  Disabled: meas itself."""
        if not self.enabled:
            return meas
        if isinstance(meas, torch.Tensor) and meas.is_cuda:
            return _hip.sensor_noise(meas, seq, self.seed, self.sigma, self.gain, self.bits, self.scale(frames), out=out)
        a = meas.numpy() if isinstance(meas, torch.Tensor) else np.asarray(meas)
        if a.dtype != np.float32 or a.ndim < 1:
            raise ValueError(f"SensorNoise.apply: float32 (bsz, H, W) expected, got {a.dtype} {a.shape}")
        bsz = a.shape[0]
        n = a.size // bsz if bsz else 1
        got = sensor_f32(a.reshape(bsz, n), normal_host(bsz, n, seq, self.seed), self.sigma, self.gain, self.bits,
                         self.scale(frames)).reshape(a.shape)
        return torch.from_numpy(got) if isinstance(meas, torch.Tensor) else got


def add_noise_arguments(group):
    """The sensor-noise flags of deqsci_amd.cli and `python -m deqsci_amd.synth write`."""
    group.add_argument("--meas_noise_sigma", type=float, default=0.0, help="read noise in 8-bit grey levels (divided by 255, as FFDNet's sigma is)")
    group.add_argument("--meas_noise_gain", type=float, default=0.0, help="shot noise: variance per unit of signal (grey / 255, summed over the frames)")
    group.add_argument("--meas_bits", type=int, default=0, help="ADC width in bits; 0: no quantiser")
    group.add_argument("--meas_full_scale", type=float, default=None, help="the ADC's top; default: the frames per measurement")
    group.add_argument("--noise_seed", type=int, default=None, help="the generator's 64-bit key; default: --seed, or 0")


def noise_from_arguments(a, seed=None):
    """-> the SensorNoise the flags describe, None when they describe none."""
    key = a.noise_seed if a.noise_seed is not None else (seed if seed is not None else 0)
    model = SensorNoise(sigma=a.meas_noise_sigma / 255.0, gain=a.meas_noise_gain, bits=a.meas_bits, full_scale=a.meas_full_scale, seed=int(key))
    return model if model.enabled else None
