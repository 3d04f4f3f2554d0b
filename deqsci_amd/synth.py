"""Training samples out of raw video: what the reference made ahead of time with MATLAB scripts it does not ship (mask.mat, gt/*.mat,
measurement/*.mat under --trainpath), made per batch from a pool of uint8 frames.

    load_video(path)                 .npy (T,H,W) / (T,H,W,3) uint8, or .mat with key 'orig' (H,W,T) as the shipped clips -> (T,H,W) uint8
    VideoPool(videos, device)        the frames of all videos as ONE uint8 buffer on the device (on "cpu": numpy) + the per-video table
    PatchSpec                        one descriptor row of csrc/synth.hip: where a (H,W,B) block is cut out of a video and how it is turned
    sample_specs(pool, n, H, W, B, rng, ...)   n descriptors that fit, a video drawn in proportion to its number of admissible crops
    synthesize(pool, specs, mask)    -> (gt (n,H,W,B), meas (n,H,W)): ONE launch per 64 samples on a device pool (_hip.synth_batch), the
                                     numpy / fp32 restatement of the same order of operations on a CPU pool
    SynthTrainLoader(...)            what train_solver_sci takes as train_dataloader: dicts {'gt', 'meas', 'mask'}, epoch e drawn from
                                     np.random.default_rng([seed, e]) - a resumed run draws the batches the uninterrupted run would have
    write_training_directory(...)    the same samples in the reference's directory format (what SCITrainingDatasetSubset reads)

    python -m deqsci_amd.synth write --videos DIR --mask FILE --out DIR --n N --seed S [--patch_size 256] [--frames 8] [--augment ...]
                                     [--meas_noise_sigma S --meas_noise_gain G --meas_bits N --meas_full_scale F --noise_seed K]

synthesize, SynthTrainLoader and write_training_directory take noise=, a noise.SensorNoise: the measurement (never gt) goes through the
sensor model of csrc/noise.hip, each sample under a sequence number that names it whatever the batch size.

A sample is a choice of crop and orientation; the stored measurement is redundant (meas = sum_b mask_b gt_b).  The arithmetic is pinned
(include/deqsci_hip.h, Y1): fp32 s <- s + mask_b u_b for b ascending, one fp32 division by 255.  With a mask of zeros and ones and
B <= 64 that is the float nearest sum / 255 - the value load_mat returns for the written file - and from the `orig` frames and the mask
of the shipped clips it regenerates their measurements bit for bit.  Decoding PNG or MP4 is out of scope: bring frames as .npy.
"""
import os
from collections import namedtuple

import numpy as np
import torch

from . import _hip

FLIP_H, FLIP_V, TRANSPOSE = _hip.SYNTH_FLIP_H, _hip.SYNTH_FLIP_V, _hip.SYNTH_TRANSPOSE
MAX_FRAMES = _hip.SYNTH_MAX_FRAMES
AUGMENT_ALL = ("flip", "transpose", "reverse")

PatchSpec = namedtuple("PatchSpec", "video_offset T Hv Wv t0 dt y0 x0 ds flags")
Video = namedtuple("Video", "name offset T H W")


def rgb_to_gray(rgb):
    """(..., 3) uint8 -> (...) uint8: (77 R + 150 G + 29 B + 128) >> 8, the integer statement of csrc/synth.hip's Y0."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape[-1] != 3:
        raise ValueError(f"rgb_to_gray: (..., 3) uint8 expected, got {rgb.dtype} {rgb.shape}")
    v = rgb.astype(np.uint32)
    return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).astype(np.uint8)


def _as_frames(a, what):
    """(T,H,W) or (T,H,W,3) of integers in 0..255 -> (T,H,W) uint8 (colour through Y0's formula)"""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        if a.size and not (np.all(a == np.floor(a)) and a.min() >= 0 and a.max() <= 255):
            raise ValueError(f"{what}: frames must hold the integers 0..255, got {a.dtype} in [{a.min()}, {a.max()}]")
        a = a.astype(np.uint8)
    if a.ndim == 4 and a.shape[3] == 3:
        a = rgb_to_gray(a)
    if a.ndim != 3 or 0 in a.shape:
        raise ValueError(f"{what}: (T,H,W) or (T,H,W,3) frames expected, got shape {a.shape}")
    return np.ascontiguousarray(a)


def load_video(path):
    """-> (T,H,W) uint8.  .npy: (T,H,W) or (T,H,W,3) uint8; .mat: key 'orig', (H,W,T), as the shipped test clips store it."""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
        if a.dtype != np.uint8:
            raise ValueError(f"{path}: uint8 frames expected, got {a.dtype}")
        return _as_frames(a, path)
    if ext == ".mat":
        import scipy.io as sio
        f = sio.loadmat(path)
        if "orig" not in f:
            raise KeyError(f"{path}: no key 'orig'")
        return _as_frames(np.asarray(f["orig"]).transpose(2, 0, 1), path)
    raise ValueError(f"{path}: .npy or .mat expected (decoding images or movies is out of scope: store the frames as .npy)")


def list_videos(directory):
    """The .npy / .mat files of a directory, sorted."""
    names = sorted(f for f in os.listdir(directory) if f.lower().endswith((".npy", ".mat")) and not f.startswith("."))
    if not names:
        raise FileNotFoundError(f"{directory}: no .npy or .mat video found")
    return [os.path.join(directory, f) for f in names]


class VideoPool:
    """The frames of every video, concatenated: `data`, a flat uint8 tensor on `device` (a numpy array on "cpu"), and `videos`, one
    Video(name, offset, T, H, W) per entry.  videos: paths (load_video) or (T,H,W) / (T,H,W,3) arrays; a colour array goes through
    Y0 - on the device where there is one."""

    def __init__(self, videos, device="cuda"):
        self.device = torch.device(device)
        self.videos, parts, offset = [], [], 0
        for k, v in enumerate(videos):
            name = str(v) if isinstance(v, (str, os.PathLike)) else f"video[{k}]"
            if isinstance(v, (str, os.PathLike)):
                frames = load_video(v)
            else:
                v = np.asarray(v)
                if self.device.type == "cuda" and v.dtype == np.uint8 and v.ndim == 4 and v.shape[3] == 3 and v.size:
                    frames = _hip.rgb_to_gray(torch.from_numpy(np.ascontiguousarray(v)).to(self.device)).cpu().numpy()
                else:
                    frames = _as_frames(v, name)
            T, H, W = frames.shape
            self.videos.append(Video(name, offset, T, H, W))
            parts.append(frames.reshape(-1))
            offset += frames.size
        if not parts:
            raise ValueError("VideoPool: no video given")
        flat = np.concatenate(parts)
        self.data = flat if self.device.type == "cpu" else torch.from_numpy(flat).to(self.device)
        self.nbytes = int(flat.size)

    def __len__(self):
        return len(self.videos)

    def video_at(self, offset):
        """The Video whose frames start at byte `offset`."""
        for v in self.videos:
            if v.offset == offset:
                return v
        raise ValueError(f"no video of the pool starts at byte {offset}")

    def frames(self, k):
        """Video k as a (T,H,W) uint8 numpy array (a copy from the device)."""
        v = self.videos[k]
        flat = self.data[v.offset:v.offset + v.T * v.H * v.W]
        return (flat.copy() if isinstance(flat, np.ndarray) else flat.cpu().numpy()).reshape(v.T, v.H, v.W)


def check_spec(pool, spec, H, W, B):
    """The entry point's own test of a row, on the host: ValueError when the row names no video of the pool or reads outside it."""
    s = PatchSpec(*(int(x) for x in spec))
    v = pool.video_at(s.video_offset)
    Hc, Wc = (W, H) if s.flags & TRANSPOSE else (H, W)
    ok = (s.T, s.Hv, s.Wv) == (v.T, v.H, v.W) and s.ds >= 1 and s.dt != 0 and 0 <= s.flags <= 7 and 1 <= B <= MAX_FRAMES \
        and 0 <= s.t0 < s.T and 0 <= s.t0 + s.dt * (B - 1) < s.T and 0 <= s.y0 and s.y0 + s.ds * (Hc - 1) < s.Hv \
        and 0 <= s.x0 and s.x0 + s.ds * (Wc - 1) < s.Wv
    if not ok:
        raise ValueError(f"{s} does not fit {v} at patch {H}x{W}x{B}")
    return s


def sample_specs(pool, n, H, W, B, rng, augment=AUGMENT_ALL, max_dt=1, max_ds=1):
    """n PatchSpecs that fit.  Every admissible (video, |dt| <= max_dt, ds <= max_ds, orientation of the crop, t0, y0, x0) is equally
    likely, so a video contributes in proportion to its number of admissible crops; the flips and the sign of dt (augment: "flip",
    "reverse") are fair coins on top, "transpose" admits the (W,H) crop beside the (H,W) one.  A video no crop fits in raises
    ValueError with its name.  rng: a numpy Generator; the draws are a function of its state alone."""
    augment = tuple(augment or ())
    unknown = set(augment) - set(AUGMENT_ALL)
    if unknown or max_dt < 1 or max_ds < 1 or not 1 <= B <= MAX_FRAMES or H < 1 or W < 1:
        raise ValueError(f"sample_specs: augment {augment} of {AUGMENT_ALL}, max_dt / max_ds >= 1, 1 <= B <= {MAX_FRAMES}, H, W >= 1")
    orientations = (0, TRANSPOSE) if "transpose" in augment else (0,)
    configs, counts = [], []
    for v in pool.videos:
        found = 0
        for tr in orientations:
            Hc, Wc = (W, H) if tr else (H, W)
            for dt in range(1, max_dt + 1):
                nt = v.T - dt * (B - 1)
                for ds in range(1, max_ds + 1):
                    ny, nx = v.H - ds * (Hc - 1), v.W - ds * (Wc - 1)
                    if nt >= 1 and ny >= 1 and nx >= 1:
                        configs.append((v, tr, dt, ds, nt, ny, nx))
                        counts.append(nt * ny * nx)
                        found += 1
        if not found:
            raise ValueError(f"sample_specs: no {H}x{W}x{B} patch fits video {v.name!r} ({v.T} frames of {v.H}x{v.W})")
    p = np.asarray(counts, dtype=np.float64)
    picks = rng.choice(len(configs), size=int(n), p=p / p.sum())
    out = []
    for k in picks:
        v, tr, dt, ds, nt, ny, nx = configs[int(k)]
        first, y0, x0 = int(rng.integers(nt)), int(rng.integers(ny)), int(rng.integers(nx))
        flags = tr
        if "flip" in augment:
            flags |= (FLIP_H if rng.integers(2) else 0) | (FLIP_V if rng.integers(2) else 0)
        if "reverse" in augment and rng.integers(2):
            t0, dt = first + dt * (B - 1), -dt                       # the same frames, last to first
        else:
            t0 = first
        out.append(PatchSpec(v.offset, v.T, v.H, v.W, t0, dt, y0, x0, ds, flags))
    return out


def spec_table(specs):
    """-> the (n, 10) int64 array the entry point reads"""
    return np.asarray([tuple(int(x) for x in s) for s in specs], dtype=np.int64).reshape(len(specs), _hip.SYNTH_ROW_WORDS)


def gather_u8(pool, spec, H, W, B):
    """The (H,W,B) uint8 block a spec names, by the geometry of include/deqsci_hip.h (Y1), out of a CPU pool."""
    s = check_spec(pool, spec, H, W, B)
    video = pool.data[s.video_offset:s.video_offset + s.T * s.Hv * s.Wv].reshape(s.T, s.Hv, s.Wv)
    Hc, Wc = (W, H) if s.flags & TRANSPOSE else (H, W)
    r, c = np.arange(Hc), np.arange(Wc)
    if s.flags & FLIP_V:
        r = Hc - 1 - r
    if s.flags & FLIP_H:
        c = Wc - 1 - c
    crop = video[s.t0 + s.dt * np.arange(B)][:, s.y0 + s.ds * r][:, :, s.x0 + s.ds * c]          # [b, r, c]
    return np.ascontiguousarray(crop.transpose(2, 1, 0) if s.flags & TRANSPOSE else crop.transpose(1, 2, 0))


def snapshot_f32(u, mask):
    """(gt, meas) of one uint8 block in Y1's arithmetic: fp32, s <- s + mask_b u_b for b ascending (product and sum rounded separately),
    then one division by 255; gt = u / 255."""
    uf, mask = u.astype(np.float32), np.asarray(mask, dtype=np.float32)
    s = np.zeros(u.shape[:2], np.float32)
    for b in range(u.shape[2]):
        s = s + mask[..., b] * uf[..., b]
    return uf / np.float32(255), s / np.float32(255)


def _mask_for(mask, n, H, W, B):
    shape = tuple(mask.shape)
    if shape not in ((H, W, B), (n, H, W, B)):
        raise ValueError(f"mask {shape}: ({H},{W},{B}) or ({n},{H},{W},{B}) expected")
    return len(shape) == 4


def _noise_seq(noise, seq, n, what):
    """None where `noise` draws nothing; otherwise the n sequence numbers, which the caller must have given."""
    if noise is None or not noise.enabled or n == 0:
        return None
    if seq is None or len(seq) != n:
        raise ValueError(f"{what}: an enabled noise model needs seq, one sequence number per sample ({n})")
    return [int(v) for v in seq]


def synthesize(pool, specs, mask, noise=None, seq=None):
    """-> (gt (n,H,W,B), meas (n,H,W)) fp32: torch tensors on a device pool's device (csrc/synth.hip, one launch per 64 samples, no host
    round trip), numpy arrays from a CPU pool (the restatement).  mask: (H,W,B) for all samples or (n,H,W,B); its shape sets the patch.
    noise: a noise.SensorNoise; where it is enabled, meas goes through it after Y1 - in place, as a launch of its own (csrc/noise.hip,
    N2), sample k drawn with sequence number seq[k]; gt stays clean.  None or a disabled model: no launch, the same bits as ever."""
    n = len(specs)
    H, W, B = (int(x) for x in mask.shape[-3:])
    per_sample = _mask_for(mask, n, H, W, B)
    seq = _noise_seq(noise, seq, n, "synthesize")
    if pool.device.type != "cpu":
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32))
        gt, meas = _hip.synth_batch(pool.data, spec_table(specs), m.to(pool.device, torch.float32).contiguous(), H, W, B)
        if seq is not None:
            noise.apply(meas, seq, frames=B, out=meas)
        return gt, meas
    mask = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    gt, meas = np.empty((n, H, W, B), np.float32), np.empty((n, H, W), np.float32)
    for k, s in enumerate(specs):
        gt[k], meas[k] = snapshot_f32(gather_u8(pool, s, H, W, B), mask[k] if per_sample else mask)
    if seq is not None:
        meas = noise.apply(meas, seq, frames=B)
    return gt, meas


class SynthTrainLoader:
    """train_solver_sci's train_dataloader, from a VideoPool: len(self) = patches_per_epoch // batch_size batches per epoch, each a dict
    {'gt' (bsz,H,W,B), 'meas' (bsz,H,W), 'mask' (bsz,H,W,B)} of fp32 tensors on the pool's device.  Every __iter__ draws its epoch's
    descriptors from np.random.default_rng([seed, epoch]) and advances the epoch, so a run resumed with start_epoch=e draws what the
    uninterrupted run drew in epoch e.  mask: (H,W,B) zeros and ones (anything else trains too, but then a written directory would not
    hold the same bits).  **sampling: sample_specs' augment, max_dt, max_ds.
    noise: a noise.SensorNoise for the measurements (gt stays clean).  Sample i of epoch e - i its position in epoch_specs(e) - is drawn
    with sequence number e * patches_per_epoch + i: its noise depends neither on batch_size nor on where a run was resumed."""

    def __init__(self, pool, mask, batch_size, patches_per_epoch, H, W, B, seed, start_epoch=0, noise=None, **sampling):
        mask = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32))
        if tuple(mask.shape) != (H, W, B):
            raise ValueError(f"SynthTrainLoader: mask {tuple(mask.shape)} is not the patch ({H},{W},{B})")
        if batch_size < 1 or patches_per_epoch < batch_size:
            raise ValueError(f"SynthTrainLoader: batch_size {batch_size} >= 1 and patches_per_epoch {patches_per_epoch} >= batch_size expected")
        self.pool, self.batch_size, self.patches_per_epoch = pool, int(batch_size), int(patches_per_epoch)
        self.H, self.W, self.B, self.seed, self.epoch, self.sampling = int(H), int(W), int(B), int(seed), int(start_epoch), dict(sampling)
        self.noise = noise if noise is not None and noise.enabled else None
        self.mask = mask.to(pool.device, torch.float32).contiguous()
        self.mask_batch = self.mask[None].repeat(self.batch_size, 1, 1, 1).contiguous()          # what a DataLoader's collate would build
        sample_specs(pool, 0, self.H, self.W, self.B, np.random.default_rng(0), **self.sampling)  # a pool nothing fits in fails here, by name

    def __len__(self):
        return self.patches_per_epoch // self.batch_size

    def epoch_specs(self, epoch):
        """The descriptors of an epoch, batch after batch."""
        return sample_specs(self.pool, len(self) * self.batch_size, self.H, self.W, self.B, np.random.default_rng([self.seed, int(epoch)]),
                            **self.sampling)

    def epoch_seq(self, epoch):
        """The sequence numbers of an epoch's samples, in epoch_specs' order."""
        first = int(epoch) * self.patches_per_epoch
        return list(range(first, first + len(self) * self.batch_size))

    def batch(self, specs, seq=None):
        gt, meas = synthesize(self.pool, specs, self.mask, self.noise, seq)
        if self.pool.device.type == "cpu":
            gt, meas = torch.from_numpy(gt), torch.from_numpy(meas)
        return {'gt': gt, 'meas': meas, 'mask': self.mask_batch}

    def __iter__(self):
        specs, seq = self.epoch_specs(self.epoch), self.epoch_seq(self.epoch)
        self.epoch += 1
        bsz = self.batch_size
        return (self.batch(specs[k * bsz:(k + 1) * bsz], seq[k * bsz:(k + 1) * bsz]) for k in range(len(self)))


def write_training_directory(out_dir, pool, mask, specs, noise=None, seq=None):
    """The reference's training directory for these samples: mask.mat (key 'mask'), gt/%06d.mat (key 'patch_save', uint8 (H,W,B)),
    measurement/%06d.mat (key 'meas', float64 sum_b mask_b u_b) - sample k in file k, so a sorted listing keeps the order of `specs`.
    -> the directory with the trailing '/' SCITrainingDatasetSubset's string joins need.
    noise (a noise.SensorNoise) and seq (one sequence number per sample): the measurement written is the noisy one, from the HOST
    restatement - Y1's fp32 snapshot through SensorNoise.apply on a CPU array, stored as float64(meas_fp32) * 255.  It equals what a
    SynthTrainLoader with the same model and sequence numbers yields to within the tolerance of the normals (the device's logf and
    sincospif against float64), NOT bit for bit; gt stays clean."""
    import scipy.io as sio
    mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask, dtype=np.float64)
    H, W, B = mask.shape
    seq = _noise_seq(noise, seq, len(specs), "write_training_directory")
    host = pool if pool.device.type == "cpu" else _host_view(pool)
    out_dir = str(out_dir)
    os.makedirs(os.path.join(out_dir, "gt"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "measurement"), exist_ok=True)
    sio.savemat(os.path.join(out_dir, "mask.mat"), {"mask": mask})
    for k, s in enumerate(specs):
        u = gather_u8(host, s, H, W, B)
        sio.savemat(os.path.join(out_dir, "gt", "%06d.mat" % k), {"patch_save": u})
        if seq is None:
            meas = (mask * u.astype(np.float64)).sum(axis=2)
        else:
            clean = snapshot_f32(u, mask.astype(np.float32))[1]
            meas = noise.apply(clean[None], seq[k:k + 1], frames=B)[0].astype(np.float64) * 255.0
        sio.savemat(os.path.join(out_dir, "measurement", "%06d.mat" % k), {"meas": meas})
    return out_dir.rstrip("/") + "/"


def _host_view(pool):
    """A CPU pool over the same frames (the writer works on the host)."""
    host = VideoPool.__new__(VideoPool)
    host.device, host.videos, host.nbytes, host.data = torch.device("cpu"), list(pool.videos), pool.nbytes, pool.data.cpu().numpy()
    return host


def load_mask(path, H, W, B):
    """--trainmask: key 'mask' of a .mat (a test clip will do), its leading (H,W,B) corner."""
    import scipy.io as sio
    f = sio.loadmat(str(path))
    if "mask" not in f:
        raise KeyError(f"{path}: no key 'mask'")
    mask = np.asarray(f["mask"], dtype=np.float32)
    if mask.ndim != 3 or mask.shape[0] < H or mask.shape[1] < W or mask.shape[2] < B:
        raise ValueError(f"{path}: mask {mask.shape} is smaller than the patch ({H},{W},{B})")
    return np.ascontiguousarray(mask[:H, :W, :B])


def parse_augment(text):
    """'flip,transpose,reverse' / 'none' -> sample_specs' augment"""
    names = tuple(v.strip() for v in str(text).split(",") if v.strip() and v.strip() != "none")
    if set(names) - set(AUGMENT_ALL):
        raise ValueError(f"augment {text!r}: a comma-separated choice of {', '.join(AUGMENT_ALL)}, or none")
    return names


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m deqsci_amd.synth", description="training samples out of raw video")
    sub = p.add_subparsers(dest="command", required=True)
    w = sub.add_parser("write", help="write the reference's training directory (mask.mat, gt/, measurement/)")
    w.add_argument("--videos", required=True, help="directory of .npy / .mat videos")
    w.add_argument("--mask", required=True, help=".mat with key 'mask'")
    w.add_argument("--out", required=True)
    w.add_argument("--n", type=int, required=True)
    w.add_argument("--seed", type=int, default=0)
    w.add_argument("--patch_size", type=int, default=256)
    w.add_argument("--frames", type=int, default=8)
    w.add_argument("--augment", default=",".join(AUGMENT_ALL))
    w.add_argument("--max_dt", type=int, default=1)
    w.add_argument("--max_ds", type=int, default=1)
    from .noise import add_noise_arguments, noise_from_arguments
    add_noise_arguments(w.add_argument_group("sensor noise", "the measurements written are noisy; sample k is drawn with sequence number k"))
    a = p.parse_args(argv)
    pool = VideoPool(list_videos(a.videos), "cpu")
    mask = load_mask(a.mask, a.patch_size, a.patch_size, a.frames)
    specs = sample_specs(pool, a.n, a.patch_size, a.patch_size, a.frames, np.random.default_rng([a.seed, 0]), augment=parse_augment(a.augment),
                         max_dt=a.max_dt, max_ds=a.max_ds)
    noise = noise_from_arguments(a, a.seed)
    out = write_training_directory(a.out, pool, mask, specs, noise, list(range(len(specs))))
    print(f"{len(specs)} samples of {a.patch_size}x{a.patch_size}x{a.frames} from {len(pool)} videos -> {out}")
    if noise is not None:
        print(f"sensor noise on the measurements: {noise.describe(a.frames)}")
    return out


if __name__ == "__main__":
    main()
