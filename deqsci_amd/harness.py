"""Evaluation harness: clips in, reconstructions + PSNR out.

The unit of work here is a CLIP (one .mat file: mask, M snapshot measurements, 8*M ground-truth frames).
`reconstruct_clip` hands ALL measurements of a clip to the DEQ module as one batch sharing the clip's mask
(the reference feeds them one by one, training/sci_equilibrium_training.py:171-181; rows of a batch are
independent problems, so the results are the same unless the whole-batch tolerance test fires - SURVEY 8(a)
caveat), optionally sharded over the ranks of a process group (deqsci_amd.distributed).  `evaluate` walks a
directory of clips; `test_solver_sci` is a thin adapter with the reference's signature, return value,
printed lines and PNG naming (ibid. :152-205) on top of the two.

    load_test_data / SCITestDataset   utils/sci_dataloader.py:241-274 (MATLAB v5 files, sorted file order)
    psnr                              skimage.metrics.peak_signal_noise_ratio for float input, data range 1
    ssim / clip_ssim                  pytorch_ssim._ssim per frame (this build's addition: the reference harness reports PSNR only)
    frame_payload                     the float image the reference hands to cv2.imwrite (ibid. :19-21)
    init="gaptv" / method="gaptv"     the DEQ started from GAP-TV (utils/cg_utils.py:234, commented out there) / GAP-TV alone
                                      (this build's additions, deqsci_amd.gaptv)
"""
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import distributed, operators

FIRST_MEASUREMENT_ONLY = ("drop", "runner")      # clips the reference scores on snapshot 0 only (:167-168)


def load_test_data(matfile):
    """-> {'gt' (H,W,B*M) in [0,1], 'mask' (H,W,B), 'meas' (H,W,M) scaled by 1/255}, all float32."""
    import scipy.io as sio
    try:
        f = sio.loadmat(matfile)
        meas, mask, orig = np.float32(f['meas']), np.float32(f['mask']), np.float32(f['orig'])
    except NotImplementedError as e:                      # MATLAB v7.3 = HDF5 (utils/sci_dataloader.py:249-254)
        try:
            import h5py
        except ImportError:
            raise NotImplementedError(f"{matfile}: MATLAB v7.3 files need h5py, which is not installed") from e
        with h5py.File(matfile, 'r') as f:                # HDF5 keeps MATLAB's column-major order: transpose back
            meas = np.float32(f['meas']).transpose()
            mask = np.float32(f['mask']).transpose()
            orig = np.float32(f['orig']).transpose()
    return {'gt': orig / 255, 'mask': mask, 'meas': meas / 255}


def directory_filelist(target_directory):
    return [f for f in sorted(os.listdir(target_directory))
            if os.path.isfile(os.path.join(target_directory, f)) and not f.startswith('.')]


class SCITestDataset(torch.utils.data.Dataset):
    def __init__(self, dir):
        self.dir = dir
        self.filelist = directory_filelist(dir)

    def __len__(self):
        return len(self.filelist)

    def __getitem__(self, item):
        data = load_test_data(os.path.join(self.dir, self.filelist[item]))
        data['file'] = self.filelist[item]
        return data


def psnr(rec, gt):
    a = np.asarray(gt, dtype=np.float32)
    b = np.asarray(rec, dtype=np.float32)
    return 10.0 * math.log10(1.0 / np.mean((a - b) ** 2, dtype=np.float64))


def clip_psnr(rec, gt, ids):
    """PSNR of every scored measurement of a clip: rec (M,H,W,B) on its device, gt (H,W,B*Mall) on the host.  The same
    arithmetic as `psnr` (float32 difference and square, float64 mean), evaluated where rec lives so that only M scalars
    cross PCIe."""
    B = rec.shape[-1]
    g = torch.stack([torch.as_tensor(gt[..., B * m:B * (m + 1)]) for m in ids]).to(rec.device, torch.float32)
    d = rec.detach().clamp(0, 1) - g
    mse = (d * d).double().mean(dim=(1, 2, 3))
    return [10.0 * math.log10(1.0 / float(v)) for v in mse.cpu()]


def ssim(rec, gt, window=11):
    """SSIM of one frame (H,W) against its ground truth: the reference's pytorch_ssim on a (1,1,H,W) image.  Device tensors go through
    the HIP kernel, anything else through the float64 restatement (deqsci_amd.pytorch_ssim.ssim_float64)."""
    from . import _hip, pytorch_ssim
    if isinstance(rec, torch.Tensor) and rec.is_cuda:
        g = torch.as_tensor(gt).to(rec.device, torch.float32)
        return float(_hip.ssim_frames(_hip.f32c(rec.detach())[None, None], g.contiguous()[None, None], _hip.LAYOUT_BHW, window)[0, 0])
    a = torch.as_tensor(np.asarray(rec, dtype=np.float32))[None, None]
    b = torch.as_tensor(np.asarray(gt, dtype=np.float32))[None, None]
    return float(pytorch_ssim.ssim_float64(a, b, window))


def clip_ssim(rec, gt, ids, mode="same"):
    """SSIM of every scored measurement of a clip, the twin of clip_psnr: rec (M,H,W,B) on its device, gt (H,W,B*Mall) on the host.
    rec is clamped to [0,1] as for the PSNR; per measurement the mean over its B frames of the per-frame SSIM (window 11, mode "same" or
    "valid"), computed where rec lives, so that only M scalars cross PCIe."""
    from . import _hip
    B = rec.shape[-1]
    g = torch.stack([torch.as_tensor(gt[..., B * m:B * (m + 1)]) for m in ids]).to(rec.device, torch.float32).contiguous()
    per = _hip.ssim_frames(_hip.f32c(rec.detach()), g, _hip.LAYOUT_HWB, 11, mode, clamp_x=True)
    return [float(v) for v in per.mean(dim=1).cpu()]


def frame_payload(frame):
    """One reconstructed frame (H,W) -> the (H,W,1) float image in [0,255] that goes to the PNG writer."""
    return (frame.detach().clamp(0, 1).cpu().numpy() * 255.)[:, :, None]


tensor_to_np = frame_payload          # the reference's name for it


def write_png(path, img):
    """cv2.imwrite(path, float image) casts with saturate_cast<uchar>(round-half-even); PIL is what is
    installed here, so that rounding is restated (np.rint = half-to-even, then clip) - unpinned: no cv2."""
    from PIL import Image
    a = np.clip(np.rint(np.asarray(img, dtype=np.float64)), 0, 255).astype(np.uint8)
    Image.fromarray(a[..., 0] if a.ndim == 3 else a).save(path)


# ----------------------------------------------------------------------------- clips
@dataclass
class ClipResult:
    name: str
    rec: torch.Tensor                 # (M,H,W,B) reconstructions of the scored measurements, on the device
    psnr: list                        # per measurement, dB
    res: list                         # per measurement: relative fixed-point residual at exit (None if unknown)
    frames: int = 0
    seconds: float = 0.0
    info: dict = field(default_factory=dict)
    ssim: list | None = None          # per measurement, the mean SSIM over its B frames (only when asked for)
    # (only when asked for) {K: {"psnr": [...], "res": [...], "ssim": [...] or None, "rec": (M,H,W,B)}}: the run with and_maxiters=K, scored as above
    snapshots: dict | None = None
    trace: dict | None = None         # (only when asked for) {"psnr": (M, n_calls), "res": (M, n_calls)}: every f-call of the iteration
    # (only when asked for) {"lipschitz_f": [...], "rho_f": [...], "lipschitz_denoiser": [...]} per measurement, at its reconstruction
    # (deqsci_amd.jacobian), and "histories": {name: (M, n_iters)}
    jacobian: dict | None = None

    @property
    def mean_psnr(self):
        return sum(self.psnr) / len(self.psnr)

    @property
    def mean_ssim(self):
        return None if self.ssim is None else sum(self.ssim) / len(self.ssim)


def as_clip(sample):
    """A dataset item, with or without the DataLoader's leading batch dimension of 1 -> plain (H,W,*) tensors."""
    name = sample['file']
    if isinstance(name, (list, tuple)):
        name = name[0]

    def plain(v, nd):
        t = torch.as_tensor(v)
        return t[0] if t.dim() == nd + 1 else t
    return {'file': name, 'gt': plain(sample['gt'], 3), 'mask': plain(sample['mask'], 3), 'meas': plain(sample['meas'], 3)}


def scored_measurements(name, n_meas):
    """Indices of the snapshot measurements the benchmark scores for this clip."""
    return [0] if any(k in name for k in FIRST_MEASUREMENT_ONLY) else list(range(n_meas))


def _residuals(deep_eq_module, n):
    eng = getattr(deep_eq_module, "_engine", None)
    info = eng[1].last_info if eng else None
    if info and len(info.get("res_per_sample", ())) == n:
        return list(info["res_per_sample"]), info
    r = getattr(deep_eq_module, "forward_res", None)
    if isinstance(r, list):
        r = r[-1] if r else None
    return [r] * n, (info or {})


def _gt_batch(gt, ids, B, device):
    """The ground truth of the measurements ids as an (M,H,W,B) fp32 tensor on the device (what clip_psnr scores against)."""
    return torch.stack([torch.as_tensor(gt[..., B * m:B * (m + 1)]) for m in ids]).to(device, torch.float32).contiguous()


def _rows(rows):
    """Per-measurement rows -> an (M, n_calls) float64 array (a list of arrays if early stops left them of different lengths)."""
    rows = [np.asarray(r, dtype=np.float64) for r in rows]
    return np.stack(rows) if rows and all(r.shape == rows[0].shape for r in rows) else rows


class _Horizons:
    """The snapshots= / trace= options around the forward calls of one harness batch: sets them on the DEQ module for each call
    (DEQFixedPoint.snapshots / .trace / .trace_gt), collects what the calls leave (last_snapshots / last_trace), and gathers the
    per-measurement results over the process group as the reconstructions and the PSNR scalars are gathered."""

    def __init__(self, module, snapshots, trace, method):
        self.module, self.snapshots, self.trace = module, (None if snapshots is None else tuple(snapshots)), bool(trace)
        self.on = self.snapshots is not None or self.trace
        if self.on and method != "deq":
            raise ValueError("snapshots / trace are the DEQ iteration's: not available with method='gaptv'")
        if self.on and not hasattr(module, "last_snapshots"):
            raise NotImplementedError(f"snapshots / trace need this package's DEQFixedPoint, not {type(module).__name__}")
        self.recs = {K: [] for K in (self.snapshots or ())}
        self.res = {K: [] for K in (self.snapshots or ())}
        self.t_psnr, self.t_res = [], []

    def forward(self, call, gt_part):
        """call() = the module's forward for one batch whose ground truth is gt_part (M_part,H,W,B) on the device."""
        if not self.on:
            return call()
        mod = self.module
        old = (mod.snapshots, mod.trace, mod.trace_gt)
        mod.snapshots, mod.trace, mod.trace_gt = self.snapshots, self.trace, (gt_part if self.trace else None)
        try:
            rec = call()
        finally:
            mod.snapshots, mod.trace, mod.trace_gt = old
        for K, v in (mod.last_snapshots or {}).items():
            self.recs[K].append(v["rec"].detach())
            self.res[K].extend(v["res_per_sample"])
        if self.trace:
            tr = mod.last_trace
            self.t_psnr.extend(tr["psnr"][:, j] for j in range(tr["psnr"].shape[1]))
            self.t_res.extend(tr["res_per_sample"][:, j] for j in range(tr["res_per_sample"].shape[1]))
        return rec

    def finish(self, y, Phi, group):
        """-> ({K: {"rec" (M,H,W,B), "res" [M]}} or None, {"psnr" (M,n_calls), "res" (M,n_calls)} or None) over ALL measurements."""
        snaps = trace = None
        if self.snapshots is not None:
            snaps = {}
            for K in self.snapshots:
                local = torch.cat(self.recs[K]) if self.recs[K] else None
                rec = distributed.sharded_reconstruct(lambda a, b: local, y, Phi, group=group) if distributed._active(group) else local
                snaps[K] = {"rec": rec, "res": distributed.gather_scalars(self.res[K], group=group)}
        if self.trace:
            trace = {"psnr": _rows(distributed.gather_scalars(self.t_psnr, group=group)),
                     "res": _rows(distributed.gather_scalars(self.t_res, group=group))}
        return snaps, trace


JACOBIAN_KEYS = ("lipschitz_f", "rho_f", "lipschitz_denoiser")
_JACOBIAN_HISTORIES = ("lipschitz_f_history", "rho_f_growth", "rho_f_rayleigh", "lipschitz_denoiser_history")


class _Jacobians:
    """The jacobian= option around the forward calls of one harness batch: after each call the module's jacobian_report at the
    reconstruction it returned (the batch as one call, per-sample norms), gathered over the process group as the PSNR scalars are."""

    def __init__(self, module, options, method):
        self.module, self.on = module, options is not None
        if not self.on:
            return
        if method != "deq":
            raise ValueError("jacobian= is the DEQ map's: not available with method='gaptv'")
        if not hasattr(module, "jacobian_report"):
            raise NotImplementedError(f"jacobian= needs this package's DEQFixedPoint, not {type(module).__name__}")
        self.options = dict(options)
        unknown = set(self.options) - {"n_iters", "window", "seed"}
        if unknown:
            raise ValueError(f"jacobian=: unknown option(s) {sorted(unknown)} (n_iters, window, seed)")
        self.vals = {k: [] for k in JACOBIAN_KEYS + _JACOBIAN_HISTORIES}

    def after(self, y_part, Phi_part, Phi_sum, rec):
        if self.on:
            r = self.module.jacobian_report(y_part, Phi_part, Phi_sum, rec, **self.options)
            for k in JACOBIAN_KEYS:
                self.vals[k].extend(float(v) for v in r[k])
            for k in _JACOBIAN_HISTORIES:
                self.vals[k].extend(r[k][:, j] for j in range(r[k].shape[1]))

    def finish(self, group):
        if not self.on:
            return None
        return {k: distributed.gather_scalars(v, group=group) for k, v in self.vals.items()}


def _jac_slice(jac, lo, hi):
    if jac is None:
        return None
    out = {k: list(jac[k][lo:hi]) for k in JACOBIAN_KEYS}
    out["histories"] = {k: _rows(jac[k][lo:hi]) for k in _JACOBIAN_HISTORIES}
    return out


def _scored(snaps, trace, lo, hi, gt, ids, ssim, ssim_mode):
    """ClipResult.snapshots / .trace of the measurements [lo, hi) of a batch: every snapshot scored exactly as the final result is."""
    out = None
    if snaps is not None:
        out = {}
        for K, v in snaps.items():
            r = v["rec"][lo:hi]
            out[K] = {"psnr": clip_psnr(r, gt, ids), "res": list(v["res"][lo:hi]),
                      "ssim": clip_ssim(r, gt, ids, ssim_mode) if ssim else None, "rec": r}
    return out, (None if trace is None else {k: v[lo:hi] for k, v in trace.items()})


def _start(init, y, Phi, Phi_sum):
    """The DEQ's starting point: "At" = initial_point (the reference's), "gaptv" = initial_point_gaptv (its commented-out one)."""
    with torch.no_grad():
        if init == "At":
            return operators.initial_point(y, Phi, Phi_sum, None)
        if init == "gaptv":
            return operators.initial_point_gaptv(y, Phi, Phi_sum, None)
    raise ValueError(f"init must be 'At' or 'gaptv', got {init!r}")


def noise_seq(clip_index, measurement):
    """The sequence number a scored measurement is noised under: (position of its clip in evaluate's order << 32) | measurement index."""
    return (int(clip_index) << 32) | int(measurement)


def _noisy(noise, y, seqs, B):
    """The measurements y (M,H,W) through the sensor model (noise.SensorNoise), measurement i under seqs[i]: done once, on the full set
    and before anything reads y, so what a measurement becomes depends on (seed, clip, measurement) only - not on how the harness batches
    or shards.  None or a disabled model: y itself."""
    if noise is None or not noise.enabled or y.shape[0] == 0:
        return y
    with torch.no_grad():
        return noise.apply(y, seqs, frames=B)


def _shard_start(M, group):
    """Index of the first of M measurements that this rank reconstructs (distributed.sharded_reconstruct); 0 without a process group."""
    if not distributed._active(group):
        return 0
    return distributed.shard_bounds(M, torch.distributed.get_world_size(group), torch.distributed.get_rank(group))[0]


def _check_method(method, init):
    if method not in ("deq", "gaptv"):
        raise ValueError(f"method must be 'deq' or 'gaptv', got {method!r}")
    if init not in ("At", "gaptv"):
        raise ValueError(f"init must be 'At' or 'gaptv', got {init!r}")


def reconstruct_clip(deep_eq_module, clip, device="cuda", batch=True, group=None, ssim=False, ssim_mode="same", init="At", method="deq",
                     snapshots=None, trace=False, jacobian=None, noise=None, clip_index=0):
    """All scored measurements of one clip through `deep_eq_module.forward(y, Phi, Phi_sum, initial_point=, train_flag=False)`.
    batch=True: one call with y (M,H,W) and the shared mask (1,H,W,B); batch=False: M calls of batch 1 (the reference's
    schedule).  With a process group the measurements are sharded over its ranks and all-gathered.  ssim=True: also the
    per-measurement SSIM (clip_ssim, after the timed part).  init: the DEQ's start, "At" (default) or "gaptv" (GAP-TV, timed with the
    reconstruction).  method="gaptv": GAP-TV alone, no DEQ (deep_eq_module is not used; res is None).
    snapshots=(K1, ...): ClipResult.snapshots[K] = the clip as a run with and_maxiters=K would score it, from the same run
    (DEQSCIEngine.reconstruct); trace=True: ClipResult.trace = PSNR and residual of every f-call, per measurement.
    jacobian=dict(n_iters=, window=, seed=): ClipResult.jacobian = the local Lipschitz constant and spectral radius of f and the Lipschitz
    constant of the noise predictor at every measurement's reconstruction (DEQFixedPoint.jacobian_report, outside the timed part's meaning:
    it is added to `seconds`).
    noise: a noise.SensorNoise (this build's); measurement m goes through it under the sequence number noise_seq(clip_index, m) before
    the starting point, GAP-TV or anything else reads it; the score is against the clean ground truth."""
    import time
    clip = as_clip(clip)
    Phi = clip['mask'].to(device)[None].contiguous()                  # (1,H,W,B)
    B = Phi.shape[-1]
    ids = scored_measurements(clip['file'], clip['meas'].shape[-1])
    y = clip['meas'].to(device).permute(2, 0, 1)[ids].contiguous()    # (M,H,W)
    y = _noisy(noise, y, [noise_seq(clip_index, m) for m in ids], B)
    Phi_sum = operators.phi_sum(Phi)
    _check_method(method, init)
    hz = _Horizons(deep_eq_module, snapshots, trace, method)
    jc = _Jacobians(deep_eq_module, jacobian, method)
    gts = _gt_batch(clip['gt'], ids, B, device) if hz.trace else None

    def run(y_part, Phi_part, lo=0):
        if method == "gaptv":
            return _start("gaptv", y_part, Phi_part, Phi_sum), [None] * y_part.shape[0]
        x0 = _start(init, y_part, Phi_part, Phi_sum)
        rec = hz.forward(lambda: deep_eq_module.forward(y_part, Phi_part, Phi_sum, initial_point=x0, train_flag=False),
                         None if gts is None else gts[lo:lo + y_part.shape[0]])
        res, _ = _residuals(deep_eq_module, y_part.shape[0])
        jc.after(y_part, Phi_part, Phi_sum, rec.detach())
        return rec.detach(), res

    t0 = time.perf_counter()
    res = []
    if batch:
        def run_collect(y_part, Phi_part):
            rec, r = run(y_part, Phi_part, _shard_start(y.shape[0], group))
            res.extend(r)
            return rec
        rec = distributed.sharded_reconstruct(run_collect, y, Phi, group=group)
        res = distributed.gather_scalars(res, group=group)
    else:
        parts = []
        for i in range(len(ids)):
            r, rr = run(y[i:i + 1], Phi, i)
            parts.append(r)
            res.extend(rr)
        rec = torch.cat(parts)
    if rec.is_cuda:
        torch.cuda.synchronize(rec.device)
    dt = time.perf_counter() - t0
    ps = clip_psnr(rec, clip['gt'], ids)
    snaps, tr = _scored(*hz.finish(y, Phi, group if batch else None), 0, len(ids), clip['gt'], ids, ssim, ssim_mode)
    return ClipResult(name=clip['file'], rec=rec, psnr=ps, res=res, frames=B * len(ids), seconds=dt,
                      info={"measurements": ids, "batched": bool(batch)},
                      ssim=clip_ssim(rec, clip['gt'], ids, ssim_mode) if ssim else None, snapshots=snaps, trace=tr,
                      jacobian=_jac_slice(jc.finish(group if batch else None), 0, len(ids)))


def reconstruct_clips_together(deep_eq_module, clips, device="cuda", group=None, ssim=False, ssim_mode="same", init="At", method="deq",
                               snapshots=None, trace=False, jacobian=None, noise=None, clip_index=0):
    """The scored measurements of SEVERAL clips of one frame size as ONE engine batch, every measurement with its own clip's mask
    ((M,H,W,B) masks: nothing couples the measurements of a batch - alpha, residual, the ranges of the split-fp16 activations are all per
    measurement - so a measurement's reconstruction is the one it gets in any other batch, bit for bit).  What the reference's loop over
    clips and measurements (training/sci_equilibrium_training.py:157,171) becomes when the device wants eight measurements per call: the
    three shipped clips (1 + 1 + 6 measurements) are one call.  -> [ClipResult] in the clips' order; a clip's `seconds` is its share of
    the call by frames.  ssim=True: also the per-measurement SSIM; init, method, snapshots, trace and jacobian as in reconstruct_clip.
    noise: as in reconstruct_clip, clip_index the position of the FIRST of these clips (the others follow it)."""
    import time
    clips = [as_clip(c) for c in clips]
    ids = [scored_measurements(c['file'], c['meas'].shape[-1]) for c in clips]
    Phi = torch.cat([c['mask'].to(device)[None].expand(len(i), -1, -1, -1) for c, i in zip(clips, ids)]).contiguous()      # (M,H,W,B)
    y = torch.cat([c['meas'].to(device).permute(2, 0, 1)[i] for c, i in zip(clips, ids)]).contiguous()                        # (M,H,W)
    B = Phi.shape[-1]
    y = _noisy(noise, y, [noise_seq(clip_index + k, m) for k, i in enumerate(ids) for m in i], B)
    res = []
    _check_method(method, init)
    hz = _Horizons(deep_eq_module, snapshots, trace, method)
    jc = _Jacobians(deep_eq_module, jacobian, method)
    gts = torch.cat([_gt_batch(c['gt'], i, B, device) for c, i in zip(clips, ids)]) if hz.trace else None

    def run(y_part, Phi_part):
        Ps = operators.phi_sum(Phi_part)
        if method == "gaptv":
            res.extend([None] * y_part.shape[0])
            return _start("gaptv", y_part, Phi_part, Ps)
        x0 = _start(init, y_part, Phi_part, Ps)
        lo = _shard_start(y.shape[0], group)
        rec = hz.forward(lambda: deep_eq_module.forward(y_part, Phi_part, Ps, initial_point=x0, train_flag=False),
                         None if gts is None else gts[lo:lo + y_part.shape[0]])
        res.extend(_residuals(deep_eq_module, y_part.shape[0])[0])
        jc.after(y_part, Phi_part, Ps, rec.detach())
        return rec.detach()
    t0 = time.perf_counter()
    rec = distributed.sharded_reconstruct(run, y, Phi, group=group)
    res = distributed.gather_scalars(res, group=group)
    if rec.is_cuda:
        torch.cuda.synchronize(rec.device)
    dt = time.perf_counter() - t0
    out, a = [], 0
    all_snaps, all_trace = hz.finish(y, Phi, group)
    all_jac = jc.finish(group)
    for c, i in zip(clips, ids):
        r = rec[a:a + len(i)]
        snaps, tr = _scored(all_snaps, all_trace, a, a + len(i), c['gt'], i, ssim, ssim_mode)
        out.append(ClipResult(name=c['file'], rec=r, psnr=clip_psnr(r, c['gt'], i), res=list(res[a:a + len(i)]), frames=B * len(i),
                              seconds=dt * len(i) / y.shape[0], info={"measurements": i, "batched": "all"},
                              ssim=clip_ssim(r, c['gt'], i, ssim_mode) if ssim else None, snapshots=snaps, trace=tr,
                              jacobian=_jac_slice(all_jac, a, a + len(i))))
        a += len(i)
    return out


def evaluate(deep_eq_module, clips, device="cuda", batch=True, group=None, on_clip=None, ssim=False, ssim_mode="same", init="At",
             method="deq", snapshots=None, trace=False, jacobian=None, noise=None):
    """-> (mean over clips of the clip's mean PSNR, [ClipResult]).  batch: False = one measurement per call (the reference's schedule),
    True = a clip's measurements per call, "all" = the measurements of consecutive clips of one frame size per call
    (reconstruct_clips_together: the three shipped clips are ONE call of eight measurements).  ssim=True fills every ClipResult.ssim
    (window 11, ssim_mode "same" or "valid"); the mean over clips of the clip's mean SSIM is then sum(r.mean_ssim ...) / len(results).
    init: the DEQ's start, "At" (default) or "gaptv"; method="gaptv": reconstruct by GAP-TV alone (deep_eq_module may be None).
    snapshots=(K1, ...) fills every ClipResult.snapshots (the clip at and_maxiters=K, out of the same run), trace=True every
    ClipResult.trace; `horizon_means(results)` is the mean over clips per horizon.  jacobian=dict(n_iters=, window=, seed=) fills every
    ClipResult.jacobian (ValueError with method="gaptv").
    noise: a noise.SensorNoise; scored measurement m of the clip at position k of `clips` is noised under the sequence number
    (k << 32) | m, so its noisy value depends on (noise.seed, k, m) alone - not on `batch`, not on the number of ranks; method="gaptv"
    sees the same noisy measurement."""
    _check_method(method, init)
    kw = dict(ssim=ssim, ssim_mode=ssim_mode, init=init, method=method)
    if jacobian is not None:
        if method != "deq":
            raise ValueError("jacobian= is the DEQ map's: not available with method='gaptv'")
        kw.update(jacobian=jacobian)
    if snapshots is not None or trace:
        kw.update(snapshots=snapshots, trace=trace)
    noisy = noise is not None and noise.enabled

    def at(k):
        return dict(kw, noise=noise, clip_index=k) if noisy else kw
    results = []
    if batch == "all":
        pending = []

        def flush():
            if pending:
                for r in reconstruct_clips_together(deep_eq_module, pending, device=device, group=group, **at(len(results))):
                    results.append(r)
                    if on_clip is not None:
                        on_clip(r)
                del pending[:]
        for sample in clips:
            c = as_clip(sample)
            if pending and tuple(as_clip(pending[0])['mask'].shape) != tuple(c['mask'].shape):
                flush()
            pending.append(c)
        flush()
        return sum(r.mean_psnr for r in results) / len(results), results
    for k, sample in enumerate(clips):
        r = reconstruct_clip(deep_eq_module, sample, device=device, batch=batch, group=group, **at(k))
        results.append(r)
        if on_clip is not None:
            on_clip(r)
    return sum(r.mean_psnr for r in results) / len(results), results


def horizon_means(results):
    """{K: (mean over clips of the clip's mean PSNR, the same of the SSIM or None)} of results evaluated with snapshots=."""
    out = {}
    for K in (getattr(results[0], "snapshots", None) or {}) if results else ():
        ps = [sum(r.snapshots[K]["psnr"]) / len(r.snapshots[K]["psnr"]) for r in results]
        ss = None if results[0].snapshots[K]["ssim"] is None else [sum(r.snapshots[K]["ssim"]) / len(r.snapshots[K]["ssim"]) for r in results]
        out[K] = (sum(ps) / len(ps), None if ss is None else sum(ss) / len(ss))
    return out


def print_horizons(results):
    """One '[and_maxiters K] Total Average PSNR' line per snapshot horizon (and the SSIM where it was scored)."""
    for K, (p, s) in horizon_means(results).items():
        if s is None:
            print('---------------------------------', '[and_maxiters %d] Total Average PSNR: %.2f dB' % (K, p))
        else:
            print('---------------------------------', '[and_maxiters %d] Total Average PSNR: %.2f dB' % (K, p), '  SSIM: %.4f' % s)


def solver_line(deep_eq_module):
    """'solver: NAME (settings)' of a DEQFixedPoint: which fixed-point solver its forward runs, with the keyword arguments it passes."""
    name = getattr(deep_eq_module.solver, "__name__", type(deep_eq_module.solver).__name__)
    return "solver: %s (%s)" % (name, ", ".join("%s=%s" % kv for kv in sorted(deep_eq_module.kwargs.items())))


def clip_line(r, ssim=False):
    """The pieces of a clip's printed line: the reference's, then this build's additions that were asked for."""
    parts = [[r.name], '  PSNR: %.2f dB' % r.mean_psnr]
    if ssim:
        parts.append('  SSIM: %.4f' % r.mean_ssim)
    if getattr(r, "jacobian", None) is not None:
        m = {k: float(np.mean(r.jacobian[k])) for k in JACOBIAN_KEYS}
        parts.append('  Lip(f): %.4f  rho(f): %.4f  Lip(D): %.4f' % (m["lipschitz_f"], m["rho_f"], m["lipschitz_denoiser"]))
    return parts


def print_jacobian_totals(results):
    """One 'Total Average' line per Jacobian quantity (the mean over clips of the clip's mean), when jacobian= was asked for."""
    if not results or getattr(results[0], "jacobian", None) is None:
        return
    for k, label in zip(JACOBIAN_KEYS, ("Lip(f)", "rho(f)", "Lip(D)")):
        print('---------------------------------', 'Total Average %s: %.4f' % (label, sum(float(np.mean(r.jacobian[k])) for r in results) / len(results)))


def jacobian_document(results):
    """{clip: {measurement: {"lipschitz_f", "rho_f", "lipschitz_denoiser", "histories": {...}}}}: what `--jacobian_json FILE` writes."""
    doc = {}
    for r in results:
        if r.jacobian is not None:
            doc[r.name] = {str(m): {**{k: float(r.jacobian[k][i]) for k in JACOBIAN_KEYS},
                                    "histories": {k: [float(v) for v in h[i]] for k, h in r.jacobian["histories"].items()}}
                           for i, m in enumerate(r.info["measurements"])}
    return doc


def trace_document(results):
    """{clip: {measurement: {"psnr": [...], "res": [...]}}}: what `--trace FILE.json` writes, one value per issued f-call of the iteration."""
    doc = {}
    for r in results:
        if r.trace is not None:
            doc[r.name] = {str(m): {"psnr": [float(v) for v in r.trace["psnr"][i]], "res": [float(v) for v in r.trace["res"][i]]}
                           for i, m in enumerate(r.info["measurements"])}
    return doc


def png_payloads(result, prefix=""):
    """{path: (H,W,1) float image} for every frame of a clip, named like the reference's export (:185-187):
    '<prefix><file>_reconstruction_<frame index within the scored frames>.png'."""
    out = {}
    B = result.rec.shape[-1]
    for i in range(result.rec.shape[0]):
        for b in range(B):
            out[prefix + '%s_reconstruction_%d.png' % (result.name, i * B + b)] = frame_payload(result.rec[i, :, :, b])
    return out


def test_solver_sci(deep_eq_module, test_dataloader=None, save_img_path=None, verbose=True, save_image=True,
                    device="cuda", records=None, batch_measurements=False, ssim=False, init="At", method="deq", snapshots=None, trace=False,
                    jacobian=None, noise=None):
    """Adapter with the reference's signature (training/sci_equilibrium_training.py:152): returns
    (average PSNR, {png path: float image}); prints one line per clip and the total; writes the PNGs.
    Default = the reference's schedule, one measurement per call (:171-181); batch_measurements="all" hands the measurements of all clips of
    one frame size to the engine as ONE batch (the three shipped clips: one call of eight); batch_measurements=True hands a clip's
    measurements to the engine as one batch (faster; on the chaotic FFDNet + Anderson @180 clip a different - equally valid -
    realisation, because the FFDNet head kernel is chosen by launch size).  ssim=True (this build's addition): every record gains "ssim",
    every clip line '  SSIM: %.4f' and a 'Total Average SSIM' line follows the PSNR total; the return value is unchanged.  init="gaptv"
    starts the DEQ from GAP-TV, method="gaptv" reconstructs by GAP-TV alone (both this build's additions, as in evaluate).
    snapshots=(K1, ...) / trace=True (this build's, as in evaluate): every record gains "snapshots" ({K: {"psnr", "res", "ssim", "rec"}}) /
    "trace" ({"psnr", "res"} per f-call), and one '[and_maxiters K] Total Average PSNR' line per horizon follows the totals.
    jacobian=dict(n_iters=, window=, seed=) (this build's): every record gains "jacobian" ({"lipschitz_f", "rho_f", "lipschitz_denoiser"}),
    every clip line '  Lip(f): %.4f  rho(f): %.4f  Lip(D): %.4f' (means over the clip's measurements), and one 'Total Average' line per quantity follows.
    noise (this build's): a noise.SensorNoise for the test measurements, as in evaluate; one 'sensor noise on the test measurements' line says so."""
    images = {}
    if verbose and noise is not None and noise.enabled:
        print('sensor noise on the test measurements: %s' % noise.describe())

    def on_clip(r):
        images.update(png_payloads(r, save_img_path or ""))
        if records is not None:
            for i, m in enumerate(r.info["measurements"]):
                records.append({"id": f"{r.name}:{m}", "psnr": r.psnr[i], "res": r.res[i], "rec": r.rec[i:i + 1].cpu()})
                if ssim:
                    records[-1]["ssim"] = r.ssim[i]
                if r.snapshots is not None:
                    records[-1]["snapshots"] = {K: {"psnr": v["psnr"][i], "res": v["res"][i], "ssim": None if v["ssim"] is None else v["ssim"][i],
                                                    "rec": v["rec"][i:i + 1].cpu()} for K, v in r.snapshots.items()}
                if r.trace is not None:
                    records[-1]["trace"] = {k: np.asarray(v[i]) for k, v in r.trace.items()}
                if r.jacobian is not None:
                    records[-1]["jacobian"] = {k: r.jacobian[k][i] for k in JACOBIAN_KEYS}
        if verbose:
            print(*clip_line(r, ssim))
    avg, results = evaluate(deep_eq_module, test_dataloader, device=device, batch=batch_measurements, on_clip=on_clip, ssim=ssim, init=init,
                            method=method, snapshots=snapshots, trace=trace, **({} if jacobian is None else {"jacobian": jacobian}),
                            **({} if noise is None else {"noise": noise}))
    if verbose:
        print('---------------------------------', 'Total Average PSNR: %.2f dB' % avg)
        if ssim:
            print('---------------------------------', 'Total Average SSIM: %.4f' % (sum(r.mean_ssim for r in results) / len(results)))
        print_horizons(results)
        print_jacobian_totals(results)
    if save_image:
        for path, img in images.items():
            write_png(path, img)
    return avg, images
