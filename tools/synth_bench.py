#!/usr/bin/env python3
"""Training batches out of raw video (csrc/synth.hip) at 256 x 256 x 8, batch 1 and 8, from the three shipped clips:

  Y1 alone     one deqsci_synth_batch_u8 call, HIP events, with the bytes it has to move per sample (H W B read as uint8, 4 H W B of mask,
               4 H W B + 4 H W written) over its time
  one batch    one batch out of SynthTrainLoader (descriptors drawn before the clock starts: the epoch's table is drawn once) against
               one batch of the only path there was - DataLoader(SCITrainingDatasetSubset) over a written directory - plus its copies
               to the device; host clock around work that ends in a device synchronise
  one step     one whole step of train_solver_sci (SimpleCNN, --and_maxiters 30, the device backend) with each source; the time from
               the end of one step to the end of the next, so the batch's fetch is inside

The median of `--reps` after `--warmup`.  Prints one line per measurement and a JSON line; the numbers go to profiles/synth.md.  No
threshold: the feature is that training from video is possible at all.

    python tools/synth_bench.py [--reps 10] [--warmup 2] [--iters 30] [--kernel-only]
    python tools/synth_bench.py --noise      N1 / N2 of csrc/noise.hip beside Y1, and a loader batch with and without sensor noise
                                             (profiles/noise.md)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deqsci_amd import _hip, checkpoint, synth, training  # noqa: E402
from deqsci_amd.cli import build_pipeline  # noqa: E402
from deqsci_amd.optim import DeviceAdam  # noqa: E402

H = W = 256
B = 8
CLIPS = os.path.join(ROOT, "data", "test_gray")


def sample_bytes():
    return H * W * B + 4 * H * W * B + 4 * H * W * B + 4 * H * W


def kernel_alone(pool, mask, bsz, reps, warmup, augment=synth.AUGMENT_ALL):
    specs = synth.sample_specs(pool, bsz, H, W, B, np.random.default_rng([1, bsz]), augment=augment)
    table = synth.spec_table(specs)
    gt = torch.empty(bsz, H, W, B, device="cuda")
    meas = torch.empty(bsz, H, W, device="cuda")
    ms = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.synth_batch(pool.data, table, mask, H, W, B, gt=gt, meas=meas)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return {"ms": med, "min_ms": min(ms), "bytes": bsz * sample_bytes(), "GBps": bsz * sample_bytes() / med / 1e6}


def event_timed(call, reps, warmup):
    """(median, min) ms of HIP events around one call on an idle stream."""
    ms = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def noise_alone(pool, mask_host, reps, warmup):
    """--noise: N1 and N2 (csrc/noise.hip) alone beside Y1, at 8 and 64 samples of 256 x 256, and one loader batch with and without the
    sensor model.  Bytes: N1 writes 4 per pixel, N2 reads 4 and writes 4; both do the 40 integer multiplies of Philox per four pixels."""
    from deqsci_amd.noise import SensorNoise
    model = SensorNoise(sigma=5 / 255, gain=0.01, bits=10, seed=1)
    mask = torch.from_numpy(mask_host).cuda()
    out = {}
    for bsz in (8, 64):
        n, seq = H * W, list(range(bsz))
        nrm = torch.empty(bsz, n, device="cuda")
        y = torch.rand(bsz, H, W, device="cuda") * B
        o = torch.empty_like(y)
        r = {"Y1": kernel_alone(pool, mask, bsz, reps, warmup)}
        for name, nbytes, call in (("N1", 4 * bsz * n, lambda: _hip.philox_normal(seq, n, 1, out=nrm)),
                                   ("N2", 8 * bsz * n, lambda: model.apply(y, seq, frames=B, out=o)),
                                   ("N2_in_place", 8 * bsz * n, lambda: model.apply(o, seq, frames=B, out=o))):
            med, lo = event_timed(call, reps, warmup)
            r[name] = {"ms": med, "min_ms": lo, "bytes": nbytes, "GBps": nbytes / med / 1e6}
        for name in ("Y1", "N1", "N2", "N2_in_place"):
            print(f"bsz {bsz}: {name} events around the call {r[name]['ms'] * 1e3:.1f} us (min {r[name]['min_ms'] * 1e3:.1f}), "
                  f"{r[name]['bytes'] / 1e6:.2f} MB -> {r[name]['GBps']:.0f} GB/s", flush=True)
        for name, noise in (("batch_clean_ms", None), ("batch_noisy_ms", model)):
            loader = synth.SynthTrainLoader(pool, mask_host, bsz, (warmup + reps + 1) * bsz, H, W, B, seed=5, noise=noise)
            r[name] = host_timed(loader, reps, warmup)
        print(f"bsz {bsz}: one batch  clean {r['batch_clean_ms']:.3f} ms | with sensor noise {r['batch_noisy_ms']:.3f} ms", flush=True)
        out[f"bsz{bsz}"] = r
    return out


def host_timed(batches, reps, warmup):
    """Median ms per batch of an iterator whose batches end on the device."""
    ms = []
    it = iter(batches)
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = next(it)
        for k in ("gt", "meas", "mask"):
            batch[k] = batch[k].to("cuda")
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def step_times(loader, iters, reps, warmup):
    solver, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), iters)
    solver.nonlinear_op.train()
    training.configure_training(deq, "device")
    opt = DeviceAdam(solver.parameters(), lr=1e-4)
    stamps = []

    def on_step(step):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    with tempfile.TemporaryDirectory() as tmp:
        training.train_solver_sci(solver, loader, opt, tmp + "/", "device", 1, deq, print_every_n_steps=10 ** 9, save_every_n_steps=10 ** 9,
                                  max_steps=warmup + reps + 1, on_step=on_step)
    gaps = [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])][warmup:]
    return statistics.median(gaps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kernel-only", action="store_true",
                    help="only Y1, at batch 1, 8 and 64, plain crops and augmented ones: the launches of a kernel trace "
                         "(rocprofv3 --kernel-trace --stats -- python tools/synth_bench.py --kernel-only --reps 18)")
    ap.add_argument("--noise", action="store_true",
                    help="only the random source and the sensor model (csrc/noise.hip): N1 and N2 alone beside Y1 at batch 8 and 64, and one "
                         "loader batch with and without noise; the numbers go to profiles/noise.md")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "synth_bench needs an MI355X"
    pool = synth.VideoPool(synth.list_videos(CLIPS), "cuda")
    mask_host = synth.load_mask(os.path.join(CLIPS, "traffic_cacti.mat"), H, W, B)
    mask = torch.from_numpy(mask_host).cuda()
    out = {"device": torch.cuda.get_device_name(0), "shape": [H, W, B], "reps": a.reps, "warmup": a.warmup, "and_maxiters": a.iters}
    if a.noise:
        out.update(noise_alone(pool, mask_host, a.reps, a.warmup))
        print(json.dumps(out))
        return
    if a.kernel_only:
        for bsz in (1, 8, 64):
            for augment in ((), synth.AUGMENT_ALL):
                r = kernel_alone(pool, mask, bsz, a.reps, a.warmup, augment)
                print(f"bsz {bsz} augment {','.join(augment) or 'none'}: events around the call {r['ms'] * 1e3:.1f} us (min {r['min_ms'] * 1e3:.1f})", flush=True)
        return
    n_batches = a.warmup + a.reps + 1
    for bsz in (1, 8):
        r = {"kernel": kernel_alone(pool, mask, bsz, a.reps, a.warmup)}
        print(f"bsz {bsz}: Y1 alone {r['kernel']['ms'] * 1e3:.1f} us (min {r['kernel']['min_ms'] * 1e3:.1f}), {r['kernel']['bytes'] / 1e6:.2f} MB "
              f"-> {r['kernel']['GBps']:.0f} GB/s", flush=True)
        loader = synth.SynthTrainLoader(pool, mask_host, bsz, n_batches * bsz, H, W, B, seed=5)
        with tempfile.TemporaryDirectory() as tmp:
            d = synth.write_training_directory(tmp, pool, mask_host, loader.epoch_specs(0))
            ds = training.SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")

            def files():
                return torch.utils.data.DataLoader(ds, batch_size=bsz, shuffle=False, drop_last=True, pin_memory=True)
            r["batch_synth_ms"] = host_timed(loader, a.reps, a.warmup)
            r["batch_files_ms"] = host_timed(files(), a.reps, a.warmup)
            print(f"bsz {bsz}: one batch  SynthTrainLoader {r['batch_synth_ms']:.3f} ms | files + copies {r['batch_files_ms']:.3f} ms "
                  f"-> {r['batch_files_ms'] / r['batch_synth_ms']:.1f}x", flush=True)
            loader.epoch = 0
            r["step_synth_ms"] = step_times(loader, a.iters, a.reps, a.warmup)
            r["step_files_ms"] = step_times(files(), a.iters, a.reps, a.warmup)
            print(f"bsz {bsz}: one step   SynthTrainLoader {r['step_synth_ms']:.2f} ms | files {r['step_files_ms']:.2f} ms "
                  f"-> {r['step_files_ms'] / r['step_synth_ms']:.3f}x", flush=True)
        out[f"bsz{bsz}"] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
