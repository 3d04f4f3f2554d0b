#!/usr/bin/env python3
"""Generate tests/golden/synth.npz: a dozen training samples written by deqsci_amd.synth.write_training_directory and read back by the
REFERENCE's own loader (utils/sci_dataloader.py: SCITrainingDatasetSubset), imported on the CPU through ref_shims.

    python tests/golden/make_synth_golden.py

The video is the 64 x 64 x 16 corner of traffic_cacti.mat's `orig`, the mask the 16 x 16 x 8 corner of its mask; the twelve rows cover
the eight orientations, both signs of dt, |dt| = 2 and ds = 2, and crops pinned to the video's edges.  Stored: the video, the mask, the
rows, and what the reference's loader returns for the written directory (gt, meas, mask), item after item.  Data only: nothing of the
reference's text.  Runs only where the reference is mounted."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the package
import ref_shims  # noqa: E402

ref_shims.install()

from utils.sci_dataloader import SCITrainingDatasetSubset  # noqa: E402

from deqsci_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))
H = W = 16
B = 8
T, HV, WV = 16, 64, 64
# (t0, dt, y0, x0, ds, flags)
ROWS = [(0, 1, 0, 0, 1, 0), (15, -1, 48, 48, 1, 1), (3, 1, 0, 48, 1, 2), (12, -1, 48, 0, 1, 3),
        (8, 1, 5, 7, 1, 4), (7, -1, 31, 2, 1, 5), (1, 1, 17, 40, 1, 6), (10, -1, 9, 33, 1, 7),
        (0, 2, 0, 0, 2, 0), (15, -2, 33, 33, 2, 7), (1, 2, 20, 1, 2, 4), (14, -2, 3, 30, 1, 3)]


def main():
    import scipy.io as sio
    clip = sio.loadmat(os.path.join(ROOT, "data", "test_gray", "traffic_cacti.mat"))
    video = np.ascontiguousarray(np.asarray(clip["orig"])[:HV, :WV, :T].transpose(2, 0, 1)).astype(np.uint8)
    mask = np.ascontiguousarray(np.float32(clip["mask"])[:H, :W, :B])
    assert set(np.unique(mask)) <= {0.0, 1.0}
    pool = synth.VideoPool([video], "cpu")
    specs = [synth.PatchSpec(0, T, HV, WV, *row) for row in ROWS]
    assert {s.flags for s in specs} == set(range(8)) and {np.sign(s.dt) for s in specs} == {1, -1}
    with tempfile.TemporaryDirectory() as tmp:
        d = synth.write_training_directory(tmp, pool, mask, specs)
        ds = SCITrainingDatasetSubset(d + "gt/", d + "measurement/", d + "mask.mat")
        assert len(ds) == len(specs) and [os.path.basename(f) for f in ds.full_gt_filelist] == ["%06d.mat" % k for k in range(len(specs))]
        items = [ds[k] for k in range(len(ds))]
    gt = np.stack([np.asarray(it["gt"]) for it in items])
    meas = np.stack([np.asarray(it["meas"]) for it in items])
    assert gt.dtype == np.float32 and meas.dtype == np.float32 and gt.shape == (len(specs), H, W, B) and meas.shape == (len(specs), H, W)
    fn = os.path.join(HERE, "synth.npz")
    np.savez_compressed(fn, video=video, mask=mask, specs=synth.spec_table(specs), gt=gt, meas=meas, ref_mask=np.asarray(items[0]["mask"]))
    print("->", fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
