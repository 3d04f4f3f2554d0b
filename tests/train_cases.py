"""The tiny training set and the settings the training tests and tests/golden/make_train_golden.py share.  A helper module, not a test.

Four samples of shape (24, 20, 4) - make_golden.py's g8 sizes, which the device backward serves at batch 2 - : uint8 ground truth, one
Bernoulli(0.5) mask with two all-zero pixels (Phi_sum = 0 there: the loop's `Phi_sum[Phi_sum == 0] = 1`), meas = sum_b mask_b gt_b.
Written as the reference's training directory: mask.mat, gt/*.mat, measurement/*.mat.  The ground truth sits under a different one of the
loader's four keys in every file, and the file names sort differently from the order they are written in."""
import os

import numpy as np
import torch

H, W, B, N_SAMPLES = 24, 20, 4, 4
SEED = 2024
NAMES = ("9.mat", "10.mat", "b.mat", "a.mat")                  # sample i -> file NAMES[i]; the data set lists them sorted
GT_KEYS = ("patch_save", "p1", "p2", "p3")                     # sample i's key
SORTED = tuple(sorted(range(N_SAMPLES), key=lambda i: NAMES[i]))    # data set item j is sample SORTED[j]

# the run of tests/golden/train_simplecnn.npz
BATCH, ITERS, LR, EPOCHS, STEPS_PER_EPOCH = 2, 12, 1e-4, 2, 2
ORDER = ((2, 0, 3, 1), (1, 3, 0, 2))                           # data set items per epoch, in the order they are drawn


def samples():
    """-> (mask (H,W,B) float64 of 0 / 1, gt (4,H,W,B) uint8, meas (4,H,W) float64)"""
    rng = np.random.RandomState(SEED)
    mask = (rng.rand(H, W, B) < 0.5).astype(np.float64)
    mask[0, :2, :] = 0
    gt = rng.randint(0, 256, size=(N_SAMPLES, H, W, B)).astype(np.uint8)
    meas = (mask[None] * gt.astype(np.float64)).sum(axis=3)
    return mask, gt, meas


def write(directory):
    """Write the training directory -> its path with the trailing '/' the reference's string joins need."""
    import scipy.io as sio
    directory = str(directory)
    mask, gt, meas = samples()
    os.makedirs(os.path.join(directory, "gt"), exist_ok=True)
    os.makedirs(os.path.join(directory, "measurement"), exist_ok=True)
    sio.savemat(os.path.join(directory, "mask.mat"), {"mask": mask})
    for i, name in enumerate(NAMES):
        sio.savemat(os.path.join(directory, "gt", name), {GT_KEYS[i]: gt[i]})
        sio.savemat(os.path.join(directory, "measurement", name), {"meas": meas[i]})
    return directory.rstrip("/") + "/"


class RecordedSampler(torch.utils.data.Sampler):
    """The data set items of epoch after epoch from a recorded table: every iteration over the sampler hands out the next row."""

    def __init__(self, order=ORDER, start=0):
        self.order, self.epoch = [list(r) for r in order], start

    def __iter__(self):
        row = self.order[self.epoch % len(self.order)]
        self.epoch += 1
        return iter(row)

    def __len__(self):
        return len(self.order[0])
