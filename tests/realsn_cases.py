"""The seeded inputs of tests/golden/realsn_train.npz and how its tensors are stored and compared - shared by the generator
(tests/golden/make_realsn_golden.py, which runs the reference on them) and by tests/test_realsn_host.py / tests/test_realsn_gpu.py."""
import hashlib

import numpy as np
import torch

LAYERS = ((1, 64), (64, 64), (64, 1))
MAPS = ((40, 40), (7, 9), (2, 3), (1, 1))
ITERS_N = (1, 3)
SIGMA, EPS = 0.84, 1e-12
SCALES = (1.7, 0.6, 2.3, 0.9)          # (b): weight_orig of rsn_cnn.ckpt scaled per layer
U_SEED = 77                            # (b): layer i's starting weight_u is unit_u(shape, U_SEED + i)
ITERS = 12
WHOLE = 2048                           # a tensor of more elements is stored as a slice and two float64 sums

CASES = [(cin, cout, h, w, n) for cin, cout in LAYERS for h, w in MAPS for n in ITERS_N]


def sha16(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).tobytes()).hexdigest()[:16]


def case_tag(cin, cout, h, w, n):
    return f"a.{cin}x{cout}.{h}x{w}.n{n}"


def inputs(cin, cout, h, w, n):
    """(W, u, R) of a layer case: W = 0.3 randn, u a unit-norm randn, R randn from one generator per case, in this order."""
    g = torch.Generator().manual_seed(100000 * n + 1000 * (h * 41 + w) + cin + 2 * cout)
    W = 0.3 * torch.randn(cout, cin, 3, 3, generator=g)
    u = torch.randn(1, cout, h, w, generator=g)
    u = u / u.norm()
    R = torch.randn(cout, cin, 3, 3, generator=g)
    return W, u, R


def unit_u(shape, seed):
    u = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    return u / u.norm()


def problem():
    """make_golden.py's g8 problem: (Phi, gt), shape (2,24,20,4), a Bernoulli(0.5) mask with two all-zero pixels."""
    g = torch.Generator().manual_seed(2024)
    bsz, H, W, B = 2, 24, 20, 4
    Phi = (torch.rand(bsz, H, W, B, generator=g) < 0.5).float()
    Phi[:, 0, :2, :] = 0
    gt = torch.rand(bsz, H, W, B, generator=g)
    return Phi, gt


def denoiser_input():
    """The batch of (b)'s denoiser-level half: (8,1,24,20), uniform in [0,1)."""
    return torch.rand(8, 1, 24, 20, generator=torch.Generator().manual_seed(2025))


def _slice(t):
    """The stored part of a large tensor: the first two output channels of a (C_out, C_in, 3, 3) weight, the first channel of a
    (1, C, h, w) map."""
    return t[:2] if t.shape[0] > 1 else t[:, :1]


def put(out, key, t):
    """Store t under key: whole up to WHOLE elements, else `.slice`, `.sum` and `.sumsq` (float64)."""
    t = t.detach()
    if t.numel() <= WHOLE:
        out[key] = t.clone()
    else:
        out[key + ".slice"] = _slice(t).clone()
        out[key + ".sum"] = t.double().sum()
        out[key + ".sumsq"] = (t.double() ** 2).sum()


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def deviation(golden, key, t):
    """How far t is from the tensor stored under key, as a relative L2 figure.  A tensor stored whole: exactly that.  A sliced one: the
    largest of the slice's relative L2 and the two figures the sums bound from below - |sum a - sum b| <= sqrt(N) |a - b| and
    | |a| - |b| | <= |a - b|, each divided by |b| - so that a figure above a tolerance proves the whole tensor misses it."""
    t = t.detach().double().cpu()
    if key in golden:
        return rel_l2(t.numpy(), golden[key])
    norm = float(np.sqrt(golden[key + ".sumsq"]))
    figures = [rel_l2(_slice(t).numpy(), golden[key + ".slice"]),
               abs(float(t.sum()) - float(golden[key + ".sum"])) / (np.sqrt(t.numel()) * norm),
               abs(float(t.norm()) - norm) / norm]
    return max(figures)
