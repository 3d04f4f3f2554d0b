"""GAP-TV and the Chambolle kernel of csrc/tv.hip where test_gaptv.py's configurations do not reach: frame counts B other than 8 (the
three paths of gap_step_kernel's frame sum), distinct per-measurement masks, the shared and mixed mask forms, ragged planes with
partial tiles, one-row and one-column planes, planes of 65 and 77 tiles (the last workgroup's 64-lane fold), constant planes.

Yardsticks: the float64 restatements (deqsci_amd.gaptv, tv_planes_float64 / gaptv_planes_float64 of test_gaptv.py) and
tests/golden/gaptv_shapes.npz, the reference's own GAP_TV_rec on seeded cases (tests/golden/make_gaptv_golden.py --shapes).

Exactness: the kernels repeat every fp64 operation of the restatement in its order (-ffp-contract=off); only the plane sums of the
energy E are added in another order, and E only decides the stop.  So wherever no stop test comes within TIE of firing the other way,
the stops are equal and the fp32 output is bit for bit the restatement's float64 result rounded to fp32."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_gaptv import DEV, EPS, TIE, gaptv_planes_float64, image, tv_planes_float64

# name, H, W, B, maxiter, step_size, tv_weight, mask, seed: as SHAPES of tests/golden/make_gaptv_golden.py
SHAPES = (("b1", 19, 23, 1, 6, 1.0, 0.3, "float", 1),
          ("b5", 17, 130, 5, 4, 1.0, 0.3, "binary", 2),
          ("b13", 11, 23, 13, 4, 1.0, 0.3, "zeros", 3),
          ("b16", 9, 21, 16, 4, 1.5, 0.3, "float", 4),
          ("b128", 5, 7, 128, 3, 1.0, 0.1, "binary", 5))


def shapes_golden():
    return np.load(os.path.join(GOLDEN, "gaptv_shapes.npz"))


def shape_case(H, W, B, mask, seed):
    """make_gaptv_golden.shape_case restated -> y (1,H,W), Phi (1,H,W,B) float32 numpy.  mask: "float" uniform in [0,1), "binary" 0/1,
    "zeros" uniform with column 0 and the centre pixel zero in every frame."""
    rs = np.random.RandomState(seed)
    x = rs.random_sample((1, H, W, B))
    x = (x + np.roll(x, 1, axis=1) + np.roll(x, 1, axis=2)) / 3.0
    u = rs.random_sample((1, H, W, B))
    Phi = (u < 0.5).astype(np.float32) if mask == "binary" else u.astype(np.float32)
    if mask == "zeros":
        Phi[0, :, 0, :] = 0
        Phi[0, H // 2, W // 2, :] = 0
    y = np.sum(x * Phi, axis=3).astype(np.float32)
    return y, Phi


def golden_case(name, H, W, B, mask, seed):
    gd = shapes_golden()
    y, Phi = shape_case(H, W, B, mask, seed)
    sha = hashlib.sha256(y.tobytes() + Phi.tobytes()).hexdigest()[:16]
    assert sha == str(gd[f"{name}_sha"]), "the seeded inputs changed: numpy's RandomState stream is not what made the golden"
    return gd, torch.from_numpy(y), torch.from_numpy(Phi)


def phi_sum_t(Phi):
    """Phi_sum as the reference's callers form it: the float32 sum over the frames, zeros replaced by one."""
    s = torch.sum(Phi, dim=3)
    s[s == 0] = 1
    return s


# ----------------------------------------------------------------------------- CPU
def test_frame_sum_is_numpys_pairwise_sum():
    """frame_sum_float64 equals np.sum(t, axis=-1) bit for bit for every B in 1..300, across numpy's recursive split above 128."""
    from deqsci_amd.gaptv import frame_sum_float64
    rs = np.random.RandomState(7)
    for B in range(1, 301):
        t = rs.standard_normal((2, 3, B)) * 10.0 ** rs.uniform(-4, 4, (2, 3, B))
        assert torch.equal(frame_sum_float64(torch.from_numpy(t)), torch.from_numpy(np.sum(t, axis=-1))), B


def test_restatement_sqrt_is_correctly_rounded():
    import math
    from deqsci_amd.gaptv import sqrt_float64
    x = torch.from_numpy(np.random.RandomState(8).random_sample(20000) * 4.0)
    assert sqrt_float64(x).tolist() == [math.sqrt(v) for v in x.tolist()]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_cpu_gaptv_vs_reference_shapes(case):
    from deqsci_amd.gaptv import gaptv_float64
    name, H, W, B, maxiter, step, weight, mask, seed = case
    gd, y, Phi = golden_case(name, H, W, B, mask, seed)
    assert np.array_equal(gd[f"{name}_params"], [H, W, B, maxiter, step, weight, seed])
    assert gd[f"{name}_tie"].min() >= TIE
    f, stop = gaptv_float64(y, Phi, phi_sum_t(Phi), maxiter, step, weight, return_stop=True)
    assert rel_l2(f.numpy(), gd[f"{name}_rec64"]) < 1e-12
    assert np.array_equal(stop.numpy(), gd[f"{name}_stop"][0])
    # every operation is numpy's, the square root correctly rounded (gaptv.sqrt_float64): bit for bit
    assert np.array_equal(f.numpy(), gd[f"{name}_rec64"])


def test_shapes_golden_masks_are_what_they_claim():
    gd = shapes_golden()
    assert os.path.getsize(os.path.join(GOLDEN, "gaptv_shapes.npz")) <= 300 * 1024
    kinds = {}
    for name, H, W, B, _, _, _, mask, seed in SHAPES:
        _, _, Phi = golden_case(name, H, W, B, mask, seed)
        binary = bool(((Phi == 0) | (Phi == 1)).all())
        zero_px = bool((Phi.sum(dim=3) == 0).any())
        kinds[mask] = (binary, zero_px)
        assert gd[f"{name}_rec64"].shape == (1, H, W, B)
    assert kinds["binary"][0] and not kinds["float"][0] and not kinds["zeros"][0]
    assert kinds["zeros"][1] and not kinds["float"][1]


# ----------------------------------------------------------------------------- GPU: GAP-TV
def batch_case(H, W, B, bsz, masks, seed):
    """bsz measurements, measurement m with its own seeded picture and a mask of kind masks[m % len(masks)] -> y (bsz,H,W),
    Phi (bsz,H,W,B), Phi_sum (bsz,H,W) float32 CPU tensors; the masks are asserted to differ."""
    ys, Phis = [], []
    for m in range(bsz):
        y, Phi = shape_case(H, W, B, masks[m % len(masks)], 1000 * seed + m)
        ys.append(torch.from_numpy(y))
        Phis.append(torch.from_numpy(Phi))
    y, Phi = torch.cat(ys), torch.cat(Phis)
    for m in range(1, bsz):
        assert not torch.equal(Phi[m], Phi[0])
    return y, Phi, phi_sum_t(Phi)


def assert_exact(out, stop, want, wstop, tie):
    """Per measurement whose every stop test clears TIE: equal stops, and the output equal to the restatement rounded to fp32."""
    keep = tie >= TIE
    assert keep.any()
    out, stop = out.cpu(), stop.cpu()
    assert torch.equal(stop[keep], wstop[keep]), (stop, wstop)
    assert torch.equal(out[keep], want[keep].float())
    return keep


# H, W, B, bsz, maxiter, step, weight, masks, n_iter_max
GAPTV_CASES = [(19, 23, 1, 3, 6, 1.0, 0.3, ("float", "binary", "zeros"), 30),
               (17, 130, 5, 2, 4, 1.0, 0.3, ("zeros", "float"), 30),          # three tile columns, the last ragged
               (11, 23, 13, 4, 4, 1.0, 0.3, ("float", "binary", "zeros"), 30),
               (9, 21, 16, 3, 4, 1.5, 0.3, ("float", "zeros"), 30),
               (5, 7, 128, 2, 3, 1.0, 0.1, ("binary", "float"), 30),
               (13, 70, 8, 2, 3, 1.0, 0.3, ("float",), 1),                    # n_iter_max 1: every TV call returns its input
               (21, 66, 13, 2, 1, 0.7, 0.2, ("zeros", "binary"), 30)]        # maxiter 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", GAPTV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-bsz{c[3]}-it{c[4]}-tv{c[8]}" for c in GAPTV_CASES])
def test_device_gaptv_vs_restatement(case):
    from deqsci_amd import _hip
    H, W, B, bsz, maxiter, step, weight, masks, n_iter_max = case
    y, Phi, Ps = batch_case(H, W, B, bsz, masks, H + B)
    want, wstop, tie = gaptv_planes_float64(y, Phi, Ps, maxiter, step, weight, n_iter_max)
    out, stop = _hip.gaptv(y.to(DEV), Phi.to(DEV), Ps.to(DEV), maxiter, step, weight, EPS, n_iter_max, return_stop=True)
    assert out.shape == (bsz, H, W, B) and stop.shape == (bsz, maxiter, B)
    keep = assert_exact(out, stop, want, wstop, tie)
    assert keep.all()
    if n_iter_max == 1:
        assert (stop.cpu() == 1).all()


@pytest.mark.gpu
def test_device_gaptv_mask_forms_are_bit_identical():
    """A shared mask (Phi and Phi_sum (1,...)) and both mixed forms _hip.gaptv expands equal the call with every measurement's copy."""
    from deqsci_amd import _hip
    H, W, B, bsz = 18, 67, 13, 3
    y1, Phi, _ = batch_case(H, W, B, 1, ("float",), 11)
    Ps = phi_sum_t(Phi)
    rs = np.random.RandomState(12)
    y = (y1 * torch.from_numpy(rs.uniform(0.5, 1.5, (bsz, 1, 1)).astype(np.float32))).to(DEV)   # distinct measurements
    dPhi, dPs = Phi.to(DEV), Ps.to(DEV)
    full = (dPhi.expand(bsz, -1, -1, -1).contiguous(), dPs.expand(bsz, -1, -1).contiguous())
    out, stop = _hip.gaptv(y, *full, 4, return_stop=True)
    for phi, ps in ((dPhi, dPs), (dPhi, full[1]), (full[0], dPs)):
        o, s = _hip.gaptv(y, phi, ps, 4, return_stop=True)
        assert torch.equal(o, out) and torch.equal(s, stop), (tuple(phi.shape), tuple(ps.shape))
    want, wstop, tie = gaptv_planes_float64(y.cpu(), full[0].cpu(), full[1].cpu(), 4, 1.0, 0.3)
    assert_exact(out, stop, want, wstop, tie)


@pytest.mark.gpu
def test_device_gaptv_maxiter_zero_is_the_adjoint():
    from deqsci_amd import At_torch_, _hip
    y, Phi, Ps = batch_case(15, 70, 13, 3, ("float", "binary", "zeros"), 21)
    dy, dPhi = y.to(DEV), Phi.to(DEV)
    out, stop = _hip.gaptv(dy, dPhi, Ps.to(DEV), 0, return_stop=True)
    assert stop.shape == (3, 0, 13)
    assert torch.equal(out, At_torch_(dy, dPhi))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_device_gaptv_rec_vs_reference_shapes(case):
    """GAP_TV_rec on the device against the reference's own records (gaptv_shapes.npz): every stop, and the output equal to the
    reference's float64 result rounded to fp32 (what the reference returns)."""
    from deqsci_amd import A_torch_, At_torch_, GAP_TV_rec
    name, H, W, B, maxiter, step, weight, mask, seed = case
    gd, y, Phi = golden_case(name, H, W, B, mask, seed)
    out, stop = GAP_TV_rec(y.to(DEV), Phi.to(DEV), phi_sum_t(Phi).to(DEV), None, A_torch_, At_torch_, maxiter, step, weight,
                           return_stop=True)
    assert np.array_equal(stop.cpu().numpy(), gd[f"{name}_stop"])
    assert torch.equal(out.cpu(), torch.from_numpy(gd[f"{name}_rec64"].astype(np.float32)))


# ----------------------------------------------------------------------------- GPU: the Chambolle kernel at tile edges
# (n, H, W): single pixel, one row, one column, exactly one tile, one column past a tile, two full tile columns and a ragged third, 65 tiles
# (13 x 5, both ragged), 77 tiles (7 x 11, both ragged), 300 small planes in one launch
EDGE_SHAPES = [(1, 1, 1), (2, 1, 200), (2, 150, 1), (3, 16, 64), (3, 17, 65), (2, 33, 130), (2, 200, 300), (2, 100, 700), (300, 5, 7)]
EDGE_CASES = [(s, w, tau) for s in EDGE_SHAPES for w, tau in ((0.3, 1. / 6.), (0.1, 1. / 4.))]


def check_tv(x, weight, n_iter_max, tau):
    from deqsci_amd import _hip
    want, wstop, tie = tv_planes_float64(x, weight, EPS, n_iter_max, tau)
    got, stop = _hip.tv_chambolle(x.to(DEV), weight, EPS, n_iter_max, tau, return_stop=True)
    keep = tie >= TIE
    assert keep.any()
    assert rel_l2(got.cpu()[keep].numpy(), want[keep].numpy()) < 1e-7
    assert torch.equal(stop.cpu()[keep], wstop[keep]), (stop.cpu(), wstop)
    assert torch.equal(got.cpu()[keep], want[keep].float())
    return stop.cpu(), keep


@pytest.mark.gpu
@pytest.mark.parametrize("shape,weight,tau", EDGE_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-w{w}-tau{4 if t == 0.25 else 6}" for s, w, t in EDGE_CASES])
def test_tv_kernel_tile_edges_vs_float64_restatement(shape, weight, tau):
    n, H, W = shape
    x = image(shape, 300 + H + W)
    stop, keep = check_tv(x, weight, 100, tau)
    assert keep.float().mean() > 0.9
    if H * W > 1:
        assert (stop < 100).any()                                                         # the stop fires somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 65), (33, 130)])
def test_tv_kernel_mixed_planes_stop_apart(H, W):
    """Zero, constant, smooth, noisy and very noisy planes in one launch: the constant ones never stop (E_init = 0), the others at
    different iterations, each as the restatement."""
    base = image((1, H, W), 7)[0]
    noise = torch.randn(3, H, W, generator=torch.Generator().manual_seed(8))
    x = torch.stack([torch.zeros(H, W), torch.full((H, W), 0.37), base - 0.1 * noise[0], base, base + 0.3 * noise[1],
                     torch.full((H, W), -2.5), 0.5 + noise[2]]).float()
    for tau in (1. / 6., 1. / 4.):
        stop, keep = check_tv(x, 0.2, 200, tau)
        assert keep.all()
        assert stop[0] == 200 and stop[1] == 200 and stop[5] == 200
        assert len(set(stop[[2, 3, 4, 6]].tolist())) >= 3 and (stop[[2, 3, 4, 6]] < 200).all()


def late_detail(shape, seed, r0, c0):
    """image(shape, seed) kept only in rows >= r0 and columns >= c0, every other pixel the mean of its part: nearly all of E lies in the
    tiles a 64-lane fold reaches second (tile index >= 64 for the two shapes below)."""
    x = image(shape, seed)
    x[:, :r0, :] = x[:, :r0, :].mean()
    x[:, r0:, :c0] = x[:, r0:, :c0].mean()
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("shape,r0,c0", [((2, 200, 300), 176, 192), ((2, 100, 700), 80, 512)], ids=["65tiles", "77tiles"])
def test_tv_kernel_fold_of_more_than_64_tiles(shape, r0, c0):
    x = late_detail(shape, 9 + shape[1], r0, c0)
    for weight, tau in ((0.3, 1. / 6.), (0.1, 1. / 4.), (0.05, 1. / 6.)):
        _, keep = check_tv(x, weight, 100, tau)
        assert keep.all()
