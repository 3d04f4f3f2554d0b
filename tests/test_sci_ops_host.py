"""CPU: tests/sci_ops_ref.py against itself and against tests/golden/ops.npz - the fp32 emulation of every kernel path of csrc/sci_ops.hip
within the derived bounds of the float64 reference (no atol: the bounds scale with the data), path_of against a hand-written table of the
shapes tests/test_sci_ops_gpu.py runs, and the reach of a NaN / Inf through the emulation."""
import os

import numpy as np
import pytest
import torch

import sci_ops_ref as so
from conftest import GOLDEN
from sci_ops_ref import BHW, HWB

TREE_B = (4, 8, 16, 32)
SEQ_B = (4, 5, 8, 12, 16, 19, 32)
P_HOST = 15000


def _kernels(B):
    """Every order of summation a launch with B frames can take."""
    return ([f"hwb{B // 4}"] if B in TREE_B else []) + ["generic"]


def _mask(kind, P, B, gen):
    if kind == "binary":
        Phi = (torch.rand(1, P, B, generator=gen) < 0.5).float()
        Phi[:, :2] = 0
        return Phi
    return so.uniform_mask(1, P, B, gen) if kind == "uniform" else so.signed_mask(1, P, B, gen)


def _phisum(Phi):
    s = Phi.double().sum(-1)
    return torch.where(s == 0, torch.ones_like(s), s).float()          # (the float64 sum rounded once: any fp32 Phi_sum is a valid INPUT of the step)


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e3])
@pytest.mark.parametrize("kind", ["binary", "uniform", "signed"])
@pytest.mark.parametrize("B", sorted(set(TREE_B + SEQ_B)))
def test_emulation_of_every_path_is_within_the_bound(B, kind, scale):
    gen = torch.Generator().manual_seed(1000 * B + len(kind))
    Phi = _mask(kind, P_HOST, B, gen)
    z = torch.randn(2, P_HOST, B, generator=gen) * scale
    y = torch.rand(2, P_HOST, generator=gen) * (B / 4) * scale
    s = _phisum(Phi)
    ex_f, bd_f = so.ref_forward(z, Phi)
    ex_s, bd_s, zero = so.ref_phi_sum(Phi)
    ex_g, bd_g = so.ref_gap(z, Phi, y, s)
    assert bool(zero.any()) == (kind != "signed")
    for k in _kernels(B):
        rf = so.ratio(so.emu_forward(z, Phi, k), ex_f, bd_f)
        got_s = so.emu_phi_sum(Phi, k)
        assert (got_s[zero] == 1).all()
        rs = so.ratio(got_s, ex_s, bd_s)
        rg = so.ratio(so.emu_gap(z, Phi, y, s, k), ex_g, bd_g)
        print(f"B={B} {kind} x{scale:g} {k}: forward {rf:.3f} phi_sum {rs:.3f} gap {rg:.3f} of the bound")
        assert rf <= 1 and rs <= 1 and rg <= 1, (k, rf, rs, rg)
    assert torch.equal(so.emu_adjoint(y, Phi), so.ref_adjoint(y, Phi))


def test_the_bounds_bite():
    """What the bounds must not let through, on unit-scale data with a uniform mask: one frame's product dropped from the forward, the last
    butterfly level dropped, and a GAP step whose residual is off by one part in 2^20 (a 'dropped low-order term')."""
    B, gen = 32, torch.Generator().manual_seed(7)
    Phi = so.uniform_mask(1, 4096, B, gen)
    z = torch.randn(1, 4096, B, generator=gen)
    y = torch.rand(1, 4096, generator=gen) * 8
    s = _phisum(Phi)
    ex_f, bd_f = so.ref_forward(z, Phi)
    ex_g, bd_g = so.ref_gap(z, Phi, y, s)
    live = Phi[0, :, 5] != 0
    assert so.ratio((so.emu_forward(z, Phi, "generic") - z[..., 5] * Phi[..., 5])[:, live], ex_f[:, live], bd_f[:, live]) > 1e3
    half = so.emu_forward(z[..., :16].contiguous(), Phi[..., :16].contiguous(), "hwb4")
    assert so.ratio(half[:, live], ex_f[:, live], bd_f[:, live]) > 1e3
    off = z + ((y - so.emu_forward(z, Phi, "hwb8")) * (1 + 2.0 ** -20) / s).unsqueeze(-1) * Phi
    assert so.ratio(off, ex_g, bd_g) > 1


def test_emulation_vs_reference_golden():
    """tests/golden/ops.npz (the reference's own A_torch_ / GAP step on the CPU): the emulation of every order within the bound of the golden
    values' float64 reference, the golden values themselves within it, and - c0 and grey (B = 8), where the sum of the CPU that wrote the file
    runs left to right (at B = 16 and B = 5 its vectorised sum takes another order, which no kernel path shares) - the sequential emulation
    bit-equal to the golden GAP step (both) and forward (c0; the grey case stores none)."""
    g = np.load(os.path.join(GOLDEN, "ops.npz"))
    T = lambda k: torch.from_numpy(g[k])
    flat = lambda t: t.reshape(t.shape[0], -1, t.shape[-1]) if t.dim() == 4 else t.reshape(t.shape[0], -1)
    for c in ("c0_", "c1_", "c2_", "grey_"):
        Phi, z, y, s = flat(T(c + "Phi")), flat(T(c + "z")), flat(T(c + "y")), flat(T(c + "Phi_sum"))
        B = Phi.shape[-1]
        ex_g, bd_g = so.ref_gap(z, Phi, y, s)
        assert so.ratio(flat(T(c + "z1")), ex_g, bd_g) <= 1
        ex_s, bd_s, zero = so.ref_phi_sum(Phi)
        if c in ("c0_", "grey_"):                              # (grey: the one fixture whose products are inexact - mul, sum, sub, div, add each rounded as the reference rounds them)
            assert torch.equal(so.emu_gap(z, Phi, y, s, "generic"), flat(T(c + "z1"))), c
        for k in _kernels(B):
            assert so.ratio(so.emu_gap(z, Phi, y, s, k), ex_g, bd_g) <= 1, (c, k)
            got_s = so.emu_phi_sum(Phi, k)
            assert so.ratio(got_s, ex_s, bd_s) <= 1 and (got_s[zero] == 1).all()
            if c != "grey_":
                assert torch.equal(got_s, s)                   # (a binary mask sums exactly in any order)
        if c == "grey_":
            continue
        x = flat(T(c + "x"))
        assert torch.equal(so.emu_adjoint(y, Phi), flat(T(c + "Aty")))
        for a, want in ((x, y), (z, flat(T(c + "Az")))):
            ex_f, bd_f = so.ref_forward(a, Phi)
            assert so.ratio(want, ex_f, bd_f) <= 1
            for k in _kernels(B):
                assert so.ratio(so.emu_forward(a, Phi, k), ex_f, bd_f) <= 1, (c, k)
            if c == "c0_":
                assert torch.equal(so.emu_forward(a, Phi, "generic"), want)


# (op, layout_in, layout_out, B, H, W) -> kernel: the shapes of tests/test_sci_ops_gpu.py, written out by hand from the launchers
PATH_TABLE = (
    [(op, HWB, HWB, B, H, W, f"hwb{B // 4}") for op in ("forward", "adjoint", "phi_sum", "gap") for B in (4, 8, 16, 32) for (H, W) in ((5, 7), (33, 31), (32, 32))] +
    [(op, BHW, BHW, B, H, W, "bhw") for op in ("forward", "adjoint", "phi_sum") for B in (5, 8, 19, 32) for (H, W) in ((6, 6), (36, 30))] +
    [("gap", BHW, BHW, B, H, W, f"bhw{B}") for B in (4, 8, 16) for (H, W) in ((6, 6), (36, 30))] +
    [("gap", BHW, BHW, B, 6, 6, "generic") for B in (32, 5)] +
    [("gap", HWB, BHW, B, H, W, f"hwb2bhw{B // 4}") for B in (4, 8, 16, 32) for (H, W) in ((6, 6), (10, 26), (36, 30))] +
    [(op, lay, lay, B, H, W, "generic") for op in ("forward", "adjoint", "phi_sum", "gap") for lay in (HWB, BHW) for (B, H, W) in ((5, 5, 7), (12, 17, 23))] +
    [(op, BHW, BHW, 8, 5, 7, "generic") for op in ("forward", "adjoint", "phi_sum", "gap")] +
    [("gap", HWB, BHW, 8, 5, 7, "generic"), ("gap", BHW, HWB, 8, 5, 7, "generic"), ("gap", BHW, HWB, 8, 6, 6, "generic"), ("gap", BHW, HWB, 12, 17, 23, "generic"),
     ("gap", HWB, BHW, 12, 17, 23, "generic"), ("gap", HWB, HWB, 12, 17, 23, "generic")] +
    [("transpose", a, b, B, H, W, "transpose_fast") for (a, b) in ((HWB, BHW), (BHW, HWB)) for B in (4, 8, 16, 32) for (H, W) in ((6, 6), (10, 26), (36, 30))] +
    [("transpose", a, b, 8, 5, 7, "transpose_generic(8224)") for (a, b) in ((HWB, BHW), (BHW, HWB))] +
    [("transpose", a, b, 12, 17, 23, "transpose_generic(12336)") for (a, b) in ((HWB, BHW), (BHW, HWB))] +
    [("transpose", HWB, BHW, 63, 17, 23, "transpose_generic(64764)"), ("transpose", HWB, BHW, 64, 17, 23, "transpose_generic(65792)"),
     ("transpose", HWB, BHW, 65, 17, 23, "transpose_generic(66820)"), ("transpose", BHW, HWB, 159, 17, 23, "transpose_generic(163452)"),
     ("transpose", HWB, BHW, 160, 17, 23, "unsupported"), ("transpose", BHW, HWB, 160, 17, 23, "unsupported"), ("transpose", HWB, BHW, 4097, 2, 2, "unsupported")] +
    [("residual_out", BHW, BHW, 3, 1, 1, "sub_flat"), ("residual_out", BHW, BHW, 5, 5, 7, "sub_flat"), ("residual_out", BHW, BHW, 8, 6, 6, "sub_flat"),
     ("residual_out", BHW, HWB, 8, 6, 6, "bhw2hwb2"), ("residual_out", BHW, HWB, 32, 36, 30, "bhw2hwb8"), ("residual_out", BHW, HWB, 5, 5, 7, "unsupported"),
     ("residual_out", BHW, HWB, 8, 5, 7, "unsupported")])


def test_path_of_against_the_hand_written_table():
    for op, li, lo, B, H, W, kernel in PATH_TABLE:
        got = so.path_of(op, li, lo, B, H * W, so.traffic_bytes(op, 3, H * W, B))
        assert got == (kernel, "default"), (op, li, lo, B, H, W, got)
    # the 64 KiB of dynamic LDS a kernel gets without asking end between B = 63 and B = 64 (257 floats per frame), the 160 KiB of a workgroup at 159
    assert 63 * 257 * 4 <= so.LDS_OPT_IN < 64 * 257 * 4 and 159 * 257 * 4 <= so.LDS_MAX < 160 * 257 * 4


def test_path_of_policy_and_block_counts():
    """The streaming side of each launcher's own byte formula, and the grids the GPU cases rely on (one block / a ragged last block)."""
    P = 508 * 488
    assert so.traffic_bytes("forward", 4, P, 8) == 4 * P * 68 >= so.STREAM_MIN_BYTES > so.traffic_bytes("forward", 3, P, 8)
    assert so.path_of("forward", HWB, HWB, 8, P, so.traffic_bytes("forward", 4, P, 8)) == ("hwb2", "streaming")
    assert so.path_of("forward", BHW, BHW, 8, P, so.traffic_bytes("forward", 4, P, 8)) == ("bhw", "streaming")
    assert so.path_of("forward", HWB, HWB, 8, P, so.traffic_bytes("forward", 3, P, 8)) == ("hwb2", "default")
    assert so.path_of("forward", HWB, HWB, 5, P, so.traffic_bytes("forward", 8, P, 5)) == ("generic", "default")          # (no policy in the fallbacks)
    assert so.path_of("gap", HWB, BHW, 8, P, so.STREAM_MIN_BYTES) == ("hwb2bhw2", "streaming")
    assert so.path_of("gap", HWB, BHW, 8, P, so.STREAM_MIN_BYTES - 1) == ("hwb2bhw2", "default")
    assert so.path_of("transpose", HWB, BHW, 8, P, so.STREAM_MIN_BYTES) == ("transpose_fast", "streaming")
    assert so.path_of("residual_out", BHW, BHW, 5, 7, so.STREAM_MIN_BYTES) == ("sub_flat", "streaming")
    assert so.path_of("transpose", HWB, BHW, 12, P, so.STREAM_MIN_BYTES) == ("transpose_generic(12336)", "default")
    assert [so.blocks_of(f"hwb{B // 4}", B, 35) for B in (4, 8, 16, 32)] == [1, 1, 1, 1]
    assert [so.blocks_of(f"hwb{B // 4}", B, 1023) for B in (4, 8, 16, 32)] == [1, 2, 4, 8]
    assert [(1023 * lp) % 1024 for lp in (1, 2, 4, 8)] == [1023, 1022, 1020, 1016]
    assert so.blocks_of("bhw", 8, 36) == 1 and so.blocks_of("bhw", 8, 1080) == 2
    assert so.blocks_of("hwb2bhw2", 8, 260) == 2 and so.blocks_of("generic", 12, 17 * 23) == 2
    assert (P * 2) % 1024 == 192


@pytest.mark.parametrize("kernel,B", [("hwb8", 32), ("hwb2", 8), ("generic", 8), ("generic", 12)])
def test_nonfinite_reach_of_the_emulation(kernel, B):
    """A poisoned z, y or Phi element: the emulation is non-finite exactly where the float64 reference is - y[n, p] of the forward, all B
    frames of (n, p) of the GAP step - and every other element keeps the bits of the clean run."""
    P, n = 1080, 1
    gen = torch.Generator().manual_seed(B)
    bits = lambda t: t.contiguous().view(torch.int32)
    for mask in ("uniform", "binary"):
        Phi = _mask(mask, P, B, gen).expand(3, P, B).contiguous()
        z = torch.randn(3, P, B, generator=gen)
        y = torch.rand(3, P, generator=gen) * 4
        s = _phisum(Phi)
        clean_f, clean_g = so.emu_forward(z, Phi, kernel), so.emu_gap(z, Phi, y, s, kernel)
        for p in so.poison_pixels(P):
            b = so.poison_frame(p, B)
            for val in so.POISONS.values():
                for which in ("z", "y", "Phi"):
                    zz, yy, pp = z.clone(), y.clone(), Phi.clone()
                    if which == "y":
                        yy[n, p] = val
                    else:
                        (zz if which == "z" else pp)[n, p, b] = val
                    hit_g = so.nonfinite_gap(zz, pp, yy, s)
                    want_g = torch.zeros(3, P, B, dtype=torch.bool)
                    want_g[n, p] = True
                    assert torch.equal(hit_g, want_g), (mask, p, val, which)
                    got_g = so.emu_gap(zz, pp, yy, s, kernel)
                    assert torch.equal(~torch.isfinite(got_g), hit_g)
                    assert torch.equal(bits(got_g)[~hit_g], bits(clean_g)[~hit_g])
                    if which != "y":
                        hit_f = so.nonfinite_forward(zz, pp)
                        want_f = torch.zeros(3, P, dtype=torch.bool)
                        want_f[n, p] = True
                        got_f = so.emu_forward(zz, pp, kernel)
                        assert torch.equal(hit_f, want_f) and torch.equal(~torch.isfinite(got_f), hit_f)
                        assert torch.equal(bits(got_f)[~hit_f], bits(clean_f)[~hit_f])
    # phi_sum: a NaN is not the 0 that becomes 1
    pp = Phi.clone()
    pp[n, 0, 0] = float("nan")
    got = so.emu_phi_sum(pp, kernel)
    assert torch.isnan(got[n, 0]) and int(torch.isnan(got).sum()) == 1
