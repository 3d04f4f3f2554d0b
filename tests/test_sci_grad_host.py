"""CPU: tests/sci_grad_ref.py - the statement of what csrc/sci_grad.hip computes - held to torch's float64 autograd and to itself, the C ABI's
argument validation of the three entries (which happens before any launch, so it needs no GPU), and tests/golden/mask_grad.npz."""
import functools
import os

import numpy as np
import pytest
import torch

import sci_grad_ref as sg
import sci_ops_ref as so
from sci_ops_ref import BHW, HWB
from deqsci_amd import _hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(B, H, W, kernel, mask, shared) for (B, H, W, kernel) in sg.GRID for mask in ("uniform", "binary") for shared in (False, True)]
IDS = [f"B{c[0]}-{c[1]}x{c[2]}-{c[4]}-{'shared' if c[5] else 'persample'}" for c in CASES]


@functools.lru_cache(maxsize=None)
def data(H, W, B, mask, shared):
    return sg.case_data(H, W, B, mask, shared)


def close64(a, b):
    """float64 formulas against float64 autograd: rounding of a few operations apart, relative to the largest entry."""
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


# ----------------------------------------------------------------------------- the formulas against autograd
@pytest.mark.parametrize("shared", [False, True])
def test_float64_formulas_are_torch_autograd(shared):
    Phi, z, g, y, s, a, gs_in = data(5, 7, 8, "uniform", shared)
    zd, yd, gd = z.double().requires_grad_(), y.double().requires_grad_(), g.double()
    pd, sd = Phi.double().requires_grad_(), s.double().requires_grad_()
    z1 = zd + ((yd - (zd * pd).sum(-1)) / sd).unsqueeze(-1) * pd                                    # z + At((y - A z) / s)
    gz, gy, gphi, gs = torch.autograd.grad(z1, [zd, yd, pd, sd], gd)
    ref = sg.ref_gap_grad(z, Phi, g, y, s)
    assert close64(ref["gphi"][0], gphi) and close64(ref["gs"][0], gs) and close64(ref["gz"][0], gz) and close64(ref["gy"][0], gy)
    assert ref["gphi"][0].shape == Phi.shape and ref["gs"][0].shape == s.shape
    # A and At
    pd = Phi.double().requires_grad_()
    (gp,) = torch.autograd.grad((zd.detach() * pd).sum(-1), pd, a.double())                         # y = A(x, Phi), a = grad y, v = x
    assert close64(sg.ref_mask_grad(a, z, shared)[0], gp)
    (gp,) = torch.autograd.grad(a.double().unsqueeze(-1) * pd, pd, gd)                              # x = At(y, Phi), a = y, v = grad x
    assert close64(sg.ref_mask_grad(a, g, shared)[0], gp)
    # sum, zeros -> 1
    pd = Phi.double().requires_grad_()
    S = pd.sum(-1)
    S = torch.where(S == 0, torch.ones_like(S), S)
    (gp,) = torch.autograd.grad(S, pd, gs_in.double())
    want = sg.ref_phi_sum_grad(Phi, gs_in)
    assert torch.equal(want.double(), gp) and (want[Phi.double().sum(-1) == 0] == 0).all() and (want != 0).any()


# ----------------------------------------------------------------------------- the emulations within the bounds
@pytest.mark.parametrize("B,H,W,kernel,mask,shared", CASES, ids=IDS)
def test_emulation_of_every_path_is_within_the_bound(B, H, W, kernel, mask, shared):
    P, nm = H * W, 1 if shared else sg.BSZ
    for op in sg.OPS:
        assert sg.path_of(op, HWB, B, P, sg.traffic_bytes(op, sg.BSZ, nm, P, B, sg.OUTPUTS)) == (kernel, "default")
    Phi, z, g, y, s, a, gs_in = data(H, W, B, mask, shared)
    ref, emu = sg.ref_gap_grad(z, Phi, g, y, s), sg.emu_gap_grad(z, Phi, g, y, s, kernel)
    for k in sg.OUTPUTS:
        ex, bd = ref[k]
        assert emu[k].shape == ex.shape and emu[k].dtype == torch.float32
        r = sg.ratio(emu[k], ex, bd)
        assert 0 < r <= 1, (k, r)
    assert emu["gphi"].shape == Phi.shape and emu["gs"].shape == s.shape
    for v in (z, g):
        ex, bd = sg.ref_mask_grad(a, v, shared)
        got = sg.emu_mask_grad(a, v, shared)
        assert sg.ratio(got, ex, bd) <= 1
        if not shared:
            assert torch.equal(got, ex.float())
    assert torch.equal(sg.emu_phi_sum_grad(Phi, gs_in, kernel), sg.ref_phi_sum_grad(Phi, gs_in))


def test_the_bounds_bite():
    """An error of one part in 2^17 in the emulation's r is far outside every G1 bound that r enters: the bounds are first-order tight, not slack."""
    Phi, z, g, y, s, _, _ = data(37, 53, 8, "uniform", False)
    ref = sg.ref_gap_grad(z, Phi, g, y, s)
    emu = sg.emu_gap_grad(z, Phi, g, y * (1 + 2.0 ** -17), s, "hwb2")
    assert sg.ratio(emu["gphi"], *ref["gphi"]) > 1 and sg.ratio(emu["gs"], *ref["gs"]) > 1
    emu = sg.emu_gap_grad(z, Phi, g * (1 + 2.0 ** -17), y, s, "hwb2")
    assert sg.ratio(emu["gz"], *ref["gz"]) > 1 and sg.ratio(emu["gy"], *ref["gy"]) > 1


def test_traffic_and_paths():
    P, B = 256 * 256, 8
    assert sg.traffic_bytes("gap_grad", 1, 1, 1, B) == 16 * B + 12 and sg.traffic_bytes("gap_grad", 1, 1, 1, B, sg.OUTPUTS) == 20 * B + 16
    assert sg.traffic_bytes("gap_grad", 8, 1, 1, B) == 8 * (8 * B + 4) + (8 * B + 8)                # shared: Phi, s read once, 4B + 4 written once
    n = sg.traffic_bytes("gap_grad", 8, 8, P, B)
    assert sg.traffic_bytes("gap_grad", 7, 7, P, B) < so.STREAM_MIN_BYTES <= n
    assert sg.path_of("gap_grad", HWB, B, P, n) == ("hwb2", "streaming")
    assert sg.path_of("gap_grad", HWB, 12, P, n) == ("generic", "default")
    assert sg.path_of("gap_grad", BHW, B, P, n) == ("unsupported", "default")
    assert sg.blocks_of("hwb2", B, P) == 128 and sg.blocks_of("generic", 12, 37 * 53) == 8 and sg.blocks_of("hwb8", 32, 37 * 53) == 16


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_validate_before_any_launch():
    lib = _hip.load()
    g1, g2, g3 = lib.deqsci_gap_update_grad_f32, lib.deqsci_sci_mask_grad_f32, lib.deqsci_phi_sum_grad_f32
    far = 1 << 40                                                                                   # addresses only: validation dereferences nothing
    z, phi, g, y, s, gphi, gs, gz, gy = (far + (i << 24) for i in range(9))
    ins, outs, dims = [z, phi, g, y, s], [gphi, gs, gz, gy], (2, 4, 4, 8)
    # NULL -> -1: any input; all four outputs of G1 (one alone may be NULL)
    for i in range(5):
        bad = list(ins)
        bad[i] = None
        assert g1(*bad, *outs, *dims, HWB, 0, None) == -1, i
    assert g1(*ins, None, None, None, None, *dims, HWB, 0, None) == -1
    for i in range(3):
        bad = [y, z, gphi]
        bad[i] = None
        assert g2(*bad, *dims, HWB, 0, None) == -1 and g3(*bad, *dims, HWB, None) == -1, i
    assert g1(None, None, None, None, None, None, None, None, None, 0, 0, 0, 0, 7, 0, None) == -1   # NULL is checked first
    # shape -> -2
    for bad in ((0, 4, 4, 8), (2, 0, 4, 8), (2, 4, -1, 8), (2, 4, 4, 0)):
        assert g1(*ins, *outs, *bad, HWB, 0, None) == -2 and g2(y, z, gphi, *bad, HWB, 0, None) == -2 and g3(phi, gs, gphi, *bad, HWB, None) == -2
    # unsupported -> -4: planar, an unknown layout, a batch beyond gridDim.y, B beyond 4096
    for layout in (BHW, 7):
        assert g1(*ins, *outs, *dims, layout, 0, None) == -4 and g2(y, z, gphi, *dims, layout, 0, None) == -4 and g3(phi, gs, gphi, *dims, layout, None) == -4
    for bad in ((so.MAX_BSZ + 1, 4, 4, 8), (2, 4, 4, so.MAX_B + 1)):
        assert g1(*ins, *outs, *bad, HWB, 0, None) == -4 and g2(y, z, gphi, *bad, HWB, 0, None) == -4 and g3(phi, gs, gphi, *bad, HWB, None) == -4
    # alignment -> -3: every pointer, the optional ones included; shape is reported before alignment
    for i in range(9):
        bad = ins + outs
        bad[i] += 4
        assert g1(*bad, *dims, HWB, 1, None) == -3, i
    assert g1(z + 4, phi, g, y, s, *outs, 0, 4, 4, 8, HWB, 0, None) == -2
    for i in range(3):
        bad = [y, z, gphi]
        bad[i] += 8
        assert g2(*bad, *dims, HWB, 0, None) == -3 and g3(*bad, *dims, HWB, None) == -3, i


# ----------------------------------------------------------------------------- the golden
def test_mask_grad_golden_is_complete_and_well_conditioned():
    g = np.load(os.path.join(GOLDEN, "mask_grad.npz"))
    cases = [f"{kind}.{mask}.{params}" for kind in ("SimpleCNN", "ffdnet") for mask in ("ps", "sh") for params in ("train", "frozen")]
    assert list(g["cases"]) == cases and g["conditioning"].shape == (8,)
    assert 0 < float(g["conditioning"].max()) < 1e-5
    assert g["Phi.ps"].shape == (2, 24, 20, 4) and g["Phi.sh"].shape == (1, 24, 20, 4) and g["gt"].shape == (2, 24, 20, 4) and int(g["iters"]) == 12
    for mask in ("ps", "sh"):
        Phi = g["Phi." + mask]
        assert (Phi[:, 0, :2] == 0).all() and Phi[Phi != 0].min() >= 0.1 and Phi.max() <= 1.0
    for tag in cases:
        kind, mask, params = tag.split(".")
        for k in ("grad.Phi", "rec", "loss", "forward_res", "backward_res"):
            assert np.isfinite(g[f"{tag}.{k}"]).all(), (tag, k)
        assert g[f"{tag}.grad.Phi"].shape == g["Phi." + mask].shape and np.abs(g[f"{tag}.grad.Phi"]).max() > 0
        assert g[f"{tag}.rec"].shape == (2, 24, 20, 4)
        assert (f"{tag}.sigma_after" in g.files) == (kind == "ffdnet")
        grads = [k for k in g.files if k.startswith(tag + ".grad.nonlinear_op") or k.startswith(tag + ".gradslice.")]
        assert bool(grads) == (params == "train")
        if params == "train":
            assert any(k.startswith(tag + ".gradslice.") and g[k].shape == (2, 64, 3, 3) for k in grads)
            assert all(g[k].size <= 4096 for k in grads)
