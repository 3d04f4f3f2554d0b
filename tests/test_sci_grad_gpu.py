"""GPU: every kernel and instantiation of csrc/sci_grad.hip (gap_update_grad, sci_mask_grad, phi_sum_grad) against tests/sci_grad_ref.py, at the
smallest shapes where each path can still go wrong (TB = 256 threads, UNR = 4 float4 per lane): 5 x 7 is less than one block, 37 x 53 is
several blocks with a ragged last one whose last wave is not full (Q % 64 != 0: clamped lanes).  Every case asserts the path it believes it is
on (sci_grad_ref.path_of) and then holds the kernel to
  (a) the float64 reference within the derived first-order bound (no atol; G2 per sample and G3 are exact),
  (b) the fp32 emulation of that path's order of operations, bit for bit,
  (c) G1's gz to gap_update(g, Phi, 0, s) and its gy to sci_forward(g, Phi) / s, bit for bit: the two launches the backward made before,
  (d) a second launch, bit for bit.
bsz = 3, Phi shared and per sample, sci_ops_ref.uniform_mask (all-zero pixels, pixels that cancel to exactly 0) and a binary mask.  Every
output is pre-filled with NaN between sentinels, as in tests/test_sci_ops_gpu.py."""
import ctypes
import functools
import itertools

import pytest
import torch

import sci_grad_ref as sg
import sci_ops_ref as so
from sci_ops_ref import HWB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip

DEV = "cuda"
BSZ = sg.BSZ
NAN = float("nan")
SENTINEL = -7777.0
GUARD = 64


def guarded(shape, fill=NAN):
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
    body = buf[GUARD:GUARD + numel]
    body.fill_(fill)
    assert body.data_ptr() % 16 == 0
    return body.view(shape), buf


def intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def data(H, W, B, mask, shared):
    return sg.case_data(H, W, B, mask, shared)


def dev(t, H, W):
    """logical CPU (n, P[, B]) -> device (n, H, W[, B])."""
    return t.reshape(t.shape[0], H, W, *t.shape[2:]).contiguous().to(DEV)


def logical(t):
    return t.reshape(t.shape[0], t.shape[1] * t.shape[2], *t.shape[3:]).cpu()


def out_shapes(nm, bsz, H, W, B):
    return {"gphi": (nm, H, W, B), "gs": (nm, H, W), "gz": (bsz, H, W, B), "gy": (bsz, H, W)}


def run_g1(d, H, W, B, shared, want=sg.OUTPUTS, bsz=BSZ):
    """One G1 launch into guarded outputs; -> {name: device tensor} for the outputs asked for (the others must stay untouched: they are None)."""
    nm = 1 if shared else bsz
    shapes = out_shapes(nm, bsz, H, W, B)
    outs = {k: guarded(shapes[k]) for k in want}
    got = _hip.gap_update_grad(d["z"], d["Phi"], d["g"], d["y"], d["s"], need=tuple(k in want for k in sg.OUTPUTS),
                               out=tuple(outs[k][0] if k in want else None for k in sg.OUTPUTS))
    for k, t in zip(sg.OUTPUTS, got):
        assert (t is None) == (k not in want)
    assert all(intact(buf) for _, buf in outs.values())
    return {k: v for k, (v, _) in outs.items()}


CASES = [(B, H, W, kernel, mask, shared) for (B, H, W, kernel) in sg.GRID for mask in ("uniform", "binary") for shared in (False, True)]
IDS = [f"B{c[0]}-{c[1]}x{c[2]}-{c[4]}-{'shared' if c[5] else 'persample'}" for c in CASES]


@pytest.mark.parametrize("B,H,W,kernel,mask,shared", CASES, ids=IDS)
def test_gap_update_grad(B, H, W, kernel, mask, shared):
    P, nm = H * W, 1 if shared else BSZ
    assert sg.path_of("gap_grad", HWB, B, P, sg.traffic_bytes("gap_grad", BSZ, nm, P, B, sg.OUTPUTS)) == (kernel, "default")
    if kernel.startswith("hwb") and (H, W) == (37, 53):
        assert sg.blocks_of(kernel, B, P) > 1 and (P * (B // 4)) % 1024 != 0 and (P * (B // 4)) % 64 != 0
    Phi, z, g, y, s, _, _ = data(H, W, B, mask, shared)
    d = {"Phi": dev(Phi, H, W), "z": dev(z, H, W), "g": dev(g, H, W), "y": dev(y, H, W), "s": dev(s, H, W)}
    got = run_g1(d, H, W, B, shared)
    ref, emu = sg.ref_gap_grad(z, Phi, g, y, s), sg.emu_gap_grad(z, Phi, g, y, s, kernel)
    for k in sg.OUTPUTS:
        r = sg.ratio(logical(got[k]), *ref[k])
        print(f"ROW | gap_grad {k} B={B} {H}x{W} {mask} shared={shared} | {kernel} | err/bound {r:.3f} |")
        assert r <= 1, (k, r)                                                                                   # (a)
        assert torch.equal(bits(logical(got[k])), bits(emu[k])), k                                              # (b)
    zero_y = torch.zeros(BSZ, H, W, device=DEV)
    assert torch.equal(bits(got["gz"]), bits(_hip.gap_update(d["g"], d["Phi"], zero_y, d["s"], HWB, HWB)))      # (c)
    assert torch.equal(bits(got["gy"]), bits(_hip.sci_forward(d["g"], d["Phi"], HWB) / d["s"]))
    again = run_g1(d, H, W, B, shared)
    assert all(torch.equal(bits(again[k]), bits(got[k])) for k in sg.OUTPUTS)                                   # (d)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,kernel", [(8, "hwb2"), (12, "generic")])
def test_gap_update_grad_every_combination_of_null_outputs(B, kernel, shared):
    """Each of the 15 non-empty subsets of the outputs gives the bits of the launch with all four, and touches nothing else."""
    H, W = 37, 53
    Phi, z, g, y, s, _, _ = data(H, W, B, "uniform", shared)
    d = {"Phi": dev(Phi, H, W), "z": dev(z, H, W), "g": dev(g, H, W), "y": dev(y, H, W), "s": dev(s, H, W)}
    full = run_g1(d, H, W, B, shared)
    for k in range(1, 4):
        for want in itertools.combinations(sg.OUTPUTS, k):
            got = run_g1(d, H, W, B, shared, want)
            assert all(torch.equal(bits(got[name]), bits(full[name])) for name in want), want
    with pytest.raises(_hip.DeqsciHipError):
        _hip.gap_update_grad(d["z"], d["Phi"], d["g"], d["y"], d["s"], need=(False,) * 4)


@pytest.mark.parametrize("B,H,W,kernel,mask,shared", CASES, ids=IDS)
def test_sci_mask_grad_and_phi_sum_grad(B, H, W, kernel, mask, shared):
    P, nm = H * W, 1 if shared else BSZ
    for op in ("mask_grad", "phi_sum_grad"):
        assert sg.path_of(op, HWB, B, P, sg.traffic_bytes(op, BSZ, nm, P, B)) == (kernel, "default")
    Phi, z, g, y, s, a, gs_in = data(H, W, B, mask, shared)
    da, dv = dev(a, H, W), dev(g, H, W)
    for _ in range(2):                                                                                          # (d)
        out, buf = guarded((nm, H, W, B))
        _hip.sci_mask_grad(da, dv, (nm, H, W, B), out=out)
        got = logical(out)
        ex, bd = sg.ref_mask_grad(a, g, shared)
        assert intact(buf) and sg.ratio(got, ex, bd) <= 1                                                       # (a)
        assert torch.equal(bits(got), bits(sg.emu_mask_grad(a, g, shared)))                                     # (b)
        if not shared:
            assert torch.equal(got, ex.float())                                                                 # one product: exact
        out, buf = guarded((nm, H, W, B))
        _hip.phi_sum_grad(dev(Phi, H, W), dev(gs_in, H, W), out=out)
        got = logical(out)
        zero = Phi.double().sum(-1) == 0
        assert intact(buf) and zero.any() and (got[zero] == 0).all()
        assert torch.equal(bits(got), bits(sg.ref_phi_sum_grad(Phi, gs_in))) and torch.equal(bits(got), bits(sg.emu_phi_sum_grad(Phi, gs_in, kernel)))
    # the cut is where the forward kernel wrote 1, and nowhere else
    assert (logical(_hip.phi_sum(dev(Phi, H, W), HWB))[zero] == 1).all() and (got[~zero] != 0).all()


def test_refusals_launch_nothing():
    """The planar layout and a batch beyond gridDim.y: DEQSCI_ERR_UNSUPPORTED (-4), and the outputs keep their NaN."""
    lib = _hip.load()
    H, W, B = 6, 6, 8
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t = torch.randn(BSZ, H, W, B, device=DEV)
    y = torch.randn(BSZ, H, W, device=DEV)
    out, buf = guarded((BSZ, H, W, B))
    for bsz, layout in ((BSZ, 1), (so.MAX_BSZ + 1, HWB)):
        assert lib.deqsci_gap_update_grad_f32(p(t), p(t), p(t), p(y), p(y), p(out), None, None, None, bsz, H, W, B, layout, 0, None) == so.ERR_UNSUPPORTED
        assert lib.deqsci_sci_mask_grad_f32(p(y), p(t), p(out), bsz, H, W, B, layout, 0, None) == so.ERR_UNSUPPORTED
        assert lib.deqsci_phi_sum_grad_f32(p(t), p(y), p(out), bsz, H, W, B, layout, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_gap_update_grad_f32(p(t), p(t), p(t), p(y), p(y), None, None, None, None, BSZ, H, W, B, HWB, 0, None) == -1
    torch.cuda.synchronize()
    assert intact(buf) and torch.isnan(out).all()


def test_streaming_gap_update_grad():
    """(e) 8 x 256 x 256 x 8 per sample, the mask outputs alone: (16B + 12) = 140 bytes per pixel, 73.4 MB, over STREAM_MIN_BYTES - the
    non-temporal path; one measurement fewer is under it.  The float64 reference is formed on the device, the fp32 emulation on the CPU."""
    bsz, H, W, B = 8, 256, 256, 8
    P = H * W
    nbytes = sg.traffic_bytes("gap_grad", bsz, bsz, P, B)
    assert sg.traffic_bytes("gap_grad", bsz - 1, bsz - 1, P, B) < so.STREAM_MIN_BYTES <= nbytes
    assert sg.path_of("gap_grad", HWB, B, P, nbytes) == ("hwb2", "streaming")
    gen = torch.Generator(device=DEV).manual_seed(11)
    Phi = so.uniform_mask(bsz, P, B, gen, DEV)
    z = torch.randn(bsz, P, B, device=DEV, generator=gen)
    g = torch.randn(bsz, P, B, device=DEV, generator=gen)
    y = torch.rand(bsz, P, device=DEV, generator=gen) * (B / 4)
    s = so.emu_phi_sum(Phi, "generic")
    d = {"Phi": Phi.view(bsz, H, W, B), "z": z.view(bsz, H, W, B), "g": g.view(bsz, H, W, B), "y": y.view(bsz, H, W), "s": s.view(bsz, H, W)}
    got = run_g1(d, H, W, B, False, ("gphi", "gs"), bsz=bsz)
    ref = sg.ref_gap_grad(z, Phi, g, y, s)
    emu = sg.emu_gap_grad(z.cpu(), Phi.cpu(), g.cpu(), y.cpu(), s.cpu(), "hwb2")
    for k in ("gphi", "gs"):
        flat = got[k].reshape(ref[k][0].shape)
        r = sg.ratio(flat, *ref[k])
        print(f"ROW | gap_grad {k} B={B} {bsz}x{H}x{W} | hwb2 streaming | err/bound {r:.3f} |")
        assert r <= 1, (k, r)
        assert torch.equal(bits(flat.cpu()), bits(emu[k])), k
