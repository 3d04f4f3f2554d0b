"""GPU: every kernel and instantiation of csrc/sci_ops.hip (sci_forward, sci_adjoint, phi_sum, gap_update, transpose, residual_out) against
tests/sci_ops_ref.py, at the smallest shapes where each path can still go wrong (TB = 256 threads, UNR = 4 float4 per lane, TP = 256 pixels
per tile).  Every case asserts the path it believes it is on (sci_ops_ref.path_of) and then holds the kernel to
  (a) the float64 reference within the derived running-error bound (no atol; the adjoint, the transposes and the subtraction are exact),
  (b) the fp32 emulation of that path's order of operations, bit for bit (what -ffp-contract=off and dot4_seq promise),
  (c) for the GAP step under a binary mask: Phi z1 = y where the mask's sum is not 0, within sum_b |Phi_b| bound_b.
bsz = 3 (blockIdx.y offsets), Phi shared and per sample, a uniform(0, 1) mask with all-zero pixels and pixels whose entries cancel to
exactly 0 and the binary mask of make_case.  Every output is pre-filled with NaN (an unwritten element shows) and is a 16-byte-aligned
slice of a larger buffer whose sentinels before and behind it are compared afterwards (a store past either end shows).
profiles/sci_ops_tests.md has the table of cases, paths, bounds and measured err / bound."""
import ctypes
import functools

import pytest
import torch

import sci_ops_ref as so
from sci_ops_ref import BHW, HWB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip
    from test_gpu_parity import make_case

DEV = "cuda"
BSZ = 3
NAN = float("nan")
SENTINEL = -7777.0
GUARD = 64                                                     # floats on either side of an output: 256 bytes, so the slice stays 16-byte aligned
LAY = {HWB: "HWB", BHW: "BHW"}


def guarded(shape, fill=NAN):
    """(view, buffer): a contiguous fp32 view of `shape`, filled with `fill`, inside a buffer of sentinels."""
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
    body = buf[GUARD:GUARD + numel]
    body.fill_(fill)
    assert body.data_ptr() % 16 == 0
    return body.view(shape), buf


def guarded_copy(t):
    v, buf = guarded(tuple(t.shape))
    v.copy_(t)
    return v, buf


def intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def shape_of(layout, H, W, B, n=BSZ):
    return (n, H, W, B) if layout == HWB else (n, B, H, W)


def path(op, li, lo, B, P, n=BSZ):
    return so.path_of(op, li, lo, B, P, so.traffic_bytes(op, n, P, B))


def row(case, kernel, policy, bound, r):
    print(f"ROW | {case} | {kernel} | {policy} | {bound} | {r} |")


@functools.lru_cache(maxsize=None)
def data(H, W, B, mask, shared):
    """Logical CPU tensors of one case: Phi (nb, P, B), z (BSZ, P, B), y (BSZ, P), s = Phi_sum (nb, P) as a left-to-right fp32 sum with
    0 -> 1 (an INPUT of the GAP step: the same for every path).  Computed once per case and never written to."""
    P, nb = H * W, 1 if shared else BSZ
    if mask == "binary":
        Phi, _, _, z, y, _ = make_case(BSZ, H, W, B, seed=B * H + W, shared=shared)
        Phi, z, y = Phi.reshape(nb, P, B).contiguous(), z.reshape(BSZ, P, B).contiguous(), y.reshape(BSZ, P).contiguous()
        assert (Phi.sum(-1) == 0).any()
    else:
        gen = torch.Generator().manual_seed(31 * B + 7 * H + W)
        Phi = so.uniform_mask(nb, P, B, gen)
        z = torch.randn(BSZ, P, B, generator=gen)
        y = torch.rand(BSZ, P, generator=gen) * (B / 4)
        assert int((Phi.double().sum(-1) == 0).sum()) == 5 * nb and (Phi[:, 2] != 0).any()
    return Phi, z, y, so.emu_phi_sum(Phi, "generic")


def phi_sum_guarded(dPhi, layout, H, W, B):
    """deqsci_phi_sum_f32 into a NaN-filled output between sentinels; the sentinels are checked here."""
    nb = dPhi.shape[0]
    out, buf = guarded((nb, H, W))
    code = _hip.load().deqsci_phi_sum_f32(ctypes.c_void_p(dPhi.data_ptr()), ctypes.c_void_p(out.data_ptr()), nb, H, W, B, layout,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, code
    assert intact(buf)
    return out


def dev(t, layout, H, W):
    """logical CPU tensor -> device tensor in `layout` ((n, P) tensors: (n, H, W))."""
    if t.dim() == 2:
        return t.reshape(t.shape[0], H, W).to(DEV)
    return so.to_layout(t, layout, H, W).to(DEV)


def logical(t, layout):
    return so.from_layout(t, layout).cpu() if t.dim() == 4 else t.reshape(t.shape[0], -1).cpu()


# ----------------------------------------------------------------------------- forward, adjoint, phi_sum
FAP_CASES = ([(HWB, B, H, W, f"hwb{B // 4}") for B in (4, 8, 16, 32) for (H, W) in ((5, 7), (33, 31), (32, 32))] +      # one block with clamped tail lanes (Q % 64 != 0); several blocks, ragged last; no tail
             [(BHW, B, H, W, "bhw") for B in (5, 8, 19, 32) for (H, W) in ((6, 6), (36, 30))] +                        # the unroll-8 frame loop and its remainders; one block with idle lanes, two blocks
             [(HWB, 5, 5, 7, "generic"), (BHW, 5, 5, 7, "generic"), (BHW, 8, 5, 7, "generic"),                        # any B; a fast B at P % 4 != 0
              (HWB, 12, 17, 23, "generic"), (BHW, 12, 17, 23, "generic")])                                            # two blocks


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("mask", ["uniform", "binary"])
@pytest.mark.parametrize("layout,B,H,W,kernel", FAP_CASES, ids=[f"{LAY[c[0]]}-B{c[1]}-{c[2]}x{c[3]}" for c in FAP_CASES])
def test_forward_adjoint_phi_sum(layout, B, H, W, kernel, mask, shared):
    P = H * W
    for op in ("forward", "adjoint", "phi_sum"):
        assert path(op, layout, layout, B, P) == (kernel, "default")
    if kernel.startswith("hwb"):
        assert (so.blocks_of(kernel, B, P) > 1) == (P * (B // 4) > 1024) and ((P * (B // 4)) % 1024 != 0) == (P != 1024)
    Phi, z, y, _ = data(H, W, B, mask, shared)
    dPhi, dz, dy = dev(Phi, layout, H, W), dev(z, layout, H, W), dev(y, layout, H, W)
    # forward
    out, buf = guarded((BSZ, H, W))
    _hip.sci_forward(dz, dPhi, layout, out=out)
    ex, bd = so.ref_forward(z, Phi)
    got = logical(out, layout)
    r_f = so.ratio(got, ex, bd)
    assert intact(buf) and r_f <= 1, r_f
    assert torch.equal(got, so.emu_forward(z, Phi, kernel))
    # adjoint
    out, buf = guarded(shape_of(layout, H, W, B))
    _hip.sci_adjoint(dy, dPhi, layout, out=out)
    got = logical(out, layout)
    assert intact(buf) and torch.isfinite(got).all()
    assert torch.equal(got, so.ref_adjoint(y, Phi).expand(BSZ, P, B)) and torch.equal(got, so.emu_adjoint(y, Phi).expand(BSZ, P, B))
    # phi_sum (through the C ABI: the wrapper allocates its own output, which could not stand between sentinels)
    got = logical(phi_sum_guarded(dPhi, layout, H, W, B), layout)
    ex, bd, zero = so.ref_phi_sum(Phi)
    assert zero.any() and (got[zero] == 1).all()
    r_s = so.ratio(got, ex, bd)
    assert r_s <= 1, r_s
    assert torch.equal(got, so.emu_phi_sum(Phi, kernel))
    row(f"forward {LAY[layout]} B={B} {H}x{W} {mask} shared={shared}", kernel, "default", "B u sum|x Phi|", f"{r_f:.3f}")
    row(f"phi_sum {LAY[layout]} B={B} {H}x{W} {mask} shared={shared}", kernel, "default", "(B-1) u sum|Phi|", f"{r_s:.3f}")


# ----------------------------------------------------------------------------- GAP step
GAP_CASES = ([(HWB, HWB, B, H, W, f"hwb{B // 4}") for B in (4, 8, 16, 32) for (H, W) in ((5, 7), (33, 31), (32, 32))] +
             [(BHW, BHW, B, H, W, f"bhw{B}") for B in (4, 8, 16) for (H, W) in ((6, 6), (36, 30))] +
             [(BHW, BHW, 32, 6, 6, "generic"), (BHW, BHW, 5, 6, 6, "generic")] +                                      # planar B the register kernel is not built for
             [(HWB, BHW, B, H, W, f"hwb2bhw{B // 4}") for B in (4, 8, 16, 32) for (H, W) in ((6, 6), (10, 26), (36, 30))] +   # 10 x 26: the second tile holds 4 pixels, the clamp is p = P - 1
             [(li, lo, 8, 5, 7, "generic") for (li, lo) in ((BHW, BHW), (HWB, BHW), (BHW, HWB))] +                    # a fast B at P % 4 != 0
             [(li, lo, B, H, W, "generic") for (B, H, W) in ((5, 5, 7), (12, 17, 23)) for li in (HWB, BHW) for lo in (HWB, BHW)] +
             [(BHW, HWB, 8, 6, 6, "generic")])                                                                        # planar -> HWB is served by nothing else


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("mask", ["uniform", "binary"])
@pytest.mark.parametrize("li,lo,B,H,W,kernel", GAP_CASES, ids=[f"{LAY[c[0]]}to{LAY[c[1]]}-B{c[2]}-{c[3]}x{c[4]}" for c in GAP_CASES])
def test_gap_update(li, lo, B, H, W, kernel, mask, shared):
    """(a), (b), (c); and where the layouts agree, the step in place (out = z) is bit-equal to the step out of place."""
    P = H * W
    assert path("gap", li, lo, B, P) == (kernel, "default")
    if kernel.startswith("hwb2bhw"):
        assert so.blocks_of(kernel, B, P) == -(-P // 256) and (P % 256 != 0)
    Phi, z, y, s = data(H, W, B, mask, shared)
    dPhi, dz, dy, ds = dev(Phi, li, H, W), dev(z, li, H, W), dev(y, li, H, W), dev(s, li, H, W)
    out, buf = guarded(shape_of(lo, H, W, B))
    _hip.gap_update(dz, dPhi, dy, ds, li, lo, out=out)
    got = logical(out, lo)
    ex, bd = so.ref_gap(z, Phi, y, s)
    r = so.ratio(got, ex, bd)
    assert intact(buf) and r <= 1, r
    assert torch.equal(got, so.emu_gap(z, Phi, y, s, kernel))
    if mask == "binary":
        live = (Phi.sum(-1) != 0).expand(BSZ, P)
        miss = ((Phi.double() * got.double()).sum(-1) - y.double()).abs()
        lim = so.gap_miss_bound(Phi, bd)
        assert live.any() and (miss[live] <= lim[live]).all(), float((miss[live] / lim[live]).max())
    if li == lo:
        zz, zbuf = guarded_copy(dz)
        _hip.gap_update(zz, dPhi, dy, ds, li, lo, out=zz)
        assert intact(zbuf) and torch.equal(bits(zz), bits(out))
    row(f"gap {LAY[li]}->{LAY[lo]} B={B} {H}x{W} {mask} shared={shared}", kernel, "default", "GAP", f"{r:.3f}")


# ----------------------------------------------------------------------------- transpose
TR_CASES = ([(B, H, W, "transpose_fast") for B in (4, 8, 16, 32) for (H, W) in ((6, 6), (10, 26), (36, 30))] +
            [(8, 5, 7, "transpose_generic(8224)"), (12, 17, 23, "transpose_generic(12336)"),
             (63, 17, 23, "transpose_generic(64764)"),        # the last size inside the 64 KiB a kernel gets without asking
             (64, 17, 23, "transpose_generic(65792)"),        # the first size over it (257 floats per frame): the opt-in branch
             (65, 17, 23, "transpose_generic(66820)"),
             (159, 17, 23, "transpose_generic(163452)")])     # the last size inside the 160 KiB of a workgroup


@pytest.mark.parametrize("B,H,W,kernel", TR_CASES, ids=[f"B{c[0]}-{c[1]}x{c[2]}" for c in TR_CASES])
def test_transpose_both_ways_is_a_permutation(B, H, W, kernel):
    P = H * W
    assert path("transpose", HWB, BHW, B, P) == path("transpose", BHW, HWB, B, P) == (kernel, "default")
    x = torch.randn(BSZ, H, W, B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(B + P))
    want = x.permute(0, 3, 1, 2).contiguous()
    planar, buf = guarded((BSZ, B, H, W))
    _hip.transpose(x, BHW, out=planar)
    assert intact(buf) and torch.equal(bits(planar), bits(want))
    back, buf = guarded((BSZ, H, W, B))
    _hip.transpose(planar, HWB, out=back)
    assert intact(buf) and torch.equal(bits(back), bits(x))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_transpose_refuses_what_no_workgroup_can_hold():
    """B = 160: 160 x 257 floats are more than the 160 KiB of LDS - DEQSCI_ERR_UNSUPPORTED, and nothing is launched."""
    lib = _hip.load()
    H, W, B = 17, 23, 160
    assert path("transpose", HWB, BHW, B, H * W) == ("unsupported", "default")
    x = torch.randn(BSZ, H, W, B, device=DEV)
    for to in (BHW, HWB):
        out, buf = guarded((BSZ, H * W * B))
        assert lib.deqsci_transpose_f32(_p(x), _p(out), BSZ, H, W, B, to, None) == so.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert intact(buf) and torch.isnan(out).all()


# ----------------------------------------------------------------------------- residual_out
@pytest.mark.parametrize("shape,lo,kernel", [((1, 1, 1, 3), BHW, "sub_flat"),            # n4 = 0: lane 0 does everything
                                             ((2, 5, 7, 5), BHW, "sub_flat"),            # 350 elements: 87 float4 and a tail of 2
                                             ((3, 6, 6, 8), BHW, "sub_flat"),            # a multiple of 4
                                             ((3, 6, 6, 8), HWB, "bhw2hwb2"), ((3, 10, 26, 4), HWB, "bhw2hwb1"), ((3, 36, 30, 32), HWB, "bhw2hwb8"),
                                             ((2, 5, 7, 5), HWB, "unsupported"), ((3, 5, 7, 8), HWB, "unsupported")])     # the wrapper's fallback: sub_flat + transpose
def test_residual_out(shape, lo, kernel):
    n, H, W, B = shape
    assert path("residual_out", BHW, lo, B, H * W, n) == (kernel, "default")
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    z1 = torch.randn(n, B, H, W, device=DEV, generator=gen)
    noise = torch.randn(n, B, H, W, device=DEV, generator=gen)
    want = z1 - noise
    if lo == HWB:
        want = want.permute(0, 2, 3, 1).contiguous()
    out, buf = guarded(tuple(want.shape))
    _hip.residual_out(z1, noise, lo, out=out)
    assert intact(buf) and torch.equal(bits(out), bits(want))
    if lo == BHW:                                              # in place: every element is read and written by the same lane
        zz, zbuf = guarded_copy(z1)
        _hip.residual_out(zz, noise, BHW, out=zz)
        assert intact(zbuf) and torch.equal(bits(zz), bits(want))


def test_refusals_launch_nothing():
    """Aliasing the kernels cannot serve and a batch beyond gridDim.y return DEQSCI_ERR_UNSUPPORTED (-4); the outputs keep their NaN."""
    lib = _hip.load()
    H, W, B = 6, 6, 8
    t = torch.randn(BSZ, H, W, B, device=DEV)
    y = torch.randn(BSZ, H, W, device=DEV)
    s = torch.ones(BSZ, H, W, device=DEV)
    keep = t.clone()
    for li, lo in ((HWB, BHW), (BHW, HWB)):
        assert lib.deqsci_gap_update_f32(_p(t), _p(t), _p(y), _p(s), _p(t), BSZ, H, W, B, li, lo, 0, None) == so.ERR_UNSUPPORTED
    for to in (HWB, BHW):
        assert lib.deqsci_transpose_f32(_p(t), _p(t), BSZ, H, W, B, to, None) == so.ERR_UNSUPPORTED
    other = torch.randn_like(t)
    assert lib.deqsci_residual_out_f32(_p(t), _p(other), _p(t), BSZ, H, W, B, HWB, None) == so.ERR_UNSUPPORTED          # out == z1 on the HWB path
    assert lib.deqsci_residual_out_f32(_p(other), _p(t), _p(t), BSZ, H, W, B, HWB, None) == so.ERR_UNSUPPORTED          # out == noise
    big = so.MAX_BSZ + 1                                       # small real buffers: nothing may be launched
    out, buf = guarded((BSZ, H * W * B))
    assert lib.deqsci_sci_forward_f32(_p(t), _p(t), _p(out), big, H, W, B, HWB, 0, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_sci_adjoint_f32(_p(y), _p(t), _p(out), big, H, W, B, HWB, 0, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_phi_sum_f32(_p(t), _p(out), big, H, W, B, HWB, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_gap_update_f32(_p(t), _p(t), _p(y), _p(s), _p(out), big, H, W, B, HWB, HWB, 0, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_transpose_f32(_p(t), _p(out), big, H, W, B, BHW, None) == so.ERR_UNSUPPORTED
    assert lib.deqsci_residual_out_f32(_p(t), _p(other), _p(out), big, H, W, B, BHW, None) == so.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert intact(buf) and torch.isnan(out).all() and torch.equal(t, keep)


# ----------------------------------------------------------------------------- the streaming policy
def _stream_case(op, bsz, H, W, B):
    """Just over the 64 MiB of that launcher's own formula, and one measurement fewer is under it."""
    P = H * W
    nbytes = so.traffic_bytes(op, bsz, P, B)
    assert so.traffic_bytes(op, bsz - 1, P, B) < so.STREAM_MIN_BYTES <= nbytes < 1.01 * so.STREAM_MIN_BYTES
    return P, nbytes


def _dev_data(bsz, P, B, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    Phi = so.uniform_mask(bsz, P, B, gen, DEV)
    z = torch.randn(bsz, P, B, device=DEV, generator=gen)
    y = torch.rand(bsz, P, device=DEV, generator=gen) * (B / 4)
    return Phi, z, y


@pytest.mark.parametrize("layout,kernel", [(HWB, "hwb2"), (BHW, "bhw")])
def test_streaming_forward_and_adjoint(layout, kernel):
    """bsz = 4, 508 x 488, B = 8: 67.4 MB by the (8B + 4) formula; P % 4 == 0, so the planar kernel streams too; Q % 1024 = 192.
    The float64 reference is formed on the device, the fp32 emulation on the CPU (IEEE division and no contraction are certain there)."""
    bsz, H, W, B = 4, 508, 488, 8
    P, nbytes = _stream_case("forward", bsz, H, W, B)
    assert (P * 2) % 1024 == 192 and P % 4 == 0
    for op in ("forward", "adjoint"):
        assert so.path_of(op, layout, layout, B, P, nbytes) == (kernel, "streaming")
    Phi, z, y = _dev_data(bsz, P, B, 1)
    dPhi, dz = so.to_layout(Phi, layout, H, W), so.to_layout(z, layout, H, W)
    out, buf = guarded((bsz, H, W))
    _hip.sci_forward(dz, dPhi, layout, out=out)
    ex, bd = so.ref_forward(z, Phi)
    r = so.ratio(out.view(bsz, P), ex, bd)
    assert intact(buf) and r <= 1, r
    assert torch.equal(out.view(bsz, P).cpu(), so.emu_forward(z.cpu(), Phi.cpu(), kernel))
    del ex, bd
    out, buf = guarded(shape_of(layout, H, W, B, bsz))
    _hip.sci_adjoint(y.view(bsz, H, W), dPhi, layout, out=out)
    assert intact(buf) and torch.equal(so.from_layout(out, layout), so.ref_adjoint(y, Phi))
    row(f"forward {LAY[layout]} B={B} {bsz}x{H}x{W}", kernel, "streaming", "B u sum|x Phi|", f"{r:.3f}")


@pytest.mark.parametrize("layout,kernel", [(HWB, "hwb4"), (BHW, "bhw")])
def test_streaming_phi_sum(layout, kernel):
    """nb = 4, 508 x 488, B = 16: (4B + 4) = 68 bytes per pixel, the same 67.4 MB; Q % 1024 = 384."""
    nb, H, W, B = 4, 508, 488, 16
    P, nbytes = _stream_case("phi_sum", nb, H, W, B)
    assert (P * 4) % 1024 == 384
    assert so.path_of("phi_sum", layout, layout, B, P, nbytes) == (kernel, "streaming")
    Phi = so.uniform_mask(nb, P, B, torch.Generator(device=DEV).manual_seed(2), DEV)
    got = phi_sum_guarded(so.to_layout(Phi, layout, H, W), layout, H, W, B).view(nb, P)
    ex, bd, zero = so.ref_phi_sum(Phi)
    r = so.ratio(got, ex, bd)
    assert r <= 1 and zero.any() and (got[zero] == 1).all(), r
    assert torch.equal(got.cpu(), so.emu_phi_sum(Phi.cpu(), kernel))
    row(f"phi_sum {LAY[layout]} B={B} {nb}x{H}x{W}", kernel, "streaming", "(B-1) u sum|Phi|", f"{r:.3f}")


@pytest.mark.parametrize("li,lo,kernel", [(HWB, HWB, "hwb2"), (BHW, BHW, "bhw8"), (HWB, BHW, "hwb2bhw2")])
def test_streaming_gap(li, lo, kernel):
    """bsz = 3, 508 x 424, B = 8: (12B + 8) = 104 bytes per pixel, 67.2 MB; Q % 1024 = 704, P % 256 = 96 (a ragged last tile)."""
    bsz, H, W, B = 3, 508, 424, 8
    P, nbytes = _stream_case("gap", bsz, H, W, B)
    assert (P * 2) % 1024 == 704 and P % 256 == 96 and P % 4 == 0
    assert so.path_of("gap", li, lo, B, P, nbytes) == (kernel, "streaming")
    Phi, z, y = _dev_data(bsz, P, B, 3)
    s = so.emu_phi_sum(Phi, "generic")
    out, buf = guarded(shape_of(lo, H, W, B, bsz))
    _hip.gap_update(so.to_layout(z, li, H, W), so.to_layout(Phi, li, H, W), y.view(bsz, H, W), s.view(bsz, H, W), li, lo, out=out)
    got = so.from_layout(out, lo)
    ex, bd = so.ref_gap(z, Phi, y, s)
    r = so.ratio(got, ex, bd)
    assert intact(buf) and r <= 1, r
    assert torch.equal(got.cpu(), so.emu_gap(z.cpu(), Phi.cpu(), y.cpu(), s.cpu(), kernel))
    row(f"gap {LAY[li]}->{LAY[lo]} B={B} {bsz}x{H}x{W}", kernel, "streaming", "GAP", f"{r:.3f}")


def test_streaming_transpose():
    """bsz = 4, 508 x 520, B = 8: 8B = 64 bytes per pixel, 67.6 MB; P % 256 = 224."""
    bsz, H, W, B = 4, 508, 520, 8
    P, nbytes = _stream_case("transpose", bsz, H, W, B)
    assert P % 256 == 224
    assert so.path_of("transpose", HWB, BHW, B, P, nbytes) == so.path_of("transpose", BHW, HWB, B, P, nbytes) == ("transpose_fast", "streaming")
    x = torch.randn(bsz, H, W, B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    planar, buf = guarded((bsz, B, H, W))
    _hip.transpose(x, BHW, out=planar)
    assert intact(buf) and torch.equal(bits(planar), bits(x.permute(0, 3, 1, 2).contiguous()))
    back, buf = guarded((bsz, H, W, B))
    _hip.transpose(planar, HWB, out=back)
    assert intact(buf) and torch.equal(bits(back), bits(x))


@pytest.mark.parametrize("shape,lo,kernel", [((3, 611, 611, 5), BHW, "sub_flat"),        # 12B = 60 bytes per pixel, 67.2 MB; 5 599 815 elements: a tail of 3
                                             ((3, 508, 460, 8), HWB, "bhw2hwb2")])       # 96 bytes per pixel, 67.3 MB; P % 256 = 208
def test_streaming_residual_out(shape, lo, kernel):
    bsz, H, W, B = shape
    P, nbytes = _stream_case("residual_out", bsz, H, W, B)
    assert so.path_of("residual_out", BHW, lo, B, P, nbytes) == (kernel, "streaming")
    assert (bsz * P * B) % 4 == 3 if lo == BHW else P % 256 == 208
    gen = torch.Generator(device=DEV).manual_seed(5)
    z1 = torch.randn(bsz, B, H, W, device=DEV, generator=gen)
    noise = torch.randn(bsz, B, H, W, device=DEV, generator=gen)
    want = z1 - noise
    if lo == HWB:
        want = want.permute(0, 2, 3, 1).contiguous()
    out, buf = guarded(tuple(want.shape))
    _hip.residual_out(z1, noise, lo, out=out)
    assert intact(buf) and torch.equal(bits(out), bits(want))


# ----------------------------------------------------------------------------- NaN and Inf
@pytest.mark.parametrize("li,lo,B,kernel,fwd", [(HWB, HWB, 32, "hwb8", "hwb8"),          # LP = 8: three butterfly levels, nine blocks of 1024 quads
                                                (BHW, BHW, 8, "bhw8", "bhw"),            # the planar register kernels: two blocks of 1024 pixels
                                                (HWB, BHW, 32, "hwb2bhw8", None),        # the fused transpose: five tiles, the last of 56 pixels
                                                (HWB, HWB, 12, "generic", "generic")])   # five blocks of 256 pixels
def test_nonfinite_inputs_stay_in_their_pixel(li, lo, B, kernel, fwd):
    """One element of z, y or Phi of measurement 1 set to NaN, +Inf or -Inf, at sci_ops_ref.poison_pixels (first and last pixel, both
    sides of the block and tile seams), 36 x 30, a uniform mask per sample:
      P1  the output is non-finite exactly where IEEE arithmetic on the float64 reference is (y[n, p]; all B frames of (n, p) for the GAP step),
      P2  every other element has the bits of the clean launch,
      P3  a second launch gives the same bits.
    The HWB kernels clamp their tail lanes onto the last quad and combine lanes by shuffles: a leak would show at the last pixel or at a seam."""
    H, W, n = 36, 30, 1
    P = H * W
    assert path("gap", li, lo, B, P) == (kernel, "default")
    assert fwd is None or path("forward", li, li, B, P) == (fwd, "default")
    Phi, z, y, s = (t.to(DEV) for t in data(H, W, B, "uniform", False))
    run_g = lambda zz, pp, yy: so.from_layout(_hip.gap_update(so.to_layout(zz, li, H, W), so.to_layout(pp, li, H, W), yy.view(BSZ, H, W), s.view(BSZ, H, W), li, lo), lo)
    run_f = lambda zz, pp: _hip.sci_forward(so.to_layout(zz, li, H, W), so.to_layout(pp, li, H, W), li).view(BSZ, P)
    clean_g = run_g(z, Phi, y)
    clean_f = run_f(z, Phi) if fwd else None
    assert torch.isfinite(clean_g).all()
    bad = []
    for p in so.poison_pixels(P):
        b = so.poison_frame(p, B)
        for name, val in so.POISONS.items():
            for which in ("z", "y", "Phi"):
                zz, yy, pp = z.clone(), y.clone(), Phi.clone()
                if which == "y":
                    yy[n, p] = val
                else:
                    (zz if which == "z" else pp)[n, p, b] = val
                tag = (which, p, name)
                hit = so.nonfinite_gap(zz, pp, yy, s)
                assert int(hit.sum()) == B and hit[n, p].all()
                got = run_g(zz, pp, yy)
                if not torch.equal(~torch.isfinite(got), hit):
                    bad.append(("P1 gap",) + tag)
                if not torch.equal(bits(got)[~hit], bits(clean_g)[~hit]):
                    bad.append(("P2 gap",) + tag)
                if not torch.equal(bits(run_g(zz, pp, yy)), bits(got)):
                    bad.append(("P3 gap",) + tag)
                if fwd and which != "y":
                    hit = so.nonfinite_forward(zz, pp)
                    assert int(hit.sum()) == 1 and hit[n, p]
                    got = run_f(zz, pp)
                    if not torch.equal(~torch.isfinite(got), hit):
                        bad.append(("P1 forward",) + tag)
                    if not torch.equal(bits(got)[~hit], bits(clean_f)[~hit]):
                        bad.append(("P2 forward",) + tag)
                    if not torch.equal(bits(run_f(zz, pp)), bits(got)):
                        bad.append(("P3 forward",) + tag)
    assert not bad, bad


@pytest.mark.parametrize("layout,B,kernel", [(HWB, 32, "hwb8"), (BHW, 8, "bhw"), (HWB, 12, "generic")])
def test_phi_sum_keeps_a_nan(layout, B, kernel):
    """Only a sum that compares equal to 0 becomes 1: a NaN in the mask stays a NaN in its pixel's sum, and only there."""
    H, W, n = 36, 30, 1
    P = H * W
    assert path("phi_sum", layout, layout, B, P) == (kernel, "default")
    Phi = data(H, W, B, "uniform", False)[0].to(DEV)
    clean = phi_sum_guarded(so.to_layout(Phi, layout, H, W), layout, H, W, B).view(BSZ, P)
    for p in so.poison_pixels(P):
        pp = Phi.clone()
        pp[n, p, so.poison_frame(p, B)] = NAN
        got = phi_sum_guarded(so.to_layout(pp, layout, H, W), layout, H, W, B).view(BSZ, P)
        hit = torch.zeros(BSZ, P, dtype=torch.bool, device=DEV)
        hit[n, p] = True
        assert torch.equal(torch.isnan(got), hit) and torch.equal(bits(got)[~hit], bits(clean)[~hit]), p
