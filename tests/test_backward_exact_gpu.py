"""The masked kernels that every implicit backward, every mask and weight gradient and every Jacobian product runs through, and the
glue that transposes their weights, against float64 element by element: the framework of tests/test_denoiser_exact_gpu.py (hold(), Arena,
the data generators; statement, data, constants: tests/denoiser_exact_ref.py; the helper itself: tests/test_denoiser_exact_host.py;
measured ratios: profiles/denoiser_exact.md).

1. Each masked entry point - conv3x3_c64_winograd_masked, conv3x3_c1_to_64_masked, ffdnet_head_masked in its 16 x 16 and its 32 x 32
   form - with a drawn weight and with vjp._transposed of one (what the backward launches), under a random and a checker mask drawn
   and packed on the CPU (nonfinite_ref.pack_mask: no kernel sits between the data and the kernel under test):
     mode "int"   (a) torch.equal with the float64 select on integer data;
     mode "real"  (b) |got - ref64| <= c 2^-24 S mask per element: an element under a cleared bit must equal 0;
   both under (c), the mask words inside guard words that are all ones in the first launch and all zeros in the second.
2. The packs vjp._MaskedStack builds (head_f / head_t, mid_f / mid_t, tail_f / tail_t, plain and FFDNet edges): the adjoint identity
   <A u, g> == <u, A^T g> of every pair, exactly, on integer data.
3. One whole three-layer masked stack, jvp and vjp, plain and FFDNet: torch.equal with vjp.masked_jvp / masked_vjp in float64 under the
   device's own masks."""
import functools

import pytest
import torch

import denoiser_exact_ref as dx
import nonfinite_ref as nf
from test_denoiser_exact_gpu import DEV, MODES, hold, many_tiles, periodic

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip, vjp

BOOL = (False, True)


# ----------------------------------------------------------------------------- 1. the three masked kernels
def masked_case(kernel, shape, data_shape, transposed, form, mode, pack, entry, channels_last_in=False):
    """One case of a masked kernel.  shape: the launch's (n, H, W); data_shape: the shape the data is drawn at (the same, but for a launch
    that repeats dx.PERIOD distinct images, whose n the device's CU count may raise)."""
    n, H, W = shape
    x, w = dx.masked_operands(kernel, data_shape, mode, transposed)
    mb = dx.masked_bits(kernel, data_shape, form)
    ref = periodic(dx.masked_ref(kernel, data_shape, mode, transposed, form), n)
    xg = periodic(x, n).to(DEV)
    xg = dx.cl(xg) if channels_last_in else xg
    Wg = pack(w.to(DEV))
    words = periodic(nf.pack_mask(mb), n).contiguous().to(DEV)
    fills = dx.mask_guard_fills()

    def launch():
        a = dx.Arena(W, DEV)
        out = a.output((n, 64, H, W), channels_last=True)
        entry(a.operand(xg), a.operand(Wg), a.words(words, next(fills)), out=out)
        return out, [], a

    def explain(got):
        unm = periodic(dx.masked_unmasked_ref(kernel, data_shape, mode, transposed), n)
        return dx.mask_fault(got, unm.to(DEV), periodic(mb, n).to(DEV))
    bound = periodic(dx.masked_bound(kernel, data_shape, transposed, form), n) if mode == "real" else None
    hold(kernel, f"{'transposed' if transposed else 'drawn'} w, {form} mask", shape, mode, launch, ref, bound, explain)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", dx.MASK_FORMS)
@pytest.mark.parametrize("transposed", BOOL)
@pytest.mark.parametrize("sname,shape", list(dx.shapes_of("f22_masked").items()))
def test_winograd_f22_masked(sname, shape, transposed, form, mode):
    """conv3x3_c64_winograd_masked, csrc/winograd.hip with MASK = 1: the body of conv3x3_c64_winograd without bias and ReLU, then per
    2 x 2 tile the words of its four pixels (m00 / m01 / m10 / m11, half wn of each).  EXACT on integer data with the weights MULTIPLES
    OF 4, drawn or transposed (a permutation of the same numbers): U = G w G^T is an integer, |U| <= 36, |V| <= 32, a partial sum of M at
    most 64 * 36 * 32 < 2^17, the output transform adds nine: < 2^21; the select keeps the value or writes 0.  c = 2 + 1 + 2*64 + 4 on
    S = the transforms' absolute-value propagation, times the mask."""
    many_tiles(shape, 16, 16)
    masked_case("f22_masked", shape, shape, transposed, form, mode, _hip.pack_winograd_weights, _hip.conv3x3_c64_winograd_masked, True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", dx.MASK_FORMS)
@pytest.mark.parametrize("transposed", BOOL)
def test_conv_c1_to_64_masked(transposed, form, mode):
    """conv3x3_c1_to_64_masked, csrc/ffdnet_edges.hip conv_c1_to_64_kernel<3>: a lane's four channels 4 cq .. 4 cq + 3 under bits
    4 (cq & 7) .. of half cq >> 3 of the pixel's word.  The drawn (64,1,3,3) weight, and vjp._transposed of a (1,64,3,3) last layer - the
    tail's transpose in the backward.  EXACT on integer data: nine fused multiply-adds of integers, |sum| <= 9 * 8 * 4.  c = 9."""
    (sname, shape), = dx.shapes_of("c1_to_64_masked").items()
    masked_case("c1_to_64_masked", shape, shape, transposed, form, mode, _hip.pack_c1_to_64_weights, _hip.conv3x3_c1_to_64_masked)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", dx.MASK_FORMS)
@pytest.mark.parametrize("transposed", BOOL)
@pytest.mark.parametrize("sname", list(dx.shapes_of("head_masked")))
def test_ffdnet_head_masked(sname, transposed, form, mode):
    """ffdnet_head_masked, csrc/jacobian.hip: ffdnet_head_masked_kernel<16> (small launches: two images of 18 x 19 positions, and one
    position = a 2 x 2 image) and <32> (from two 32 x 32 tiles per CU on: 128 x 33 x 35, four tiles per image, ragged in both
    directions - more images where the device has more than 256 CUs; five distinct images repeat).  Which form a launch takes is
    ASSERTED from the device's CU count: the 32 x 32 form is what FFDNet's Jacobian report and its device weight gradients run on a whole
    clip.  The drawn (64,4,3,3) weight (the first layer without sigma's channel) and vjp._transposed of a (4,64,3,3) last layer.  EXACT
    on integer data: 36 packed fused multiply-adds of integers, |sum| <= 36 * 8 * 4 = 1152.  c = 36."""
    data_shape = dx.shapes_of("head_masked")[sname]
    n, H, W = data_shape
    per_image, need = -(-H // 32) * -(-W // 32), 2 * torch.cuda.get_device_properties(0).multi_processor_count
    if sname == "head_masked_ragged":
        n = max(n, -(-need // per_image))
        assert per_image == 4 and n * per_image >= need             # deqsci_ffdnet_head_masked_f32 launches ffdnet_head_masked_kernel<32>
    else:
        assert n * per_image < need                                 # ... and here <16>
    masked_case("head_masked", (n, H, W), data_shape, transposed, form, mode, _hip.pack_head_masked_weights, _hip.ffdnet_head_masked)


# ----------------------------------------------------------------------------- 2. the transposes the backward builds
def ints(shape, seed, hi=8):
    return torch.randint(-hi, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float().to(DEV)


def dot(a, b):
    """<a, b> of two integer-valued fp32 tensors, exactly: float64 products and sums of integers (every factor < 2^24, at most 2^18
    terms: the sum stays below 2^53)."""
    assert a.shape == b.shape and float(a.abs().max()) < 2.0 ** 24 and float(b.abs().max()) < 2.0 ** 24
    return float((a.double() * b.double()).sum())


@functools.lru_cache(maxsize=None)
def integer_stack(ffdnet):
    """A vjp._MaskedStack of integer layers 1 -> 64 -> 64 -> 64 -> 1 (FFDNet: 5 -> ... -> 4): weights in [-4, 4] without 0, the two middle
    ones times 4 (denoiser_exact_ref.KERNELS["f22_masked"]["wmult"]), each drawn on its own.  Its packs are the production glue's; its
    own masks (of a forward pass at a rand image) are not used here: every identity takes a drawn one.  -> (stack, (n, H, W), mask words,
    the mask as 0 / 1 numbers, all-ones words)."""
    g = torch.Generator().manual_seed(7000 + int(ffdnet))
    n, H, W = nf.CASES["head_valu" if ffdnet else "f22"]["shape"]
    f = 2 if ffdnet else 1
    draw = lambda shape, m=1: dx._ints(shape, -4, 4, g, nonzero=True) * m
    layers = [(draw((64, 5 if ffdnet else 1, 3, 3)), None, True), (draw((64, 64, 3, 3), 4), None, True), (draw((64, 64, 3, 3), 4), None, True),
              (draw((4 if ffdnet else 1, 64, 3, 3)), None, False)]
    x = torch.rand((n, 1, f * H, f * W), generator=g).to(DEV)
    stack = vjp._MaskedStack(layers, x, torch.tensor([0.1], device=DEV) if ffdnet else None)
    mb = dx.mask_bits((n, H, W), "random")
    return (stack, (n, H, W), nf.pack_mask(mb).to(DEV), dx.cl(mb.float().to(DEV)),
            torch.full((n, H, W), -1, dtype=torch.int64, device=DEV))


def adjoint(lhs_a, lhs_b, rhs_a, rhs_b, what):
    lhs, rhs = dot(lhs_a, lhs_b), dot(rhs_a, rhs_b)
    print(f"ADJOINT | {what} | {lhs!r} | {rhs!r} |")
    assert lhs != 0, f"{what}: the identity is vacuous on this data"
    assert lhs == rhs, f"{what}: <A u, g> = {lhs!r} but <u, A^T g> = {rhs!r} (off by {rhs - lhs:g}): the transposed pack is not the transpose"


@pytest.mark.parametrize("ffdnet", BOOL)
def test_first_layer_pack_and_its_transpose(ffdnet):
    """<first_masked(u, head_f, m), g> == <u, last(m . g, head_t)>: the first layer linearised (jvp) against what ends the vjp - plain:
    conv3x3_c1_to_64_masked / conv3x3_c64_to_1, FFDNet: ffdnet_head_masked / ffdnet_tail.  |A u| <= 36 * 8 * 4, |A^T g| <= 576 * 8 * 4."""
    stack, (n, H, W), m, mf, _ = integer_stack(ffdnet)
    f = 2 if ffdnet else 1
    u, g = ints((n, 1, f * H, f * W), 1), dx.cl(ints((n, 64, H, W), 2))
    first = _hip.ffdnet_head_masked if ffdnet else _hip.conv3x3_c1_to_64_masked
    last = _hip.ffdnet_tail if ffdnet else _hip.conv3x3_c64_to_1
    adjoint(first(u, stack.head_f, m), g, u, last(dx.cl(mf * g), stack.head_t), f"head_f / head_t, {'FFDNet' if ffdnet else 'plain'} edges")


@pytest.mark.parametrize("ffdnet", BOOL)
def test_last_layer_pack_and_its_transpose(ffdnet):
    """<last(m . h, tail_f), v> == <h, first_masked(v, tail_t, m)>: the last layer (jvp) against what starts the vjp."""
    stack, (n, H, W), m, mf, _ = integer_stack(ffdnet)
    f = 2 if ffdnet else 1
    h, v = dx.cl(ints((n, 64, H, W), 3)), ints((n, 1, f * H, f * W), 4)
    first = _hip.ffdnet_head_masked if ffdnet else _hip.conv3x3_c1_to_64_masked
    last = _hip.ffdnet_tail if ffdnet else _hip.conv3x3_c64_to_1
    adjoint(last(dx.cl(mf * h), stack.tail_f), v, h, first(v, stack.tail_t, m), f"tail_f / tail_t, {'FFDNet' if ffdnet else 'plain'} edges")


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("ffdnet", BOOL)
def test_middle_layer_pack_and_its_transpose(ffdnet, i):
    """<f22_masked(h, mid_f[i], m), g> == <h, f22_masked(m . g, mid_t[i], ones)>.  |values| <= 576 * 8 * 16 = 73728."""
    stack, (n, H, W), m, mf, ones = integer_stack(ffdnet)
    h, g = dx.cl(ints((n, 64, H, W), 5 + i)), dx.cl(ints((n, 64, H, W), 7 + i))
    fwd = _hip.conv3x3_c64_winograd_masked(h, stack.mid_f[i], m)
    bwd = _hip.conv3x3_c64_winograd_masked(dx.cl(mf * g), stack.mid_t[i], ones)
    adjoint(fwd, g, h, bwd, f"mid_f[{i}] / mid_t[{i}], {'FFDNet' if ffdnet else 'plain'} stack")


# ----------------------------------------------------------------------------- 3. one whole masked stack
@pytest.mark.parametrize("direction", ["jvp", "vjp"])
@pytest.mark.parametrize("ffdnet", BOOL)
def test_masked_stack_is_exact(ffdnet, direction):
    """vjp._MaskedStack.jvp / .vjp of a three-layer plan 1 -> 64 -> 64 -> 1 (FFDNet: 5 -> 64 -> 64 -> 4) on denoiser_exact_ref.stack_data:
    first and last weights +-1, middle weights +-4 (U = G w G^T an integer, |U| <= 9), v in {-1, 0, 1} (FFDNet: on one pixel phase).
    Under all-ones masks and absolute values the sums reach 9, then 9 * 576 * 4 = 20736 (the middle layer's own Winograd partial sums:
    1.4e5), then 1.1e7 < 2^24 = 1.68e7 in both directions (tests/test_denoiser_exact_host.py asserts that propagation), so the device
    must give vjp.masked_jvp / masked_vjp in float64 under its own masks bit for bit."""
    layers, x, sigma, v = dx.stack_data(ffdnet)
    stack = vjp._MaskedStack(layers, x.to(DEV), None if sigma is None else sigma.to(DEV))
    masks = [vjp.unpack_masks(m).cpu() for m in stack.masks]
    fracs = [float(m.double().mean()) for m in masks]
    got = getattr(stack, direction)(v.to(DEV))
    torch.cuda.synchronize()
    l64 = [(w.double(), None if b is None else b.double(), r) for w, b, r in layers]
    want = (vjp.masked_jvp if direction == "jvp" else vjp.masked_vjp)(l64, masks, v.double(), vjp.FFDNET_EDGES if ffdnet else vjp.PLAIN_EDGES)
    nonzero = float((want != 0).double().mean())
    print(f"STACK | {'ffdnet' if ffdnet else 'plain'} {direction} | masks set {fracs[0]:.3f} {fracs[1]:.3f} | non-zero {nonzero:.3f} | max {float(want.abs().max()):g} |")
    assert len(masks) == 2 and all(0.25 < fr < 0.75 for fr in fracs), fracs
    assert nonzero > 0.5 and float(want.abs().max()) < 2.0 ** 24
    wrong = got.double().cpu() != want
    assert got.shape == want.shape and not bool(wrong.any()), (
        f"{int(wrong.sum())} of {wrong.numel()} elements differ, the largest by {float((got.double().cpu() - want).abs().max()):g}, "
        f"first at {tuple(wrong.nonzero()[0].tolist())}")
