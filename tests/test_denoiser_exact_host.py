"""tests/denoiser_exact_ref.py held to account without a GPU: the reference implementation alone - CPU fp32 conv2d, a torch emulation of
the fp16 split - must pass the gates tests/test_denoiser_exact_gpu.py holds the kernels to, on the same seeded data; the integer data
must satisfy the caps that keep (a) from passing vacuously; the Winograd propagation must be the kernels' algebra and dominate the
direct sum's S; and the table must cover every forward entry point of _hip.SIGNATURES at shapes that are ragged as claimed.  For the
masked kernels (tests/test_backward_exact_gpu.py): the caps of their integer data under both mask forms, the select and the
transposed references against conv_transpose2d in float64, the integer guard words, what a failure message reads out of a zero
pattern, and the worst-case propagation that makes a whole masked stack exact."""
import itertools

import pytest
import torch
import torch.nn.functional as Fn

import denoiser_exact_ref as dx
import nonfinite_ref as nf
from deqsci_amd import _hip, vjp

BOOL = (False, True)


def conv64_cases():
    """(kernel, shape name, shape, bias_relu, measured) of every 64 -> 64 case of the GPU file."""
    for k in dx.CONV64:
        for (sname, shape), br in itertools.product(dx.shapes_of(k).items(), BOOL):
            for measured in (BOOL if dx.KERNELS[k].get("split") else (False,)):
                yield k, sname, shape, br, measured


def fp32_conv(x, w, b=None, relu=False):
    y = Fn.conv2d(x.float(), w.float(), None if b is None else b.float(), padding=1)
    return torch.relu(y) if relu else y


# ----------------------------------------------------------------------------- coverage
def test_every_forward_entry_point_is_in_the_table():
    listed = {s for k in dx.KERNELS.values() for s in k["symbols"]}
    forward = {name for name in _hip.SIGNATURES if name.startswith(dx.FORWARD_PREFIXES)}
    assert listed <= forward, listed - forward
    assert not (listed & set(dx.OUT_OF_SCOPE))
    missing = forward - listed - set(dx.OUT_OF_SCOPE)
    assert not missing, f"forward entry points of _hip.SIGNATURES that tests/denoiser_exact_ref.py neither covers nor excuses: {sorted(missing)}"
    assert set(dx.OUT_OF_SCOPE) <= forward
    for k, v in dx.KERNELS.items():
        assert v["exact"] is True or (isinstance(v["exact"], str) and len(v["exact"]) > 40), k      # exact, or a written reason
        assert dx.c_of(k) >= 0


def test_shapes_are_ragged_as_claimed():
    """Every nonfinite_ref shape used here: two images or more, every seam inside the shape with a partial block behind the last one,
    no side a multiple of a Winograd tile side > 1 - but for the matrix-core head's launch, whose size its threshold dictates (the
    ragged launch beside it makes up for that).  The added shapes: one pixel; more block tiles than 256 workgroups."""
    for k, v in dx.KERNELS.items():
        for name in v["nf"]:
            c = nf.CASES[name]
            n, H, W = c["shape"]
            th, tw = c["tile"]
            assert n >= 2 and all(0 < s < H for s in c["rows"]) and all(0 < s < W for s in c["cols"]), name
            if name == "head_mfma":
                continue
            assert (th == 1 or H % th) and (tw == 1 or W % tw), name
            assert (H - max(c["rows"])) < max(c["rows"]) and (W - max(c["cols"])) < max(c["cols"]), name     # a partial last block
            assert W % 2 == 1, name
        if v["wino"]:
            assert nf.CASES[v["nf"][0]]["tile"] == v["wino"], k
    n, H, W = dx.HEAD_MFMA_RAGGED
    assert H % 32 and W % 32 and W % 16 and -(-H // 32) * -(-W // 32) * n >= 2 * 256
    n, H, W = dx.MANY
    for th, tw in ((16, 16), (16, 32), (8, 64)):                     # block tiles of f22, f44 / s16, w16
        assert n * -(-H // th) * -(-W // tw) > 256
    assert dx.ONE == (1, 1, 1)


def test_guards():
    for W in (1, 16, 35, 67, 256):
        g = dx.guard_bytes(W)
        assert g % 256 == 0 and g >= 2 * W * 64 * 4
    a = dx.Arena(35, "cpu")
    t = dx.cl(torch.arange(2 * 64 * 3 * 35, dtype=torch.float32).reshape(2, 64, 3, 35))
    v = a.operand(t)
    assert torch.equal(v, t) and v.is_contiguous(memory_format=torch.channels_last)
    o = a.output((2, 64, 3, 35), channels_last=True)
    assert bool(torch.isnan(o).all()) and o.is_contiguous(memory_format=torch.channels_last) and a.intact()
    o.fill_(1.0)
    assert a.intact()
    buf, g = a.outs[0]
    buf[g - 1] = 0.0
    assert not a.intact()
    h = a.output((4, 7), torch.float16)
    assert h.dtype == torch.float16 and float(a.outs[1][0][0]) == dx.SENTINEL


# ----------------------------------------------------------------------------- Winograd propagation
@pytest.mark.parametrize("tile", [(2, 2), (4, 4), (1, 2), (1, 1)])
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 1), (1, 8, 8)])
def test_winograd_propagation(tile, shape):
    """With signs, the matrices are a convolution (they are the kernels' Winograd and no other algebra); on absolute values the
    propagation is >= the direct sum's S, element by element."""
    n, H, W = shape
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(n, 8, H, W, generator=g).double(), torch.randn(6, 8, 3, 3, generator=g).double(), torch.randn(6, generator=g).double()
    want = Fn.conv2d(x, w, b, padding=1)
    got = dx.s_wino(x, w, tile, b, signed=True)
    Sp = dx.s_plain(x.abs(), w.abs(), b.abs())
    assert bool(((got - want).abs() <= 1e-12 * dx.s_wino(x.abs(), w.abs(), tile, b.abs())).all())
    Sw = dx.s_wino(x.abs(), w.abs(), tile, b.abs())
    assert bool((Sw >= Sp * (1 - 1e-12)).all())
    if tile == (1, 1):
        assert bool(((Sw - Sp).abs() <= 1e-12 * Sp).all())
    assert bool(((dx.s_wino(x.abs(), w.abs(), tile, b.abs(), chunk=1) - Sw).abs() <= 1e-12 * Sw).all())      # (image chunks: float64 rounding only)


# ----------------------------------------------------------------------------- (a): caps and exactness of the reference arithmetic
@pytest.mark.parametrize("kernel,sname,shape,bias_relu,measured", [c for c in conv64_cases() if dx.KERNELS[c[0]]["exact"] is True])
def test_conv64_integer_data(kernel, sname, shape, bias_relu, measured):
    x, w, b, relu = dx.conv64_data(shape, "int", dx.KERNELS[kernel]["wmult"], bias_relu, measured)
    assert bool((w != 0).all()) and float(w.abs().max()) <= 4 * dx.KERNELS[kernel]["wmult"] and bool((w % dx.KERNELS[kernel]["wmult"] == 0).all())
    assert float(x.abs().max()) <= 8 and (shape == dx.ONE or 0.2 < float((x == 0).float().mean()) < 0.4)
    ref = dx.conv64_ref(x, w, b, relu)
    dx.check_caps(ref, relu, (kernel, sname, bias_relu, measured))
    assert float(dx.s_plain(x.abs(), w.abs(), None if b is None else b.abs()).max()) < 2.0 ** 24      # every partial sum, in any order
    assert torch.equal(fp32_conv(x, w, b, relu).double(), ref)


def edge_cases():
    for form_measured, relu in itertools.product(BOOL, BOOL):
        yield "c1_to_64", "c1_to_64", 1, form_measured, False, relu
    for kernel, sname in (("head_valu", "head_valu"), ("head_mfma", "head_mfma"), ("head_mfma", "head_mfma_ragged")):
        for one_sigma in BOOL:
            yield kernel, sname, 5, False, one_sigma, True
    for measured, one_sigma in itertools.product(BOOL, BOOL):
        yield "head_s16", "head_s16", 5, measured, one_sigma, True


@pytest.mark.parametrize("mode", ["int", "real"])
@pytest.mark.parametrize("kernel,sname,cin,measured,one_sigma,relu", list(edge_cases()))
def test_first_layers(kernel, sname, cin, measured, one_sigma, relu, mode):
    shape = dx.shapes_of(kernel)[sname]
    x, sig, w = dx.head_data(shape, mode, cin, measured, one_sigma)
    ref = dx.head_ref(x, sig, w, relu)
    xin = dx.head_operand(x, sig)
    got = fp32_conv(xin, w, None, relu).double()
    if mode == "int":
        assert bool((w != 0).all()) and (sig is None or bool((8 * sig == (8 * sig).round()).all()))      # (integers, or multiples of 2^-3 with their scaled image)
        dx.check_caps(ref, relu, (kernel, sname, measured, one_sigma))
        assert torch.equal(got, ref)
    else:
        assert bool(((got - ref).abs() <= 9 * cin * dx.U * dx.s_plain(xin.abs(), w.abs())).all())           # c = 9 * cin: the direct sum's


@pytest.mark.parametrize("mode", ["int", "real"])
@pytest.mark.parametrize("kernel,cout,in_bias,measured", [("tail_valu", c, ib, False) for c in (4, 1) for ib in BOOL]
                         + [("tail_s16", c, False, m) for c in (4, 1) for m in BOOL])
def test_last_layers(kernel, cout, in_bias, measured, mode):
    shape = dx.shapes_of(kernel)[f"{kernel}_{'ffdnet' if cout == 4 else 'c1'}"]
    h, w, b = dx.tail_data(shape, mode, cout, in_bias, measured)
    ref = dx.tail_ref(h, w, b)
    got = fp32_conv(dx.tail_operand(h, b).float(), w).double()
    got = Fn.pixel_shuffle(got, 2) if cout == 4 else got
    if mode == "int":
        dx.check_caps(Fn.pixel_unshuffle(ref, 2) if cout == 4 else ref, False, (kernel, cout, in_bias, measured))
        assert bool((w != 0).all()) and torch.equal(got, ref)
    else:
        S = dx.s_plain(dx.tail_operand(h, b, absolute=True), w.abs())
        S = Fn.pixel_shuffle(S, 2) if cout == 4 else S
        assert bool(((got - ref).abs() <= dx.c_of("tail_valu", in_bias) * dx.U * S).all())


# ----------------------------------------------------------------------------- (b): the reference arithmetic within the kernels' gate
@pytest.mark.parametrize("sname,shape", list(dx.shapes_of("s16").items()) + [("w16", nf.CASES["w16"]["shape"])])
@pytest.mark.parametrize("bias_relu", BOOL)
def test_cpu_fp32_conv_is_within_the_direct_sum_bound(sname, shape, bias_relu):
    """c = 9*64 + 1: a sum of 576 rounded products in any order, and the bias."""
    x, w, b, relu = dx.conv64_data(shape, "real", 1, bias_relu, False)
    ref = dx.conv64_ref(x, w, b, relu)
    S = dx.s_plain(x.abs(), w.abs(), None if b is None else b.abs())
    err = (fp32_conv(x, w, b, relu).double() - ref).abs()
    assert bool((err <= (9 * 64 + 1) * dx.U * S).all()), float((err / S).max() / dx.U)
    for tile in ((2, 2), (4, 4), (1, 2)):
        if shape != dx.MANY:
            assert bool((dx.s_wino(x.abs(), w.abs(), tile, None if b is None else b.abs()) >= S * (1 - 1e-12)).all())


@pytest.mark.parametrize("measured", BOOL)
def test_split_rule_holds_for_an_emulated_split(measured):
    """hi = fp16(2^e x), lo = fp16(2^e x - hi) in torch, e per image as _hip.act_exp derives it: within max(2^-22 |x|, 2^(-25 - e)) per
    element, on data reaching down to the subnormal lo pieces; exact on the integer data."""
    n, H, W = nf.CASES["s16"]["shape"]
    for mode in ("int", "real"):
        x = dx.conv64_data((n, H, W), mode, 1, False, measured)[0]
        if mode == "real":
            x = x * torch.logspace(0, -7, W).view(1, 1, 1, W)           # columns down to 1e-7 of the maximum
        e = [_hip.act_exp(float(v)) for v in x.abs().reshape(n, -1).amax(1)] if measured else [_hip.SP16_DEFAULT_EXP] * n
        sc = torch.tensor([2.0 ** k for k in e]).view(-1, 1, 1, 1)
        hi = (x * sc).half()
        lo = (x * sc - hi.float()).half()
        back = (hi.double() + lo.double()) / sc.double()
        err = (back - x.double()).abs()
        if mode == "int":
            assert bool((err == 0).all())
        else:
            assert bool((err <= dx.split_rule(x.abs(), e)).all())
            assert bool((err > 2.0 ** -23 * x.abs().double()).any())    # (the floor is needed: the relative rule alone does not hold)


# ----------------------------------------------------------------------------- the masked kernels (tests/test_backward_exact_gpu.py)
def masked_cases():
    for k in dx.MASKED:
        for (sname, shape), transposed in itertools.product(dx.shapes_of(k).items(), BOOL):
            yield k, sname, shape, transposed


def test_masked_shapes_and_masks_are_as_claimed():
    """The masked head's three launches: two images of 18 x 19 and one position stay below every device's threshold that has more than
    two CUs, 128 x 33 x 35 is ragged against the 32 x 32 tile in both directions with four tiles per image (the GPU test raises n where
    the device has more than 256 CUs).  The masks: p = 1/2 per bit; the checker's words are the two half-words, alternating with
    (row + column); nonfinite_ref.pack_mask and vjp.unpack_masks are inverse."""
    assert dx.shapes_of("head_masked") == {"head_valu": (2, 18, 19), "one": (1, 1, 1), "head_masked_ragged": (128, 33, 35)}
    assert dx.shapes_of("f22_masked") == {"f22": (2, 19, 35), "one": dx.ONE, "many": dx.MANY}
    assert dx.shapes_of("c1_to_64_masked") == {"c1_to_64": (2, 34, 35)}
    tiles32 = lambda s: s[0] * -(-s[1] // 32) * -(-s[2] // 32)
    assert tiles32((2, 18, 19)) == 2 and tiles32(dx.ONE) == 1 and tiles32(dx.HEAD_MFMA_RAGGED) == 4 * 128 >= 2 * 256
    assert all(s % 32 and s > 32 for s in dx.HEAD_MFMA_RAGGED[1:])
    for shape in ((2, 19, 35), (128, 33, 35), dx.MANY):
        kernel = "head_masked" if shape[0] == 128 else "f22_masked"
        r = dx.masked_bits(kernel, shape, "random")
        assert r.shape[0] == (dx.PERIOD if shape[0] == 128 else shape[0]) and 0.49 < float(r.float().mean()) < 0.51
        words = nf.pack_mask(dx.masked_bits(kernel, shape, "checker"))
        lo, hi = (1 << 32) - 1, -(1 << 32)
        assert bool((words[:, 0::2, 0::2] == lo).all()) and bool((words[:, 0::2, 1::2] == hi).all()) and bool((words[:, 1::2, 0::2] == hi).all())
        assert bool((words[:, 1::2, 1::2] == lo).all())
        assert torch.equal(vjp.unpack_masks(nf.pack_mask(r)), r)


@pytest.mark.parametrize("form", dx.MASK_FORMS)
@pytest.mark.parametrize("kernel,sname,shape,transposed", list(masked_cases()))
def test_masked_integer_data(kernel, sname, shape, transposed, form):
    """(a)'s caps for every masked case, and CPU fp32 arithmetic behind the same select passing both gates."""
    x, w = dx.masked_operands(kernel, shape, "int", transposed)
    wm = dx.KERNELS[kernel]["wmult"]
    assert bool((w != 0).all()) and float(w.abs().max()) <= 4 * wm and bool((w % wm == 0).all()) and float(x.abs().max()) <= 8
    assert tuple(w.shape) == {"f22_masked": (64, 64, 3, 3), "c1_to_64_masked": (64, 1, 3, 3), "head_masked": (64, 4, 3, 3)}[kernel]
    bits, unm = dx.masked_bits(kernel, shape, form), dx.masked_unmasked_ref(kernel, shape, "int", transposed)
    dx.check_masked_caps(unm, bits, (kernel, sname, transposed, form), one_pixel=shape == dx.ONE)
    xin = dx.masked_input(kernel, x)
    assert float(dx.s_plain(xin.abs(), w.abs()).max()) < 2.0 ** 24 and (kernel != "head_masked" or float(unm.abs().max()) <= 36 * 8 * 4)
    if dx.KERNELS[kernel]["wino"]:
        assert float(dx.s_wino(xin.abs(), w.abs(), dx.KERNELS[kernel]["wino"]).max()) < 2.0 ** 24        # every partial sum of the transforms
    ref = dx.masked_ref(kernel, shape, "int", transposed, form)
    assert torch.equal(ref, unm * bits) and bool((ref[~bits] == 0).all())
    assert torch.equal(torch.where(bits, fp32_conv(xin, w), torch.zeros(())).double(), ref)


@pytest.mark.parametrize("kernel,sname,shape,transposed", [c for c in masked_cases() if c[2] != dx.MANY])
def test_masked_real_data(kernel, sname, shape, transposed):
    """(b): CPU fp32 behind the select is within the direct sum's bound times the mask (exactly 0 under a cleared bit), and the
    kernel's own S is no smaller than the direct sum's."""
    x, w = dx.masked_operands(kernel, shape, "real", transposed)
    xin, bits = dx.masked_input(kernel, x), dx.masked_bits(kernel, shape, "random")
    ref = dx.masked_ref(kernel, shape, "real", transposed, "random")
    got = torch.where(bits, fp32_conv(xin, w), torch.zeros(())).double()
    Sp = dx.s_plain(xin.abs(), w.abs())
    assert bool(((got - ref).abs() <= 9 * w.shape[1] * dx.U * Sp * bits).all())
    b = dx.masked_bound(kernel, shape, transposed, "random")
    assert bool((b[~bits] == 0).all()) and bool((b[bits] >= dx.c_of(kernel) * dx.U * Sp[bits] * (1 - 1e-12)).all())


def test_select_and_transposed_references():
    """The references the masked cases stand on, against torch's own transposed convolution in float64 on integers (exact): a conv with
    vjp._transposed(w) is conv_transpose2d with w; FFDNet's transposed tail is the masked head's reference on _transposed(w_tail); the
    mask is a SELECT (a NaN under a cleared bit is 0, under a set bit it stays)."""
    g = torch.Generator().manual_seed(11)
    ints = lambda *s: torch.randint(-8, 9, s, generator=g).double()
    x, w = ints(2, 64, 5, 7), ints(64, 64, 3, 3)
    assert torch.equal(nf.conv_ref(x, vjp._transposed(w)), Fn.conv_transpose2d(x, w, padding=1))
    v, wt = ints(2, 1, 5, 7), ints(1, 64, 3, 3)
    assert torch.equal(nf.conv_ref(v, vjp._transposed(wt)), Fn.conv_transpose2d(v, wt, padding=1))
    v2, wt4 = ints(2, 1, 10, 14), ints(4, 64, 3, 3)            # y = pixel_shuffle(conv(h, wt4)): its transpose unshuffles, then transposes the conv
    want = Fn.conv_transpose2d(Fn.pixel_unshuffle(v2, 2), wt4, padding=1)
    assert torch.equal(nf.ffdnet_head_ref(v2, None, vjp._transposed(wt4), relu=False, with_sigma=False), want)
    h = ints(2, 64, 5, 7)
    y = torch.autograd.functional.vjp(lambda t: Fn.pixel_shuffle(Fn.conv2d(t, wt4, padding=1), 2), h, v2)[1]
    assert torch.equal(y, want)
    bits = torch.rand(2, 64, 5, 7, generator=g) < 0.5
    assert torch.equal(nf.conv_ref(x, w, mask=bits), Fn.conv2d(x, w, padding=1) * bits)
    xp = x.clone()
    xp[0, 3, 2, 2] = float("nan")
    y = nf.conv_ref(xp, w, mask=bits)
    assert bool((y[~bits] == 0).all()) and bool(torch.isnan(y[0, :, 2, 2][bits[0, :, 2, 2]]).all()) and bool(bits[0, :, 2, 2].any())


def test_integer_guards():
    a = dx.Arena(35, "cpu")
    t = torch.randint(-2 ** 62, 2 ** 62, (2, 3, 35))
    for fill in (-1, 0):
        v = a.words(t, fill)
        assert torch.equal(v, t) and v.dtype == torch.int64 and v.is_contiguous() and v.data_ptr() % 8 == 0
        buf = v.untyped_storage()
        whole = torch.tensor([], dtype=torch.int64).set_(buf)
        g = dx.guard_bytes(35) // 8
        assert whole.numel() == t.numel() + 2 * g and bool((whole[:g] == fill).all()) and bool((whole[-g:] == fill).all())
        assert g >= 2 * 35                                          # (two image rows of words and more)
    fills = dx.mask_guard_fills()
    assert (next(fills), next(fills)) == (-1, 0)


def test_mask_fault_names_what_went_wrong():
    """The reading a failing masked case adds to its message: a swapped half-word and a neighbour's word taken at the odd column of a
    2 x 2 tile are both named on the checker mask (where either changes whole half-pixels, in the same way) and told apart on the
    random one; an ignored mask is named; a correct output gives None."""
    shape = (2, 19, 35)
    unm = dx.masked_unmasked_ref("f22_masked", shape, "int", False)
    for form in dx.MASK_FORMS:
        bits = dx.mask_bits(shape, form)
        assert dx.mask_fault(unm * bits, unm, bits) is None
        unwritten = unm * bits
        unwritten[..., -1] = float("nan")
        assert dx.mask_fault(unwritten, unm, bits) is None          # (hold() reports non-finite outputs itself)
        said = dx.mask_fault(unm * bits.roll(32, 1), unm, bits)
        assert "halves of the mask word swapped" in said and (form == "checker" or "column" not in said)
        left = bits.clone()
        left[..., 1::2] = bits[..., 0::2][..., :left[..., 1::2].shape[-1]]          # (m00 for the pixel at ox + 1)
        said = dx.mask_fault(unm * left, unm, bits)
        assert "(row +0, column -1)" in said and ("swapped" in said) == (form == "checker")
        assert "mask ignored" in dx.mask_fault(unm, unm, bits)
        if form == "random":                                         # (on the checker the complement explains any misplaced zero)
            assert "no single mislaid word" in dx.mask_fault(torch.zeros_like(unm), unm, bits)


@pytest.mark.parametrize("direction", ["jvp", "vjp"])
@pytest.mark.parametrize("ffdnet", BOOL)
def test_masked_stack_data_is_exact_in_the_worst_case(ffdnet, direction):
    """Every partial sum of _MaskedStack.jvp / .vjp on dx.stack_data is an integer below 2^24: the propagation of absolute values
    under all-ones masks, the middle layer through its own Winograd transforms (U = G w G^T is an integer for w in {-4, +4}).  On the
    host's own float64 masks the data is not vacuous either: masks between a quarter and three quarters set, more than half of the
    result non-zero - and float32 host arithmetic gives the float64 result exactly."""
    layers, x, sigma, v = dx.stack_data(ffdnet)
    assert all(bool((w.abs() == m).all()) for (w, _, _), m in zip(layers, (1, 4, 1)))
    G = dx._T[2]["G"].double()
    Uw = torch.einsum("ij,ocjk,lk->ocil", G, layers[1][0].double(), G)
    assert bool((Uw == Uw.round()).all()) and float(Uw.abs().max()) <= 9
    assert bool((layers[1][1] == layers[1][1].round()).all()) and bool(((v == 0) | (v.abs() == 1)).all())
    if ffdnet:
        assert bool((Fn.pixel_unshuffle(v, 2)[:, 1:] == 0).all()) and bool((Fn.pixel_unshuffle(v, 2)[:, 0] != 0).any())
    t1, t2, t2_wino, t3 = dx.stack_worst_case(layers, v, ffdnet, direction)
    print(f"worst case {'ffdnet' if ffdnet else 'plain'} {direction}: {t1:g} {t2:g} (Winograd partial sums {t2_wino:g}) {t3:g}")
    assert t1 <= 9 and t2 <= 9 * 576 * 4 and t2_wino < 2.0 ** 24 and t3 < 2.0 ** 24
    edges = vjp.FFDNET_EDGES if ffdnet else vjp.PLAIN_EDGES
    l64 = [(w.double(), None if b is None else b.double(), r) for w, b, r in layers]
    masks = (vjp.ffdnet_plan_forward(l64, x.double(), sigma.double())[1] if ffdnet else vjp.plan_masks(l64, x.double()))
    assert len(masks) == 2 and all(0.25 < float(m.double().mean()) < 0.75 for m in masks)
    fn = vjp.masked_jvp if direction == "jvp" else vjp.masked_vjp
    want = fn(l64, masks, v.double(), edges)
    assert float((want != 0).double().mean()) > 0.5 and float(want.abs().max()) <= t3
    assert torch.equal(fn(layers, masks, v, edges).double(), want)
