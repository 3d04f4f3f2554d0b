"""Every forward kernel of the denoiser against float64, element by element (statement, data, constants: tests/denoiser_exact_ref.py;
the helper itself is held by tests/test_denoiser_exact_host.py; measured ratios: profiles/denoiser_exact.md).  The masked kernels of the
backward are held the same way, with this file's hold(), in tests/test_backward_exact_gpu.py.

Each case runs one entry point of deqsci_amd/_hip.py in one form at one shape of nonfinite_ref.CASES (64 -> 64 kernels: also one pixel
and a launch of more block tiles than persistent workgroups), twice:
  mode "int"   (a) torch.equal with the float64 reference on integer data - the argument why the kernel's arithmetic is exact on it is
               the docstring of the test;
  mode "real"  (b) |got - ref64| <= c 2^-24 S + rep on every element, one ROW line per case.
Both under (c): every operand a view inside NaN, every output a NaN-filled view inside sentinels, the padding columns of blk32 / p32
outputs still NaN afterwards, the output finite, a second launch the same bits.  A case reports every property that fails."""
import functools

import pytest
import torch
import torch.nn.functional as Fn

import denoiser_exact_ref as dx

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deqsci_amd import _hip

DEV = "cuda"
MODES = ("int", "real")
BIAS_RELU = (False, True)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def slots(a, t, measured):
    """Range slots of an (n, ...) tensor as a guarded operand - max |t| per image, what a measuring launch leaves - or None."""
    return a.operand(t.abs().reshape(t.shape[0], -1).amax(1).float().to(DEV)) if measured else None


def exps(slot, fixed, n):
    return [fixed] * n if slot is None else [_hip.act_exp(v) for v in slot.tolist()]


def hold(kernel, form, shape, mode, launch, ref, bound, explain=None):
    """(a) or (b), and (c), of one case.  launch() -> (got fp32 (n,C,H,W) on the device, [padding tensors], arena); ref: float64 on the
    CPU; bound: float64 on the CPU (mode "real"), or a function of the reference for an output that is itself split.  explain(got) ->
    a sentence or None, asked only when the case fails (the masked kernels: what was done to the mask)."""
    got, pads, arena = launch()
    again, pads2, arena2 = launch()
    torch.cuda.synchronize()
    fails = []
    if not (arena.intact() and arena2.intact()):
        fails.append("a sentinel around an output was overwritten")
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{int((~torch.isfinite(got)).sum())} non-finite outputs (an operand's NaN guard was used, or an output element not written)")
    if not all(bool(torch.isnan(p).all()) for p in pads + pads2):
        fails.append("padding columns of the output were written")
    if got.shape != again.shape or not torch.equal(bits(got), bits(again)):
        fails.append("the second launch gave other bits")
    want = ref.to(DEV)
    assert got.shape == want.shape, (got.shape, want.shape)
    if mode == "int":
        assert dx.KERNELS[kernel]["exact"] is True
        wrong = got != want.float()
        if bool(wrong.any()):
            d = (got.double() - want).abs()
            fails.append(f"not exact: {int(wrong.sum())} of {wrong.numel()} elements differ, the largest by {float(torch.nan_to_num(d, nan=float('inf')).max()):g}, "
                         f"first at {tuple(wrong.nonzero()[0].tolist())}")
    else:
        b = (bound(ref) if callable(bound) else bound).to(DEV)
        err = (got.double() - want).abs()
        ratio = float(torch.nan_to_num(err / b.clamp_min(1e-300), nan=float("inf")).max())
        print(f"ROW | {kernel} | {form} | {shape[0]}x{shape[1]}x{shape[2]} | {ratio:.3g} |")
        if not bool((err <= b).all()):
            fails.append(f"{int((~(err <= b)).sum())} elements beyond the bound, worst err/bound {ratio:.3f}")
    said = explain(got) if fails and explain is not None else None
    if said:
        fails.append(said)
    assert not fails, f"{kernel} {form} {shape} {mode}: " + "; ".join(fails)


def guard_weights(a, W):
    """A weights object's packed pieces as a guarded operand."""
    W.packed = a.operand(W.packed)
    return W


# ----------------------------------------------------------------------------- 64 -> 64: references and bounds, shared between the cases
@functools.lru_cache(maxsize=None)
def conv64_ref(shape, mode, wmult, bias_relu, measured):
    return dx.conv64_ref(*dx.conv64_data(shape, mode, wmult, bias_relu, measured))


@functools.lru_cache(maxsize=None)
def conv64_S(shape, tile, bias_relu, measured, split=False):
    """(S with |bias|, S without, the floor sums of a split-fp16 kernel or None) of the real data, S the kernel's own (tile None: the
    direct sum)."""
    x, w, b, _ = dx.conv64_data(shape, "real", 1, bias_relu, measured)
    S0 = dx.s_plain(x.abs(), w.abs()) if tile is None else dx.s_wino(x.abs(), w.abs(), tile)
    sums = dx.floor_sums(x.abs(), w.abs(), tile) if split else None
    return (S0 if b is None else S0 + b.abs().double().view(1, -1, 1, 1)), S0, sums


def conv64_case(kernel, shape, mode, bias_relu, measured=False):
    k = dx.KERNELS[kernel]
    wmult = k["wmult"] if mode == "int" else 1
    x, w, b, relu = dx.conv64_data(shape, mode, wmult, bias_relu, measured)
    ref = conv64_ref(shape, mode, wmult, bias_relu, measured)
    S = conv64_S(shape, k["wino"], bias_relu, measured, bool(k.get("split"))) if mode == "real" else (None, None, None)
    return x, w, b, relu, ref, S


def many_tiles(shape, tile_h, tile_w):
    n, H, W = shape
    if shape == dx.MANY:
        assert n * -(-H // tile_h) * -(-W // tile_w) > torch.cuda.get_device_properties(0).multi_processor_count


SHAPES64 = {k: list(dx.shapes_of(k).items()) for k in dx.CONV64}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bias_relu", BIAS_RELU)
@pytest.mark.parametrize("sname,shape", SHAPES64["f22"])
def test_winograd_f22(sname, shape, bias_relu, mode):
    """conv3x3_c64_winograd, csrc/winograd.hip.  EXACT on integer data with the weights MULTIPLIES OF 4: U = G w G^T divides by 2 on
    each side, so U is an integer, |U| <= 1.5^2 * 16 = 36; V = B^T d B adds and subtracts, |V| <= 4 * 8 = 32; everything is fp32 (no
    fp16 piece); a partial sum of M is at most 64 * 36 * 32 + |bias| (<= 32 + 4096) < 2^17, and the output transform adds nine of them:
    < 2^21 < 2^24.  c = 2 + 1 + 2*64 + 4 on S = the transforms' absolute-value propagation."""
    x, w, b, relu, ref, (S, _, _) = conv64_case("f22", shape, mode, bias_relu)
    many_tiles(shape, 16, 16)
    n, H, W = shape
    xg, Ug, bg = dx.cl(x.to(DEV)), _hip.pack_winograd_weights(w.to(DEV)), None if b is None else b.to(DEV)

    def launch():
        a = dx.Arena(W, DEV)
        out = a.output((n, 64, H, W), channels_last=True)
        _hip.conv3x3_c64_winograd(a.operand(xg), a.operand(Ug), a.operand(bg), relu, out=out)
        return out, [], a
    hold("f22", "bias+relu" if bias_relu else "plain", shape, mode, launch, ref, None if S is None else dx.c_of("f22") * dx.U * S)


@pytest.mark.parametrize("bias_relu", BIAS_RELU)
@pytest.mark.parametrize("in_blk,out_blk", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("sname,shape", SHAPES64["f44"])
def test_winograd_f44(sname, shape, in_blk, out_blk, bias_relu):
    """conv3x3_c64_winograd44, csrc/winograd44.hip, NHWC / blk32 in and out.  NOT exact on integer data and not asserted to be
    (denoiser_exact_ref.KERNELS["f44"]["exact"] says why: G divides by 6 and 24 on each side); held by the bound alone:
    c = 2*2 + 1 + 2*64 + 2*3 on S = the absolute-value propagation of F(4x4,3x3), whose B^T (entries up to 5) and A^T (up to 8) make it
    several times the direct sum's - that amplification is the kernel's own."""
    x, w, b, relu, ref, (S, _, _) = conv64_case("f44", shape, "real", bias_relu)
    many_tiles(shape, 16, 32)
    n, H, W = shape
    xg, Ug, bg = dx.cl(x.to(DEV)), _hip.pack_winograd44_weights(w.to(DEV)), None if b is None else b.to(DEV)

    def launch():
        a = dx.Arena(W, DEV)
        xin = dx.blk32_fill(_hip.Blk32(a.nan((n, 8, H, -(-W // 32), 32, 8)), n, H, W), xg) if in_blk else a.operand(xg)
        if out_blk:
            o = _hip.Blk32(a.output((n, 8, H, -(-W // 32), 32, 8)), n, H, W)
            _hip.conv3x3_c64_winograd44(xin, a.operand(Ug), a.operand(bg), relu, out=o, out_blk=True)
            return o.to_nchw(), [dx.blk32_padding(o)], a
        out = a.output((n, 64, H, W), channels_last=True)
        _hip.conv3x3_c64_winograd44(xin, a.operand(Ug), a.operand(bg), relu, out=out)
        return out, [], a
    form = f"{'blk32' if in_blk else 'nhwc'}->{'blk32' if out_blk else 'nhwc'} {'bias+relu' if bias_relu else 'plain'}"
    hold("f44", form, shape, "real", launch, ref, dx.c_of("f44") * dx.U * S)


def split_bound(kernel, S, S0, sums, e_x, e_w, e_out):
    """c 2^-24 S + rep; for an sp16 output (e_out given) a function of the reference: + the output's own split of |ref| + that bound."""
    inner = dx.c_of(kernel) * dx.U * S + dx.rep_split(S0, sums, e_x, e_w)
    if e_out is None:
        return inner
    return lambda ref: inner + dx.rep_out_split(ref.abs() + inner, e_out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bias_relu", BIAS_RELU)
@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("sname,shape", SHAPES64["s16"])
def test_split16(sname, shape, out_f32, measured, bias_relu, mode):
    """conv3x3_c64_split16, csrc/conv_s16.hip, sp16 and fp32 output, at the fixed exponent and with measured range slots (image 1 scaled
    by 2^-3: another exponent per image).  EXACT on integer data with no transform at all: 2^8 x is an integer multiple of 2^8 of at
    most 2^11 and 2^sw w (sw = 11: max |w| = 4 -> 2^13) one of 2^11 with at most three bits - every hi piece is the value, every lo
    piece 0 (to_split16 writes them; a scaled image only moves the power of two); the products are multiples of 2^19, a partial sum
    k 2^19 with |k| <= 9 * 64 * 32 = 18432 < 2^24; the epilogue's fma adds the integer bias to the rescaled sum: < 2^15 + 2^10.  The
    sp16 output of an integer |y| < 2^16 at exponent 0 (measured: 2^e y in [2^11, 2^12)) is hi + lo exactly: hi keeps 11 bits, the
    rest is an integer (a multiple of 2^e) below fp16's 11 bits.  c = 2*3*9*64 + 2."""
    x, w, b, relu, ref, (S, S0, sums) = conv64_case("s16", shape, mode, bias_relu, measured)
    many_tiles(shape, 16, 32)
    n, H, W = shape
    xg, wg, bg = dx.cl(x.to(DEV)), w.to(DEV), None if b is None else b.to(DEV)
    out_exp = 0 if mode == "int" else _hip.SP16_DEFAULT_EXP
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rin, rout = slots(a, x, measured), slots(a, ref, measured and not out_f32)
        xs = _hip.to_split16(a.operand(xg), out=_hip.Sp16(a.nan((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W), rng=rin)
        W16 = guard_weights(a, _hip.Split16Weights(wg))
        info.update(e_x=exps(rin, _hip.SP16_DEFAULT_EXP, n), e_w=W16.sw, e_out=None if out_f32 else exps(rout, out_exp, n))
        if out_f32:
            out = a.output((n, 64, H, W), channels_last=True)
            _hip.conv3x3_c64_split16(xs, W16, a.operand(bg), relu, out=out, out_f32=True)
            return out, [], a
        o = _hip.Sp16(a.output((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W)
        _hip.conv3x3_c64_split16(xs, W16, a.operand(bg), relu, out=o, out_rng=rout, out_exp=out_exp)
        return o.to_nchw(), [], a
    form = f"{'f32' if out_f32 else 'sp16'} out, {'measured' if measured else 'fixed'} {'bias+relu' if bias_relu else 'plain'}"
    bound = None
    if mode == "real":
        launch()                                               # (the exponents are the launch's own: read them back once)
        bound = split_bound("s16", S, S0, sums, info["e_x"], info["e_w"], info["e_out"])
    hold("s16", form, shape, mode, launch, ref, bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bias_relu", BIAS_RELU)
@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("sname,shape", SHAPES64["w16"])
def test_wino16(sname, shape, measured, bias_relu, mode):
    """conv3x3_c64_wino16, csrc/conv_w16.hip: F(2,3) along x, the direct sum along y, split-fp16 products.  EXACT on integer data with
    the weights MULTIPLES OF 2: U = G w divides by 2, so U is an integer, |U| <= 1.5 * 8 = 12, and 2^sw U (sw = 10) a multiple of 2^10
    below 2^14 with four bits: hi exact, lo 0.  V = B^T d is one addition of integers, |V| <= 16, 2^8 V <= 2^12 with five bits: hi
    exact, lo 0.  M[xi] sums 3 * 64 products, |M| <= 192 * 12 * 16 = 36864 (times 2^18); the output transform adds three, the fma the
    integer bias: < 2^17 + 2^12 < 2^24.  The p32 output is the fp32 number times a power of two.  c = 1 + 1 + 2*3*3*64 + 2 + 1 on S = the
    propagation of F(2,3) along x."""
    x, w, b, relu, ref, (S, S0, sums) = conv64_case("w16", shape, mode, bias_relu, measured)
    many_tiles(shape, 8, 64)
    n, H, W = shape
    xg, wg, bg = x.to(DEV), w.to(DEV), None if b is None else b.to(DEV)
    out_exp = 0 if mode == "int" else _hip.SP16_DEFAULT_EXP
    p32_shape = (n, 8, 2, H, -(-W // 64), 2, 32, 4)
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rin, rout = slots(a, x, measured), slots(a, ref, measured)
        xp = dx.p32_fill(_hip.P32(a.nan(p32_shape), n, H, W, rng=rin), xg)
        Ww = guard_weights(a, _hip.Wino16Weights(wg))
        info.update(e_x=exps(rin, _hip.SP16_DEFAULT_EXP, n), e_w=Ww.sw)
        o = _hip.P32(a.output(p32_shape), n, H, W)
        _hip.conv3x3_c64_wino16(xp, Ww, a.operand(bg), relu, out=o, out_rng=rout, out_exp=out_exp)
        return o.to_nchw(), [dx.p32_padding(o)], a
    bound = None
    if mode == "real":
        launch()
        bound = split_bound("w16", S, S0, sums, info["e_x"], info["e_w"], None)
    hold("w16", f"{'measured' if measured else 'fixed'} {'bias+relu' if bias_relu else 'plain'}", shape, mode, launch, ref, bound)


# ----------------------------------------------------------------------------- first layers
def periodic(t, n):
    """The n images of a launch whose data repeats its k distinct ones."""
    return t if t.shape[0] == n else t[torch.arange(n) % t.shape[0]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("form,measured", [("f32", False), ("sp16", False), ("sp16", True), ("p32", False), ("p32", True)])
def test_conv_c1_to_64(form, measured, relu, mode):
    """conv3x3_c1_to_64, csrc/ffdnet_edges.hip, fp32 / sp16 / p32 output.  EXACT on integer data: nine fused multiply-adds of integers,
    |sum| <= 9 * 8 * 4 = 288; the sp16 store of an integer below 2^11 times 2^0 (measured: a power of two that puts the image's
    maximum into [2^11, 2^12)) is hi alone; the p32 store a power of two times it.  c = 9."""
    (sname, shape), = dx.shapes_of("c1_to_64").items()
    n, H, W = shape
    x, _, w = dx.head_data(shape, mode, 1, measured)
    ref = dx.head_ref(x, None, w, relu)
    xg, Wg = x.to(DEV), _hip.pack_c1_to_64_weights(w.to(DEV))
    out_exp = 0 if mode == "int" else _hip.SP16_DEFAULT_EXP
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rout = slots(a, ref, measured)
        info.update(e_out=exps(rout, out_exp, n))
        if form == "f32":
            out = a.output((n, 64, H, W), channels_last=True)
            _hip.conv3x3_c1_to_64(a.operand(xg), a.operand(Wg), relu=relu, out=out)
            return out, [], a
        if form == "sp16":
            o = _hip.Sp16(a.output((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W)
            _hip.conv3x3_c1_to_64(a.operand(xg), a.operand(Wg), relu=relu, out=o, sp16=True, out_rng=rout, out_exp=out_exp)
            return o.to_nchw(), [], a
        o = _hip.P32(a.output((n, 8, 2, H, -(-W // 64), 2, 32, 4)), n, H, W)
        _hip.conv3x3_c1_to_64(a.operand(xg), a.operand(Wg), relu=relu, out=o, p32=True, out_rng=rout, out_exp=out_exp)
        return o.to_nchw(), [dx.p32_padding(o)], a
    bound = None
    if mode == "real":
        launch()
        inner = dx.c_of("c1_to_64") * dx.U * dx.s_plain(x.abs(), w.abs())
        bound = inner + dx.rep_out_split(ref.abs() + inner, info["e_out"]) if form == "sp16" else inner
    hold("c1_to_64", f"{form} {'measured' if measured else 'fixed'} {'relu' if relu else 'plain'}", shape, mode, launch, ref, bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("one_sigma", [False, True])
@pytest.mark.parametrize("kernel,sname", [("head_valu", "head_valu"), ("head_mfma", "head_mfma"), ("head_mfma", "head_mfma_ragged")])
def test_ffdnet_head(kernel, sname, one_sigma, mode):
    """ffdnet_head, csrc/ffdnet_edges.hip: the vector form (small launches) and the matrix-core form (from two 32 x 32 tiles per CU
    on: nonfinite_ref's launch, and the smallest ragged one), sigma per image and one for the batch.  EXACT on integer data: 45
    products of integers |x|, sigma <= 8 by |w| <= 4, fused multiply-adds or v_mfma_f32_16x16x4_f32 on fp32 operands; every partial
    sum is an integer of at most 45 * 32 = 1440 < 2^24.  c = 45 (one rounding per fma) / 2*48 (the accumulator's rounding is not
    stated: 2 per accumulated product of the twelve k-steps, which allows truncation).  The big launches repeat five distinct images."""
    shape = dx.shapes_of(kernel)[sname]
    n, H, W = shape
    if kernel == "head_mfma":
        assert -(-W // 32) * -(-H // 32) * n >= 2 * torch.cuda.get_device_properties(0).multi_processor_count
    else:
        assert -(-W // 32) * -(-H // 32) * n < 2 * torch.cuda.get_device_properties(0).multi_processor_count
    x, sig, w = dx.head_data(shape, mode, 5, False, one_sigma)
    ref = periodic(dx.head_ref(x, sig, w), n)
    xg, Wg = periodic(x, n).to(DEV), _hip.pack_head_weights(w.to(DEV))
    sg = (sig if one_sigma else periodic(sig, n)).to(DEV)

    def launch():
        a = dx.Arena(W, DEV)
        out = a.output((n, 64, H, W), channels_last=True)
        _hip.ffdnet_head(a.operand(xg), a.operand(Wg), a.operand(sg), out=out)
        return out, [], a
    bound = None
    if mode == "real":
        bound = periodic(dx.c_of(kernel) * dx.U * dx.s_plain(dx.head_operand(x, sig).abs(), w.abs()), n)
    hold(kernel, "one sigma" if one_sigma else "sigma per image", shape, mode, launch, ref, bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("one_sigma", [False, True])
@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("form", ["sp16", "p32"])
def test_ffdnet_head_matrix_core(form, measured, one_sigma, mode):
    """ffdnet_head_split16 / ffdnet_head_p32, csrc/conv_s16.hip head_s16_kernel.  EXACT on integer data: 2^e (image | sigma) with
    integers of at most 8 (a scaled image: multiples of 2^-3) is a power of two times an integer of at most seven bits and
    2^sw w (sw = 11) one of three: hi exact, lo 0; 48 * 3 products, the partial sums a power of two times an integer of at most
    45 * 32 * 8 < 2^24; the output an integer (a multiple of 2^-3) below 2^11 at exponent 0, or scaled into [2^11, 2^12): hi + lo
    exactly.  c = 2*3*48."""
    (sname, shape), = dx.shapes_of("head_s16").items()
    n, H, W = shape
    x, sig, w = dx.head_data(shape, mode, 5, measured, one_sigma)
    ref = dx.head_ref(x, sig, w)
    xg, wg, sg = x.to(DEV), w.to(DEV), sig.to(DEV)
    out_exp = 0 if mode == "int" else _hip.SP16_DEFAULT_EXP
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rin, rout = slots(a, x, measured), slots(a, ref, measured)
        Wh = guard_weights(a, _hip.HeadSplit16Weights(wg))
        e_in = [_hip.SP16_DEFAULT_EXP] * n if rin is None else [_hip.act_exp(max(v, abs(float(s)))) for v, s in zip(rin.tolist(), sig.expand(n).tolist())]
        info.update(e_x=e_in, e_w=Wh.sw, e_out=exps(rout, out_exp, n))
        kw = dict(in_rng=rin, out_rng=rout, out_exp=out_exp)
        if form == "sp16":
            o = _hip.Sp16(a.output((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W)
            _hip.ffdnet_head_split16(a.operand(xg), Wh, a.operand(sg), out=o, **kw)
            return o.to_nchw(), [], a
        o = _hip.P32(a.output((n, 8, 2, H, -(-W // 64), 2, 32, 4)), n, H, W)
        _hip.ffdnet_head_p32(a.operand(xg), Wh, a.operand(sg), out=o, **kw)
        return o.to_nchw(), [dx.p32_padding(o)], a
    bound = None
    if mode == "real":
        launch()
        xa = dx.head_operand(x, sig).abs()
        S = dx.s_plain(xa, w.abs())
        bound = split_bound("head_s16", S, S, dx.floor_sums(xa, w.abs().double()), info["e_x"], info["e_w"], info["e_out"] if form == "sp16" else None)
    form_s = f"{form} {'measured' if measured else 'fixed'}, {'one sigma' if one_sigma else 'sigma per image'}"
    hold("head_s16", form_s, shape, mode, launch, ref, bound)


# ----------------------------------------------------------------------------- last layers
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("in_bias", [False, True])
@pytest.mark.parametrize("cout", [4, 1])
def test_tail_valu(cout, in_bias, mode):
    """ffdnet_tail / conv3x3_c64_to_1, csrc/ffdnet_edges.hip edge_tail_kernel, plain and with in_bias (relu(h + b) on the way in).
    EXACT on integer data: h + b is an integer of at most 12, 576 fused multiply-adds, every partial sum an integer of at most
    576 * 12 * 4 = 27648 < 2^24.  c = 9*64, with in_bias 9*64 + 1 on S = conv(|h| + |b|, |w|)."""
    shape = dx.shapes_of("tail_valu")["tail_valu_ffdnet" if cout == 4 else "tail_valu_c1"]
    n, H, W = shape
    h, w, b = dx.tail_data(shape, mode, cout, in_bias, False)
    ref = dx.tail_ref(h, w, b)
    f = 2 if cout == 4 else 1
    hg, bg = dx.cl(h.to(DEV)), None if b is None else b.to(DEV)
    Wg = (_hip.pack_tail_weights if cout == 4 else _hip.pack_c64_to_1_weights)(w.to(DEV))
    fn = _hip.ffdnet_tail if cout == 4 else _hip.conv3x3_c64_to_1

    def launch():
        a = dx.Arena(W, DEV)
        out = a.output((n, 1, f * H, f * W))
        fn(a.operand(hg), a.operand(Wg), out=out, in_bias=a.operand(bg))
        return out, [], a
    bound = None
    if mode == "real":
        S = dx.s_plain(dx.tail_operand(h, b, absolute=True), w.abs())
        bound = dx.c_of("tail_valu", in_bias) * dx.U * (Fn.pixel_shuffle(S, 2) if cout == 4 else S)
    hold("tail_valu", f"cout {cout}{' in_bias' if in_bias else ''}", shape, mode, launch, ref, bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("measured", [False, True])
@pytest.mark.parametrize("form", ["sp16", "p32"])
@pytest.mark.parametrize("cout", [4, 1])
def test_tail_matrix_core(cout, form, measured, mode):
    """tail_split16 / ffdnet_tail_p32, csrc/conv_s16.hip tail_s16_kernel, COUT 4 and 1.  EXACT on integer data: 2^e h and 2^sw w
    (sw = 11) are powers of two times integers of at most seven and three bits: hi exact, lo 0; P[pixel][tap] sums 64 * 3 products,
    a power of two times an integer of at most 64 * 32 * 8; times a power of two, and the nine taps add up to at most 9 * 2048 * 8
    < 2^24.  c = 2*3*64 + 9."""
    shape = dx.shapes_of("tail_s16")["tail_s16_ffdnet" if cout == 4 else "tail_s16_c1"]
    n, H, W = shape
    h, w, _ = dx.tail_data(shape, mode, cout, False, measured)
    ref = dx.tail_ref(h, w, None)
    f = 2 if cout == 4 else 1
    hg, wg = h.to(DEV), w.to(DEV)
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rin = slots(a, h, measured)
        Wt = guard_weights(a, _hip.TailSplit16Weights(wg))
        info.update(e_x=exps(rin, _hip.SP16_DEFAULT_EXP, n), e_w=Wt.sw)
        out = a.output((n, 1, f * H, f * W))
        if form == "sp16":
            hs = _hip.to_split16(a.operand(dx.cl(hg)), out=_hip.Sp16(a.nan((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W), rng=rin)
            _hip.tail_split16(hs, Wt, out=out)
        else:
            hp = dx.p32_fill(_hip.P32(a.nan((n, 8, 2, H, -(-W // 64), 2, 32, 4)), n, H, W, rng=rin), hg)
            _hip.ffdnet_tail_p32(hp, Wt, out=out)
        return out, [], a
    bound = None
    if mode == "real":
        launch()
        S = dx.s_plain(h.abs(), w.abs())
        bound = split_bound("tail_s16", S, S, dx.floor_sums(h.abs().double(), w.abs().double()), info["e_x"], info["e_w"], None)
        bound = Fn.pixel_shuffle(bound, 2) if cout == 4 else bound
    hold("tail_s16", f"cout {cout} {form} {'measured' if measured else 'fixed'}", shape, mode, launch, ref, bound)


# ----------------------------------------------------------------------------- conversion
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("measured", [False, True])
def test_to_split16(measured, mode):
    """to_split16, csrc/conv_s16.hip.  EXACT on integer data: 2^8 x (measured: the power of two that puts the image's maximum into
    [2^11, 2^12)) of an integer of at most four bits is hi alone, lo 0, and Sp16.to_nchw returns it.  Real data: per element
    max(2^-22 |x|, 2^(-25 - e)), the rule of DESIGN.md section 5, and nothing else (c = 0)."""
    shape = dx.shapes_of("to_split16")["s16"]
    n, H, W = shape
    x = dx.conv64_data(shape, mode, 1, False, measured)[0]
    xg = dx.cl(x.to(DEV))
    info = {}

    def launch():
        a = dx.Arena(W, DEV)
        rin = slots(a, x, measured)
        info.update(e_x=exps(rin, _hip.SP16_DEFAULT_EXP, n))
        o = _hip.to_split16(a.operand(xg), out=_hip.Sp16(a.output((n, 4, 2, 2, H, W, 8), torch.float16), n, H, W), rng=rin)
        return o.to_nchw(), [], a
    bound = None
    if mode == "real":
        launch()
        bound = dx.split_rule(x.abs(), info["e_x"])
    hold("to_split16", "measured" if measured else "fixed", shape, mode, launch, x.double(), bound)
