"""tests/denoiser_exact_ref.py held to account without a GPU: the reference implementation alone - CPU fp32 conv2d, a torch emulation of
the fp16 split - must pass the gates tests/test_denoiser_exact_gpu.py holds the kernels to, on the same seeded data; the integer data
must satisfy the caps that keep (a) from passing vacuously; the Winograd propagation must be the kernels' algebra and dominate the
direct sum's S; and the table must cover every forward entry point of _hip.SIGNATURES at shapes that are ragged as claimed."""
import itertools

import pytest
import torch
import torch.nn.functional as Fn

import denoiser_exact_ref as dx
import nonfinite_ref as nf
from deqsci_amd import _hip

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
