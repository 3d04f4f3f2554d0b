"""NaN and Inf in the input of every convolution, edge and epilogue kernel of the denoiser, against float64 torch on the same poisoned
operands (tests/nonfinite_ref.py).  DESIGN.md: a non-finite activation "stays inf/NaN to the output ... never a silently wrong number".

Three exact properties per kernel, form, poison value (NaN, +Inf, -Inf), position (nonfinite_ref.positions: corners, both sides of the seam
between two images, both sides of every seam of the kernel's tiling) and channel (0, 31, 63 where the operand has channels: all three for
NaN, one of them - cycling with the position - for the infinities):
  P1  nothing swallowed: wherever the reference is non-finite the kernel's output is non-finite, and NaN wherever the reference is NaN
      (given a NaN poison);
  P2  nothing leaks: outside nonfinite_ref.reach, and in every other image, the output has the bits of the same launch on the clean input;
  P3  repeatable: a second launch on the poisoned input gives the same bits, NaN positions included.
Every run first asserts that the reference's non-finite set is not empty (tests/test_nonfinite_host.py holds the other caps on the table).
Exponents of the fp16-piece layouts are fixed (2^8, data of a few units) or, in the engine's f-calls, measured on the clean input and
reused.  A case reports every (property, run) that fails, not the first.

Before the ReLUs of the fp32 kernels became NaN-propagating (fmaxf is maxNum: ReLU(NaN) = 0), P1 is what the cases that run a ReLU through
csrc/ffdnet_edges.hip, csrc/winograd.hip, csrc/winograd44.hip or csrc/epilogue.hip could not hold; profiles/nonfinite.md has the table."""
import functools
import itertools
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import nonfinite_ref as nf

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import deqsci_amd
    from deqsci_amd import _hip, checkpoint
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.engine import DEQSCIEngine
    from oracle import deqsci_oracle as orc

DEV = "cuda"
NAN = float("nan")


def bits(t):
    """The bit patterns of a float tensor in NCHW order (torch.equal on floats would call NaN != NaN)."""
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def weights(cout, cin, seed, scale=0.05):
    w = torch.randn(cout, cin, 3, 3, device=DEV, generator=gen(seed)) * scale
    return torch.where(w.abs() < 1e-4, torch.full_like(w, scale), w)          # all nonzero: every tap carries the poison


def runs_of(name, channels):
    """(position, channel, poison name) of every run of a case."""
    out = []
    for k, pos in enumerate(nf.case_positions(name)):
        for ch in channels:
            out.append((pos, ch, "nan"))
        for val in ("+inf", "-inf"):
            out.append((pos, channels[k % len(channels)], val))
    return out


def check_case(name, x_clean, run, ref, channels=(0,), values=("nan", "+inf", "-inf"), ref_images=None, extra=None):
    """P1-P3 of one kernel form.  x_clean: the fp32 operand the poison goes into, (n,C,h,w) on the grid nonfinite_ref.case_poison names;
    run(x) -> the kernel's output as an fp32 (n,Co,Ho,Wo) tensor; ref(x) -> the float64 reference of the same shape on the CPU (of the
    images ref_images only, when given: the others must then be bit-clean); extra(got, x_poisoned): further (label, bool tensor) checks."""
    clean = run(x_clean)
    assert bool(torch.isfinite(clean).all())
    failed = []
    for pos, ch, vname in runs_of(name, channels):
        if vname not in values:
            continue
        poison = nf.case_poison(name, pos)
        (i, r, c), = poison.nonzero().tolist()
        x = x_clean.clone()
        x[i, ch, r, c] = nf.POISONS[vname]
        got, again = run(x), run(x)
        imgs = list(range(x.shape[0])) if ref_images is None else ref_images
        assert pos[0] in imgs
        want = ref(x[imgs])
        bad_ref, nan_ref = ~torch.isfinite(want), torch.isnan(want)
        assert bool(bad_ref.any()), (name, pos, ch, vname, "the reference has no non-finite value: the run would prove nothing")
        g = got[imgs]
        checks = [("P1 swallowed", bool((~torch.isfinite(g))[bad_ref.to(DEV)].all()))]
        if vname == "nan":
            checks.append(("P1 NaN became another value", bool(torch.isnan(g)[nan_ref.to(DEV)].all())))
        outside = ~nf.case_reach(name, poison).to(DEV)                          # (n, Ho, Wo): every channel of a pixel alike
        checks.append(("P2 leaked", not bool(((bits(got) != bits(clean)) & outside[:, None]).any())))
        checks.append(("P3 not repeatable", same_bits(got, again)))
        if extra is not None:
            checks += extra(got, x)
        failed += [(label, pos, ch, vname) for label, ok in checks if not ok]
    assert not failed, f"{name}: {len(failed)} failures: " + "; ".join(f"{l} at {p} ch {c} {v}" for l, p, c, v in failed[:40])


def act(name, seed, signed=False):
    """A 64-channel clean activation on the case's grid: ReLU-like (>= 0, a few units) or signed (a raw convolution output)."""
    n, H, W = nf.CASES[name]["shape"]
    x = torch.randn(n, 64, H, W, device=DEV, generator=gen(seed)) if signed else torch.rand(n, 64, H, W, device=DEV, generator=gen(seed))
    return cl(x)


def image(name, seed):
    n, H, W = nf.CASES[name]["shape"]
    f = 2 if nf.CASES[name]["src"] == "full" else 1
    return torch.rand(n, 1, f * H, f * W, device=DEV, generator=gen(seed))


BIAS_RELU = [(False, False), (True, True), (False, True)]


# ----------------------------------------------------------------------------- 64 -> 64, single launches
@pytest.mark.parametrize("use_bias,relu", BIAS_RELU)
def test_winograd_f22(use_bias, relu):
    w, b = weights(64, 64, 1), (torch.randn(64, device=DEV, generator=gen(2)) * 0.3 if use_bias else None)
    U = _hip.pack_winograd_weights(w)
    check_case("f22", act("f22", 3), lambda x: _hip.conv3x3_c64_winograd(cl(x), U, b, relu),
               lambda x: nf.conv_ref(x, w, b, relu), nf.CHANNELS)


@pytest.mark.parametrize("in_blk,out_blk", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("use_bias,relu", [(False, False), (True, True)])
def test_winograd_f44(in_blk, out_blk, use_bias, relu):
    w, b = weights(64, 64, 4), (torch.randn(64, device=DEV, generator=gen(5)) * 0.3 if use_bias else None)
    U = _hip.pack_winograd44_weights(w)

    def run(x):
        o = _hip.conv3x3_c64_winograd44(_hip.Blk32.from_nchw(x) if in_blk else cl(x), U, b, relu, out_blk=out_blk)
        return o.to_nchw() if out_blk else o
    check_case("f44", act("f44", 6), run, lambda x: nf.conv_ref(x, w, b, relu), nf.CHANNELS)


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("use_bias,relu", [(False, False), (True, True)])
def test_split16(out_f32, use_bias, relu):
    w, b = weights(64, 64, 7), (torch.randn(64, device=DEV, generator=gen(8)) * 0.3 if use_bias else None)
    W16 = _hip.Split16Weights(w)

    def run(x):
        o = _hip.conv3x3_c64_split16(_hip.to_split16(cl(x)), W16, b, relu, out_f32=out_f32)
        return o if out_f32 else o.to_nchw()
    check_case("s16", act("s16", 9), run, lambda x: nf.conv_ref(x, w, b, relu), nf.CHANNELS)


@pytest.mark.parametrize("use_bias,relu", [(False, False), (True, True)])
def test_wino16(use_bias, relu):
    w, b = weights(64, 64, 10), (torch.randn(64, device=DEV, generator=gen(11)) * 0.3 if use_bias else None)
    Ww = _hip.Wino16Weights(w)
    check_case("w16", act("w16", 12), lambda x: _hip.conv3x3_c64_wino16(_hip.P32.from_nchw(x), Ww, b, relu).to_nchw(),
               lambda x: nf.conv_ref(x, w, b, relu), nf.CHANNELS)


# ----------------------------------------------------------------------------- 64 -> 64, stack launches
STACK = {"s16": ("s16", lambda: (_hip.Split16Weights, _hip.Split16Stack, _hip.conv3x3_c64_split16_stack, _hip.conv3x3_c64_split16,
                                 lambda x: _hip.to_split16(cl(x)))),
         "w16": ("w16", lambda: (_hip.Wino16Weights, _hip.Wino16Stack, _hip.conv3x3_c64_wino16_stack, _hip.conv3x3_c64_wino16,
                                 lambda x: _hip.P32.from_nchw(x)))}


@pytest.mark.parametrize("kernel", ["s16", "w16"])
def test_stack_launch_of_three_layers(kernel):
    """Non-finite values are DATA to a stack launch: the bits of the three per-layer launches on the poisoned input, P1 against the
    three-layer float64 reference, the clean image untouched, and no wait gave up."""
    name, get = STACK[kernel]
    Wcls, Scls, launch, single, to_act = get()
    ws = [weights(64, 64, 20 + i) for i in range(3)]
    bs = [torch.randn(64, device=DEV, generator=gen(30 + i)) * 0.3 for i in range(3)]
    packs = [Wcls(w) for w in ws]
    stack = Scls([(p, b, True) for p, b in zip(packs, bs)], DEV)
    x_clean = act(name, 13)
    clean = launch(to_act(x_clean), stack).to_nchw()
    assert bool(torch.isfinite(clean).all())
    failed = []
    for k, pos in enumerate(nf.case_positions(name)):
        for vname in ("nan", "+inf", "-inf"):
            x = x_clean.clone()
            x[pos[0], nf.CHANNELS[k % 3], pos[1], pos[2]] = nf.POISONS[vname]
            got = launch(to_act(x), stack).to_nchw()
            h = to_act(x)
            for p, b in zip(packs, bs):
                h = single(h, p, b, True)
            want = nf.stack_ref(x, [(w, b, True) for w, b in zip(ws, bs)])
            bad = ~torch.isfinite(want)
            assert bool(bad.any())
            checks = [("stack != per-layer launches", same_bits(got, h.to_nchw())),
                      ("P1 swallowed", bool((~torch.isfinite(got))[bad.to(DEV)].all())),
                      ("clean image touched", same_bits(got[1 - pos[0]], clean[1 - pos[0]]))]
            if vname == "nan":
                checks.append(("P1 NaN became another value", bool(torch.isnan(got)[torch.isnan(want).to(DEV)].all())))
            failed += [(label, pos, vname) for label, ok in checks if not ok]
    assert not stack.timed_out()
    assert not failed, failed[:40]


@pytest.mark.parametrize("as_stack", [False, True])
def test_wino16_overflow_is_loud(as_stack):
    """test_split16_overflow_is_loud for the Winograd kernel: activations beyond fp16's range under the fixed exponent 2^8 must end as
    inf / NaN behind three layers (the p32 store itself is fp32: the NEXT layer's split overflows), never as a wrong finite number."""
    x = cl(torch.rand(1, 64, 16, 64, device=DEV, generator=gen(5)) * 40.0)
    w0 = torch.ones(64, 64, 3, 3, device=DEV) * 0.5                           # y ~ 64 * 9 * 20 * 0.5 = 5760 >> 255
    w1 = torch.randn(64, 64, 3, 3, device=DEV, generator=gen(6)) * 0.05
    layers = [(_hip.Wino16Weights(w), torch.zeros(64, device=DEV), True) for w in (w0, w1, w1)]
    xp = _hip.P32.from_nchw(x)
    if as_stack:
        stack = _hip.Wino16Stack(layers, DEV)
        out = _hip.conv3x3_c64_wino16_stack(xp, stack).to_nchw()
        assert not stack.timed_out()
    else:
        h = xp
        for p, b, relu in layers:
            h = _hip.conv3x3_c64_wino16(h, p, b, relu)
        out = h.to_nchw()
    assert not bool(torch.isfinite(out).all())
    want = nf.stack_ref(x, [(w0, None, True), (w1, None, True), (w1, None, True)])
    assert bool(torch.isfinite(want).all())                                   # (fp32's range holds it: only the fp16 pieces overflow)


# ----------------------------------------------------------------------------- heads
def _sigma(n):
    return torch.linspace(0.05, 0.2, n, device=DEV)


def _sigma_nan(run, x, sig, img):
    """A NaN in one image's sigma: that whole image is NaN, as in the reference (the sigma map reaches every window), the others bit-clean."""
    clean = run(x, sig)
    s = sig.clone()
    s[img] = NAN
    got = run(x, s)
    others = [i for i in range(x.shape[0]) if i != img]
    assert bool(torch.isnan(got[img]).all()), "a NaN sigma left finite values in its image"
    assert same_bits(got[others], clean[others])


def test_ffdnet_head_valu():
    n = nf.CASES["head_valu"]["shape"][0]
    w, sig = weights(64, 5, 40), _sigma(n)
    Wp = _hip.pack_head_weights(w)
    x = image("head_valu", 41)
    check_case("head_valu", x, lambda x: _hip.ffdnet_head(x, Wp, sig), lambda x: nf.ffdnet_head_ref(x, sig, w))
    _sigma_nan(lambda x, s: _hip.ffdnet_head(x, Wp, s), x, sig, 1)


def test_ffdnet_head_mfma():
    """The matrix-core form of the fp32 head is picked from two tiles per CU on: the existing (130, 128, 128) launch, one poison set
    where a row seam and a column seam of its tiling meet; the float64 reference of the poisoned image and its two neighbours."""
    n, H, W = nf.CASES["head_mfma"]["shape"]
    assert -(-W // 32) * -(-H // 32) * n >= 2 * torch.cuda.get_device_properties(0).multi_processor_count
    w, sig = weights(64, 5, 42), _sigma(n)
    Wp = _hip.pack_head_weights(w)
    x = image("head_mfma", 43)
    imgs = [76, 77, 78]
    check_case("head_mfma", x, lambda x: _hip.ffdnet_head(x, Wp, sig), lambda x: nf.ffdnet_head_ref(x, sig[imgs], w), ref_images=imgs)
    _sigma_nan(lambda x, s: _hip.ffdnet_head(x, Wp, s), x, sig, 77)


@pytest.mark.parametrize("form", ["sp16", "p32"])
def test_ffdnet_head_matrix_core(form):
    n = nf.CASES["head_s16"]["shape"][0]
    w, sig = weights(64, 5, 44), _sigma(n)
    Wh = _hip.HeadSplit16Weights(w)
    fn = _hip.ffdnet_head_split16 if form == "sp16" else _hip.ffdnet_head_p32
    x = image("head_s16", 45)
    check_case("head_s16", x, lambda x: fn(x, Wh, sig).to_nchw(), lambda x: nf.ffdnet_head_ref(x, sig, w))
    _sigma_nan(lambda x, s: fn(x, Wh, s).to_nchw(), x, sig, 0)


@pytest.mark.parametrize("form", ["fp32", "sp16", "p32"])
@pytest.mark.parametrize("relu", [False, True])
def test_conv_c1_to_64(form, relu):
    w = weights(64, 1, 46, 0.3)
    Wp = _hip.pack_c1_to_64_weights(w)

    def run(x):
        o = _hip.conv3x3_c1_to_64(x, Wp, relu=relu, sp16=form == "sp16", p32=form == "p32")
        return o if form == "fp32" else o.to_nchw()
    check_case("c1_to_64", image("c1_to_64", 47), run, lambda x: nf.conv_ref(x, w, None, relu))


def _random_mask(n, H, W, seed):
    return torch.rand(n, 64, H, W, device=DEV, generator=gen(seed)) < 0.5


def _cleared_is_zero(mbits):
    return lambda got, x: [("a value under a cleared mask bit", bool((got[~mbits] == 0).all()))]


# ----------------------------------------------------------------------------- masked layers (a select: NaN under a cleared bit is 0)
def test_conv_c1_to_64_masked():
    n, H, W = nf.CASES["c1_to_64"]["shape"]
    w = weights(64, 1, 48, 0.3)
    Wp, mbits = _hip.pack_c1_to_64_weights(w), _random_mask(n, H, W, 49)
    mask = nf.pack_mask(mbits)
    check_case("c1_to_64", image("c1_to_64", 50), lambda x: _hip.conv3x3_c1_to_64_masked(x, Wp, mask),
               lambda x: nf.conv_ref(x, w, mask=mbits), extra=_cleared_is_zero(mbits))


def test_winograd_masked():
    n, H, W = nf.CASES["f22"]["shape"]
    w = weights(64, 64, 51)
    U, mbits = _hip.pack_winograd_weights(w), _random_mask(n, H, W, 52)
    mask = nf.pack_mask(mbits)
    check_case("f22", act("f22", 53, signed=True), lambda x: _hip.conv3x3_c64_winograd_masked(cl(x), U, mask),
               lambda x: nf.conv_ref(x, w, mask=mbits), nf.CHANNELS, extra=_cleared_is_zero(mbits))


def test_ffdnet_head_masked():
    """csrc/jacobian.hip's masked head: the select of the other masked layers."""
    n, H, W = nf.CASES["head_valu"]["shape"]
    w = weights(64, 4, 54, 0.3)
    Wp, mbits = _hip.pack_head_masked_weights(w), _random_mask(n, H, W, 55)
    mask = nf.pack_mask(mbits)
    check_case("head_valu", image("head_valu", 56), lambda x: _hip.ffdnet_head_masked(x, Wp, mask),
               lambda x: nf.ffdnet_head_ref(x, None, w, relu=False, mask=mbits, with_sigma=False), extra=_cleared_is_zero(mbits))


# ----------------------------------------------------------------------------- tails
# (with in_bias the tail reads relu(h + b): -Inf becomes 0 there and the reference stays finite - no non-finite set, nothing to hold)
@pytest.mark.parametrize("cout", [4, 1])
@pytest.mark.parametrize("in_bias", [False, True])
def test_tail_valu(cout, in_bias):
    name = "tail_valu_ffdnet" if cout == 4 else "tail_valu_c1"
    w = weights(cout, 64, 60)
    b = torch.randn(64, device=DEV, generator=gen(61)) * 0.3 if in_bias else None
    Wp = (_hip.pack_tail_weights if cout == 4 else _hip.pack_c64_to_1_weights)(w)
    fn = _hip.ffdnet_tail if cout == 4 else _hip.conv3x3_c64_to_1
    check_case(name, act(name, 62, signed=in_bias), lambda x: fn(cl(x), Wp, in_bias=b), lambda x: nf.tail_ref(x, w, b, shuffle=cout == 4),
               nf.CHANNELS, values=("nan", "+inf") if in_bias else ("nan", "+inf", "-inf"))


@pytest.mark.parametrize("cout", [4, 1])
@pytest.mark.parametrize("form", ["sp16", "p32"])
def test_tail_matrix_core(cout, form):
    name = "tail_s16_ffdnet" if cout == 4 else "tail_s16_c1"
    w = weights(cout, 64, 63)
    Wt = _hip.TailSplit16Weights(w)

    def run(x):
        return _hip.tail_split16(_hip.to_split16(cl(x)), Wt) if form == "sp16" else _hip.ffdnet_tail_p32(_hip.P32.from_nchw(x), Wt)
    check_case(name, act(name, 64), run, lambda x: nf.tail_ref(x, w, shuffle=cout == 4), nf.CHANNELS)


# ----------------------------------------------------------------------------- bias_relu_
@pytest.mark.parametrize("layout,shape", [("nchw", (2, 3, 36, 36)), ("channels_last", (2, 12, 5, 7))])
@pytest.mark.parametrize("relu", [True, False])
def test_bias_relu_epilogue(layout, shape, relu):
    """NCHW with two blocks per plane (36 * 36 / 4 > 256 lanes) and channels_last with C = 12: the NaN set equals torch's and every
    other element is equal."""
    h0 = torch.randn(shape, device=DEV, generator=gen(70))
    b = torch.randn(shape[1], device=DEV, generator=gen(71))
    flat = [0, 1023, 1024, 1295, 1296, h0.numel() - 1] if layout == "nchw" else [0, 11, 12, 419, 420, h0.numel() - 1]
    for k, vname in itertools.product(flat, nf.POISONS):
        h = h0.clone()
        h.view(-1)[k] = nf.POISONS[vname]
        want = h + b.view(1, -1, 1, 1)
        want = torch.relu(want) if relu else want
        hin = cl(h) if layout == "channels_last" else h.clone()
        got = _hip.bias_relu_(hin, b, relu)
        assert bool((~torch.isfinite(want)).any()) == (not (relu and vname == "-inf"))
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (k, vname)
        assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)), (k, vname)
        assert same_bits(got, _hip.bias_relu_(cl(h) if layout == "channels_last" else h.clone(), b, relu))


# ----------------------------------------------------------------------------- one f-call per engine path
DNCNN17 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dncnn_noise15.npz")
# path -> (build_pipeline's denoiser, weights, _hip.FORCE_CONV64 (64 x 64 frames take F(2x2,3x3) under every default policy: the
# split-fp16 paths are pinned as tests/test_denoiser_launches_gpu.py pins them), DEQSCIEngine's keywords, den.last_path)
FCALLS = {
    "ffdnet-w16-stack": ("ffdnet", "ffdnet_gray", "s16", {}, "w16 stack launch"),
    "ffdnet-s16-stack": ("ffdnet", "ffdnet_gray", "s16", {"stack_kernel": "s16"}, "s16 stack launch"),
    "ffdnet-per-layer": ("ffdnet", "ffdnet_gray", "s16", {"stack": False}, "per layer"),
    "ffdnet-fast32": ("ffdnet", "ffdnet_gray", None, {"conv64": "fast32"}, "per layer"),
    "ffdnet-fast32-f44": ("ffdnet", "ffdnet_gray", "f44", {"conv64": "fast32"}, "per layer"),
    "ffdnet-torch-edges": ("ffdnet", "ffdnet_gray", None, {"fused_edges": False}, "per layer"),
    "cnn-default": ("SimpleCNN", "cnn", "s16", {}, "w16 per layer"),
    "cnn-s16": ("SimpleCNN", "cnn", "s16", {"stack_kernel": "s16"}, "per layer"),
    "cnn-fast32": ("SimpleCNN", "cnn", None, {"conv64": "fast32"}, "per layer"),
    "cnn-fast32-f44": ("SimpleCNN", "cnn", "f44", {"conv64": "fast32"}, "per layer"),
    "dncnn17-w16-stack": ("DnCNN", None, "s16", {}, "w16 stack launch"),
}


@functools.lru_cache(maxsize=None)
def _net(kind, wname):
    return build_pipeline(kind, DNCNN17 if wname is None else checkpoint.shipped(wname), 8)[0].nonlinear_op


@functools.lru_cache(maxsize=None)
def _crop(bsz):
    """bsz measurements of 64 x 64 x 8 (the crop of __graft_entry__.smoke) -> (y (bsz,64,64), Phi (1,64,64,8)) on the CPU."""
    d = orc.load_clip(os.path.join(orc.DATA_DIR, "traffic_cacti.mat"))
    sl = (slice(96, 160), slice(64, 128))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"][sl]))[None]
    y = torch.from_numpy(np.ascontiguousarray(np.moveaxis(d["meas"][sl][..., :bsz], -1, 0)))
    return y, Phi


def _module_f64(den, x, sigma):
    """The float64 module on the f-call's input x (n,1,H,W): den.fast's layers, FFDNet's concatenate and pixel shuffle around them."""
    h = x.double().cpu()
    if den.edges.ffdnet:
        h = Fn.pixel_unshuffle(h, 2)
        h = torch.cat((sigma.double().cpu().view(1, 1, 1, 1).expand(h.shape[0], 1, h.shape[2], h.shape[3]), h), 1)
    h = nf.stack_ref(h, den.fast)
    return Fn.pixel_shuffle(h, 2) if den.edges.ffdnet else h


@pytest.mark.parametrize("path", list(FCALLS))
def test_fcall_on_a_poisoned_frame(path):
    """Ranges measured on the clean input (f-call 0) and reused, as test_ranges_of_the_first_call_serve_the_whole_loop does; then one
    NaN in one frame of z: P1 on that frame against the float64 module, the other seven frames the bits of the clean call."""
    kind, wname, pin, ctor, last_path = FCALLS[path]
    net = _net(kind, wname)
    y, Phi = _crop(1)
    z = deqsci_amd.initial_point(y.to(DEV), Phi.to(DEV), None, None).permute(0, 3, 1, 2).contiguous()      # (1, 8, 64, 64)
    old, _hip.FORCE_CONV64 = _hip.FORCE_CONV64, pin
    try:
        den = DEQSCIEngine(net, max_iter=8, use_graph=False, **ctor).den
        den.prepare(16, DEV, n_img=8)
        den.run(z, 0, calibrate=True)
        r0 = None if den.ranges is None else den.ranges.clone()
        clean = den.run(z, 1)[0].clone()
        assert den.last_path == last_path and bool(torch.isfinite(clean).all())
        zp = z.clone()
        zp[0, 3, 21, 42] = NAN
        got = den.run(zp, 1)[0].clone()
        again = den.run(zp, 1)[0].clone()
        assert not den.stack_timed_out() and (r0 is None or torch.equal(den.ranges, r0))
    finally:
        _hip.FORCE_CONV64 = old
    sigma = den.sigma_table[1:2] if den.edges.ffdnet else None
    want = _module_f64(den, zp[0, 3][None, None], sigma)[0, 0]
    assert bool(torch.isnan(want).any())
    assert bool(torch.isnan(got[0, 3])[torch.isnan(want).to(DEV)].all()), "a NaN of the reference came out as a number"
    others = [f for f in range(8) if f != 3]
    assert same_bits(got[0, others], clean[0, others]), "a clean frame changed"
    assert same_bits(got, again)


# ----------------------------------------------------------------------------- two iterations end to end
@pytest.mark.parametrize("kind,wname", [("SimpleCNN", "cnn"), ("ffdnet", "ffdnet_gray")])
def test_two_picard_iterations_with_a_nan_pixel_in_y(kind, wname):
    """reconstruct, Picard, 2 iterations, two measurements, one NaN pixel in y[0]: wherever the CPU oracle's result is non-finite the
    engine's is, and measurement 1 comes out with the bits it has in the clean batch."""
    y, Phi = _crop(2)
    yp = y.clone()
    yp[0, 30, 17] = NAN
    Ps = orc.phi_sum(Phi)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want, _ = orc.deq_forward(orc.ProxGradSCI(kind), orc.forward_iteration, yp, Phi, Ps, orc.initial_point(yp, Phi), max_iter=2, tol=1e-5)
        eng = DEQSCIEngine(_net(kind, wname), iterator="picard", max_iter=2, use_graph=False)
        clean = eng.reconstruct(y.to(DEV), Phi.to(DEV)).clone()
        got = eng.reconstruct(yp.to(DEV), Phi.to(DEV)).clone()
    bad = ~torch.isfinite(want)
    assert bool(bad[0].any()) and bool(torch.isfinite(clean).all())
    assert got.shape == want.shape and bool((~torch.isfinite(got))[bad.to(DEV)].all()), "the oracle's non-finite values came out finite"
    assert same_bits(got[1], clean[1]), "the clean measurement of the batch changed"
