"""The denoiser's forward kernels, and the masked kernels its backward and Jacobian products run through, element by element: stated
once for tests/test_denoiser_exact_host.py (this helper against itself and CPU fp32), tests/test_denoiser_exact_gpu.py (the forward
kernels) and tests/test_backward_exact_gpu.py (the masked kernels, the transposed packs vjp._MaskedStack builds, one whole masked
stack).  A helper module, not a test.  Shapes and seams: tests/nonfinite_ref.py.

(a) EXACT.  Integer operands - x in [-8, 8] with a seeded quarter exactly 0, weights in [-4, 4] without 0 (times KERNELS[k]["wmult"]
    where a transform divides), integer bias and sigma - make every product and every partial sum of a kernel an integer (or one
    power of two times an integer) below 2^24: fp32 holds them all, in any order of summation and under any rounding of the matrix
    cores' accumulators, so the kernel must return the float64 reference's value bit for bit (torch.equal).  The per-kernel argument
    is the docstring of the case in tests/test_denoiser_exact_gpu.py; check_caps below is what keeps the data from passing vacuously.
(b) BOUND.  x = randn, w = 0.05 randn (signed: sums cancel); for every output element
        |got - ref64| <= c 2^-24 S + rep
    S: the same operation in float64 on |x|, |w|, |bias| (s_plain), or for a Winograd kernel the absolute-value propagation of its own
    transforms |A^T| [ (|G| |w| |G^T|) . (|B^T| |x| |B|) ] |A| summed over the input channels (s_wino): the quantity its roundings are
    relative to.  c: KERNELS[k]["c"], an expression COUNTED from the kernel's code (one rounding per fused multiply-add, per addition
    of a transform on its longest path, per fp32 rounding of a host-transformed weight; an accumulation on the matrix cores, whose
    rounding neither the code nor the guides state: 2 per accumulated product, which allows truncation).  rep, the split-fp16 forms
    only (csrc/common.hpp): an operand a is held as hi + lo with |a - hi - lo| <= 2^-22 |a|, or 2^(-25 - e)
    where the lo piece is subnormal (e the operand's exponent: with 2^e max|a| in [2^11, 2^12) that is 2^-36 of the maximum), and the
    lo . lo product is dropped (<= 2^-22 |x| |w|): rep = (3 2^-22 S + floors)(1 + 2^-10), the last factor for the products of two errors.
    An sp16 OUTPUT adds its own split: 2^-22 |y| + 2^(-25 - e_out).  No atol, nothing fitted.
(c) GUARDS.  Arena: every operand a view inside a buffer of NaN, every output a view pre-filled with NaN inside a buffer of sentinels;
    guards of at least two image rows of 64 channels, a multiple of 256 bytes.
A MASKED kernel is the unmasked sum behind a select (mask ? v : 0; nonfinite_ref.conv_ref(mask=)): (a) on the same integer data under a
mask drawn on the CPU (mask_bits; check_masked_caps keeps it from passing vacuously), (b) the unmasked kernel's c 2^-24 S times the mask -
an element under a cleared bit must equal 0 -, (c) with the int64 mask words inside guard words that are all ones in the case's first
launch and all zeros in its second (Arena.words)."""
import functools
import itertools
import math

import torch
import torch.nn.functional as Fn

import nonfinite_ref as nf
from deqsci_amd import vjp as _vjp

U = 2.0 ** -24
SENTINEL = -7776.0                # (a multiple of 4: the same number in fp16)
MANY = (300, 16, 16)              # more block tiles than persistent workgroups (one per CU, 256 CUs), runs of tiles crossing images
ONE = (1, 1, 1)
HEAD_MFMA_RAGGED = (128, 33, 35)  # the matrix-core head's launch threshold (2 tiles of 32 x 32 per CU) at a ragged size: 4 tiles per image

# ----------------------------------------------------------------------------- the kernels, their entry points, their constants
# symbols: the entries of _hip.SIGNATURES the case launches.  nf: the shapes' names in nonfinite_ref.CASES.  c: rounding count (the
# expression and where each term comes from).  wino: (rows, columns) of the output tile of its Winograd transform, None = a direct sum.
# wmult: what integer weights are multiplied by so that the weight transform stays integer.  exact: (a) holds (else: why not).
KERNELS = {
    "f22": dict(symbols=("deqsci_conv3x3_c64_winograd_f32",), nf=("f22",), wino=(2, 2), wmult=4, exact=True,
                # csrc/winograd.hip: transform() 2 additions deep (rows, columns); pack_winograd_weights rounds U once; 64 products
                # accumulated by v_mfma_f32_16x16x4_f32 (the bias is the accumulator's first value); epilogue (m0+m1)+m2 twice: 4
                c="2 + 1 + 2*64 + 4"),
    "f44": dict(symbols=("deqsci_conv3x3_c64_winograd44_layout_f32",), nf=("f44",), wino=(4, 4), wmult=None,
                exact="G of F(4x4,3x3) divides by 6 and 24 on each side: integer U needs weights that are multiples of 576, and then "
                      "max |U| 576 x max |V| 100 * 8 x 64 channels = 2.9e7 > 2^24 - no integer data keeps every partial sum exact "
                      "under a worst-case argument; held by (b) and (c)",
                # csrc/winograd44.hip: bt_lo / bt_hi 2 roundings deep per pass (fma, fma | fma, add); U rounded once; 64 products on the
                # matrix cores; epilogue per pass 3 deep (a = m1+m2, (m0+a)+cc | d, fma, + m5; then s, W0+s, += the partner wave's half)
                c="2*2 + 1 + 2*64 + 2*3"),
    "s16": dict(symbols=("deqsci_conv3x3_c64_split16",), nf=("s16",), wino=None, wmult=1, exact=True, split=True,
                # csrc/conv_s16.hip: 3 products (hi hi, hi lo, lo hi) x 9 taps x 64 channels on v_mfma_f32_32x32x16_f16 in two chains;
                # epilogue fma(a0 + a1, 2^k, 2^e bias): one addition, one fma
                c="2*3*9*64 + 2"),
    "w16": dict(symbols=("deqsci_conv3x3_c64_wino16",), nf=("w16",), wino=(1, 2), wmult=2, exact=True, split=True,
                # csrc/conv_w16.hip: V one v_sub / v_add; Wino16Weights rounds U = G w to fp32 once; 3 products x 3 rows x 64 channels
                # per M[xi]; epilogue (m0+m1)+m2: 2; fma(., 2^k, 2^e bias): 1
                c="1 + 1 + 2*3*3*64 + 2 + 1"),
    # csrc/ffdnet_edges.hip conv_c1_to_64_kernel: nine fma4 from zero; the sp16 / p32 stores scale by a power of two
    "c1_to_64": dict(symbols=("deqsci_conv3x3_c1_to_64_f32", "deqsci_conv3x3_c1_to_64_sp16", "deqsci_conv3x3_c1_to_64_p32"),
                     nf=("c1_to_64",), wino=None, wmult=1, exact=True, c="9"),
    # ffdnet_head_kernel<16>: 9 sigma taps + 36 image taps, each one v_pk_fma_f32
    "head_valu": dict(symbols=("deqsci_ffdnet_head_f32",), nf=("head_valu",), wino=None, wmult=1, exact=True, c="45"),
    # ffdnet_head_mfma_kernel: 12 k-steps of v_mfma_f32_16x16x4_f32 = 48 accumulated products (3 of them zero)
    "head_mfma": dict(symbols=("deqsci_ffdnet_head_f32",), nf=("head_mfma",), wino=None, wmult=1, exact=True, c="2*48"),
    # csrc/conv_s16.hip head_s16_kernel: 3 products x 48 (45 taps padded) on v_mfma_f32_32x32x16_f16; in / out scales are powers of two
    "head_s16": dict(symbols=("deqsci_ffdnet_head_split16", "deqsci_ffdnet_head_p32"), nf=("head_s16",), wino=None, wmult=1, exact=True,
                     split=True, c="2*3*48"),
    # edge_tail_kernel: 9 taps x 64 channels of fmaf; in_bias: one more rounding in relu(h + b)
    "tail_valu": dict(symbols=("deqsci_ffdnet_tail_f32", "deqsci_conv3x3_c64_to_1_f32"), nf=("tail_valu_ffdnet", "tail_valu_c1"), wino=None,
                      wmult=1, exact=True, c="9*64", c_in_bias="9*64 + 1"),
    # tail_s16_kernel: P[pixel][tap] = 3 products x 64 channels on the matrix cores, then o += P over nine taps
    "tail_s16": dict(symbols=("deqsci_ffdnet_tail_split16", "deqsci_conv3x3_c64_to_1_split16", "deqsci_ffdnet_tail_p32",
                              "deqsci_conv3x3_c64_to_1_p32"), nf=("tail_s16_ffdnet", "tail_s16_c1"), wino=None, wmult=1, exact=True, split=True,
                     c="2*3*64 + 9"),
    # f32_to_split16: held to the representation rule directly (no sum: c = 0)
    "to_split16": dict(symbols=("deqsci_f32_to_split16",), nf=("s16",), wino=None, wmult=1, exact=True, split=True, c="0"),
    # ---- the masked kernels of the backward and of the Jacobian products (tests/test_backward_exact_gpu.py): y = mask ? conv : 0, no bias,
    # no ReLU; the select rounds nothing, so c is the sum's alone
    # csrc/winograd.hip winograd_conv64_body<MASK = 1>: the same body as "f22" - transform() 2 additions deep, U rounded once by
    # pack_winograd_weights, 64 products on v_mfma_f32_16x16x4_f32 (from zero: no bias), epilogue (m0+m1)+m2 twice: 4
    "f22_masked": dict(symbols=("deqsci_conv3x3_c64_winograd_masked_f32",), nf=("f22",), wino=(2, 2), wmult=4, exact=True,
                       c="2 + 1 + 2*64 + 4"),
    # csrc/ffdnet_edges.hip conv_c1_to_64_kernel<3>: nine fma4 from zero
    "c1_to_64_masked": dict(symbols=("deqsci_conv3x3_c1_to_64_masked_f32",), nf=("c1_to_64",), wino=None, wmult=1, exact=True, c="9"),
    # csrc/jacobian.hip ffdnet_head_masked_kernel<16 | 32>: 6 patch rows x 6 patch columns = 4 channels x 9 taps, each one v_pk_fma_f32
    # per register pair, from zero (no sigma plane)
    "head_masked": dict(symbols=("deqsci_ffdnet_head_masked_f32",), nf=("head_valu",), wino=None, wmult=1, exact=True, c="36"),
}
MASKED = ("f22_masked", "c1_to_64_masked", "head_masked")
# forward denoiser entries of _hip.SIGNATURES that this table leaves out, and why (tests/test_denoiser_exact_host.py: no other may be missing)
OUT_OF_SCOPE = {
    "deqsci_conv3x3_c64_split16_stack": "stack launch: held bit for bit to per-layer launches",
    "deqsci_conv3x3_c64_wino16_stack": "stack launch: held bit for bit to per-layer launches",
    "deqsci_conv3x3_c64_winograd_timed_f32": "the same kernel and arguments as deqsci_conv3x3_c64_winograd_f32 between two events",
    "deqsci_conv3x3_c64_winograd44_f32": "the NHWC / NHWC instantiation of the layout entry, which is what _hip launches",
    "deqsci_conv3x3_c64_winograd44_timed_f32": "the NHWC / NHWC instantiation of the layout entry, which is what _hip launches",
}
FORWARD_PREFIXES = ("deqsci_conv3x3_c", "deqsci_ffdnet_head", "deqsci_ffdnet_tail", "deqsci_f32_to_split16")
CONV64 = ("f22", "f44", "s16", "w16")


def c_of(kernel, in_bias=False):
    """The rounding count of a kernel as a number (its expression holds digits, +, * only)."""
    expr = KERNELS[kernel]["c_in_bias" if in_bias else "c"]
    assert set(expr) <= set("0123456789+* ")
    return eval(expr)


def shapes_of(kernel):
    """name -> (n, H, W) of the grid the kernel tiles: nonfinite_ref's, and for a 64 -> 64 kernel one pixel and the many-tile launch;
    the masked head: one position (a 2 x 2 image), and the smallest ragged launch of its 32 x 32 form (the matrix-core head's threshold)."""
    out = {name: nf.CASES[name]["shape"] for name in KERNELS[kernel]["nf"]}
    if kernel in CONV64 or kernel == "f22_masked":
        out.update(one=ONE, many=MANY)
    if kernel == "head_mfma":
        out["head_mfma_ragged"] = HEAD_MFMA_RAGGED
    if kernel == "head_masked":
        out.update(one=ONE, head_masked_ragged=HEAD_MFMA_RAGGED)
    return out


# the (1, 1, 1) launch has ONE output per channel, and "every channel has a non-zero output" then asks for every pre-activation to be
# positive under ReLU: its integer bias is lifted by this much per unit of wmult (the pixel's sum of 64 products has a standard
# deviation of 4.2 x 2.9 x 8 = 98 per unit of wmult: ten of them)
BIAS_LIFT_ONE = 1024


# ----------------------------------------------------------------------------- data (CPU tensors: both test files see the same numbers)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, g, nonzero=False, zero_frac=0.0):
    v = torch.randint(lo, hi + 1, shape, generator=g).float()
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, float(hi)), v)
    if zero_frac:
        v = torch.where(torch.rand(shape, generator=g) < zero_frac, torch.zeros_like(v), v)
    return v


def image_scales(n, measured):
    """Per-image powers of two of the measured-range cases (powers of two rescale exactly): image i times 2^(-3 (i % 2))."""
    s = torch.ones(n)
    if measured:
        s[1::2] = 2.0 ** -3
    return s


@functools.lru_cache(maxsize=None)
def conv64_data(shape, mode, wmult, bias_relu, measured):
    """(x (n,64,H,W), w (64,64,3,3), bias (64,) or None, relu) of a 64 -> 64 case; mode "int" | "real"."""
    n, H, W = shape
    for attempt in range(64):
        g = _gen(1000 + 7 * H + W + (1 if bias_relu else 0) + 100000 * attempt)
        if mode == "int":
            x = _ints((n, 64, H, W), -8, 8, g, zero_frac=0.25)
            w = _ints((64, 64, 3, 3), -4, 4, g, nonzero=True) * wmult
            b = _ints((64,), -32, 32, g) + (BIAS_LIFT_ONE * wmult if shape == ONE else 0)
        else:
            x = torch.randn((n, 64, H, W), generator=g)
            w = torch.randn((64, 64, 3, 3), generator=g) * 0.05
            b = torch.randn((64,), generator=g) * 0.3
        # one pixel: a channel's only output is one sum of 64 products, and one in four draws has a channel where it is exactly 0 -
        # the first seed without one (check_caps: every channel must have a non-zero output)
        if shape != ONE or bool((w[:, :, 1, 1] @ x[0, :, 0, 0] != 0).all()):
            break
    x = x * image_scales(n, measured).view(-1, 1, 1, 1)
    return x, w, (b if bias_relu else None), bias_relu


PERIOD = 5    # the big matrix-core head launches repeat five distinct images (and sigmas): the float64 reference is formed once per image


@functools.lru_cache(maxsize=None)
def head_data(shape, mode, cin, measured, one_sigma=False):
    """FFDNet's first layer (cin = 5: x (n,1,2H,2W), sigma (n,) or (1,), w (64,5,3,3)) or the plain one (cin = 1: x (n,1,H,W), w (64,1,3,3),
    sigma None)."""
    n, H, W = shape
    f = 2 if cin == 5 else 1
    g = _gen(2000 + 7 * H + W + cin)
    k = min(n, PERIOD) if n > 8 else n
    if mode == "int":
        x = _ints((k, 1, f * H, f * W), -8, 8, g, zero_frac=0.25)
        w = _ints((64, cin, 3, 3), -4, 4, g, nonzero=True)
        sig = _ints((k,), 1, 8, g)
    else:
        x = torch.randn((k, 1, f * H, f * W), generator=g)
        w = torch.randn((64, cin, 3, 3), generator=g) * (0.05 if cin == 5 else 0.3)
        sig = torch.linspace(0.05, 0.2, k)
    # measured ranges: image AND sigma of every other image times 2^-3 (the whole operand: under a small image the sigma plane alone
    # would decide each channel's sign, and ReLU would zero whole channels); with one sigma for the batch the images stay as they are
    sc = image_scales(k, measured and not (one_sigma and cin == 5))
    x, sig = x * sc.view(-1, 1, 1, 1), sig * sc
    if one_sigma:
        sig = sig[:1]
    return x, (sig if cin == 5 else None), w


@functools.lru_cache(maxsize=None)
def tail_data(shape, mode, cout, in_bias, measured):
    """(h (n,64,H,W), w (cout,64,3,3), in_bias (64,) or None) of a last layer."""
    n, H, W = shape
    g = _gen(3000 + 7 * H + W + cout + (10 if in_bias else 0))
    if mode == "int":
        h = _ints((n, 64, H, W), -8, 8, g, zero_frac=0.25)
        w = _ints((cout, 64, 3, 3), -4, 4, g, nonzero=True)
        b = _ints((64,), -4, 4, g)
    else:
        h = torch.randn((n, 64, H, W), generator=g)
        w = torch.randn((cout, 64, 3, 3), generator=g) * 0.05
        b = torch.randn((64,), generator=g) * 0.3
    h = h * image_scales(n, measured).view(-1, 1, 1, 1)
    return h, w, (b if in_bias else None)


# ----------------------------------------------------------------------------- the masked kernels: operands, masks, reference, S
MASK_FORMS = ("random", "checker")


@functools.lru_cache(maxsize=None)
def mask_bits(shape, form, k=None):
    """bool (k, 64, H, W), drawn on the CPU (k distinct images of a launch that repeats them; None: the shape's n).  "random": every bit
    independent, p = 1/2.  "checker": pixels of even (row + column) hold a word with only bits 0..31 set, the others only bits 32..63 -
    a swapped half-word, or the word of a neighbouring pixel, changes whole half-pixels."""
    n, H, W = shape
    k = n if k is None else k
    if form == "random":
        return torch.rand((k, 64, H, W), generator=_gen(4000 + 7 * H + W)) < 0.5
    assert form == "checker"
    even = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2 == 0).view(1, 1, H, W)
    low = (torch.arange(64) < 32).view(1, 64, 1, 1)
    return (even == low).expand(k, 64, H, W).contiguous()


def masked_bits(kernel, shape, form):
    """The mask of a masked case: one image of bits per distinct image of its operand."""
    return mask_bits(shape, form, masked_operands(kernel, shape, "int", False)[0].shape[0])


def mask_guard_fills():
    """The guard words of the two launches of a masked case (Arena.words): all ones, then all zeros (and so on)."""
    return itertools.cycle((-1, 0))


@functools.lru_cache(maxsize=None)
def masked_operands(kernel, shape, mode, transposed):
    """(x, w) of a masked case.  x: the unmasked kernel's own drawn operand - (n,64,H,W), (n,1,H,W), or the masked head's (k,1,2H,2W).  w:
    the drawn forward weight ((64,64,3,3), (64,1,3,3), (64,4,3,3) = FFDNet's first layer without sigma's channel), or with transposed
    what the backward launches: vjp._transposed of a weight in the shape of the layer it transposes ((64,64,3,3), the last layers'
    (1,64,3,3) and (4,64,3,3))."""
    n, H, W = shape
    wmult = KERNELS[kernel]["wmult"] if mode == "int" else 1
    if kernel == "f22_masked":
        x, w, _, _ = conv64_data(shape, mode, wmult, False, False)
        return x, (_vjp._transposed(w) if transposed else w)
    cin = 1 if kernel == "c1_to_64_masked" else 5
    x, _, w = head_data(shape, mode, cin, False)
    if not transposed:
        return x, (w if cin == 1 else w[:, 1:5].contiguous())
    g = _gen(5000 + 7 * H + W + cin)
    last = (1 if cin == 1 else 4, 64, 3, 3)
    wt = _ints(last, -4, 4, g, nonzero=True) if mode == "int" else torch.randn(last, generator=g) * 0.05
    return x, _vjp._transposed(wt)


def masked_input(kernel, x):
    """What a masked kernel convolves, float64: the activation, the image, or the masked head's four unshuffled channels."""
    return Fn.pixel_unshuffle(x.double(), 2) if kernel == "head_masked" else x.double()


@functools.lru_cache(maxsize=None)
def masked_unmasked_ref(kernel, shape, mode, transposed):
    """The float64 convolution WITHOUT the mask (k distinct images), formed once per case: the caps need it, and (a)'s reference is its select."""
    x, w = masked_operands(kernel, shape, mode, transposed)
    return nf.ffdnet_head_ref(x, None, w, relu=False, with_sigma=False) if kernel == "head_masked" else nf.conv_ref(x, w)


def masked_ref(kernel, shape, mode, transposed, form):
    """nonfinite_ref's masked reference itself (a select: an element under a cleared bit is 0), k distinct images."""
    x, w = masked_operands(kernel, shape, mode, transposed)
    bits = masked_bits(kernel, shape, form)
    if kernel == "head_masked":
        return nf.ffdnet_head_ref(x, None, w, relu=False, mask=bits, with_sigma=False)
    return nf.conv_ref(x, w, mask=bits)


@functools.lru_cache(maxsize=None)
def masked_S(kernel, shape, transposed):
    """S of the real data: the unmasked kernel's own (the propagation of F(2x2,3x3), or the direct sum)."""
    x, w = masked_operands(kernel, shape, "real", transposed)
    xa = masked_input(kernel, x).abs()
    return s_wino(xa, w.abs(), KERNELS[kernel]["wino"]) if KERNELS[kernel]["wino"] else s_plain(xa, w.abs())


def masked_bound(kernel, shape, transposed, form):
    """(b) of a masked kernel: the unmasked kernel's c 2^-24 S times the mask - an element under a cleared bit must EQUAL 0."""
    return c_of(kernel) * U * masked_S(kernel, shape, transposed) * masked_bits(kernel, shape, form)


def check_masked_caps(unmasked, bits, what, one_pixel=False):
    """(a) of a masked kernel cannot pass vacuously: magnitudes below 2^24; the unmasked integer reference non-zero on at least a quarter
    of ALL elements under a set bit, and on a quarter of all elements under a cleared bit (a kernel that ignores the mask fails); every
    output channel of every image with a non-zero reference element under a set bit.  One pixel: the magnitude alone."""
    assert float(unmasked.abs().max()) < 2.0 ** 24, what
    if one_pixel:
        return None
    live = unmasked != 0
    kept, cleared = float((live & bits).double().mean()), float((live & ~bits).double().mean())
    assert kept >= 0.25 and cleared >= 0.25, (what, kept, cleared)
    n, C = unmasked.shape[:2]
    assert bool((live & bits).reshape(n, C, -1).any(-1).all()), (what, "a channel of an image has no non-zero element under a set bit")
    return kept, cleared


def mask_fault(got, unmasked, bits):
    """What a masked kernel did to its mask, read from the zero pattern of its output alone (so it serves (a) and (b)): None when every
    element is zero exactly where the select says, else every one of these readings of the mask that explains ALL misplaced zeros -
    the two 32-bit halves of the word swapped, the word of a neighbouring pixel (the checker mask cannot tell these two apart, the
    random one can), the mask ignored - or that none of them does.  All three tensors (n,64,H,W) on one device."""
    live = unmasked != 0
    z = got != 0
    bad = (z != (bits & live)) & torch.isfinite(got)          # (an element never written, or NaN, is no reading of the mask: hold() names it)
    if not bool(bad.any()):
        return None
    readings = [("the two 32-bit halves of the mask word swapped (channel c under bit c ^ 32)", bits.roll(32, 1))]
    for dy, dx_ in ((0, -1), (-1, 0), (-1, -1), (0, 1), (1, 0), (1, 1)):
        readings.append((f"the word of the pixel at (row {dy:+d}, column {dx_:+d}) taken for this one", bits.roll((-dy, -dx_), (2, 3))))
    readings.append(("the mask ignored: elements under a cleared bit were kept", torch.ones_like(bits)))
    names = [name for name, alt in readings if bool(((alt & live) == z)[bad].all())]
    if names:
        return f"{int(bad.sum())} elements zero / non-zero against the mask: " + ", or ".join(names)
    return f"{int(bad.sum())} elements zero / non-zero against the mask, by no single mislaid word (first at {tuple(bad.nonzero()[0].tolist())})"


# ----------------------------------------------------------------------------- one whole masked stack on integers (both directions)
@functools.lru_cache(maxsize=None)
def stack_data(ffdnet):
    """(layers, x, sigma, v): a three-layer plan 1 -> 64 -> 64 -> 1 (FFDNet's twin: 5 -> 64 -> 64 -> 4, sigma (1,)) whose Jacobian
    products are integers below 2^24 under a worst-case argument (stack_worst_case: all-ones masks, absolute values): first and last
    weights in {-1, +1}, middle weights in {-4, +4} (U = G w G^T an integer, |U| <= 9), integer middle bias, v in {-1, 0, 1} - for
    FFDNet supported on one pixel phase (rows and columns even: one unshuffled channel).  x = rand: the masks are those of a real
    forward pass."""
    g = _gen(6000 + int(ffdnet))
    sign = lambda shape, m: (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * m
    n, H, W = nf.CASES["head_valu" if ffdnet else "f22"]["shape"]
    f = 2 if ffdnet else 1
    layers = [(sign((64, 5 if ffdnet else 1, 3, 3), 1), None, True), (sign((64, 64, 3, 3), 4), _ints((64,), -8, 8, g), True),
              (sign((4 if ffdnet else 1, 64, 3, 3), 1), None, False)]
    x = torch.rand((n, 1, f * H, f * W), generator=g)
    v = torch.randint(-1, 2, (n, 1, f * H, f * W), generator=g).float()
    if ffdnet:
        phase = torch.zeros(1, 1, f * H, f * W)
        phase[..., ::2, ::2] = 1
        v = v * phase
    return layers, x, (torch.tensor([0.1]) if ffdnet else None), v


def stack_worst_case(layers, v, ffdnet, direction):
    """The largest absolute value that any partial sum of _MaskedStack.jvp / .vjp can take on (layers, v), float64: every mask all ones,
    every operand its absolute value.  -> the maxima behind the first launch, behind the middle one (its values: the direct sum), of
    the middle one's own partial sums (the propagation of its F(2x2,3x3) transforms), and behind the last launch."""
    read, cin, write = _vjp.FFDNET_EDGES if ffdnet else _vjp.PLAIN_EDGES
    w0, w1, w2 = (l[0].double().abs() for l in layers)
    w0 = w0[:, cin]
    if direction == "vjp":
        w0, w1, w2 = _vjp._transposed(w2), _vjp._transposed(w1), _vjp._transposed(w0)
    t1 = s_plain(read(v.double().abs()), w0)
    t2 = s_plain(t1, w1)
    return float(t1.max()), float(t2.max()), float(s_wino(t1, w1, (2, 2)).max()), float(s_plain(t2, w2).max())


# ----------------------------------------------------------------------------- float64 references and S
def conv64_ref(x, w, b, relu):
    return nf.conv_ref(x, w, b, relu)


def head_ref(x, sig, w, relu=True):
    return nf.conv_ref(x, w, None, relu) if sig is None else nf.ffdnet_head_ref(x, sig.expand(x.shape[0]) if sig.numel() == 1 else sig, w, relu)


def head_operand(x, sig):
    """The five-channel operand FFDNet's head convolves (float64), or the image itself."""
    if sig is None:
        return x.double()
    xd = Fn.pixel_unshuffle(x.double(), 2)
    n, _, H, W = xd.shape
    return torch.cat((sig.double().expand(n).reshape(n, 1, 1, 1).expand(n, 1, H, W), xd), 1)


def tail_ref(h, w, b):
    return nf.tail_ref(h, w, b, shuffle=w.shape[0] == 4)


def tail_operand(h, b, absolute=False):
    """What the last layer convolves: h, or relu(h + b); absolute: the bound's |h| + |b| instead (>= |relu(h + b)|)."""
    hd = h.double()
    if absolute:
        return hd.abs() if b is None else hd.abs() + b.double().abs().view(1, -1, 1, 1)
    return hd if b is None else torch.relu(hd + b.double().view(1, -1, 1, 1))


def s_plain(x_abs, w_abs, b_abs=None):
    """The direct sum on absolute values, float64: conv2d(|x|, |w|) + |bias|."""
    return Fn.conv2d(x_abs.double(), w_abs.double(), None if b_abs is None else b_abs.double(), padding=1)


# Winograd matrices as the kernels use them (pack_winograd_weights, pack_winograd44_weights, Wino16Weights; the B^T / A^T comments of
# csrc/winograd.hip, winograd44.hip, conv_w16.hip).  F1: the direct sum as a "transform" with one output (a 3-tap window, identities).
_T = {
    1: dict(Bt=torch.eye(3), G=torch.eye(3), At=torch.ones(1, 3)),
    2: dict(Bt=torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
            G=torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]),
            At=torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]])),
    4: dict(Bt=torch.tensor([[4., 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                             [0, 4, 0, -5, 0, 1]]),
            G=torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                            [0, 0, 1]], dtype=torch.float64),
            At=torch.tensor([[1., 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])),
}


def s_wino(x_abs, w_abs, tile, b_abs=None, chunk=64, signed=False):
    """|A^T| [ sum_c (|G| |w| |G^T|) . (|B^T| |x| |B|) ] |A| + |bias| for the output tile (my, mx), float64, tiles aligned at the image's
    origin as every kernel's are.  signed=True: the transform itself on signed operands (the host test holds it to conv2d: the matrices
    above are then the kernels' Winograd, not some other algebra)."""
    my, mx = tile
    f = (lambda m: m.double()) if signed else (lambda m: m.double().abs())
    By, Gy, Ay = (f(_T[my][k]) for k in ("Bt", "G", "At"))
    Bx, Gx, Ax = (f(_T[mx][k]) for k in ("Bt", "G", "At"))
    n, C, H, W = x_abs.shape
    ty, tx = -(-H // my), -(-W // mx)
    Uw = torch.einsum("ij,ocjk,lk->ocil", Gy, w_abs.double(), Gx)                                      # (o, c, ay, ax)
    ay, ax = By.shape[0], Bx.shape[0]
    outs = []
    for i0 in range(0, n, chunk):
        xa = x_abs[i0:i0 + chunk].double()
        xp = Fn.pad(xa, (1, tx * mx + 1 - W, 1, ty * my + 1 - H))
        P = Fn.unfold(xp, (ay, ax), stride=(my, mx)).reshape(xa.shape[0], C, ay, ax, ty * tx)         # (n, c, ay, ax, T)
        V = torch.einsum("ij,ncjkt,lk->ncilt", By, P, Bx)
        M = torch.einsum("ocil,ncilt->noilt", Uw, V)
        Y = torch.einsum("pi,noilt,ql->nopqt", Ay, M, Ax)                                             # (n, o, my, mx, T)
        Y = Y.reshape(xa.shape[0], -1, my, mx, ty, tx).permute(0, 1, 4, 2, 5, 3).reshape(xa.shape[0], -1, ty * my, tx * mx)
        outs.append(Y[:, :, :H, :W])
    S = torch.cat(outs, 0)
    return S if b_abs is None else S + f(b_abs).view(1, -1, 1, 1)


def pow2_floor_exp(e):
    """The absolute error of an fp16-split operand whose lo piece is subnormal, in the operand's own units: half of fp16's subnormal
    spacing 2^-24 under the scale 2^e."""
    return 2.0 ** (-25 - e)


def floor_sums(x_abs, w_abs, tile=None):
    """What the floors of rep_split multiply: (the sum on all-ones activations and |w|, the sum on |x| and all-ones weights) - an
    absolute error on every element of one operand times the other operand's magnitude.  For a Winograd kernel the split operands are
    the TRANSFORMED ones: the propagation of all-ones is >= 1 wherever a transformed element can be non-zero and 0 in the zero padding,
    which is split exactly."""
    s = s_plain if tile is None else (lambda a, b: s_wino(a, b, tile))
    return s(torch.ones_like(x_abs), w_abs), s(x_abs, torch.ones_like(w_abs))


def rep_split(S, sums, e_x, e_w):
    """The representation term of a split-fp16 sum (module docstring).  S: the sum without the bias; sums: floor_sums of the operands;
    e_x: the activation's exponent per image (list), e_w: the weights' (Split16Weights.sw and its like)."""
    fx = torch.tensor([pow2_floor_exp(e) for e in e_x], dtype=torch.float64).view(-1, 1, 1, 1)
    floors = fx * sums[0] + pow2_floor_exp(e_w) * sums[1]
    return (3 * 2.0 ** -22 * S + floors) * (1 + 2.0 ** -10)


def rep_out_split(y_abs, e_out):
    """An sp16 output's own split: 2^-22 |y| + 2^(-25 - e_out(image))."""
    fo = torch.tensor([pow2_floor_exp(e) for e in e_out], dtype=torch.float64).view(-1, 1, 1, 1)
    return 2.0 ** -22 * y_abs + fo


def split_rule(x_abs, e_x):
    """to_split16 itself: max(2^-22 |x|, 2^(-25 - e)) per element (e per image)."""
    fx = torch.tensor([pow2_floor_exp(e) for e in e_x], dtype=torch.float64).view(-1, 1, 1, 1)
    return torch.maximum(2.0 ** -22 * x_abs.double(), fx.expand_as(x_abs))


# ----------------------------------------------------------------------------- (a)'s caps
def check_caps(ref, relu, what):
    """The integer reference cannot let a test pass vacuously: magnitudes below 2^24, with ReLU a quarter of the outputs non-zero, and
    every output channel non-zero somewhere in every image (ref (n, C, H, W); FFDNet's tail: its four channels before the shuffle are
    the four pixel phases)."""
    assert float(ref.abs().max()) < 2.0 ** 24, what
    if relu:
        assert float((ref != 0).double().mean()) >= 0.25, (what, float((ref != 0).double().mean()))
    n, C = ref.shape[:2]
    assert bool((ref.reshape(n, C, -1) != 0).any(-1).all()), (what, "a channel of an image is all zero")


# ----------------------------------------------------------------------------- (c)'s guards
def guard_bytes(W):
    """At least two image rows of 64 fp32 channels, a multiple of 256 bytes (the wrappers' alignment survives)."""
    return max(256, -(-(2 * W * 64 * 4) // 256) * 256)


class Arena:
    """Guarded operands and outputs of one launch on `device`.  operand(t): t's values in a view of t's shape (dense, in t's memory
    format) inside a buffer of NaN.  output(shape, dtype, channels_last): a NaN-filled view inside a buffer of SENTINEL; intact():
    every sentinel of every output still there."""

    def __init__(self, W, device):
        self.gb, self.device, self.outs = guard_bytes(W), device, []

    def _carve(self, shape, dtype, fill, channels_last):
        numel = math.prod(shape)
        g = self.gb // torch.empty((), dtype=dtype).element_size()
        buf = torch.full((numel + 2 * g,), fill, dtype=dtype, device=self.device)
        inner = buf[g:g + numel]
        if channels_last:
            n, c, h, w = shape
            view = inner.view(n, h, w, c).permute(0, 3, 1, 2)
        else:
            view = inner.view(shape)
        assert (view.data_ptr() - buf.data_ptr()) % 256 == 0          # (the device allocator aligns buf itself to 512 bytes)
        return buf, g, view

    def operand(self, t):
        if t is None:
            return None
        cl = t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)
        assert cl or t.is_contiguous()
        _, _, view = self._carve(tuple(t.shape), t.dtype, float("nan"), cl)
        view.copy_(t)
        return view

    def words(self, t, fill):
        """An integer operand (the int64 mask words: no NaN exists for them) in a view of t's shape inside guard words of the caller's
        `fill`.  A case launches once inside all-ones and once inside all-zero words: a kernel that takes any word from outside the mask
        then differs between its two launches, or from the reference."""
        assert not t.dtype.is_floating_point and t.is_contiguous()
        _, _, view = self._carve(tuple(t.shape), t.dtype, fill, False)
        view.copy_(t)
        return view

    def nan(self, shape, dtype=torch.float32):
        """An operand's container still to be filled (all NaN, inside NaN)."""
        return self._carve(tuple(shape), dtype, float("nan"), False)[2]

    def output(self, shape, dtype=torch.float32, channels_last=False):
        buf, g, view = self._carve(tuple(shape), dtype, SENTINEL, channels_last)
        view.fill_(float("nan"))
        self.outs.append((buf, g))
        return view

    def intact(self):
        return all(bool((buf[:g] == SENTINEL).all()) and bool((buf[-g:] == SENTINEL).all()) for buf, g in self.outs)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def p32_fill(o, x):
    """P32.from_nchw into the existing container o (its t a guarded view), the padding columns NaN: no kernel may use them."""
    n, c, H, W = x.shape
    sc = torch.tensor([2.0 ** e for e in o.exponents()], dtype=torch.float32, device=x.device).view(-1, 1, 1, 1)
    nb = o.t.shape[4]
    xp = torch.full((n, 64, H, nb * 64), float("nan"), dtype=torch.float32, device=x.device)
    xp[..., :W] = x * sc
    o.t.copy_(xp.reshape(n, 8, 2, 4, H, nb, 32, 2).permute(0, 1, 2, 4, 5, 7, 6, 3))
    return o


def p32_padding(o):
    """The padding columns (>= W) of a P32's last block, as stored: (n, 64, H, pad)."""
    nb = o.t.shape[4]
    return o.t.permute(0, 1, 2, 7, 3, 4, 6, 5).reshape(o.n, 64, o.H, nb * 64)[..., o.W:]


def blk32_fill(o, x):
    """Blk32.from_nchw into the existing container o (padding columns NaN)."""
    n, c, H, W = x.shape
    Wb = o.t.shape[3]
    xp = torch.full((n, 64, H, Wb * 32), float("nan"), dtype=torch.float32, device=x.device)
    xp[..., :W] = x
    t = xp.reshape(n, 8, 8, H, Wb, 32).permute(0, 1, 3, 4, 5, 2)
    o.t[:, :, :, :, type(o)._pos().to(x.device), :] = t
    return o


def blk32_padding(o):
    t = o.t[:, :, :, :, type(o)._pos().to(o.t.device), :]
    return t.permute(0, 1, 5, 2, 3, 4).reshape(o.n, 64, o.H, -1)[..., o.W:]
