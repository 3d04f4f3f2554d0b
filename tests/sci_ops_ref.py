"""What csrc/sci_ops.hip computes, stated once without a GPU: which kernel a launcher picks (path_of), a float64 reference of every
operation with a running-error bound per element, an fp32 emulation of every path's order of operations, and where a NaN or an Inf in
an input may show in the output.  tests/test_sci_ops_host.py holds this module to itself and to tests/golden/ops.npz on the CPU,
tests/test_sci_ops_gpu.py holds the kernels to it.  A helper module, not a test.

Tensors here are LOGICAL: x, z, Phi are (n, P, B) - pixel p = h * W + w, frame b - whatever the memory layout of the launch
(to_layout / from_layout convert), y and Phi_sum are (n, P); a shared mask has n = 1 and broadcasts.  Everything is torch and runs on
the device of its operands.

THE BOUNDS.  u = 2^-24, first order in u (Higham's gamma_k ~ k u), per element, and independent of the order of a sum: a sum of k
terms in ANY order of k - 1 additions has |error| <= (k - 1) u sum |t_i|, so one bound serves the xor-butterfly, the left-to-right
loops and any fused multiply-add that drops a rounding.
  forward   y = sum_b x_b Phi_b:   B products rounded once, B - 1 additions     B u sum_b |x_b Phi_b|
  phi_sum   s = sum_b Phi_b:       B - 1 additions                              (B - 1) u sum_b |Phi_b|;  s == 0 -> 1 exactly
  adjoint   x_b = y Phi_b:         ONE product of two fp32 numbers: exact in float64 (24 + 24 bits), rounded once -> no bound, bit equality
  residual  out = a - b:           one subtraction -> bit equality with the same fp32 subtraction
  GAP step  z1_b = z_b + ((y - fb) / s) Phi_b with fb = sum_b z_b Phi_b, S = sum_b |z_b Phi_b|, r = (y - fb) / s (exact values):
            fb carries B u S, and reaches z1_b through the factor |Phi_b| / |s|; the subtraction, the division and the product round
            once each on a quantity of size |r Phi_b| (the subtraction's share written as |Phi_b| / |s| |y - fb|), the last addition
            once on |z1_b|:
                u [ |Phi_b| / |s| (B S + |y - fb|) + 2 |r Phi_b| + |z1_b| ]        times 1.01 for the terms of second order.
THE EMULATIONS round every product, sum, difference and quotient separately in fp32 (torch's elementwise fp32 operations on the CPU are
single IEEE operations; nothing contracts), in the order of the kernel path named:
  hwb<LP>, hwb2bhw<LP>   per quad of four frames ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (dot4_seq), then the butterfly over the LP quads of the
                         pixel: LP = 2: q0 + q1, LP = 4: (q0 + q1) + (q2 + q3), LP = 8: one more level (addition commutes bit for bit, so
                         every lane of the group holds the same sum)
  bhw, bhw<BT>, generic  left to right from frame 0
  GAP                    fb as above, d = y - fb, r = d / s, p = r Phi_b, z1 = z + p."""
import torch

HWB, BHW = 0, 1
U = 2.0 ** -24                            # unit roundoff of fp32
TB, UNR, TP = 256, 4, 256                 # csrc/sci_ops.hip: threads per block, float4 positions per lane, pixels per LDS tile
STREAM_MIN_BYTES = 64 << 20               # csrc/common.hpp: from here on a launch uses non-temporal loads and stores
LP_OK = (4, 8, 16, 32)
MAX_BSZ, MAX_B = 65535, 4096              # check_dims
LDS_OPT_IN, LDS_MAX = 64 * 1024, 160 * 1024
ERR_UNSUPPORTED = -4
OPS = ("forward", "adjoint", "phi_sum", "gap", "transpose", "residual_out")


# ----------------------------------------------------------------------------- dispatch
def traffic_bytes(op, bsz, P, B):
    """The byte count each launcher hands to pick_policy."""
    per_pixel = {"forward": 8 * B + 4, "adjoint": 8 * B + 4, "phi_sum": 4 * B + 4, "gap": 12 * B + 8, "transpose": 8 * B, "residual_out": 12 * B}[op]
    return bsz * P * per_pixel


def path_of(op, layout_in, layout_out, B, P, nbytes):
    """(kernel, policy) of a launch: the launchers' if-chains restated.  For "transpose" layout_out is to_layout and layout_in the other one;
    for "residual_out" the input is planar.  Only the templated fast kernels and sub_flat take a cache policy."""
    assert op in OPS and layout_in in (HWB, BHW) and layout_out in (HWB, BHW)
    if B > MAX_B:
        return "unsupported", "default"
    lp = B in LP_OK
    stream = "streaming" if nbytes >= STREAM_MIN_BYTES else "default"
    if op in ("forward", "adjoint", "phi_sum"):
        assert layout_in == layout_out
        if layout_in == HWB and lp:
            return f"hwb{B // 4}", stream
        if layout_in == BHW and P % 4 == 0:
            return "bhw", stream
        return "generic", "default"
    if op == "gap":
        if layout_in == HWB and layout_out == HWB and lp:
            return f"hwb{B // 4}", stream
        if layout_in == BHW and layout_out == BHW and P % 4 == 0 and B in (4, 8, 16):
            return f"bhw{B}", stream
        if layout_in == HWB and layout_out == BHW and lp and P % 4 == 0:
            return f"hwb2bhw{B // 4}", stream
        return "generic", "default"
    if op == "transpose":
        assert layout_in != layout_out
        if lp and P % 4 == 0:
            return "transpose_fast", stream
        lds = B * (TP + 1) * 4
        if lds > LDS_MAX:
            return "unsupported", "default"
        return f"transpose_generic({lds})", "default"
    if layout_out == BHW:                                      # residual_out
        return "sub_flat", stream
    if lp and P % 4 == 0:
        return f"bhw2hwb{B // 4}", stream
    return "unsupported", "default"                            # (the Python wrapper composes sub_flat + transpose)


def blocks_of(kernel, B, P):
    """Workgroups per measurement (gridDim.x) of a kernel path."""
    if kernel.startswith("hwb2bhw") or kernel.startswith("bhw2hwb") or kernel.startswith("transpose"):
        return -(-P // TP)
    if kernel.startswith("hwb"):
        return -(-(P * (B // 4)) // (TB * UNR))
    if kernel.startswith("bhw"):
        return -(-(P // 4) // TB)
    if kernel == "generic":
        return -(-P // TB)
    raise ValueError(kernel)


# ----------------------------------------------------------------------------- layouts
def to_layout(t, layout, H, W):
    """logical (n, P, B) -> contiguous (n, H, W, B) or (n, B, H, W)."""
    n, P, B = t.shape
    assert P == H * W
    t = t.reshape(n, H, W, B)
    return t.contiguous() if layout == HWB else t.permute(0, 3, 1, 2).contiguous()


def from_layout(t, layout):
    """(n, H, W, B) or (n, B, H, W) -> logical (n, P, B)."""
    if layout == BHW:
        t = t.permute(0, 2, 3, 1)
    n, H, W, B = t.shape
    return t.reshape(n, H * W, B)


# ----------------------------------------------------------------------------- masks
def uniform_mask(nb, P, B, gen, device="cpu"):
    """uniform(0, 1) with three all-zero pixels (0, 1 and P - 1) and two pixels whose entries cancel to a sum of exactly 0 (+a, -a, zeros
    elsewhere: pixel 2 in frames 0 and B - 1, pixel P - 2 in frames 1 and 2) - in any order of summation."""
    assert P >= 6 and B >= 3
    Phi = torch.rand(nb, P, B, generator=gen, device=device)
    Phi[:, (0, 1, P - 1)] = 0
    for p, (i, j) in ((2, (0, B - 1)), (P - 2, (1, 2))):
        a = Phi[:, p, i].clone()
        Phi[:, p] = 0
        Phi[:, p, i] = a
        Phi[:, p, j] = -a
    return Phi


def signed_mask(nb, P, B, gen, device="cpu"):
    """uniform(-1, 1): entries of either sign (sums that cancel in part), no special pixels."""
    return torch.rand(nb, P, B, generator=gen, device=device) * 2 - 1


# ----------------------------------------------------------------------------- float64 references and bounds
def ref_forward(x, phi):
    """(exact, bound), both float64 (n, P)."""
    t = x.double() * phi.double()
    return t.sum(-1), x.shape[-1] * U * t.abs().sum(-1)


def ref_adjoint(y, phi):
    """fp32 (n, P, B): the exact product rounded once."""
    return (y.double().unsqueeze(-1) * phi.double()).float()


def ref_phi_sum(phi):
    """(exact with 0 -> 1, bound, zero): float64 (nb, P) twice and the bool mask of the pixels whose exact sum is 0 (the output is 1.0f there)."""
    p = phi.double()
    s = p.sum(-1)
    zero = s == 0
    return torch.where(zero, torch.ones_like(s), s), (phi.shape[-1] - 1) * U * p.abs().sum(-1), zero


def ref_gap(z, phi, y, s):
    """(exact, bound), both float64 (n, P, B); s is the Phi_sum the kernel is GIVEN (fp32, 0 already replaced by 1)."""
    B = z.shape[-1]
    zd, pd, yd, sd = z.double(), phi.double(), y.double(), s.double()
    t = zd * pd
    d = (yd - t.sum(-1)).unsqueeze(-1)
    S = t.abs().sum(-1).unsqueeze(-1)
    sd = sd.unsqueeze(-1)
    rp = d / sd * pd
    z1 = zd + rp
    bound = 1.01 * U * (pd.abs() / sd.abs() * (B * S + d.abs()) + 2 * rp.abs() + z1.abs())
    return z1, bound


def gap_miss_bound(phi, gap_bound):
    """Where s = sum_b Phi_b = sum_b Phi_b^2 (a BINARY mask with a non-zero sum) the exact step lands on the data, Phi z1 = y, so what the
    computed z1 misses by is sum_b Phi_b (z1_b - exact_b): at most sum_b |Phi_b| bound_b.  (A grey mask does not land: the reference
    divides by sum Phi, not sum Phi^2.)"""
    return (phi.double().abs() * gap_bound).sum(-1)


def ratio(got, exact, bound):
    """max |got - exact| / bound; an error where the bound is zero must be zero; got must be finite."""
    err = (got.double() - exact).abs()
    assert torch.isfinite(got).all()
    assert (err[bound == 0] == 0).all()
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ----------------------------------------------------------------------------- fp32 emulations
def _tree(kernel):
    return kernel.startswith("hwb")                            # hwb<LP> and hwb2bhw<LP>: dot4_seq + butterfly; everything else left to right


def _f32(*ts):
    for t in ts:
        assert t.dtype == torch.float32


def _sum_frames(m, kernel):
    """(n, P, B) fp32 terms -> (n, P) in the order of the path."""
    n, P, B = m.shape
    if _tree(kernel):
        assert B in LP_OK
        q = m.reshape(n, P, B // 4, 4)
        s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        while s.shape[-1] > 1:
            s = s[..., 0::2] + s[..., 1::2]
        return s[..., 0]
    acc = m[..., 0].clone()
    for b in range(1, B):
        acc = acc + m[..., b]
    return acc


def emu_forward(x, phi, kernel):
    _f32(x, phi)
    return _sum_frames(x * phi, kernel)


def emu_adjoint(y, phi):
    _f32(y, phi)
    return y.unsqueeze(-1) * phi


def emu_phi_sum(phi, kernel):
    _f32(phi)
    s = _sum_frames(phi, kernel)
    return torch.where(s == 0, torch.ones_like(s), s)          # (a NaN compares unequal to 0: it stays)


def emu_gap(z, phi, y, s, kernel):
    _f32(z, phi, y, s)
    fb = _sum_frames(z * phi, kernel)
    d = y - fb
    r = d / s
    p = r.unsqueeze(-1) * phi
    return z + p


# ----------------------------------------------------------------------------- non-finite inputs
POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def poison_pixels(P):
    """The pixels of one measurement a poison goes to, one per run: the first; the last (the address the clamped tail lanes of the HWB
    kernels re-read); both sides of the seam between two blocks of 1024 quads at LP = 8 (quad 1023 is the last quarter of pixel 127, quad
    1024 the first of pixel 128); both sides of the first seam of the 256-pixel tiles and blocks (255 / 256); both sides of the seam of the
    planar kernels' blocks of 1024 pixels."""
    return [p for p in (0, 127, 128, 255, 256, 1023, 1024, P - 1) if 0 <= p < P]


def poison_frame(p, B):
    """The frame the poison of pixel p sits in: the side of the pixel's frame column that faces the seam."""
    return B - 1 if p % 2 else 0


def nonfinite_forward(x, phi):
    """bool (n, P): where IEEE arithmetic on the float64 reference leaves y non-finite."""
    return ~torch.isfinite((x.double() * phi.double()).sum(-1))


def nonfinite_gap(z, phi, y, s):
    """bool (n, P, B), likewise for the GAP step."""
    zd, pd = z.double(), phi.double()
    r = (y.double() - (zd * pd).sum(-1)) / s.double()
    return ~torch.isfinite(zd + r.unsqueeze(-1) * pd)
