"""What csrc/sci_grad.hip computes, stated once without a GPU, in the manner of tests/sci_ops_ref.py (whose layouts, masks, `ratio` and
frame-sum emulation it uses): which kernel a launcher picks (path_of), a float64 reference of every entry with a first-order bound per
element, and an fp32 emulation of every path's order of operations.  tests/test_sci_grad_host.py holds this module to torch's float64
autograd and to itself on the CPU, tests/test_sci_grad_gpu.py and tests/test_mask_grad_gpu.py hold the kernels to it.  A helper, not a test.

Tensors are LOGICAL as in sci_ops_ref: z, g, v, Phi are (n, P, B), y, a, s = Phi_sum and gs are (n, P); a shared mask has n = 1, and its
gradients have n = 1 and hold the sum over the batch.

G1, the backward of z1 = z + ((y - fb) / s) Phi, fb = sum_b z_b Phi_b, for a gradient g of z1 (s is an INPUT: the Phi_sum the step was given):
    q = sum_b g_b Phi_b     r = (y - fb) / s     t = q / s
    gPhi_b = r g_b - t z_b     gs = -t r     gz_b = g_b - t Phi_b     gy = t
  (d z1_c / d Phi_b = -z_b Phi_c / s + r [b = c], d z1_c / d s = -r Phi_c / s: contract with g_c.)
THE BOUNDS.  u = 2^-24, first order, times 1.01 for the second order, no absolute tolerance.  S_z = sum_b |z_b Phi_b|, S_g = sum_b |g_b Phi_b|.
A sum of B rounded products in any order of B - 1 additions is off by at most B u S (sci_ops_ref), so
    fb, q     carry B u S_z, B u S_g
    r         the subtraction rounds once on |y - fb|, the division once on |r|:     dr <= u [ (B S_z + |y - fb|) / |s| + |r| ]
    t         the division rounds once on |t|:                                       dt <= u [ B S_g / |s| + |t| ]
    gPhi_b    two products (u |r g_b|, u |t z_b|) and a difference (u |gPhi_b|):      |g_b| dr + |z_b| dt + u (|r g_b| + |t z_b| + |gPhi_b|)
    gs        one product:                                                           |r| dt + |t| dr + u |t r|
    gz_b      a product and a difference:                                            |Phi_b| dt + u (|t Phi_b| + |gz_b|)
    gy        dt
  a shared mask sums bsz such terms left to right: the sum of the terms' bounds plus (bsz - 1) u sum_n |term_n|.
G2  gPhi_b = a v_b: one product of two fp32 numbers - exact in float64, rounded once: bit equality per sample, no bound; a shared mask:
    bsz rounded products and bsz - 1 additions, bsz u sum_n |a_n v_nb|.
G3  gPhi_b = gs, or 0 where sum_b Phi_b is 0: a copy, bit equality.  The kernel forms the sum again in fp32 in the forward kernel's
    order; the reference decides on the exact sum (a sum of non-negative entries is 0 in fp32 exactly when it is 0; sci_ops_ref.uniform_mask's
    cancelling pixels are +a - a and zeros, 0 in any order).
THE EMULATIONS round every product, sum, difference, quotient and negation-free step separately in fp32 on the CPU, in the kernel's order:
fb and q by sci_ops_ref._sum_frames (dot4_seq + butterfly for hwb<LP>, left to right for generic), then d = y - fb, r = d / s, t = q / s,
(r g_b) - (t z_b), -(t r), g_b - (t Phi_b); the batch sum of a shared mask starts from the term of n = 0 and adds n = 1 .. bsz - 1."""
import torch

import sci_ops_ref as so
from sci_ops_ref import HWB, BHW, U

OPS = ("gap_grad", "mask_grad", "phi_sum_grad")
OUTPUTS = ("gphi", "gs", "gz", "gy")


# ----------------------------------------------------------------------------- dispatch
def traffic_bytes(op, bsz, nm, P, B, outputs=("gphi", "gs")):
    """The byte count each launcher hands to pick_policy: what the launch reads and writes.  nm = masks (1 when shared, else bsz).
    gap_grad per sample: 16B + 12 per pixel for the mask outputs, 20B + 16 with gz and gy."""
    if op == "gap_grad":
        n = bsz * P * (8 * B + 4) + nm * P * (4 * B + 4)
        n += nm * P * 4 * B if "gphi" in outputs else 0
        n += nm * P * 4 if "gs" in outputs else 0
        n += bsz * P * 4 * B if "gz" in outputs else 0
        n += bsz * P * 4 if "gy" in outputs else 0
        return n
    if op == "mask_grad":
        return bsz * P * (4 * B + 4) + nm * P * 4 * B
    assert op == "phi_sum_grad"
    return nm * P * (8 * B + 4)


def path_of(op, layout, B, P, nbytes):
    """(kernel, policy): the launchers' if-chains restated.  HWB only; the generic kernels take no cache policy."""
    assert op in OPS
    if layout != HWB or B > so.MAX_B:
        return "unsupported", "default"
    if B in so.LP_OK:
        return f"hwb{B // 4}", "streaming" if nbytes >= so.STREAM_MIN_BYTES else "default"
    return "generic", "default"


def blocks_of(kernel, B, P):
    """gridDim.x; gridDim.y is the number of masks (1 when shared)."""
    return so.blocks_of(kernel, B, P)


# ----------------------------------------------------------------------------- float64 references and bounds
def _batch_sum(term, bound, shared):
    """A shared mask's gradient: the sum over the batch (dim 0, kept) and its bound."""
    if not shared:
        return term, bound
    n = term.shape[0]
    return term.sum(0, keepdim=True), bound.sum(0, keepdim=True) + 1.01 * (n - 1) * U * term.abs().sum(0, keepdim=True)


def ref_gap_grad(z, phi, g, y, s):
    """{"gphi" | "gs" | "gz" | "gy": (exact, bound)}, float64.  phi (nm, P, B), s (nm, P); nm = 1 < bsz: shared."""
    B = z.shape[-1]
    shared = phi.shape[0] == 1 and z.shape[0] > 1
    zd, pd, gd, yd, sd = z.double(), phi.double(), g.double(), y.double(), s.double()
    tz, tg = zd * pd, gd * pd
    d = yd - tz.sum(-1)
    Sz, Sg = tz.abs().sum(-1), tg.abs().sum(-1)
    r, t = d / sd, tg.sum(-1) / sd
    dr = U * ((B * Sz + d.abs()) / sd.abs() + r.abs())
    dt = U * (B * Sg / sd.abs() + t.abs())
    r4, t4, dr4, dt4 = (a.unsqueeze(-1) for a in (r, t, dr, dt))
    gphi = r4 * gd - t4 * zd
    b_gphi = 1.01 * (gd.abs() * dr4 + zd.abs() * dt4 + U * ((r4 * gd).abs() + (t4 * zd).abs() + gphi.abs()))
    gs = -(t * r)
    b_gs = 1.01 * (r.abs() * dt + t.abs() * dr + U * (t * r).abs())
    gz = gd - t4 * pd
    b_gz = 1.01 * (pd.abs() * dt4 + U * ((t4 * pd).abs() + gz.abs())).expand_as(gz)
    return {"gphi": _batch_sum(gphi, b_gphi, shared), "gs": _batch_sum(gs, b_gs, shared), "gz": (gz, b_gz), "gy": (t, 1.01 * dt)}


def ref_mask_grad(a, v, shared):
    """(exact, bound), float64; per sample the bound is the one rounding of the product (the tests ask for bit equality there)."""
    term = a.double().unsqueeze(-1) * v.double()
    if not shared:
        return term, U * term.abs()
    return term.sum(0, keepdim=True), term.shape[0] * U * term.abs().sum(0, keepdim=True)


def ref_phi_sum_grad(phi, gs):
    """fp32 (nb, P, B): gs on every frame, 0 where the exact sum of the mask is 0."""
    zero = (phi.double().sum(-1) == 0).unsqueeze(-1)
    return torch.where(zero, torch.zeros((), dtype=gs.dtype, device=gs.device), gs.unsqueeze(-1)).expand_as(phi).contiguous()


ratio = so.ratio


# ----------------------------------------------------------------------------- fp32 emulations
def _left_to_right(term):
    acc = term[0:1].clone()
    for n in range(1, term.shape[0]):
        acc = acc + term[n:n + 1]
    return acc


def emu_gap_grad(z, phi, g, y, s, kernel):
    """{"gphi", "gs", "gz", "gy"} in fp32, in the order of `kernel` ("hwb<LP>" or "generic")."""
    so._f32(z, phi, g, y, s)
    shared = phi.shape[0] == 1 and z.shape[0] > 1
    fb = so._sum_frames(z * phi, kernel)
    q = so._sum_frames(g * phi, kernel)
    d = y - fb
    r = d / s
    t = q / s
    r4, t4 = r.unsqueeze(-1), t.unsqueeze(-1)
    gphi = (r4 * g) - (t4 * z)
    gs = -(t * r)
    gz = g - (t4 * phi)
    if shared:
        gphi, gs = _left_to_right(gphi), _left_to_right(gs)
    return {"gphi": gphi, "gs": gs, "gz": gz, "gy": t}


def emu_mask_grad(a, v, shared):
    so._f32(a, v)
    term = a.unsqueeze(-1) * v
    return _left_to_right(term) if shared else term


def emu_phi_sum_grad(phi, gs, kernel):
    so._f32(phi, gs)
    s = so._sum_frames(phi, kernel)
    return torch.where((s == 0).unsqueeze(-1), torch.zeros((), dtype=torch.float32, device=phi.device), gs.unsqueeze(-1)).expand_as(phi).contiguous()


# ----------------------------------------------------------------------------- the case grid shared by the host and the GPU tests
BSZ = 3
GRID = [(B, H, W, f"hwb{B // 4}") for B in (4, 8, 16, 32) for (H, W) in ((5, 7), (37, 53))] + \
       [(B, H, W, "generic") for B in (3, 12) for (H, W) in ((5, 7), (37, 53))]


def case_data(H, W, B, mask, shared):
    """Logical CPU tensors (Phi, z, g, y, s, a, gs_in) of one case of the grid.  mask "uniform": sci_ops_ref.uniform_mask (all-zero pixels and
    pixels that cancel to 0); "binary": the mask of test_gpu_parity.make_case, rand < 0.5 with the first two pixels all zero, and a y that a
    scene under that mask produces.  s = Phi_sum as phi_sum gives it (left to right, 0 -> 1), an input of G1.  g: the gradient of z1; a: an
    (n, P) factor for G2; gs_in: the incoming gradient of G3.  Computed once per case by the tests and never written to."""
    P, nb = H * W, 1 if shared else BSZ
    gen = torch.Generator().manual_seed(131 * B + 17 * H + W + (7 if shared else 0))
    if mask == "binary":
        Phi = (torch.rand(nb, P, B, generator=gen) < 0.5).float()
        Phi[:, :2] = 0
        y = (torch.rand(BSZ, P, B, generator=gen) * Phi).sum(-1)
        assert (Phi.sum(-1) == 0).any()
    else:
        Phi = so.uniform_mask(nb, P, B, gen)
        y = torch.rand(BSZ, P, generator=gen) * (B / 4)
        assert int((Phi.double().sum(-1) == 0).sum()) == 5 * nb and (Phi[:, 2] != 0).any()
    z = torch.randn(BSZ, P, B, generator=gen)
    g = torch.randn(BSZ, P, B, generator=gen)
    a = torch.randn(BSZ, P, generator=gen)
    gs_in = torch.randn(nb, P, generator=gen)
    return Phi, z, g, y, so.emu_phi_sum(Phi, "generic"), a, gs_in
