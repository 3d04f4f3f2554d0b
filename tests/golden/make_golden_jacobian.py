#!/usr/bin/env python3
"""Generate tests/golden/jacobian.npz: Jacobian products and a dense Jacobian of the REFERENCE's fixed-point map.

Imports the reference on the CPU with the shims make_golden.py documents (tests/golden/ref_shims.py); stores seeded inputs and the
numbers the reference computes from them, none of its text.  Runs only where the reference is mounted.

    python tests/golden/make_golden_jacobian.py

The reference's f(z) = z1 - D(z1), z1 = z + At((y - A z) / Phi_sum), is piecewise linear, so its Jacobian at z is that of the linear piece
z lies in, and forward-mode autograd of the reference's own float64 forward (torch.autograd.functional.jvp / jacobian: ReLU'(0) = 0)
gives J v exactly.  Central differences in float64, (f(z + h v) - f(z - h v)) / 2h, give the same numbers only while no ReLU unit changes
sign within +-h v, and at these points that cannot be had together with 1e-9: on the 16x16x8 crop the differences at h and h/10 still
differ by 7e-4 (SimpleCNN) at h = 1e-7 - the pre-activations of flat image regions cluster at zero, the flipped fraction falls only like
h^0.55 - and below h = 1e-8 the rounding error eps |f| / h takes over (4e-8 at 1e-9).  No seed passes "h and h/10 agree to 1e-9".  The
differences are therefore kept as a recorded cross-check (a_fd_rel: the relative L2 distance between the autograd product and the
differences at h = 1e-9), not as the source of the numbers.  FFDNet's own autograd returns zero through x.data, and the reference's
FFDNet cannot run in float64 (fixed tensor types in its functions.py), so for FFDNet the products are those of this package's functional
float64 restatement (deqsci_amd.vjp.ffdnet_plan_forward) under torch's autograd - not of the hand-written ffdnet_plan_jvp / _vjp under test -
and that restatement is pinned here to the reference's forward at the same points: this package's FFDNet module (the same layers,
BatchNorm unfolded) in fp32 against the reference in fp32 to 1e-6, and the folded float64 plan against that module in float64 to 1e-12;
1e-6 is the tolerance of the FFDNet goldens
(nets.npz).  SimpleCNN and RealSN_SimpleCNN run the reference's own modules in float64.

Contents, per case c in SimpleCNN, RealSN_SimpleCNN, ffdnet_s0 (sigma = 60/255), ffdnet_s1 (sigma = 60/255 * 0.971^10):
  (a) c/a_*   a 16x16x8 crop of traffic measurement 0 (the first whose ReLU decisions an fp32 forward resolves: decisions_resolved),
              z after 10 reference Anderson iterations: z, y, Phi, Phi_sum, sigma, seeded v
              and w, Jv (forward-mode autograd), JTw (the reference's autograd; SimpleCNN and RealSN only), the two sides of the adjoint identity, a_fd_rel
  (b) c/b_*   an 8x8x2 case, N = 128: the dense J_f and J_D built column by column; stored are their action and their transposes' action on
              8 seeded probe vectors (the matrices themselves would exceed the size limit), numpy's svd and eigvals of both, and the power iterations of
              deqsci_amd/jacobian.py restated in numpy on the dense matrices with their full histories; b_n_iters = the smallest of
              30, 60, 120 at which that numpy Lipschitz estimate reaches 0.99 of the dense sigma_max (a condition on the case)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402  (installs the shims, imports the reference)

from deqsci_amd import vjp  # noqa: E402
from deqsci_amd.jacobian import start_vector  # noqa: E402

SIGMAS = {"ffdnet_s0": 0, "ffdnet_s1": 10}          # f-call index of the sigma schedule


def sigma_at(call):
    s = np.float32(60 / 255)
    for _ in range(call):
        s = np.float32(s * np.float32(0.971))
    return float(s)


def problem(H, W, B, r0, c0):
    d = mg.load_test_data(mg.DATA + "traffic_cacti.mat")
    sl = (slice(r0, r0 + H), slice(c0, c0 + W))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"][sl][..., :B]))[None]
    gt = torch.from_numpy(np.ascontiguousarray(d["gt"][sl][..., :B]))[None]
    y = torch.from_numpy(np.ascontiguousarray(d["meas"][sl][..., 0]))[None] if B == 8 else mg.A_torch_(gt, Phi)
    Phi_sum = torch.sum(Phi, axis=3)
    Phi_sum[Phi_sum == 0] = 1
    return y, Phi, Phi_sum, gt


def point(name, y, Phi, Phi_sum, gt):
    """z after 10 Anderson iterations of the reference (fp32), as the reference's DEQ returns it."""
    _, deq = mg.build_deq("ffdnet" if name.startswith("ffdnet") else name, 10)
    z = deq.forward(y, Phi, Phi_sum, initial_point=mg.initial_point(y, Phi, Phi_sum, gt), train_flag=False)      # (it registers its hook: a tape is needed)
    return z.detach()


class Case:
    """f and D of one case in float64: the reference's own solver module (SimpleCNN, RealSN) or, for FFDNet, the pinned restatement."""

    def __init__(self, name, y, Phi, Phi_sum):
        self.name, self.ffdnet = name, name.startswith("ffdnet")
        self.y, self.Phi, self.Phi_sum = y.double(), Phi.double(), Phi_sum.double()
        if self.ffdnet:
            self.net32 = mg.build_denoiser("ffdnet")
            self.sigma = sigma_at(SIGMAS[name])
            from deqsci_amd.networks import FFDNet
            own = FFDNet(1, "ffdnet").eval()
            own.load_state_dict(self.net32.state_dict())
            import copy
            self.own, self.own64 = own, copy.deepcopy(own).double()
            self.layers = vjp.ffdnet_plan(self.own64)                 # (the BatchNorm folded in float64)
        else:
            self.sigma = 0.0
            self.solver = mg.build_solver(name).double().eval()

    def z1(self, z):
        return z + mg.At_torch_((self.y - mg.A_torch_(z, self.Phi)) / self.Phi_sum, self.Phi)

    def D(self, x):
        """the noise predictor on (n,1,H,W) float64"""
        if self.ffdnet:
            return vjp.ffdnet_plan_forward(self.layers, x, self.sigma)[0]
        return self.solver.nonlinear_op(x)

    def f(self, z):
        if not self.ffdnet:
            return self.solver(z, self.y, self.Phi, self.Phi_sum)
        bsz, H, W, B = z.shape
        z1 = self.z1(z)
        x = z1.permute(0, 3, 1, 2).contiguous().view(bsz * B, 1, H, W)
        return z1 - self.D(x).view(bsz, B, H, W).permute(0, 2, 3, 1)

    def pin(self, z):
        """FFDNet: the restatement against the reference's fp32 forward at this point."""
        if not self.ffdnet:
            return 0.0
        bsz, H, W, B = z.shape
        x = self.z1(z).permute(0, 3, 1, 2).contiguous().view(bsz * B, 1, H, W)
        with torch.no_grad():
            want = self.net32(x.float(), torch.full((bsz * B,), self.sigma, dtype=torch.float32)).double()
            sg = torch.full((bsz * B,), self.sigma, dtype=torch.float64)
            got = self.own(x.float(), sg.float()).double()      # fp32 against fp32, as the FFDNet goldens: the same layers, BN unfolded
            err64 = float((self.D(x) - self.own64(x, sg)).norm() / want.norm())      # ... and the folded float64 plan is those layers
        assert err64 < 1e-12, (self.name, err64)
        err = float((got - want).norm() / want.norm())
        assert err < 1e-6, (self.name, err)
        return err


EPS32 = 2.0 ** -24


def decisions_resolved(case, z):
    """A condition on the case, checked from float64 numbers alone: every ReLU decision at this point is one that ANY fp32 forward takes
    the same way.  An fp32 evaluation of a pre-activation sum_k w_k h_k (+ b) in any order, Winograd's included, errs by a small multiple
    of eps32 * (sum_k |w_k| |h_k| + |b|); a unit whose float64 pre-activation is smaller than 8 x that may be decided either way, and
    then the Jacobian of an fp32 implementation is that of the neighbouring linear piece (one such unit moved J v by 9e-4 on the first
    crop tried).  The golden products are stored at a point without such units."""
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import SHIPPED, build_pipeline
    import torch.nn.functional as F
    bsz, H, W, B = z.shape
    x = case.z1(z).permute(0, 3, 1, 2).contiguous().view(bsz * B, 1, H, W)
    if case.ffdnet:
        layers = case.layers
        h = torch.cat((vjp._sigma_map(case.sigma, x), F.pixel_unshuffle(x, 2)), 1)
    else:
        net = build_pipeline(case.name, checkpoint.shipped(SHIPPED[case.name]), device="cpu")[0].nonlinear_op.eval().double()
        assert float((net(x) - case.D(x)).norm()) <= 1e-12 * float(case.D(x).norm())          # the shipped weights are the reference's
        layers, h = vjp.host_plan(net)[0], x
    worst = float("inf")
    for w, b, _ in layers[:-1]:
        pre = F.conv2d(h, w, b, padding=1)
        size = F.conv2d(h.abs(), w.abs(), None if b is None else b.abs(), padding=1)
        worst = min(worst, float((pre.abs() / (8 * EPS32 * size)).min()))
        h = torch.relu(pre)
    return worst >= 1.0, worst


def diff(fun, z, v, h):
    with torch.no_grad():
        return (fun(z + h * v) - fun(z - h * v)) / (2 * h)


def products(case, z, out, p):
    g = torch.Generator().manual_seed(100)
    v = torch.randn(z.shape, generator=g, dtype=torch.float32).double()
    w = torch.randn(z.shape, generator=g, dtype=torch.float32).double()
    Jv = torch.autograd.functional.jvp(case.f, z, v)[1].detach()
    fd = diff(case.f, z, v, 1e-9)
    out.update({p + "z": z, p + "y": case.y, p + "Phi": case.Phi, p + "Phi_sum": case.Phi_sum, p + "sigma": torch.tensor(case.sigma, dtype=torch.float64),
                p + "v": v, p + "w": w, p + "Jv": Jv, p + "seed": torch.tensor(100), p + "wJv": (w * Jv).sum(),
                p + "fd_rel": (fd - Jv).norm() / Jv.norm()})
    if not case.ffdnet:
        z0 = z.clone().requires_grad_()
        JTw = torch.autograd.grad(case.f(z0), z0, w)[0]
        out.update({p + "JTw": JTw, p + "JTwv": (JTw * v).sum()})
        assert abs(float((w * Jv).sum() - (JTw * v).sum())) <= 1e-12 * float(w.norm() * Jv.norm()), case.name
    out[p + "pin"] = torch.tensor(case.pin(z))


def numpy_power(J, JD, v0, n_iters, window):
    """The iterations of deqsci_amd/jacobian.py on dense matrices (J for f in (H,W,B) order, JD for D in the planar (B,H,W) order)."""
    def gram(M):
        v, hist = v0.copy(), []
        for _ in range(n_iters):
            w = M @ v
            hist.append(np.linalg.norm(w))
            u = M.T @ (w / hist[-1])
            v = u / np.linalg.norm(u)
        return np.array(hist)
    v, grow, ray = v0.copy(), [], []
    for _ in range(n_iters):
        w = J @ v
        grow.append(np.linalg.norm(w))
        ray.append(v @ w)
        v = w / grow[-1]
    grow = np.array(grow)
    return gram(J), grow, np.array(ray), float(np.exp(np.log(grow[-window:]).mean())), gram(JD)


def dense(case, z, out, p):
    bsz, H, W, B = z.shape
    N = H * W * B
    x = case.z1(z).permute(0, 3, 1, 2).contiguous().view(B, 1, H, W)
    J = torch.autograd.functional.jacobian(case.f, z).reshape(N, N).numpy()
    JD = np.zeros((N, N))                                        # D acts frame by frame: (frame, pixel) x (frame, pixel)
    JD[:] = torch.autograd.functional.jacobian(case.D, x).reshape(N, N).numpy()
    sv, svd_ = np.linalg.svd(J, compute_uv=False), np.linalg.svd(JD, compute_uv=False)
    v0 = start_vector(N, 0).double().numpy()
    for n_iters in (30, 60, 120):
        lip, grow, ray, rho, lipd = numpy_power(J, JD, v0, n_iters, 10)
        if lip[-1] >= 0.99 * sv[0] and lipd[-1] >= 0.99 * svd_[0]:
            break
    else:
        return False
    ev, evd = np.linalg.eigvals(J), np.linalg.eigvals(JD)
    # the dense matrices themselves (128 KiB each) would not fit the size limit of a golden file: they are stored through their action,
    # and their transposes' action, on 8 seeded probe vectors (columns; J in (H,W,B) order, JD in the planar (B,H,W) order)
    probes = np.stack([start_vector(N, 1000 + k).double().numpy() for k in range(8)], axis=1)
    T = torch.from_numpy
    out.update({p + "z": z, p + "y": case.y, p + "Phi": case.Phi, p + "Phi_sum": case.Phi_sum, p + "sigma": torch.tensor(case.sigma, dtype=torch.float64),
                p + "probes": T(probes), p + "J_probes": T(J @ probes), p + "JT_probes": T(J.T @ probes),
                p + "JD_probes": T(JD @ probes), p + "JDT_probes": T(JD.T @ probes), p + "svd_J": T(sv), p + "svd_JD": T(svd_), p + "eig_J_re": T(ev.real.copy()),
                p + "eig_J_im": T(ev.imag.copy()), p + "eig_JD_re": T(evd.real.copy()), p + "eig_JD_im": T(evd.imag.copy()),
                p + "n_iters": torch.tensor(n_iters), p + "window": torch.tensor(10), p + "lip_hist": T(lip), p + "growth": T(grow),
                p + "rayleigh": T(ray), p + "rho": torch.tensor(rho, dtype=torch.float64), p + "lipd_hist": T(lipd), p + "pin": torch.tensor(case.pin(z))})
    print(f"   dense {case.name}: sigma_max(J_f) {sv[0]:.6f}  rho(J_f) {np.abs(ev).max():.6f}  sigma_max(J_D) {svd_[0]:.6f}  n_iters {n_iters}"
          f"  power: lip {lip[-1]:.6f} rho {rho:.6f} lipD {lipd[-1]:.6f}")
    return True


def main():
    out = {}
    for name in ("SimpleCNN", "RealSN_SimpleCNN", "ffdnet_s0", "ffdnet_s1"):
        for k in range(64):                                      # (a): the first crop whose ReLU decisions fp32 resolves
            r0, c0 = 96 + 16 * (k // 8), 64 + 16 * (k % 8)
            y, Phi, Phi_sum, gt = problem(16, 16, 8, r0, c0)
            case = Case(name, y, Phi, Phi_sum)
            z = point(name, y, Phi, Phi_sum, gt).double()
            ok, margin = decisions_resolved(case, z)
            if ok:
                break
        else:
            raise RuntimeError(f"{name}: no crop whose decisions fp32 resolves")
        products(case, z, out, f"{name}/a_")
        out[f"{name}/a_crop"] = torch.tensor([r0, c0])
        print("(a)", name, "crop", (r0, c0), "decision margin", margin, "fd_rel", float(out[f"{name}/a_fd_rel"]), "pin", float(out[f"{name}/a_pin"]))
        for k in range(8):                                       # (b): the first crop whose numpy power iteration meets the 0.99 condition
            y, Phi, Phi_sum, gt = problem(8, 8, 2, 96 + 8 * k, 64)
            case = Case(name, y, Phi, Phi_sum)
            if dense(case, point(name, y, Phi, Phi_sum, gt).double(), out, f"{name}/b_"):
                out[f"{name}/b_crop"] = torch.tensor(k)
                break
        else:
            raise RuntimeError(f"{name}: no dense case meets the 0.99 condition")
    fn = HERE + "/jacobian.npz"
    arrays = {k: np.asarray(v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    for k, a in arrays.items():                                  # what the reference produced in fp32 is stored as fp32 (exactly)
        if a.dtype == np.float64 and a.size > 16 and np.array_equal(a.astype(np.float32).astype(np.float64), a):
            arrays[k] = a.astype(np.float32)
    np.savez_compressed(fn, **arrays)
    print("->", fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
