"""Jacobian diagnostics of the fixed-point map: the two local numbers that say whether z -> f(z) = z1 - D(z1), z1 = P z + c, converges.

    lipschitz_f         the largest singular value of J_f at the point = the local Lipschitz constant of f.  Power iteration on
                        J^T J:  w = J v_k,  v_{k+1} = J^T w / |J^T w|;  the estimate after step k is |J v_k|, the square root of a
                        Rayleigh quotient of the symmetric J^T J, so it is non-decreasing in k and never above sigma_max.
    rho_f               the spectral radius of J_f.  v_{k+1} = J v_k / |J v_k|; the history holds the growth factors |J v_k| and the
                        Rayleigh quotients <v_k, J v_k>.  J is NOT normal and its dominant eigenvalues may be a complex pair: a single
                        Rayleigh quotient (or a single growth factor) then oscillates with the phase of the pair instead of converging.
                        The product of m consecutive growth factors is |J^m v| / |v| -> rho^m, so rho_f is the GEOMETRIC MEAN OF THE
                        LAST `window` GROWTH FACTORS, which averages over the rotation; the Rayleigh quotients are returned for reading
                        (they settle on rho only for a real, simple dominant eigenvalue).
    lipschitz_denoiser  the same J^T J iteration on J_D alone, D the noise predictor - the quantity RealSN bounds by 1.

All three per sample (measurement) of the batch: vectors (bsz,H,W,B) for f, the denoiser's planar (bsz*B,1,H,W) viewed per measurement for
D.  The start vector comes from a seeded CPU generator, drawn in fp32, normalised and copied to the device; EVERY sample starts from the
same vector, so a measurement's numbers do not depend on what else is in the batch.  The device loop is the products
(EquilibriumProxGradSCI.device_jacobian: masked HIP layers) plus csrc/jacobian.hip's power step - per-sample norms, inner products and the
renormalisation in two launches, nothing read back; the float64 table crosses to the host once at the end.  power_report_host is the
float64 CPU twin over the host plans of deqsci_amd/vjp.py (HostMapJacobian), started from the identical vector.
"""
import numpy as np
import torch

from . import _hip, vjp as _vjp

OF = ("f", "denoiser")


def start_vector(N, seed=0):
    """The (N,) fp32 start vector of every sample: seeded CPU generator, drawn in fp32, normalised (in float64, rounded once)."""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randn(int(N), generator=g, dtype=torch.float32).double()
    return (v / v.norm()).float()


def _check(n_iters, window, of):
    if int(n_iters) < 1 or int(window) < 1 or int(window) > int(n_iters):
        raise ValueError(f"power_report: 1 <= window <= n_iters required, got n_iters={n_iters}, window={window}")
    of = tuple(of)
    if not of or any(o not in OF for o in of):
        raise ValueError(f"power_report: of={of!r}: a non-empty subset of {OF}")
    return int(n_iters), int(window), of


class _DeviceSteps:
    """The power step on the device: rows of a (3 * n_iters, bsz, 2) float64 table, one scratch row, one workspace - allocated once."""

    def __init__(self, bsz, N, n_rows, device):
        self.table = torch.full((n_rows + 1, bsz, 2), float("nan"), device=device, dtype=torch.float64)
        self.ws = _hip.power_workspace(bsz, N, device)
        self.bsz, self.N = bsz, N

    def start(self, v0, shape):
        return v0.to(self.table.device).view(1, -1).expand(self.bsz, -1).contiguous().view(shape)

    def step(self, w, v_prev, row):
        """table[row] = (|w|^2, <v_prev, w>) per sample; -> w / |w| (in place).  row None: the scratch row."""
        flat = w.view(self.bsz, self.N)
        _hip.power_step(flat, None if v_prev is None else v_prev.view(self.bsz, self.N), flat, self.table[-1 if row is None else row], self.ws)
        return w

    def rows(self, lo, hi):
        return self._host[lo:hi]

    def finish(self):
        self._host = self.table[:-1].cpu().numpy()            # the one copy back


class _HostSteps:
    def __init__(self, bsz, N, n_rows):
        self._host = np.full((n_rows, bsz, 2), np.nan)
        self.bsz, self.N = bsz, N

    def start(self, v0, shape):
        return v0.double().view(1, -1).expand(self.bsz, -1).contiguous().view(shape)

    def step(self, w, v_prev, row):
        flat = w.reshape(self.bsz, self.N)
        a = (flat * flat).sum(dim=1)
        ok = (a > 0) & torch.isfinite(a)
        if row is not None:
            b = (v_prev.reshape(self.bsz, self.N) * flat).sum(dim=1) if v_prev is not None else torch.full_like(a, float("nan"))
            nan = torch.full_like(a, float("nan"))
            self._host[row, :, 0] = torch.where(ok, a, nan).numpy()
            self._host[row, :, 1] = torch.where(ok, b, nan).numpy()
        scale = torch.where(ok, 1.0 / torch.sqrt(torch.where(ok, a, torch.ones_like(a))), torch.zeros_like(a))
        return (torch.where(ok.view(-1, 1), flat, torch.zeros_like(flat)) * scale.view(-1, 1)).reshape(w.shape)

    def rows(self, lo, hi):
        return self._host[lo:hi]

    def finish(self):
        pass


def _gram_iteration(fwd, bwd, v, steps, row0, n_iters):
    """Power iteration on J^T J: rows row0 .. row0 + n_iters - 1 receive (|J v_k|^2, <v_k, J v_k>)."""
    for k in range(n_iters):
        w = steps.step(fwd(v), v, row0 + k)
        v = steps.step(bwd(w), None, None)


def _plain_iteration(fwd, v, steps, row0, n_iters):
    """v <- J v / |J v|: rows row0 .. receive the squared growth factors and the Rayleigh quotients."""
    for k in range(n_iters):
        v = steps.step(fwd(v), v, row0 + k)


def _report(op, shape, steps, n_iters, window, seed, of):
    bsz, H, W, B = shape
    v0 = start_vector(H * W * B, seed)
    dshape = (bsz * B, 1, H, W)
    row = 0
    with torch.no_grad():
        if "f" in of:
            _gram_iteration(op.jv, op.jtv, steps.start(v0, shape), steps, 0, n_iters)
            _plain_iteration(op.jv, steps.start(v0, shape), steps, n_iters, n_iters)
            row = 2 * n_iters
        if "denoiser" in of:
            _gram_iteration(op.denoiser.jvp, op.denoiser.vjp, steps.start(v0, dshape), steps, row, n_iters)
    steps.finish()
    out = {"n_iters": n_iters, "window": window, "seed": int(seed)}
    with np.errstate(invalid="ignore", divide="ignore"):
        if "f" in of:
            hist = np.sqrt(steps.rows(0, n_iters)[:, :, 0])
            grow = np.sqrt(steps.rows(n_iters, 2 * n_iters)[:, :, 0])
            out.update(lipschitz_f=hist[-1].copy(), lipschitz_f_history=hist, rho_f_growth=grow,
                       rho_f_rayleigh=steps.rows(n_iters, 2 * n_iters)[:, :, 1].copy(),
                       rho_f=np.exp(np.log(grow[-window:]).mean(axis=0)))
        if "denoiser" in of:
            hist = np.sqrt(steps.rows(row, row + n_iters)[:, :, 0])
            out.update(lipschitz_denoiser=hist[-1].copy(), lipschitz_denoiser_history=hist)
    return out


def power_report(op, shape, n_iters=30, window=10, seed=0, of=OF):
    """op: EquilibriumProxGradSCI.device_jacobian(...) (.jv, .jtv on (bsz,H,W,B); .denoiser.jvp, .vjp on (bsz*B,1,H,W)); shape
    (bsz,H,W,B).  -> float64 numpy arrays, one value per sample: "lipschitz_f", "rho_f", "lipschitz_denoiser" (those `of` asks for), and the
    histories (n_iters, bsz): "lipschitz_f_history", "rho_f_growth", "rho_f_rayleigh", "lipschitz_denoiser_history".  A sample whose
    iteration meets a zero or non-finite vector reports NaN.  One host synchronisation: the copy of the table at the end."""
    n_iters, window, of = _check(n_iters, window, of)
    bsz, H, W, B = (int(s) for s in shape)
    device = op.Phi.device if hasattr(op, "Phi") else torch.device("cuda")
    steps = _DeviceSteps(bsz, H * W * B, 3 * n_iters, device)
    return _report(op, (bsz, H, W, B), steps, n_iters, window, seed, of)


def power_report_host(op, shape, n_iters=30, window=10, seed=0, of=OF):
    """power_report's float64 CPU twin: op with the same four products on float64 CPU tensors (HostMapJacobian, or any linear maps)."""
    n_iters, window, of = _check(n_iters, window, of)
    bsz, H, W, B = (int(s) for s in shape)
    return _report(op, (bsz, H, W, B), _HostSteps(bsz, H * W * B, 3 * n_iters), n_iters, window, seed, of)


class _HostDenoiser:
    def __init__(self, net, x, sigma, masks, mask_dtype):
        ok, why = _vjp.jacobian_eligibility(net)
        if not ok:
            raise ValueError(f"HostMapJacobian: {why}")
        xm = x if mask_dtype is None else x.to(mask_dtype)
        if why == _vjp.FFDNET_THROUGH_INPUT:
            if sigma is None:
                raise ValueError("HostMapJacobian: FFDNet is linearised at a noise level: sigma is required")
            _vjp._even(x, "HostMapJacobian")
            self.layers, self.edges = _vjp.ffdnet_plan(net), _vjp.FFDNET_EDGES
            self.masks = masks if masks is not None else _vjp.ffdnet_plan_forward(self.layers, xm, sigma)[1]
        else:
            self.layers, self.edges = _vjp.host_plan(net)[0], _vjp.PLAIN_EDGES
            self.masks = masks if masks is not None else _vjp.plan_masks(self.layers, xm)

    def jvp(self, v):
        return _vjp.masked_jvp(self.layers, self.masks, v, self.edges)

    def vjp(self, v):
        return _vjp.masked_vjp(self.layers, self.masks, v, self.edges)


class HostMapJacobian:
    """MapJacobian's host statement in `dtype` (float64) on the CPU over vjp.masked_jvp / masked_vjp: the same four products.
    masks: explicit ReLU masks ((bsz*B,64,H,W) bool per layer, e.g. the device's through vjp.unpack_masks) instead of those of the
    forward pass at z1; mask_dtype: the precision of that forward pass (torch.float32: the decisions an fp32 forward takes)."""

    def __init__(self, net, z, y, Phi, Phi_sum, sigma=None, masks=None, mask_dtype=None, dtype=torch.float64):
        to = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
        z, y, self.Phi, self.Phi_sum = to(z), to(y), to(Phi), to(Phi_sum)
        if self.Phi.dim() == 3:
            self.Phi = self.Phi[None]
        self.Phi_sum = self.Phi_sum.reshape(-1, z.shape[1], z.shape[2])
        self.shape = tuple(z.shape)
        bsz, H, W, B = self.shape
        z1 = z + ((y - (z * self.Phi).sum(dim=3)) / self.Phi_sum).unsqueeze(3) * self.Phi
        self.z1 = z1.permute(0, 3, 1, 2).contiguous().view(bsz * B, 1, H, W)
        if isinstance(sigma, torch.Tensor):
            sigma = sigma.detach().cpu().to(dtype)
        if masks is not None:
            masks = [m.cpu() for m in masks]
        self.denoiser = _HostDenoiser(net, self.z1, sigma, masks, mask_dtype)

    def _P(self, v):
        return v - ((v * self.Phi).sum(dim=3) / self.Phi_sum).unsqueeze(3) * self.Phi

    def _planar(self, v):
        bsz, H, W, B = self.shape
        return v.permute(0, 3, 1, 2).contiguous().view(bsz * B, 1, H, W)

    def _hwb(self, p):
        bsz, H, W, B = self.shape
        return p.view(bsz, B, H, W).permute(0, 2, 3, 1).contiguous()

    def jv(self, v):
        pv = self._P(v)
        return pv - self._hwb(self.denoiser.jvp(self._planar(pv)))

    def jtv(self, v):
        return self._P(v - self._hwb(self.denoiser.vjp(self._planar(v))))
