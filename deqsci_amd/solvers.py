"""Drop-in solver surface of the reference, backed by the HIP kernels.

    EquilibriumProxGradSCI(A, At, nonlinear_operator, eta, minval, maxval).forward(z, y, Phi, Phi_sum)
                                   solvers/equilibrium_solvers_yaping.py:382-436
    andersonexp(f, x0, m, lam, max_iter, tol, beta) -> (z, res)
                                   solvers/new_equilibrium_utils_yaping.py:153-189
    forward_iteration(f, x0, max_iter, tol) -> (z, [res])            ibid. :213-222
    DEQFixedPoint(f, solver, **kwargs).forward(y, Phi, Phi_sum, initial_point, train_flag)
                                   ibid. :241-281 (inference; with a tape: the training forward + backward hook)

Same names, argument meaning and error behaviour, tensors in the reference's (bsz,H,W,B) layout.
`andersonexp` / `forward_iteration` accept ANY callable f (kernels K4-K7 on flat (bsz,N) views, one
residual read-back per iteration exactly like the reference's `.item()`); when DEQFixedPoint is
given this module's EquilibriumProxGradSCI together with one of these two iterators it routes the
whole loop to deqsci_amd.engine.DEQSCIEngine (planar state, fused kernels, no per-iteration sync).
"""
import torch
import torch.nn as nn

from . import _hip, autograd as _ag, vjp as _vjp
from ._hip import LAYOUT_BHW, LAYOUT_HWB
from .engine import SIGMA0, SIGMA_DECAY, DEQSCIEngine, sigma_schedule
from .operators import A_torch_, At_torch_


class EquilibriumProxGradSCI(nn.Module):
    def __init__(self, A, At, nonlinear_operator, eta, minval=-1, maxval=1):
        super().__init__()
        self.A = A
        self.At = At
        self.nonlinear_op = nonlinear_operator
        self.minval = minval
        self.maxval = maxval
        self.y = 0
        self.noise_sigma = None
        self._y_ref = None          # the measurement tensor of the previous call (held, so its storage cannot be recycled)
        self._y_ver = -1
        self._taped = None          # (z1 planar (bsz*B,1,H,W), sigma or None) of the last taped call: the point device_vjp linearises at

    def _sigma(self, y, n):
        """sigma bookkeeping of :408-413: restart at 60/255 when y.mean() changes, else *0.971.
        The reference compares the means on every call (one host sync each); here the comparison is skipped only when
        the SAME tensor object, unmodified, is passed again - which is how the DEQ loop calls f."""
        if y is self._y_ref and y._version == self._y_ver:
            changed = False
        else:
            ym = y.mean()
            changed = bool(torch.as_tensor(self.y != ym))
            self.y = ym
            self._y_ref, self._y_ver = y, y._version
        if changed or self.noise_sigma is None:
            self.noise_sigma = torch.full((1,), SIGMA0, dtype=torch.float32, device=y.device).expand(n)
        else:
            self.noise_sigma = self.noise_sigma * SIGMA_DECAY
        return self.noise_sigma

    def _sigma_resume(self, y, n, sigma):
        """Leave the sigma bookkeeping where f-calls made elsewhere (the engine's solve of a training step, which reads sigma from its table)
        left it: `sigma` (one element) is the noise level of the last of those calls on y, so the next _sigma(y, n) decays it once more."""
        self.y = y.mean()
        self._y_ref, self._y_ver = y, y._version
        self.noise_sigma = sigma.reshape(1).to(torch.float32).expand(n)

    def _forward_taped(self, z, y, Phi, Phi_sum):
        """The same map with autograd recording (training: :268-272 of the DEQ wrapper call f with the tape on): the GAP
        projection is the HIP kernel behind an autograd.Function, the denoiser is the PyTorch module itself and the
        layout shuffles are torch views, exactly the operations of :399-420."""
        bsz, w, h, c = z.shape
        op = self.nonlinear_op
        tag = getattr(op, "tag", None)
        if self.A is A_torch_ and self.At is At_torch_:
            z1 = _ag.gap_update(z, y, Phi, Phi_sum)
        else:
            z1 = z + self.At((y - self.A(z, Phi)) / Phi_sum, Phi)
        zp = z1.permute(0, 3, 1, 2).contiguous()
        self._taped = (zp.detach().view(bsz * c, 1, w, h), None)
        if tag == 'conv2d':
            return op(zp.view(bsz * c, 1, w, h)).view(bsz, c, w, h).permute(0, 2, 3, 1)
        if tag == 'conv3d':
            return op(zp.view(bsz, 1, c, w, h)).view(bsz, c, w, h).permute(0, 2, 3, 1)
        if tag == 'ffdnet':
            sigma = self._sigma(y, bsz * c)
            self._taped = (self._taped[0], sigma)
            noise = op(zp.view(bsz * c, 1, w, h), sigma)
        elif tag == 'denoiser':
            noise = op(zp.view(bsz * c, 1, w, h))
        elif tag == '3d_denoiser':
            noise = op(zp.view(bsz, 1, c, w, h))
        else:
            print('unknown nonlinear_op tag!')
            raise UnboundLocalError("local variable 'z_tplus1' referenced before assignment")
        return z1 - noise.view(bsz, c, w, h).permute(0, 2, 3, 1)

    def _param_mode(self, modes):
        """(mode, reason): the first of the vjp.GradModes `modes` (vjp.switch_modes: what a parameter_backward string serves, in order) whose
        DenoiserParamGrads serves the denoiser - or (None, why not): a refusal may name the mode the net belongs to instead
        (vjp._Refusal.other), and the reason is found by following those names from the first mode, until one names no mode tried or one passed already."""
        op = self.nonlinear_op
        if not (self.A is A_torch_ and self.At is At_torch_):
            return None, "custom A / At: the device call uses the HIP GAP projection"
        whys = {}
        for mode in modes:
            ok, why = mode.eligibility(op)
            if ok:
                if isinstance(op, _vjp._modules()[1]) and getattr(op, "tag", None) != "ffdnet":
                    return None, f"FFDNet under nonlinear_op tag {getattr(op, 'tag', None)!r}: it gets its noise level under 'ffdnet' only"
                return mode, why
            whys[mode.name] = why
        name, passed = modes[0].name, []
        while name not in passed:
            passed.append(name)
            other = getattr(whys[name], "other", None)
            if other not in whys:
                break
            name = other
        return None, whys[name]

    @staticmethod
    def _keyword_modes(who, frozen_bn, train_bn, train_realsn):
        """The modes the keywords ask to try: those of the switch of the one they name - train_realsn before train_bn before frozen_bn."""
        return _vjp.switch_modes(_vjp.grad_mode(who, frozen_bn and not (train_bn or train_realsn), train_bn and not train_realsn, train_realsn).switch)

    def device_param_eligibility(self, frozen_bn=False, train_bn=False, train_realsn=False):
        """(ok, reason): whether forward_param_device can serve this map under the same keywords: HIP GAP operators, and a denoiser one of the
        modes the keyword's switch serves accepts (vjp.GRAD_MODES; FFDNet under tag 'ffdnet' only)."""
        mode, why = self._param_mode(self._keyword_modes("device_param_eligibility", frozen_bn, train_bn, train_realsn))
        return mode is not None, why

    def forward_param_device(self, z, y, Phi, Phi_sum, frozen_bn=False, train_bn=False, train_realsn=False):
        """The taped call f(z) = z1 - D(z1) whose backward forms the denoiser's weight gradients on the HIP kernels: gap_update ->
        autograd.denoiser_noise (vjp.DenoiserParamGrads) -> z1 - noise.  The torch module itself is not called.  Serves what
        device_param_eligibility accepts under the same keywords, in the first mode that does; FFDNet with _forward_taped's sigma
        bookkeeping.  A train mode moves the module's buffers once, as its own forward would."""
        mode, why = self._param_mode(self._keyword_modes("forward_param_device", frozen_bn, train_bn, train_realsn))
        if mode is None:
            raise ValueError(f"forward_param_device: {why}")
        return self._forward_param(mode, z, y, Phi, Phi_sum)

    def _forward_param(self, mode, z, y, Phi, Phi_sum):
        """forward_param_device on the vjp.GradMode _param_mode answered."""
        bsz, w, h, c = z.shape
        op = self.nonlinear_op
        z1 = _ag.gap_update(z, y, Phi, Phi_sum)
        zp = z1.permute(0, 3, 1, 2).contiguous()
        self._taped = (zp.detach().view(bsz * c, 1, w, h), None)
        sigma = None
        if isinstance(op, _vjp._modules()[1]):
            sigma = self._sigma(y, bsz * c)
            self._taped = (self._taped[0], sigma)
        noise = _ag.denoiser_noise(op, zp.view(bsz * c, 1, w, h), sigma, mode=mode)
        return z1 - noise.view(bsz, c, w, h).permute(0, 2, 3, 1)

    def device_vjp_eligibility(self, train_realsn=False):
        """(ok, reason): whether device_vjp can serve this map (HIP GAP operators and a denoiser deqsci_amd.vjp.eligibility accepts;
        train_realsn=True: also a train-mode RealSN net, vjp.eligibility(net, train_realsn=True))."""
        if not (self.A is A_torch_ and self.At is At_torch_):
            return False, "custom A / At: the device map uses the HIP GAP projection"
        return _vjp.eligibility(self.nonlinear_op, train_realsn)

    def device_vjp(self, Phi, Phi_sum, train_realsn=False):
        """The map v -> J_f(z0)^T v = P (v - J_D(z1)^T v) of the LAST taped call f(z0) (its z1 and sigma: no further call of f, the
        sigma state stays where that call left it), on the HIP kernels: v and the result (bsz,H,W,B) fp32 on the GPU, no host sync."""
        if self._taped is None:
            raise RuntimeError("device_vjp: no taped call of this map to linearise at")
        ok, why = self.device_vjp_eligibility(train_realsn)
        if not ok:
            raise ValueError(f"device_vjp: {why}")
        z1p, sigma = self._taped
        jd = _vjp.DenoiserVJP(self.nonlinear_op, z1p, sigma, train_realsn)
        Phi, Phi_sum = _hip.f32c(Phi), _hip.f32c(Phi_sum)
        zero_y = None

        def jmap(v):
            nonlocal zero_y
            v = _hip.f32c(v)
            if zero_y is None:
                zero_y = torch.zeros(v.shape[:3], device=v.device, dtype=torch.float32)
            if not jd.zero:
                vp = _hip.transpose(v, LAYOUT_BHW)                                    # (bsz,B,H,W) = the denoiser's (bsz*B,1,H,W)
                v = _hip.residual_out(vp, jd(vp.view(jd.shape)).view(vp.shape), LAYOUT_HWB)   # v - J_D^T v, back in (bsz,H,W,B)
            return _hip.gap_update(v, Phi, zero_y, Phi_sum, LAYOUT_HWB, LAYOUT_HWB)
        return jmap

    def device_jacobian_eligibility(self):
        """(ok, reason): whether device_jacobian can serve this map (HIP GAP operators and a denoiser vjp.jacobian_eligibility accepts)."""
        if not (self.A is A_torch_ and self.At is At_torch_):
            return False, "custom A / At: the device map uses the HIP GAP projection"
        return _vjp.jacobian_eligibility(self.nonlinear_op)

    def device_jacobian(self, z, y, Phi, Phi_sum, sigma=None):
        """The Jacobian of this map at an explicit point z (bsz,H,W,B), in both directions on the HIP kernels (a diagnostic:
        deqsci_amd.jacobian.power_report).  z1 = P z + c comes from the GAP kernel itself; nothing here calls f or advances the sigma
        state - FFDNet is linearised through its input at the given sigma (a float or a tensor of 1 or bsz*B elements).  -> a
        MapJacobian: .jv(v) = (I - J_D(z1)) (P v), .jtv(v) = P (v - J_D(z1)^T v) on (bsz,H,W,B) fp32 GPU tensors, P = gap_update with
        y = 0 as in device_vjp, and .denoiser, the DenoiserJacobian at z1.  No host synchronisation."""
        ok, why = self.device_jacobian_eligibility()
        if not ok:
            raise ValueError(f"device_jacobian: {why}")
        if z.dim() != 4 or not z.is_cuda:
            raise _hip.DeqsciHipError(f"device_jacobian: z must be a (bsz,H,W,B) GPU tensor, got {tuple(z.shape)} on {z.device}")
        bsz, H, W, B = z.shape
        Phi, Phi_sum = _hip.f32c(Phi), _hip.f32c(Phi_sum)
        with torch.no_grad():
            z1 = _hip.gap_update(_hip.f32c(z.detach()), Phi, _hip.f32c(y), Phi_sum, LAYOUT_HWB, LAYOUT_BHW)
            jd = _vjp.DenoiserJacobian(self.nonlinear_op, z1.view(bsz * B, 1, H, W), sigma)
        return MapJacobian(jd, Phi, Phi_sum, (bsz, H, W, B))

    def forward(self, z, y, Phi, Phi_sum):
        bsz, w, h, c = z.shape
        op = self.nonlinear_op
        tag = getattr(op, "tag", None)
        if torch.is_grad_enabled() and (_ag.taping(z, y, Phi, Phi_sum) or any(p.requires_grad for p in op.parameters())):
            return self._forward_taped(z, y, Phi, Phi_sum)
        if self.A is A_torch_ and self.At is At_torch_:
            # K3 fused with the permute(0,3,1,2).contiguous() of :415/:419
            z1 = _hip.gap_update(_hip.f32c(z), _hip.f32c(Phi), _hip.f32c(y), _hip.f32c(Phi_sum), LAYOUT_HWB, LAYOUT_BHW)
        else:
            fb = self.A(z, Phi)
            z1 = _hip.transpose(_hip.f32c(z + self.At((y - fb) / Phi_sum, Phi)), LAYOUT_BHW)
        if tag == 'conv2d':
            out = op(z1.view(bsz * c, 1, w, h))
            return _hip.transpose(_hip.f32c(out.reshape(bsz, c, w, h)), LAYOUT_HWB)
        if tag == 'conv3d':
            out = op(z1.view(bsz, 1, c, w, h))
            return _hip.transpose(_hip.f32c(out.reshape(bsz, c, w, h)), LAYOUT_HWB)
        if tag == 'ffdnet':
            noise = op(z1.view(bsz * c, 1, w, h), self._sigma(y, bsz * c))
        elif tag == 'denoiser':
            noise = op(z1.view(bsz * c, 1, w, h))
        elif tag == '3d_denoiser':
            noise = op(z1.view(bsz, 1, c, w, h))
        else:
            print('unknown nonlinear_op tag!')
            raise UnboundLocalError("local variable 'z_tplus1' referenced before assignment")
        return _hip.residual_out(z1, _hip.f32c(noise.reshape(bsz, c, w, h)), LAYOUT_HWB)


class MapJacobian:
    """J_f at a point, f(z) = z1 - D(z1), z1 = P z + c (EquilibriumProxGradSCI.device_jacobian): v and the results (bsz,H,W,B) fp32."""

    def __init__(self, denoiser, Phi, Phi_sum, shape):
        self.denoiser, self.Phi, self.Phi_sum, self.shape = denoiser, Phi, Phi_sum, tuple(shape)
        self._zero_y = torch.zeros(self.shape[:3], device=Phi.device, dtype=torch.float32)

    def _v(self, v):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"MapJacobian: v must have the shape {self.shape} of z, got {tuple(v.shape)}")
        return _hip.f32c(v)

    def jv(self, v):
        pv = _hip.gap_update(self._v(v), self.Phi, self._zero_y, self.Phi_sum, LAYOUT_HWB, LAYOUT_BHW)      # P v, planar
        return _hip.residual_out(pv, self.denoiser.jvp(pv.view(self.denoiser.shape)).view(pv.shape), LAYOUT_HWB)

    def jtv(self, v):
        vp = _hip.transpose(self._v(v), LAYOUT_BHW)
        u = _hip.residual_out(vp, self.denoiser.vjp(vp.view(self.denoiser.shape)).view(vp.shape), LAYOUT_HWB)
        return _hip.gap_update(u, self.Phi, self._zero_y, self.Phi_sum, LAYOUT_HWB, LAYOUT_HWB)


def andersonexp(f, x0, m=5, lam=1e-4, max_iter=50, tol=1e-5, beta=1.0, *, anderson_arith="reference"):
    """Anderson acceleration for fixed point iteration (generic f).
    anderson_arith (this build's keyword): "reference" - G G^T accumulated in fp32 along N and an fp32 LU, the arithmetic of the reference's
    torch.bmm + torch.solve (solvers/new_equilibrium_utils_yaping.py:177-180); "float64" - the exactly accumulated Gram."""
    if anderson_arith not in ("reference", "float64"):
        raise ValueError(f"anderson_arith={anderson_arith!r}: expected 'reference' or 'float64'")
    ref = anderson_arith == "reference"
    bsz = x0.shape[0]
    shape = x0.shape
    xa = _hip.f32c(x0).reshape(bsz, -1)
    N = xa.shape[1]
    if m < 2:
        raise IndexError("index 1 is out of bounds for dimension 1 with size %d" % m)
    ws = _hip.AndersonWorkspace(bsz, N, m, x0.device)
    xb = torch.empty_like(xa)
    flat = lambda t: _hip.f32c(t).reshape(bsz, N)
    _hip.residual_store(ws, flat(f(xa.view(shape))), None, xa, 0, 1, xb, ref=ref)       # X1 = F0
    _hip.anderson_solve(ws, 0, 1, 0, lam, 1e-5, ref=ref)
    _hip.residual_store(ws, flat(f(xb.view(shape))), None, xb, 1, 2, None, ref=ref)
    _hip.anderson_solve(ws, 1, 2, 2, lam, 1e-5, ref=ref)
    bufs = [xa.clone(), xb]
    cur = bufs[0]                                                              # X[:, 0] = x0 if the loop is skipped
    res = None
    for k in range(2, max_iter):
        n = min(k, m)
        cur = bufs[k % 2]
        _hip.anderson_mix(ws, cur, beta, n)
        nf = min(k + 1, m)
        _hip.residual_store(ws, flat(f(cur.view(shape))), None, cur, k % m, nf, None, ref=ref)
        _hip.anderson_solve(ws, k % m, nf, nf, lam, 1e-5, ref=ref)
        res = ws.res[0, 0].item()
        if res < tol:
            break
    if res is None:
        raise UnboundLocalError("local variable 'res' referenced before assignment")
    return cur.view(shape), res


def forward_iteration(f, x0, max_iter=50, tol=1e-5):
    bsz = x0.shape[0]
    shape = x0.shape
    f0 = f(x0)
    N = f0[0].numel()
    ws = _hip.AndersonWorkspace(bsz, N, 1, x0.device)
    res = []
    for k in range(max_iter):
        x = f0
        f0 = f(x)
        _hip.residual_store(ws, _hip.f32c(f0).reshape(bsz, N), None, _hip.f32c(x).reshape(bsz, N), 0, 1, None)
        _hip.anderson_solve(ws, 0, 1, 0, 0.0, 1e-7)
        res.append(ws.res[0, 0].item())
        if res[-1] < tol:
            break
    return f0, res


def _data(*tensors):
    """The measurement and the masks as data, for the graph J_f^T v is read from: J_f depends on their values only, and a tensor left on
    that graph would have its gradient formed again in every iteration of the backward solve.  (One that asks for no gradient is passed
    as it is, the same object.)"""
    return tuple(t.detach() if isinstance(t, torch.Tensor) and t.requires_grad else t for t in tensors)


class DEQFixedPoint(nn.Module):
    def __init__(self, f, solver, **kwargs):
        super().__init__()
        self.f = f
        self.solver = solver
        self.kwargs = kwargs
        self.forward_res = None
        self.use_engine = True
        self.engine_options = {}          # extra DEQSCIEngine arguments of this build, e.g. {"conv64": "fast32"} (fp32-MFMA kernels only)
        self._engine = None
        # how the backward hook of a taped forward forms J_f(z0)^T v: "autograd" (torch.autograd.grad through f0's graph, the reference's
        # way) or "device" (EquilibriumProxGradSCI.device_vjp: the HIP kernels, falling back to autograd where the denoiser has no device
        # VJP - deqsci_amd.vjp.eligibility).  last_backward_path: the path the last hook ran; backward_fallback_reason: why not "device".
        # this build's additions, engine path only (DEQSCIEngine.reconstruct): snapshots = iteration horizons whose reconstructions come out
        # of the same run (-> last_snapshots, {K: {"rec", "res", "res_per_sample"}}); trace = the residual (and, with trace_gt - the ground
        # truth (bsz,H,W,B) on the device - the PSNR) of every f-call (-> last_trace).  forward's signature stays the reference's.
        self.snapshots, self.trace, self.trace_gt = None, False, None
        self.last_snapshots, self.last_trace = None, None
        self.implicit_backward = "autograd"
        self.last_backward_path = None
        self.backward_fallback_reason = None
        # how the taped call z = f(z*) forms the denoiser's weight gradients: "autograd" (the torch module on the tape: MIOpen backward) or
        # the switch of a mode of vjp.GRAD_MODES - "device", "device+realsn", "device+bn", "device+bn-train" (EquilibriumProxGradSCI.forward_param_device
        # in the first mode the switch serves that accepts the denoiser, falling back to autograd where all of them refuse).
        # last_parameter_path: the path of the last taped forward ("device" when served); parameter_fallback_reason: why not.
        # Independent of implicit_backward.
        self.parameter_backward = "autograd"
        self.last_parameter_path = None
        self.parameter_fallback_reason = None

    def _engine_for(self):
        f = self.f.module if isinstance(self.f, nn.DataParallel) else self.f
        if not (self.use_engine and isinstance(f, EquilibriumProxGradSCI) and f.A is A_torch_ and f.At is At_torch_):
            return None
        if getattr(f.nonlinear_op, "tag", None) not in ("conv2d", "conv3d", "ffdnet", "denoiser", "3d_denoiser"):
            return None
        kw = dict(self.kwargs)
        if self.solver is andersonexp:
            # (the reference's API gets the reference's arithmetic for alpha - an fp32 Gram - unless told otherwise: DESIGN section 5, "Config 2")
            cfg = dict(iterator="anderson", m=kw.pop("m", 5), lam=kw.pop("lam", 1e-4), max_iter=kw.pop("max_iter", 50),
                       tol=kw.pop("tol", 1e-5), beta=kw.pop("beta", 1.0), anderson_arith=kw.pop("anderson_arith", "reference"))
        elif self.solver is forward_iteration:
            cfg = dict(iterator="picard", max_iter=kw.pop("max_iter", 50), tol=kw.pop("tol", 1e-5))
        else:
            return None
        if kw:
            raise TypeError(f"{self.solver.__name__}() got an unexpected keyword argument '{next(iter(kw))}'")
        key = (id(f.nonlinear_op), f.nonlinear_op.training, tuple(sorted(cfg.items())), tuple(sorted(self.engine_options.items())))
        if self._engine is None or self._engine[0] != key:
            self._engine = (key, DEQSCIEngine(f.nonlinear_op, **{**cfg, **self.engine_options}))
        return self._engine[1]

    def _train_solve_engine(self):
        """The engine that runs a training step's no-tape solve: a vjp.GradMode.engine_option is set, f is on the engine's path (not a
        DataParallel) and the denoiser is in train mode and served by that option - else None, and the solve takes the solver as it always did."""
        asked = any(self.engine_options.get(m.engine_option[0]) == m.engine_option[1] for m in _vjp.GRAD_MODES if m.engine_option)
        if not asked or isinstance(self.f, nn.DataParallel):
            return None
        eng = self._engine_for()
        if eng is None:
            return None
        eng.den._refresh()
        return eng if eng.train_mode_on_device() else None

    def _device_map(self, Phi, Phi_sum):
        """implicit_backward = "device": the device map of the taped call just made, or None (autograd) with the reason recorded."""
        if self.implicit_backward not in ("autograd", "device", "device+realsn"):
            raise ValueError(f"implicit_backward={self.implicit_backward!r}: expected 'autograd' or 'device' - or 'device+realsn', which adds "
                             "RealSNConv2d in train mode")
        realsn = self.implicit_backward == "device+realsn"
        self.backward_fallback_reason = None
        if self.implicit_backward == "autograd":
            return None
        if isinstance(self.f, nn.DataParallel) and len(self.f.device_ids or []) > 1:
            self.backward_fallback_reason = "DataParallel over several devices (the taped call ran on replicas)"
            return None
        f = self.f.module if isinstance(self.f, nn.DataParallel) else self.f
        if not isinstance(f, EquilibriumProxGradSCI):
            self.backward_fallback_reason = f"f is a {type(f).__name__}, not this package's EquilibriumProxGradSCI"
            return None
        ok, why = f.device_vjp_eligibility(realsn)
        if not ok:
            self.backward_fallback_reason = why
            return None
        return f.device_vjp(Phi, Phi_sum, realsn)

    def _taped_call(self, z, x, Phi, Phi_sum):
        """The taped call z = f(z*) (:268): on the device's weight-gradient path where parameter_backward asks for it and it is served."""
        modes = None if self.parameter_backward == "autograd" else _vjp.switch_modes(self.parameter_backward)
        if modes is None and self.parameter_backward != "autograd":
            raise ValueError(f"parameter_backward={self.parameter_backward!r}: expected 'autograd', 'device' or 'device+bn' - or 'device+bn-train', "
                             "which adds BatchNorm2d in train mode, or 'device+realsn', which adds RealSNConv2d in train mode")
        self.parameter_fallback_reason = None
        self.last_parameter_path = "autograd"
        if modes is not None:
            f = self.f.module if isinstance(self.f, nn.DataParallel) else self.f
            if isinstance(self.f, nn.DataParallel) and len(self.f.device_ids or []) > 1:
                self.parameter_fallback_reason = "DataParallel over several devices (the taped call runs on replicas)"
            elif not isinstance(f, EquilibriumProxGradSCI):
                self.parameter_fallback_reason = f"f is a {type(f).__name__}, not this package's EquilibriumProxGradSCI"
            else:
                mode, why = f._param_mode(modes)
                if mode is not None:
                    self.last_parameter_path = "device"
                    return f._forward_param(mode, z, x, Phi, Phi_sum)
                self.parameter_fallback_reason = why
        return self.f(z, x, Phi, Phi_sum)

    def jacobian_at(self, y, Phi, Phi_sum, z):
        """f's Jacobian at z - the reconstruction the last forward(y, ...) returned - as EquilibriumProxGradSCI.device_jacobian gives it
        (.jv, .jtv, .denoiser).  FFDNet is linearised at the sigma of the f-call that produced that reconstruction: row rec_call of the
        engine's sigma table, rec_call = the engine's call count less the calls behind it (the extra call, the snapshots' extra calls).
        NotImplementedError with the reason for what cannot be served: custom A / At, a denoiser without a device Jacobian, FFDNet
        off the engine's path."""
        f = self.f.module if isinstance(self.f, nn.DataParallel) else self.f
        if not isinstance(f, EquilibriumProxGradSCI):
            raise NotImplementedError(f"jacobian_report: f is a {type(f).__name__}, not this package's EquilibriumProxGradSCI")
        ok, why = f.device_jacobian_eligibility()
        if not ok:
            raise NotImplementedError(f"jacobian_report: {why}")
        sigma = None
        if getattr(f.nonlinear_op, "tag", None) == "ffdnet":
            eng = self._engine[1] if self._engine else None
            info = getattr(eng, "last_info", None)
            if not info:
                raise NotImplementedError("jacobian_report: FFDNet's sigma is read from the engine's table at the call count of the last "
                                          "forward, and no forward has run on the engine's path")
            snaps = info.get("snapshots") or {}
            rec_call = info["f_calls"] - 1 - int(bool(eng.extra_call)) - sum(1 for K in snaps if info["iterations"] >= K - 1)
            sigma = torch.from_numpy(sigma_schedule(rec_call + 1)[rec_call:]).to(z.device)      # (the engine's table: row rec_call)
        return f.device_jacobian(z, y, Phi, Phi_sum, sigma=sigma)

    def jacobian_report(self, y, Phi, Phi_sum, z, **kw):
        """The local Lipschitz constant and the spectral radius of f, and the Lipschitz constant of the noise predictor, at z - the
        reconstruction the last forward(y, ...) returned: deqsci_amd.jacobian.power_report (**kw: its n_iters, window, seed, of) on
        self.jacobian_at(y, Phi, Phi_sum, z), whose refusals (NotImplementedError) are this method's."""
        from . import jacobian as _jac
        return _jac.power_report(self.jacobian_at(y, Phi, Phi_sum, z), tuple(z.shape), **kw)

    def forward(self, x, Phi, Phi_sum, initial_point=None, train_flag=True):
        """x is the measurement y.  Without a tape (torch.no_grad(), or neither a parameter of f nor y, Phi, Phi_sum requiring a gradient) this is the
        inference path; with one it is the reference's training forward (:249-281): solve without tape, one taped f call,
        and the implicit-differentiation hook that solves  g = J_f^T g + grad  with the same solver and settings
        (`self.backward_res`).  `train_flag=False` skips the tape even when one could be recorded (the reference has that
        switch commented out, :277-279, and always records)."""
        init_point = torch.zeros_like(x) if initial_point is None else initial_point
        extras = self.snapshots is not None or bool(self.trace) or self.trace_gt is not None
        if train_flag and torch.is_grad_enabled() and (_ag.taping(x, Phi, Phi_sum) or any(p.requires_grad for p in self.f.parameters())):
            if extras:
                raise NotImplementedError("snapshots / trace exist on the engine's inference path only: this is the taped training forward "
                                          "(pass train_flag=False or run under torch.no_grad())")
            eng = self._train_solve_engine()
            if eng is not None:
                # the no-tape solve's f-calls on the engine's "train ... per layer" path (each moves the module's buffers as its own
                # forward would), sigma from the engine's table
                z = eng.solve(*_data(x, Phi, Phi_sum), initial_point=init_point.detach())
                self.forward_res = eng.last_info["res"]
                if eng.den.tag == "ffdnet":
                    n_calls = eng.last_info["f_calls"]
                    self.f._sigma_resume(x, z.shape[0] * z.shape[3], eng.den.sigma_table[n_calls - 1:n_calls])
            else:
                with torch.no_grad():
                    z, self.forward_res = self.solver(lambda z: self.f(z, x, Phi, Phi_sum), init_point, **self.kwargs)
            z = self._taped_call(z, x, Phi, Phi_sum)                           # re-engage the tape (:268)
            z0 = z.clone().detach().requires_grad_()
            f0 = self.f(z0, *_data(x, Phi, Phi_sum))                           # Jacobian-vector products come from this graph
            jmap = self._device_map(Phi, Phi_sum)

            if jmap is not None:
                def backward_hook(grad):
                    self.last_backward_path = "device"
                    g, self.backward_res = self.solver(lambda v: jmap(v) + grad, grad, **self.kwargs)
                    return g
            else:
                def backward_hook(grad):
                    self.last_backward_path = "autograd"
                    g, self.backward_res = self.solver(
                        lambda v: torch.autograd.grad(f0, z0, v, retain_graph=True)[0] + grad, grad, **self.kwargs)
                    return g
            z.register_hook(backward_hook)
            return z
        eng = self._engine_for()
        self.last_snapshots = self.last_trace = None
        if eng is not None:
            z = eng.reconstruct(x, Phi, Phi_sum, initial_point=init_point, snapshots=self.snapshots, trace=bool(self.trace), gt=self.trace_gt)
            info = eng.last_info
            self.last_snapshots, self.last_trace = info["snapshots"], info["trace"]
            if eng.iterator == "picard":
                rows = eng._ws[next(iter(eng._ws))].host_res
                self.forward_res = [float(v) for v in rows[1:info["iterations"] + 1, 0]]
            else:
                self.forward_res = info["res"]
            return z
        if extras:
            raise NotImplementedError("snapshots / trace exist on the engine's path only, and this call takes the generic solver (use_engine is "
                                      "off, f is not this package's EquilibriumProxGradSCI with A_torch_ / At_torch_, an unknown denoiser tag, "
                                      "or a solver other than andersonexp / forward_iteration, such as broyden_fixed_point)")
        with torch.no_grad():
            z, self.forward_res = self.solver(lambda z: self.f(z, x, Phi, Phi_sum), init_point, **self.kwargs)
            z = self.f(z, x, Phi, Phi_sum)
            self.f(z, x, Phi, Phi_sum)      # the reference's f0 = f(z0): advances the sigma state (:271-272)
        return z


# ----------------------------------------------------------------------------- ADMM variant
class EquilibriumADMMSCI(nn.Module):
    """solvers/equilibrium_solvers_yaping.py:438-465: one ADMM iterate (z,u) -> (z',u').  The projection is
    the same K3 kernel applied to (z+u) with Phi_sum + 1e-8; the denoiser sees z' - u and returns the CLEAN
    image (dispatch on `nonlinear_op.conv3d`, as in the reference)."""

    def __init__(self, A, At, nonlinear_operator, eta, minval=-1, maxval=1):
        super().__init__()
        self.A, self.At = A, At
        self.nonlinear_op = nonlinear_operator
        self.minval, self.maxval = minval, maxval

    def forward(self, z, u, y, Phi, Phi_sum):
        if _ag.taping(Phi, Phi_sum):
            raise NotImplementedError("EquilibriumADMMSCI has no mask gradient: Phi or Phi_sum requires one (detach them, or use "
                                      "EquilibriumProxGradSCI, whose taped call differentiates the mask)")
        bsz, w, h, c = z.shape
        zu = _hip.f32c(z + u)
        if self.A is A_torch_ and self.At is At_torch_:
            zp = _hip.gap_update(zu, _hip.f32c(Phi), _hip.f32c(y), _hip.f32c(Phi_sum + 1e-8), LAYOUT_HWB, LAYOUT_BHW)
        else:
            fb = self.A(zu, Phi)
            zp = _hip.transpose(_hip.f32c(zu + self.At((y - fb) / (Phi_sum + 1e-8), Phi)), LAYOUT_BHW)
        vin = zp - _hip.transpose(_hip.f32c(u), LAYOUT_BHW)
        if not self.nonlinear_op.conv3d:
            den = self.nonlinear_op(vin.view(bsz * c, 1, w, h)).reshape(bsz, c, w, h)
        else:
            den = self.nonlinear_op(vin.view(bsz, 1, c, w, h)).reshape(bsz, c, w, h)
        z_new = _hip.transpose(zp, LAYOUT_HWB)
        u_new = u - _hip.residual_out(zp, _hip.f32c(den), LAYOUT_HWB)          # u - (z - z_tplus1)
        return z_new, u_new


def initial_point_admm(y, Phi, Phi_sum=None, gt=None):
    """utils/cg_utils.py:238-239."""
    return [At_torch_(y, Phi), torch.zeros_like(Phi)]


def admmexp(f, x0, m=5, lam=1e-4, max_iter=50, tol=1e-2, beta=1.0):
    """solvers/new_equilibrium_utils_yaping.py:396-413: plain ADMM fixed-point iteration; on convergence the
    PREVIOUS (X,U) is returned, as in the reference.  m, lam, beta are accepted and unused there too."""
    X, U = x0[0], x0[1]
    bsz, N = X.shape[0], X[0].numel()
    ws = _hip.AndersonWorkspace(bsz, N, 1, X.device)
    res = None
    for k in range(2, max_iter):
        new_X, new_U = f(X, U)
        _hip.residual_store(ws, _hip.f32c(new_X).reshape(bsz, N), None, _hip.f32c(X).reshape(bsz, N), 0, 1, None)
        _hip.anderson_solve(ws, 0, 1, 0, 0.0, 1e-5)
        res = ws.res[0, 0].item()
        if res < tol:
            break
        X, U = new_X, new_U
    if res is None:
        raise UnboundLocalError("local variable 'res' referenced before assignment")
    return X, U, res


class DEQFixedPointADMM(nn.Module):
    """solvers/new_equilibrium_utils_yaping.py:416-451 (inference part)."""

    def __init__(self, f, solver1, solver2, **kwargs):
        super().__init__()
        self.f, self.solver1, self.solver2, self.kwargs = f, solver1, solver2, kwargs
        self.forward_res = None

    def forward(self, x, Phi, Phi_sum, initial_point=None, train_flag=True):
        init_point = [torch.zeros_like(x), torch.zeros_like(x)] if initial_point is None else initial_point
        if train_flag and _ag.taping(Phi, Phi_sum):
            raise NotImplementedError("DEQFixedPointADMM has no mask gradient: Phi or Phi_sum requires one (pass train_flag=False, run under "
                                      "torch.no_grad(), or use DEQFixedPoint with EquilibriumProxGradSCI)")
        with torch.no_grad():
            z, u, self.forward_res = self.solver1(lambda z, u: self.f(z, u, x, Phi, Phi_sum), init_point, **self.kwargs)
        return z
