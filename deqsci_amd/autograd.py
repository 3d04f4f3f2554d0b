"""Autograd wrappers of the SCI kernels, used only when a tape is being recorded (training-mode
DEQFixedPoint, solvers/new_equilibrium_utils_yaping.py:268-280 in the reference).

The operators are linear in the image / measurement, so every backward is again one of the HIP kernels:

    y = A(x, Phi)                      grad_x = At(grad_y, Phi)
    x = At(y, Phi)                     grad_y = A(grad_x, Phi)
    z1 = z + At((y - A z)/Phi_sum)     grad_z = g - At(A(g)/Phi_sum)  (= the same GAP kernel with y = 0: I - Phi^T D Phi is symmetric)
                                       grad_y = A(g) / Phi_sum

    noise = D(x; W_0 .. W_{k-1})       grad_W_i = csrc/wgrad.hip on the kept activations and the masked gradients, grad_x = J_D(x)^T g
                                       (deqsci_amd.vjp.DenoiserParamGrads; DEQFixedPoint.parameter_backward = "device")
    ... with a frozen BatchNorm        grad_W_i = s R, grad_beta = sum gm, grad_gamma = (sum W R - mean grad_beta) / sqrt(var + eps)
                                       (csrc/wgrad_bn.hip; parameter_backward = "device+bn"; FFDNet: no grad_x, its input is detached)
    ... with a train-mode BatchNorm    grad_beta = sum gm, grad_gamma = sum gm xhat, dc = gamma / sqrt(var + eps) (gm - grad_beta / P - xhat grad_gamma / P),
                                       grad_W_i = wgrad(input, dc)   (csrc/bn_train.hip; parameter_backward = "device+bn-train")

The masks are differentiable too (a learnable coded aperture); their gradients come from csrc/sci_grad.hip, in Phi's own shape - a
mask shared by the batch, (1,H,W,B) or (H,W,B), gets the sum over the batch:

    y = A(x, Phi)                      grad_Phi_b = grad_y x_b                                       (G2 sci_mask_grad)
    x = At(y, Phi)                     grad_Phi_b = y grad_x_b                                       (G2)
    s = phi_sum(Phi)                   grad_Phi_b = grad_s, 0 where sum_b Phi_b = 0 (s is 1 there)   (G3 phi_sum_grad)
    z1 = gap_update(z, y, Phi, s)      r = (y - A z)/s, t = A(g)/s:  grad_Phi_b = r g_b - t z_b,  grad_s = -t r, and in the same launch
                                       grad_z = g - t Phi, grad_y = t where asked for               (G1 gap_update_grad)

A spectrally normalised convolution in train mode (networks.simplecnn.RealSNConv2d) normalises its weight at every call:

    weight, u' = realsn(W, u)          one power-iteration step and weight = W / cur_sigma * sigma (csrc/realsn.hip R1; u', v constants)
                                       grad_W = (sigma / cur_sigma) (g - (sum(g W) / cur_sigma) C),  C = d cur_sigma / dW   (R2)

The training loop's loss (deqsci_amd.training, loss_function="device"):

    loss, stats = mse_loss_stats(rec, gt)   loss = sum (rec - gt)^2 / total with grad_rec = grad_loss 2 (rec - gt) / total formed in the forward's
                                       pass, which also sums the clamped squared error (the batch PSNR) and counts non-finite differences
                                       (csrc/train.hip L1; CPU tensors: the same arithmetic in torch)

With no mask gradient asked for, every backward makes the launches it always made.  The backwards are once-differentiable.
(bsz,H,W,B) layout, fp32, GPU - like the forward kernels; there is no CPU path, except for realsn_weight (deqsci_amd.realsn's restatement).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _hip
from ._hip import LAYOUT_HWB


class _SCIForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Phi):
        ctx.phi_shape = tuple(Phi.shape)
        x, Phi = _hip.f32c(x), _hip.f32c(Phi)
        ctx.save_for_backward(Phi, x if ctx.needs_input_grad[1] else None)
        return _hip.sci_forward(x, Phi, LAYOUT_HWB)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        Phi, x = ctx.saved_tensors
        gy = _hip.f32c(gy)
        gx = _hip.sci_adjoint(gy, Phi, LAYOUT_HWB) if ctx.needs_input_grad[0] else None
        gphi = _hip.sci_mask_grad(gy, x, ctx.phi_shape) if ctx.needs_input_grad[1] else None
        return gx, gphi


class _SCIAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, Phi):
        ctx.phi_shape = tuple(Phi.shape)
        y, Phi = _hip.f32c(y), _hip.f32c(Phi)
        ctx.save_for_backward(Phi, y if ctx.needs_input_grad[1] else None)
        return _hip.sci_adjoint(y, Phi, LAYOUT_HWB)

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        Phi, y = ctx.saved_tensors
        gx = _hip.f32c(gx)
        gy = _hip.sci_forward(gx, Phi, LAYOUT_HWB) if ctx.needs_input_grad[0] else None
        gphi = _hip.sci_mask_grad(y, gx, ctx.phi_shape) if ctx.needs_input_grad[1] else None
        return gy, gphi


class _PhiSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Phi):
        Phi = _hip.f32c(Phi)
        ctx.save_for_backward(Phi)
        return _hip.phi_sum(Phi, LAYOUT_HWB)

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        (Phi,) = ctx.saved_tensors
        return _hip.phi_sum_grad(Phi, _hip.f32c(gs))


class _GapUpdate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y, Phi, Phi_sum):
        z, y, Phi, Phi_sum = _hip.f32c(z), _hip.f32c(y), _hip.f32c(Phi), _hip.f32c(Phi_sum)
        mask = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        ctx.save_for_backward(Phi, Phi_sum, z if mask else None, y if mask else None)
        return _hip.gap_update(z, Phi, y, Phi_sum, LAYOUT_HWB, LAYOUT_HWB)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Phi, Phi_sum, z, y = ctx.saved_tensors
        g = _hip.f32c(g)
        need_z, need_y, need_phi, need_s = ctx.needs_input_grad
        if need_phi or need_s:                                     # one launch for everything that is asked for
            gphi, gs, gz, gy = _hip.gap_update_grad(z, Phi, g, y, Phi_sum, need=(need_phi, need_s, need_z, need_y))
            return gz, gy, gphi, gs
        gz = gy = None
        if need_z:
            zero_y = torch.zeros(g.shape[:3], device=g.device, dtype=torch.float32)
            gz = _hip.gap_update(g, Phi, zero_y, Phi_sum, LAYOUT_HWB, LAYOUT_HWB)
        if need_y:
            gy = _hip.sci_forward(g, Phi, LAYOUT_HWB) / Phi_sum
        return gz, gy, None, None


class _DenoiserNoise(torch.autograd.Function):
    """noise = net(x) for a net vjp.param_eligibility accepts, forward and backward on the HIP kernels.  The parameters are passed as
    inputs so that autograd routes their gradients; the forward reads them from `net` (the same tensors).  sigma: FFDNet's noise levels
    (data: no gradient); FFDNet detaches its input, so it returns no input gradient either."""

    FIXED = 4                      # the inputs in front of *params: net, x, sigma, mode

    @staticmethod
    def forward(ctx, net, x, sigma, mode, *params):
        from . import vjp
        ctx.pg = vjp.DenoiserParamGrads(net, x, sigma, mode=mode)
        return ctx.pg.noise

    @staticmethod
    def backward(ctx, gv):
        pg, ctx.pg = ctx.pg, None
        if pg is None:
            raise RuntimeError("denoiser_noise: backward ran already (the kept activations are freed after the first)")
        try:
            dws = pg.grads(gv, need=ctx.needs_input_grad[_DenoiserNoise.FIXED:])
            gx = pg.vjp(gv) if ctx.needs_input_grad[1] and not pg.ffdnet else None
        finally:
            pg.release()
        return (None, gx) + (None,) * (_DenoiserNoise.FIXED - 2) + tuple(dws)


class _RealSNWeight(torch.autograd.Function):
    """(weight, u_new) of deqsci_amd.realsn.power_iteration with the gradient of weight with respect to W; u_new carries none."""

    @staticmethod
    def forward(ctx, W, u, sigma, n, eps):
        from . import realsn
        Wd = _hip.f32c(W.detach())
        if Wd.is_cuda:
            weight, u_new, v, record = _hip.realsn_power(Wd, u.detach().clone(memory_format=torch.contiguous_format), n, sigma, eps)
        else:
            weight, u_new, v, cur_sigma = realsn.power_iteration(Wd, u, sigma, n, eps)
            record = cur_sigma
        ctx.sigma = float(sigma)
        ctx.save_for_backward(Wd, u_new, v, record)
        ctx.mark_non_differentiable(u_new)
        return weight, u_new

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _gu):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        from . import realsn
        W, u, v, record = ctx.saved_tensors
        G = _hip.f32c(G)
        if W.is_cuda:
            return _hip.realsn_grad(G, W, u, v, record, ctx.sigma), None, None, None, None
        return realsn.weight_grad(G, W, u, v, record, ctx.sigma), None, None, None, None


def realsn_weight(weight_orig, u, sigma=1.0, n_power_iterations=1, eps=1e-12):
    """-> (weight, u_new): the train-mode weight of a spectrally normalised convolution, differentiable in weight_orig (u_new and the
    right vector are constants, as in the reference), and the new weight_u.  u is not modified.  Device tensors: csrc/realsn.hip, no host
    synchronisation; CPU tensors: deqsci_amd.realsn's restatement.  Once-differentiable: a double backward raises."""
    return _RealSNWeight.apply(weight_orig, u, float(sigma), int(n_power_iterations), float(eps))


def denoiser_noise(net, x, sigma=None, frozen_bn=False, train_bn=False, train_realsn=False, *, mode=None):
    """net(x) - net(x, sigma) for FFDNet - with the weight gradients (and the input gradient, where x requires one and the net does not
    detach it) formed on the device, in the mode of vjp.GRAD_MODES the keywords name: the nets vjp.param_eligibility accepts under the same
    keywords, the gradients going to the mode's parameters (vjp.grad_parameters).  The train modes move the module's buffers as its own
    forward would: train_bn the BatchNorms' running statistics, train_realsn every RealSNConv2d's weight_u / weight.  mode: a caller's
    vjp.GradMode in hand, in place of the keywords."""
    from . import vjp
    mode = mode or vjp.grad_mode("denoiser_noise", frozen_bn, train_bn, train_realsn)
    return _DenoiserNoise.apply(net, x, sigma, mode, *mode.parameters(net))


class _MSELossStats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rec, gt):
        total = rec.numel()
        if rec.is_cuda:
            grad, stats = _hip.mse_stats_grad(_hip.f32c(rec), _hip.f32c(gt))
        else:
            # the same arithmetic in torch, in the tensors' own dtype (sums in float64, in torch's order)
            d = rec - gt
            grad = d * torch.tensor(2.0 / total, dtype=rec.dtype)
            dc = rec.clamp(0, 1) - gt
            stats = torch.stack([(d * d).double().sum(), (dc * dc).double().sum(), (~torch.isfinite(d)).sum().double()])
        ctx.grad, ctx.stats = grad, stats
        ctx.mark_non_differentiable(stats)
        return (stats[0] / total).to(rec.dtype), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_stats):
        return (g_loss * ctx.grad).view(ctx.grad.shape), None


def mse_loss_stats(rec, gt):
    """-> (loss, stats): the mean squared error of rec against gt as a 0-d tensor of rec's dtype, differentiable in rec, and - detached -
    stats (3,) float64: sum (rec - gt)^2, sum (clamp(rec, 0, 1) - gt)^2, the number of non-finite differences.  One read-back of stats gives
    the loss (stats[0] / total), the NaN check (stats[2], or the loss itself) and the batch PSNR, 10 log10(total / stats[1]).  Device
    tensors (fp32): csrc/train.hip L1, which forms the gradient 2 (rec - gt) / total in the same pass - backward is one multiplication
    by the incoming gradient; no host synchronisation.  CPU tensors: the same arithmetic in torch.  gt gets no gradient."""
    if tuple(rec.shape) != tuple(gt.shape) or rec.dtype != gt.dtype or rec.device != gt.device:
        raise ValueError(f"mse_loss_stats: rec {tuple(rec.shape)} {rec.dtype} on {rec.device} and gt {tuple(gt.shape)} {gt.dtype} on {gt.device} differ")
    return _MSELossStats.apply(rec, gt.detach())


def taping(*tensors):
    """True when autograd is recording and one of the tensors takes part in it."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def sci_forward(x, Phi):
    return _SCIForward.apply(x, Phi)


def sci_adjoint(y, Phi):
    return _SCIAdjoint.apply(y, Phi)


def gap_update(z, y, Phi, Phi_sum):
    return _GapUpdate.apply(z, y, Phi, Phi_sum)


def phi_sum(Phi):
    return _PhiSum.apply(Phi)
