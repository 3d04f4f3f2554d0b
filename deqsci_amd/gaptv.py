"""GAP-TV: the reference's classical reconstruction (utils/cg_utils.py:207-224) and its TV denoiser, scikit-image 0.17.2's
denoise_tv_chambolle, for torch tensors.

    denoise_tv_chambolle(image, weight=0.1, eps=2e-4, n_iter_max=200, multichannel=False)
    GAP_TV_rec(y, Phi, Phi_sum, gt, A, At, maxiter, step_size, tv_weight)

Tensors on a HIP device go through the kernels of csrc/tv.hip (fp64 state, fp32 in and out); CPU tensors through a float64 torch
restatement of the same algorithm (`tv_chambolle_float64`, `gaptv_float64`), as deqsci_amd.pytorch_ssim does for SSIM.

denoise_tv_chambolle keeps skimage's semantics, including tau = 1 / (2 ndim) with ndim the dimension of the array each channel is
(a (1,H,W) channel is denoised with tau 1/6, an (H,W) one with 1/4, and the results differ).  On a device, the per-channel array must
be 2-D, or higher-D with every axis but the last two of length 1; other shapes raise NotImplementedError (the kernel couples the
pixels of a plane only).  The result has the input's dtype.

GAP_TV_rec reconstructs each measurement of a batch on its own, as the reference's harness calls it with batch size 1.  (Handed a
batch, the reference's numpy code would denoise each frame as a 3-D (bsz,H,W) array and couple the measurements along axis 0; this
build does not - DESIGN.md section 5.)
"""
import math

import numpy as np
import torch

from . import _hip, operators

TV_EPS = 2e-4                      # skimage's default, which the reference keeps
TV_ITERS = 30                      # n_iter_max of the reference's call (cg_utils.py:221)


# ----------------------------------------------------------------------------- float64 restatement (CPU path and test yardstick)
def sqrt_float64(x):
    """The correctly rounded square root of a float64 CPU tensor, as numpy's and the device's.  (torch's vectorised CPU sqrt is not:
    with AVX-512 it is one ulp off on about 0.7 % of uniform inputs.)"""
    return torch.from_numpy(np.sqrt(x.contiguous().numpy()))


def tv_chambolle_float64(image, weight=0.1, eps=TV_EPS, n_iter_max=200, return_stop=False):
    """skimage 0.17.2 _denoise_tv_chambolle_nd on one array of any dimension, in float64 torch, every operation in skimage's order.
    -> out (float64), and with return_stop=True also (stop iteration or n_iter_max, margin |E_prev - E| - eps E_init of the last
    stop test)."""
    image = image.double()
    ndim = image.dim()
    p = torch.zeros((ndim,) + tuple(image.shape), dtype=torch.float64, device=image.device)
    g = torch.zeros_like(p)
    d = torch.zeros_like(image)
    tau = 1. / (2. * ndim)
    stop, margin = n_iter_max, float("nan")
    E_init = E_previous = 0.0
    out = image
    for i in range(n_iter_max):
        if i > 0:
            s = p[0]
            for ax in range(1, ndim):
                s = s + p[ax]
            d = -s
            for ax in range(ndim):
                n = image.shape[ax]
                if n > 1:
                    d.narrow(ax, 1, n - 1).add_(p[ax].narrow(ax, 0, n - 1))
            out = image + d
        else:
            out = image
        E = float((d ** 2).sum())
        for ax in range(ndim):
            n = image.shape[ax]
            if n > 1:
                g[ax].narrow(ax, 0, n - 1).copy_(out.narrow(ax, 1, n - 1) - out.narrow(ax, 0, n - 1))
        sq = g[0] ** 2
        for ax in range(1, ndim):
            sq = sq + g[ax] ** 2
        norm = sqrt_float64(sq)
        E += weight * float(norm.sum())
        norm = norm * (tau / weight)
        norm = norm + 1.
        p = (p - tau * g) / norm
        E /= float(image.numel())
        if i == 0:
            E_init = E_previous = E
        else:
            margin = abs(E_previous - E) - eps * E_init
            if abs(E_previous - E) < eps * E_init:
                stop = i
                break
            E_previous = E
    return (out, stop, margin) if return_stop else out


def frame_sum_float64(t):
    """np.sum(t, axis=-1) for a float64 tensor, in numpy's pairwise_sum order: fewer than 8 terms left to right (from 0.); up to 128,
    eight running sums r_k over k, k + 8, ... folded ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 last terms in
    order; above 128, the two halves split at n2 = n // 2 rounded down to a multiple of 8, each summed the same way, then added."""
    n = t.shape[-1]
    if n > 128:
        n2 = n // 2
        n2 -= n2 % 8
        return frame_sum_float64(t[..., :n2]) + frame_sum_float64(t[..., n2:])
    if n < 8:
        s = t[..., 0] + 0.
        b = 1
    else:
        r = [t[..., k] for k in range(8)]
        b = 8
        while b + 8 <= n:
            r = [r[k] + t[..., b + k] for k in range(8)]
            b += 8
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for k in range(b, n):
        s = s + t[..., k]
    return s


def gaptv_float64(y, Phi, Phi_sum, maxiter, step_size, tv_weight, eps=TV_EPS, n_iter_max=TV_ITERS, return_stop=False):
    """The reference's GAP_TV_rec in float64 torch for ONE measurement: y (1,H,W), Phi (1,H,W,B), Phi_sum (1,H,W) float32 ->
    (1,H,W,B) float64, and with return_stop=True also the (maxiter, B) stop indices."""
    Phi64 = Phi.double()
    f = (y[..., None] * Phi).double()                              # At_: the float32 product, stored in a float64 array
    y1 = torch.zeros(y.shape, dtype=torch.float64)
    stops = torch.zeros((maxiter, Phi.shape[-1]), dtype=torch.int32)
    for it in range(maxiter):
        fb = frame_sum_float64(f * Phi64)                          # A_: np.sum(f * Phi, axis=3)
        y1 = y1 + (y.double() - fb)
        r = (y1 - fb) / Phi_sum.double()
        f = f + step_size * (r[..., None] * Phi64)
        out = torch.empty_like(f)
        for c in range(f.shape[-1]):                              # multichannel: every frame a (1,H,W) array on its own
            out[..., c], stops[it, c], _ = tv_chambolle_float64(f[..., c], tv_weight, eps, n_iter_max, return_stop=True)
        f = out
    return (f, stops) if return_stop else f


# ----------------------------------------------------------------------------- public API
def _device_planes_ok(shape):
    return len(shape) >= 2 and all(s == 1 for s in shape[:-2])


def denoise_tv_chambolle(image, weight=0.1, eps=2.e-4, n_iter_max=200, multichannel=False):
    """skimage 0.17.2 denoise_tv_chambolle for a floating-point torch tensor (see the module docstring)."""
    if not isinstance(image, torch.Tensor) or not image.is_floating_point():
        raise TypeError("denoise_tv_chambolle expects a floating-point torch tensor")
    chan_shape = tuple(image.shape[:-1]) if multichannel else tuple(image.shape)
    if not image.is_cuda:
        if multichannel:
            out = torch.empty(image.shape, dtype=torch.float64)
            for c in range(image.shape[-1]):
                out[..., c] = tv_chambolle_float64(image[..., c], weight, eps, n_iter_max)
        else:
            out = tv_chambolle_float64(image, weight, eps, n_iter_max)
        return out.to(image.dtype)
    if not _device_planes_ok(chan_shape):
        raise NotImplementedError(f"denoise_tv_chambolle on a device: each channel must be a 2-D array, or one whose axes but the last two "
                                  f"have length 1; got channels of shape {chan_shape}")
    tau = 1. / (2. * len(chan_shape))
    H, W = chan_shape[-2:]
    if multichannel:
        planes = image.reshape(H, W, image.shape[-1]).permute(2, 0, 1)
    else:
        planes = image.reshape(1, H, W)
    out = _hip.tv_chambolle(_hip.f32c(planes), weight, eps, n_iter_max, tau)
    if multichannel:
        out = out.permute(1, 2, 0)
    return out.reshape(image.shape).to(image.dtype)


def _psnr(ref, img):
    """cg_utils.psnr: 20 log10(1 / sqrt(mean((ref - img)^2))), 100 for a perfect match."""
    mse = float(((ref.detach().double().cpu() - img.detach().double().cpu()) ** 2).mean())
    return 100 if mse == 0 else 20 * math.log10(1. / math.sqrt(mse))


def GAP_TV_rec(y, Phi, Phi_sum, gt, A, At, maxiter, step_size, tv_weight, return_stop=False):
    """The reference's GAP_TV_rec: y (bsz,H,W), Phi (bsz|1,H,W,B), Phi_sum (bsz|1,H,W) -> (bsz,H,W,B) float32 on y's device, each
    measurement reconstructed on its own.  A and At must be this package's A_torch_ and At_torch_ (the maps the reference's numpy
    A_ / At_ compute).  Prints 'GAP-TV: PSNR = ..' against gt when gt has the output's shape; gt=None is silent.  return_stop=True
    (this build's) also returns the (bsz, maxiter, B) int32 stop indices of the TV calls."""
    if A is not operators.A_torch_ or At is not operators.At_torch_:
        raise ValueError("GAP_TV_rec: A and At must be deqsci_amd.A_torch_ and deqsci_amd.At_torch_")
    if y.dim() != 3 or Phi.dim() != 4 or Phi_sum.dim() != 3:
        raise ValueError(f"GAP_TV_rec: y (bsz,H,W), Phi (bsz,H,W,B), Phi_sum (bsz,H,W) expected, got {tuple(y.shape)}, {tuple(Phi.shape)}, "
                         f"{tuple(Phi_sum.shape)}")
    if y.is_cuda:
        out, stop = _hip.gaptv(_hip.f32c(y), _hip.f32c(Phi), _hip.f32c(Phi_sum), maxiter, step_size, tv_weight, TV_EPS, TV_ITERS,
                               return_stop=True)
    else:
        outs, stops = [], []
        for m in range(y.shape[0]):
            P = Phi[m if Phi.shape[0] > 1 else 0][None].float()
            Ps = Phi_sum[m if Phi_sum.shape[0] > 1 else 0][None].float()
            f, s = gaptv_float64(y[m][None].float(), P, Ps, maxiter, step_size, tv_weight, return_stop=True)
            outs.append(f.float())
            stops.append(s)
        out, stop = torch.cat(outs), torch.stack(stops)
    if gt is not None and tuple(gt.shape) == tuple(out.shape):
        print("GAP-TV: PSNR = %2.2f dB" % (_psnr(torch.as_tensor(gt), out)))
    return (out, stop) if return_stop else out
