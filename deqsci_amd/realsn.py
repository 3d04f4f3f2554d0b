"""Real spectral normalisation of a 3x3 convolution in TRAIN mode: the power-iteration step the reference's forward pre-hook runs at
every call of a spectrally normalised layer (networks/provable/model/conv_sn_chen.py:29-50,60-64), and the gradient of the normalised
weight.  With W = weight_orig (C_out, C_in, 3, 3) and u = weight_u (1, C_out, h, w):

    repeat n times:   t1 = W^T u (conv_transpose2d(u, W, padding=1))     v = t1 / max(|t1|, eps)
                      t2 = W v   (conv2d(v, W, padding=1))               u = t2 / max(|t2|, eps)
    cur_sigma = sum(u * (W v))           u, v constants; differentiable in W
    weight    = W / cur_sigma * sigma    in this order

and, for G = dL/dweight and C[o,i,ky,kx] = sum_p u[o,p] v[i, p + (ky-1, kx-1)] = d cur_sigma / dW,

    dL/dW = (sigma / cur_sigma) * (G - (sum(G * W) / cur_sigma) * C)

Device tensors run on csrc/realsn.hip (_hip.realsn_power, _hip.realsn_grad: 3 n + 1 and 2 launches, no host synchronisation).  CPU
tensors run the torch restatement below, in the arithmetic of the kernels: fp32 tensors, the two sums of squares, cur_sigma and
sum(G * W) in float64, sqrt in float64, then the rounded norm, max(., eps) and the division in fp32.  It is the CPU path and the tests'
yardstick; `power_iteration_float64` / `weight_grad` on float64 tensors are the same in float64 throughout.

`operator_norm` / `layer_sigmas` run the same step from a seeded start until it has converged: the operator norm a layer's stored weight
really has, against the sigma it claims.
"""
import torch
import torch.nn.functional as F

from . import _hip


def _denominator(t, eps):
    """(max(|t|, eps) in t's dtype, |t| in float64): the sum of squares and its root in float64, one rounding, eps only where eps > norm
    (Python's max(norm, eps): a NaN norm stays NaN)."""
    norm64 = torch.sqrt((t.double() * t.double()).sum())
    norm = norm64.to(t.dtype)
    floor = torch.as_tensor(eps, dtype=t.dtype, device=t.device)
    return torch.where(floor > norm, floor, norm), norm64


def _restatement(W, u, sigma, n, eps):
    if int(n) < 1:
        raise ValueError(f"n_power_iterations must be at least 1, got {n}")
    if W.dim() != 4 or tuple(W.shape[2:]) != (3, 3) or u.dim() != 4 or u.shape[0] != 1 or u.shape[1] != W.shape[0]:
        raise ValueError(f"weight_orig (C_out, C_in, 3, 3) and u (1, C_out, h, w) expected, got {tuple(W.shape)} and {tuple(u.shape)}")
    with torch.no_grad():
        for _ in range(int(n)):
            t1 = F.conv_transpose2d(u, W, padding=1)
            v = t1 / _denominator(t1, eps)[0]
            t2 = F.conv2d(v, W, padding=1)
            u = t2 / _denominator(t2, eps)[0]
        cur_sigma = (u.double() * t2.double()).sum()
        weight = W / cur_sigma.to(W.dtype) * torch.as_tensor(sigma, dtype=W.dtype, device=W.device)
    return weight, u, v, cur_sigma


def power_iteration(weight_orig, u, sigma=1.0, n_power_iterations=1, eps=1e-12):
    """-> (weight, u_new, v, cur_sigma): n_power_iterations steps from u and the weight normalised by the estimated operator norm.
    fp32; on the device through the HIP kernels, on the CPU through the restatement.  u is not modified.  cur_sigma: a 0-dim float64
    tensor (the float64 sum the weight's fp32 divisor is rounded from).  No gradient is recorded: autograd.realsn_weight is the taped form."""
    W = weight_orig.detach()
    if W.dtype != torch.float32 or u.dtype != torch.float32:
        raise TypeError(f"power_iteration is fp32 (power_iteration_float64 for float64), got {W.dtype} and {u.dtype}")
    if W.is_cuda:
        weight, u_new, v, record = _hip.realsn_power(_hip.f32c(W), u.detach().clone(memory_format=torch.contiguous_format), n_power_iterations,
                                                     sigma, eps)
        return weight, u_new, v, record[2]
    return _restatement(W, u.detach(), sigma, n_power_iterations, eps)


def power_iteration_float64(weight_orig, u, sigma=1.0, n_power_iterations=1, eps=1e-12):
    """power_iteration in float64 throughout, on the tensors' own device by torch operations: what the fp32 paths are measured against."""
    return _restatement(weight_orig.detach().double(), u.detach().double(), sigma, n_power_iterations, eps)


def sigma_jacobian(u, v):
    """C = d cur_sigma / dW (C_out, C_in, 3, 3): C[o,i,ky,kx] = sum_p u[o,p] v[i, p + (ky-1, kx-1)], zero outside the map."""
    return F.conv2d(v.permute(1, 0, 2, 3), u.permute(1, 0, 2, 3), padding=1).permute(1, 0, 2, 3)


def weight_grad(G, weight_orig, u, v, cur_sigma, sigma=1.0):
    """dL/dweight_orig from G = dL/dweight by the formula above, in the tensors' dtype (sum(G * W) and its quotient in float64)."""
    W = weight_orig.detach()
    cs64 = cur_sigma.double()
    s = ((G.double() * W.double()).sum() / cs64).to(W.dtype)
    a = torch.as_tensor(sigma, dtype=W.dtype, device=W.device) / cs64.to(W.dtype)
    return a * (G - s * sigma_jacobian(u, v))


def operator_norm(weight, size=(40, 40), n_iters=50, seed=0, return_trace=False):
    """The operator norm of x -> conv2d(x, weight, padding=1) on (h, w) = size maps: n_iters power-iteration steps (the step above) from a
    seeded unit u - a generator of its own, the global random stream is not touched - and the last |W v|, as a float.  In weight's dtype
    and on its device (fp32 device weights: the HIP kernel).  return_trace: also the list of every step's |W v|."""
    W = weight.detach()
    h, w = size
    g = torch.Generator().manual_seed(int(seed))
    u = torch.randn(1, W.shape[0], h, w, generator=g, dtype=torch.float64)
    u = (u / u.norm()).to(device=W.device, dtype=W.dtype)
    norms = []
    if W.is_cuda and W.dtype == torch.float32:
        W = _hip.f32c(W)
        ws = _hip.realsn_workspace(W.shape[1], W.shape[0], h, w, W.device)
        for _ in range(int(n_iters)):
            record = _hip.realsn_power(W, u, 1, 1.0, 1e-12, workspace=ws)[3]
            norms.append(record[1])
    else:
        for _ in range(int(n_iters)):
            t1 = F.conv_transpose2d(u, W, padding=1)
            v = t1 / _denominator(t1, 1e-12)[0]
            t2 = F.conv2d(v, W, padding=1)
            d, norm64 = _denominator(t2, 1e-12)
            u = t2 / d
            norms.append(norm64)
    trace = torch.stack(norms).cpu().tolist() if norms else []
    if return_trace:
        return trace[-1], trace
    return trace[-1]


def layer_sigmas(net, **kw):
    """[{"layer", "sigma", "norm"}] for every RealSNConv2d of net: the sigma the layer claims and operator_norm(its stored weight, **kw) -
    whether a checkpoint's layers really have the norm they claim."""
    from .networks.simplecnn import RealSNConv2d
    kw.setdefault("size", None)
    out = []
    for name, m in net.named_modules():
        if isinstance(m, RealSNConv2d):
            opts = dict(kw)
            if opts["size"] is None:
                opts["size"] = tuple(m.weight_u.shape[2:])
            out.append({"layer": name, "sigma": float(m.sigma), "norm": operator_norm(m.weight, **opts)})
    return out
