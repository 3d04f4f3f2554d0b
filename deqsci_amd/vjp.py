"""The DEQ's implicit backward on the device: vector-Jacobian products J_D(x)^T v of a denoiser plugin on the HIP kernels.

The training forward's hook (solvers/new_equilibrium_utils_yaping.py:273-276) solves  g = J_f(z0)^T g + grad, and with
f(z) = z1 - D(z1), z1 = P z + c and P = I - Phi^T diag(1/Phi_sum) Phi symmetric,

    J_f(z0)^T v = P (v - J_D(z1)^T v)          (P u = the GAP kernel with y = 0, as in deqsci_amd/autograd.py)

For a conv [+BN-eval] + ReLU stack (SimpleCNN, RealSN_SimpleCNN in eval mode, DnCNN-17-style plugins) J_D^T v runs the layers
backwards: each conv with its BN-folded weight (w * s) transposed and flipped and no bias, each ReLU replaced by its unit's mask
from ONE forward pass at x (ReLU'(0) = 0, as in PyTorch).  The masks are fixed for all of the hook's iterations, so every
product is linear in v:

    v (n,1,H,W) -> conv3x3(1 -> 64) * mask[k-2] -> [conv3x3(64 -> 64) * mask[i-1]] for i = k-2 .. 1 -> conv3x3(64 -> 1)

= csrc/ffdnet_edges.hip's 1 -> 64 stencil with the masked epilogue (the tail's transpose), csrc/winograd.hip's F(2x2,3x3) kernel with
the masked epilogue, and the existing 64 -> 1 stencil (the head's transpose); the masks are packed one 64-bit word per pixel by
csrc/vjp.hip.  FFDNet detaches its input (networks/ffdnet/models.py in the reference, deqsci_amd/networks/ffdnet.py), so for it
J_D^T = 0 and the hook's product is P v alone.

The same masked kernels compute J_D(x) v (forward mode) when they are handed the untransposed weights in forward order: DenoiserJacobian
(the diagnostics of deqsci_amd/jacobian.py) has both directions, and for FFDNet it differentiates THROUGH the input - the Jacobian of
the map the iteration applies, sigma a constant of the linearisation - on csrc/jacobian.hip's masked first layer and the existing last
layer's kernel.  DenoiserVJP and eligibility are the training hook's and do not change.

The weight gradients (dD/dtheta)^T v of a bias-free conv + ReLU stack come from the same walk: the forward keeps each layer's input, the
transposed masked layers carry v down, and layer i's dW_i is the correlation of its input with the masked gradient behind it
(csrc/wgrad.hip: W0 for a 64 -> 64 layer, W1 for the two edge layers).  plan_param_grads is the host statement, DenoiserParamGrads the
device's, param_eligibility says which nets qualify (DEQFixedPoint.parameter_backward = "device").

With a frozen (eval-mode) BatchNorm behind a conv - FFDNet, a conv + BN + ReLU DnCNN; parameter_backward = "device+bn",
param_eligibility(net, frozen_bn=True) - the layer is y = relu(s c + t), c = conv(x, W), s = gamma / sqrt(var + eps), t = beta - mean s, and
with gm the masked gradient behind the ReLU and R = wgrad(x, gm):

    dW = s R        dbeta = sum_p gm        dgamma = (sum_{ci,tap} W R - mean dbeta) / sqrt(var + eps)

(sum_p gm c = sum W R: no stored pre-activation and no division by gamma, exact for gamma = 0 and gamma < 0; csrc/wgrad_bn.hip's W0-BN gives
the three sums from one pass).  FFDNet's edge layers are read through the 2x2 pixel-(un)shuffle by W2 of the same file, sigma's channel of
the first weight included.  grad_parameters names the parameters, plan_param_grads_frozen_bn is the host statement.

With the BatchNorm in TRAIN mode - what the reference trains: it calls .eval() under --inference only; parameter_backward =
"device+bn-train", param_eligibility(net, train_bn=True) - the layer is y = relu(gamma xhat + beta), xhat = (c - mean) / sqrt(var + eps) with
the mean and the biased variance of c = conv(x, W) over the batch's P = n H W pixels, and with gm the masked gradient behind the ReLU:

    dbeta = sum_p gm        dgamma = sum_p gm xhat        dc = gamma / sqrt(var + eps) (gm - dbeta / P - xhat dgamma / P)        dW = wgrad(x, dc)

(csrc/bn_train.hip: T1 statistics and the running buffers' update, T2 apply + mask, T3 the two sums, T4 dc; dc goes down through the UNFOLDED
transposed weight).  The statistic terms reach the pixels the ReLU masked too.  plan_forward_train_bn / plan_param_grads_train_bn are the
host statements.
"""
import torch
import torch.nn.functional as F

from . import _hip
from .layers import conv_bn_stack, conv_stack

_FFDNET_OK = "FFDNet detaches its input: J_D^T = 0"


def _modules():
    from .networks import DnCNN, FFDNet
    from .networks.simplecnn import RealSNConv2d
    return DnCNN, FFDNet, RealSNConv2d


def host_plan(net):
    """(layers, reason): the denoiser as [(weight, bias or None, relu)] with eval-mode BatchNorm folded into the conv (layers.conv_stack:
    weight * s, bias = beta - mean * s), or (None, why not) when the net is not a conv [+BN-eval] + ReLU stack of 3x3, pad-1
    convolutions without bias.  Usable on the CPU."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if not isinstance(net, DnCNN):
        return None, f"not a conv [+BN] + ReLU stack: {type(net).__name__}"
    return conv_stack(net.dncnn)


def eligibility(net):
    """(ok, reason): whether DenoiserVJP (and DEQFixedPoint.implicit_backward = "device") can differentiate through `net`.  CPU-safe."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if isinstance(net, FFDNet):
        if net.num_input_channels != 1:
            return False, "FFDNet with 3 channels (the HIP kernels cover the grayscale network only)"
        if any(isinstance(m, torch.nn.BatchNorm2d) and m.training for m in net.modules()):
            return False, "FFDNet with BatchNorm2d in train mode"
        return True, _FFDNET_OK
    if getattr(net, "tag", None) != "denoiser":
        return False, f"nonlinear_op tag {getattr(net, 'tag', None)!r}: only 'denoiser' and 'ffdnet' plugins have a device VJP"
    layers, why = host_plan(net)
    if layers is None:
        return False, why
    shapes = [tuple(w.shape) for w, _, _ in layers]
    if len(layers) < 2 or shapes[0] != (64, 1, 3, 3) or shapes[-1] != (1, 64, 3, 3) or any(s != (64, 64, 3, 3) for s in shapes[1:-1]):
        return False, f"layer shapes {shapes}: the kernels cover 1 -> 64 -> ... -> 64 -> 1"
    if layers[0][1] is not None or layers[-1][1] is not None:
        return False, "bias on the first or the last layer"
    if not all(r for _, _, r in layers[:-1]) or layers[-1][2]:
        return False, "ReLU pattern other than after every layer but the last"
    return True, "conv [+BN-eval] + ReLU stack"


def _transposed(w):
    """conv_transpose2d(g, w, padding=1) == conv2d(g, _transposed(w), padding=1) for a 3x3 kernel."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


# ----------------------------------------------------------------------------- the host plans: one masked walk in each direction
# How a stack's edge layers meet the image: (what the first layer reads of it, the input channels of the first weight that carry it, what
# the last layer's output becomes).  FFDNet: 2x2 pixel-unshuffle in (channel 0 of its first weight is sigma's, a constant of the
# linearisation), pixel-shuffle out.  The shuffles are permutations, so the transposed walk reads and writes the same way.
PLAIN_EDGES = (lambda v: v, slice(None), lambda t: t)
FFDNET_EDGES = (lambda v: F.pixel_unshuffle(v, 2), slice(1, 5), lambda t: F.pixel_shuffle(t, 2))


def masked_forward(layers, h):
    """One forward pass of all layers but the last on the first layer's input h, in h's dtype.  -> (the last layer's input, masks):
    masks[i] is the (n,C,H,W) bool ReLU decision behind layer i, None for a layer without ReLU."""
    masks = []
    for w, b, relu in layers[:-1]:
        h = F.conv2d(h, w.to(h), None if b is None else b.to(h), padding=1)
        masks.append(h > 0 if relu else None)
        if relu:
            h = torch.relu(h)
    return h, masks


def masked_jvp(layers, masks, v, edges=PLAIN_EDGES):
    """J v: the layers in forward order, every conv without its bias, every ReLU replaced by its mask."""
    read, cin, write = edges
    t = read(v)
    for i, (w, _, _) in enumerate(layers[:-1]):
        t = F.conv2d(t, (w[:, cin] if i == 0 else w).to(v), padding=1)
        if masks[i] is not None:
            t = t * masks[i]
    return write(F.conv2d(t, layers[-1][0].to(v), padding=1))


def masked_vjp(layers, masks, v, edges=PLAIN_EDGES):
    """J^T v: the layers in reverse order, every conv transposed, layer i's output masked by the ReLU in front of it."""
    read, cin, write = edges
    g = read(v)
    for i in range(len(layers) - 1, 0, -1):
        g = F.conv2d(g, _transposed(layers[i][0].to(v)), padding=1)
        if masks[i - 1] is not None:
            g = g * masks[i - 1]
    return write(F.conv2d(g, _transposed(layers[0][0][:, cin].to(v)), padding=1))


def plan_masks(layers, x):
    """The ReLU masks of one forward pass of the stack `layers` at x, in x's dtype: one (n,C,H,W) bool tensor (or None) per layer but the last."""
    return masked_forward(layers, x)[1]


def plan_vjp(layers, x, v, masks=None):
    """J_D(x)^T v of the stack `layers` (host_plan) evaluated in x's dtype with F.conv2d and explicit masks - the host statement of what
    DenoiserVJP runs (tests: float64 against torch.autograd.grad).  masks: those of another forward pass (the device's, unpack_masks)
    instead of the ones at x.  Returns (vjp, masks)."""
    masks = plan_masks(layers, x) if masks is None else masks
    return masked_vjp(layers, masks, v), masks


def plan_jvp(layers, x, v, masks=None):
    """J_D(x) v of the stack `layers` - the host statement of DenoiserJacobian.jvp, next to plan_vjp.  Returns (jvp, masks)."""
    masks = plan_masks(layers, x) if masks is None else masks
    return masked_jvp(layers, masks, v), masks


def plan_param_grads(layers, x, v, masks=None):
    """(dD/dtheta)^T v of the stack `layers` at x, one tensor per conv weight, in x's dtype - the host statement of what
    DenoiserParamGrads.grads runs, next to plan_vjp: one masked forward keeps each layer's input, the layers are walked backwards with
    masked_vjp's steps, and dW_i comes from layer i's input and the masked gradient behind it.  masks: those of another forward pass (the
    device's, unpack_masks) in place of the decisions at x.  Returns ([dW_0 .. dW_{k-1}], masks)."""
    inputs, used, h = [x], [], x
    for i, (w, b, relu) in enumerate(layers[:-1]):
        h = F.conv2d(h, w.to(x), None if b is None else b.to(x), padding=1)
        m = (masks[i] if masks is not None else h > 0) if relu else None
        used.append(m)
        if m is not None:
            h = h * m
        inputs.append(h)
    grads, g = [None] * len(layers), v
    for i in range(len(layers) - 1, -1, -1):
        grads[i] = torch.nn.grad.conv2d_weight(inputs[i], layers[i][0].shape, g, padding=1)
        if i > 0:
            g = F.conv2d(g, _transposed(layers[i][0].to(v)), padding=1)
            if used[i - 1] is not None:
                g = g * used[i - 1]
    return grads, used


_FROZEN_BN_OK, _FROZEN_FFDNET_OK = "bias-free conv [+ frozen BN] + ReLU stack", "FFDNet with its BatchNorm frozen"


def _bn_refusal(mods):
    """Why a BatchNorm2d of `mods` is not a fixed affine map with parameters of its own, or None."""
    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            if not m.track_running_stats or m.running_mean is None or m.running_var is None:
                return "BatchNorm2d without running statistics (track_running_stats=False: it normalises by the batch's)"
            if m.training:
                return "BatchNorm2d in train mode (batch statistics have no device kernel)"
            if not m.affine or m.weight is None or m.bias is None:
                return "BatchNorm2d without affine parameters (affine=False)"
    return None


def _train_bn_refusal(mods):
    """Why a BatchNorm2d of `mods` is not a train-mode BatchNorm the batch-statistics kernels serve, or None."""
    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            if not m.training:
                return 'BatchNorm2d in eval mode (frozen statistics: that is parameter_backward = "device+bn")'
            if not m.affine or m.weight is None or m.bias is None:
                return "BatchNorm2d without affine parameters (affine=False)"
            if not m.track_running_stats or m.running_mean is None or m.running_var is None or m.num_batches_tracked is None:
                return "BatchNorm2d without running statistics (track_running_stats=False: the kernels update them)"
            if m.momentum is None:
                return "BatchNorm2d with momentum=None (the cumulative moving average has no device kernel)"
            if isinstance(m.momentum, bool) or not isinstance(m.momentum, float):
                return f"BatchNorm2d with momentum={m.momentum!r}: a float is required"
    return None


def _frozen_bn_stack(net):
    """(stack, ffdnet, reason): layers.conv_bn_stack of a net the frozen-BatchNorm weight gradients serve - [(conv, bn or None, relu)] and
    whether its edge layers are FFDNet's - or (None, None, why not)."""
    return _bn_stack(net, False)


def _bn_stack(net, train):
    """_frozen_bn_stack (train=False), or the same for a net whose BatchNorms are in train mode (train=True)."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    ffdnet = isinstance(net, FFDNet)
    if ffdnet:
        if net.num_input_channels != 1:
            return None, None, "FFDNet with 3 channels (the HIP kernels cover the grayscale network only)"
        mods = list(net.intermediate_dncnn.itermediate_dncnn)
    else:
        if getattr(net, "tag", None) != "denoiser":
            return None, None, f"nonlinear_op tag {getattr(net, 'tag', None)!r}: only 'denoiser' and 'ffdnet' plugins have device weight gradients"
        if not isinstance(net, DnCNN):
            return None, None, f"not a conv [+BN] + ReLU stack: {type(net).__name__}"
        mods = list(net.dncnn)
    if any(isinstance(m, RealSNConv2d) for m in mods):
        return None, None, "RealSNConv2d (its parameter is weight_orig behind the spectral normalisation)"
    why = _train_bn_refusal(mods) if train else _bn_refusal(mods)
    if why is not None:
        return None, None, ("FFDNet: " if ffdnet else "") + why
    stack, why = conv_bn_stack(mods, train_bn=train)
    if stack is None:
        return None, None, why
    shapes = [tuple(c.weight.shape) for c, _, _ in stack]
    first, last = ((64, 5, 3, 3), (4, 64, 3, 3)) if ffdnet else ((64, 1, 3, 3), (1, 64, 3, 3))
    if len(stack) < 2 or shapes[0] != first or shapes[-1] != last or any(s != (64, 64, 3, 3) for s in shapes[1:-1]):
        return None, None, f"layer shapes {shapes}: the kernels cover {first[1]} -> 64 -> ... -> 64 -> {last[0]}"
    if not all(r for _, _, r in stack[:-1]) or stack[-1][2]:
        return None, None, "ReLU pattern other than after every layer but the last"
    if stack[0][1] is not None or stack[-1][1] is not None:
        return None, None, "BatchNorm2d behind the first or the last layer (the edge kernels have no scale)"
    if not all(isinstance(c.weight, torch.nn.Parameter) for c, _, _ in stack):
        return None, None, "a conv weight that is not an nn.Parameter"
    return stack, ffdnet, None


_TRAIN_BN_OK, _TRAIN_FFDNET_OK = "bias-free conv [+ train-mode BN] + ReLU stack", "FFDNet with its BatchNorm in train mode"


def param_eligibility(net, frozen_bn=False, train_bn=False):
    """(ok, reason): whether DenoiserParamGrads (and DEQFixedPoint.parameter_backward = "device") can form the weight gradients of `net`:
    a bias-free conv + ReLU stack 1 -> 64 -> ... -> 64 -> 1 whose conv weights are nn.Parameters - SimpleCNN, DnCNN(..., lip=0.0,
    no_bn=True) of any depth >= 2.  frozen_bn=True (parameter_backward = "device+bn") accepts in addition an eval-mode affine BatchNorm2d
    with running statistics behind every 64 -> 64 conv - DnCNN(..., no_bn=False).eval() - and the grayscale FFDNet with its BatchNorms in
    eval mode.  train_bn=True (parameter_backward = "device+bn-train") accepts those two families with their BatchNorms in TRAIN mode -
    affine, with running statistics and a float momentum (csrc/bn_train.hip) - and refuses an eval-mode BatchNorm.  CPU-safe."""
    if train_bn:
        if frozen_bn:
            raise ValueError("param_eligibility: frozen_bn and train_bn exclude one another")
        stack, ffdnet, why = _bn_stack(net, True)
        if stack is None:
            return False, why
        return True, _TRAIN_FFDNET_OK if ffdnet else _TRAIN_BN_OK
    if frozen_bn:
        stack, ffdnet, why = _frozen_bn_stack(net)
        if stack is None:
            return False, why
        return True, _FROZEN_FFDNET_OK if ffdnet else _FROZEN_BN_OK
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if isinstance(net, FFDNet):
        return False, "FFDNet: its 5 -> 64 / 64 -> 4 edge layers and BatchNorm2d parameters have no device weight gradient"
    if getattr(net, "tag", None) != "denoiser":
        return False, f"nonlinear_op tag {getattr(net, 'tag', None)!r}: only 'denoiser' plugins have device weight gradients"
    if not isinstance(net, DnCNN):
        return False, f"not a conv + ReLU stack: {type(net).__name__}"
    mods = list(net.dncnn)
    if any(isinstance(m, torch.nn.BatchNorm2d) for m in mods):
        return False, "BatchNorm2d (its gamma / beta gradients, and the batch statistics in train mode, have no device kernel)"
    if any(isinstance(m, RealSNConv2d) for m in mods):
        return False, "RealSNConv2d (its parameter is weight_orig behind the spectral normalisation)"
    layers, why = conv_stack(mods)
    if layers is None:
        return False, why
    shapes = [tuple(w.shape) for w, _, _ in layers]
    if len(layers) < 2 or shapes[0] != (64, 1, 3, 3) or shapes[-1] != (1, 64, 3, 3) or any(s != (64, 64, 3, 3) for s in shapes[1:-1]):
        return False, f"layer shapes {shapes}: the kernels cover 1 -> 64 -> ... -> 64 -> 1"
    if not all(r for _, _, r in layers[:-1]) or layers[-1][2]:
        return False, "ReLU pattern other than after every layer but the last"
    if not all(isinstance(m.weight, torch.nn.Parameter) for m in mods if isinstance(m, torch.nn.Conv2d)):
        return False, "a conv weight that is not an nn.Parameter"
    return True, "bias-free conv + ReLU stack"


def conv_weights(net):
    """The conv weights of a net param_eligibility accepts, in layer order: the parameters DenoiserParamGrads.grads answers for."""
    return [m.weight for m in net.dncnn if isinstance(m, torch.nn.Conv2d)]


def grad_parameters(net, train_bn=False):
    """The nn.Parameters of a net param_eligibility(net, frozen_bn=True) accepts, in module order - per layer the conv weight, then its
    BatchNorm's weight (gamma) and bias (beta): the parameters DenoiserParamGrads(..., frozen_bn=True).grads answers for.  train_bn=True:
    the same for a net param_eligibility(net, train_bn=True) accepts."""
    stack, _, why = _bn_stack(net, bool(train_bn))
    if stack is None:
        raise ValueError(f"grad_parameters: {why}")
    out = []
    for conv, bn, _ in stack:
        out.append(conv.weight)
        if bn is not None:
            out += [bn.weight, bn.bias]
    return out


def _bn_scale(bn, like):
    """(s, mean, 1 / sqrt(var + eps)) of a frozen BatchNorm in like's dtype and device."""
    T = lambda p: p.detach().to(like)
    inv = 1.0 / torch.sqrt(T(bn.running_var) + bn.eps)
    return T(bn.weight) * inv, T(bn.running_mean), inv


def plan_param_grads_frozen_bn(net, x, v, sigma=None, masks=None):
    """(dD/dtheta)^T v of a net param_eligibility(net, frozen_bn=True) accepts, at x, in x's dtype - the host statement of what
    DenoiserParamGrads(..., frozen_bn=True).grads runs: one masked forward of the unfolded layers y = relu(s conv(x, W) + t) keeps each
    layer's input, the walk back carries gm with the folded transposed weights, and per layer R = conv2d_weight(input, gm) gives
    dW = s R, dbeta = sum gm, dgamma = (sum W R - mean dbeta) / sqrt(var + eps).  FFDNet goes through FFDNET_EDGES at the noise level sigma
    (1 or n values; sigma's channel of the first weight included) and differentiates nothing through its input.  masks: those of another
    forward pass (the device's, unpack_masks).  Returns (gradients in grad_parameters order, masks)."""
    stack, ffdnet, why = _frozen_bn_stack(net)
    if stack is None:
        raise ValueError(f"plan_param_grads_frozen_bn: {why}")
    T = lambda p: p.detach().to(x)
    if ffdnet:
        _even(x, "plan_param_grads_frozen_bn")
        if sigma is None:
            raise ValueError("plan_param_grads_frozen_bn: FFDNet is evaluated at a noise level: sigma is required")
        read = FFDNET_EDGES[0]
        h, g = torch.cat((_sigma_map(sigma, x), read(x)), 1), read(v)
    else:
        h, g = x, v
    inputs, used, bns = [h], [], []
    for i, (conv, bn, relu) in enumerate(stack):
        bns.append(None if bn is None else _bn_scale(bn, x))
        if i == len(stack) - 1:
            break
        h = F.conv2d(h, T(conv.weight), padding=1)
        if bn is not None:
            s, mean, _ = bns[i]
            h = h * s.view(1, -1, 1, 1) + (T(bn.bias) - mean * s).view(1, -1, 1, 1)
        m = (masks[i] if masks is not None else h > 0) if relu else None
        used.append(m)
        if m is not None:
            h = h * m
        inputs.append(h)
    per_layer = [None] * len(stack)
    for i in range(len(stack) - 1, -1, -1):
        W = T(stack[i][0].weight)
        R = torch.nn.grad.conv2d_weight(inputs[i], W.shape, g, padding=1)
        if bns[i] is None:
            per_layer[i], folded = [R], W
        else:
            s, mean, inv = bns[i]
            dbeta = g.sum((0, 2, 3))
            per_layer[i] = [s.view(-1, 1, 1, 1) * R, ((W * R).sum((1, 2, 3)) - mean * dbeta) * inv, dbeta]
            folded = W * s.view(-1, 1, 1, 1)
        if i > 0:
            g = F.conv2d(g, _transposed(folded), padding=1)
            if used[i - 1] is not None:
                g = g * used[i - 1]
    return [t for layer in per_layer for t in layer], used


# ----------------------------------------------------------------------------- BatchNorm in train mode: the host statements
def _train_bn_walk(who, net, x, sigma, masks, update):
    """One train-mode forward of a net param_eligibility(net, train_bn=True) accepts, in x's dtype.  -> (stack, ffdnet, noise, tape), tape =
    per layer but the last (input, c, xhat or None, 1 / sqrt(var + eps) or None, mask or None), then the last layer's input."""
    stack, ffdnet, why = _bn_stack(net, True)
    if stack is None:
        raise ValueError(f"{who}: {why}")
    T = lambda p: p.detach().to(x)
    if ffdnet:
        _even(x, who)
        if sigma is None:
            raise ValueError(f"{who}: FFDNet is evaluated at a noise level: sigma is required")
        h = torch.cat((_sigma_map(sigma, x), F.pixel_unshuffle(x, 2)), 1)
    else:
        h = x
    tape = []
    for i, (conv, bn, relu) in enumerate(stack[:-1]):
        c = F.conv2d(h, T(conv.weight), padding=1)
        xhat = inv = None
        y = c
        if bn is not None:
            P = c.numel() // c.shape[1]
            if P < 2:
                raise ValueError(f"{who}: expected more than 1 value per channel when training, got input size {list(c.shape)}")
            mean, var = c.mean((0, 2, 3)), c.var((0, 2, 3), unbiased=False)
            inv = 1.0 / torch.sqrt(var + bn.eps)
            xhat = (c - mean.view(1, -1, 1, 1)) * inv.view(1, -1, 1, 1)
            y = xhat * T(bn.weight).view(1, -1, 1, 1) + T(bn.bias).view(1, -1, 1, 1)
            if update:
                with torch.no_grad():
                    m = bn.momentum
                    bn.running_mean.copy_((1.0 - m) * bn.running_mean.to(mean) + m * mean)
                    bn.running_var.copy_((1.0 - m) * bn.running_var.to(var) + m * (var * (P / (P - 1))))
                    bn.num_batches_tracked += 1
        m = (masks[i] if masks is not None else y > 0) if relu else None
        tape.append((h, c, xhat, inv, m))
        h = y if m is None else y * m
    tape.append(h)
    noise = F.conv2d(h, T(stack[-1][0].weight), padding=1)
    return stack, ffdnet, (F.pixel_shuffle(noise, 2) if ffdnet else noise), tape


def plan_forward_train_bn(net, x, sigma=None, update=True):
    """One train-mode forward of a net param_eligibility(net, train_bn=True) accepts, restated in x's dtype: per BatchNorm layer the mean and
    the biased variance of c = conv(x, W) over the batch, y = gamma (c - mean) / sqrt(var + eps) + beta, the ReLU; FFDNet at the noise level
    sigma through its pixel-(un)shuffle.  update=True moves the module's buffers as torch does: running_mean <- (1 - m) running_mean + m mean,
    running_var <- (1 - m) running_var + m var P / (P - 1), num_batches_tracked += 1.  -> (noise, masks)."""
    _, _, noise, tape = _train_bn_walk("plan_forward_train_bn", net, x, sigma, None, update)
    return noise, [t[4] for t in tape[:-1]]


def _train_bn_backward(stack, ffdnet, tape, v):
    """The walk back of plan_param_grads_train_bn.  -> (gradients in grad_parameters order, the input gradient or None for FFDNet)."""
    T = lambda p: p.detach().to(v)
    per_layer = [None] * len(stack)
    dc = F.pixel_unshuffle(v, 2) if ffdnet else v
    for i in range(len(stack) - 1, -1, -1):
        conv, bn, _ = stack[i]
        W = T(conv.weight)
        inp = tape[i] if i == len(stack) - 1 else tape[i][0]
        if i < len(stack) - 1:
            _, c, xhat, inv, m = tape[i]
            gm = g if m is None else g * m
            if bn is None:
                per_layer[i], dc = [None], gm
            else:
                P = c.numel() // c.shape[1]
                dbeta, dgamma = gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))
                dc = (T(bn.weight) * inv).view(1, -1, 1, 1) * (gm - (dbeta / P).view(1, -1, 1, 1) - xhat * (dgamma / P).view(1, -1, 1, 1))
                per_layer[i] = [None, dgamma, dbeta]
        else:
            per_layer[i] = [None]
        per_layer[i][0] = torch.nn.grad.conv2d_weight(inp, W.shape, dc, padding=1)
        if i > 0:
            g = F.conv2d(dc, _transposed(W), padding=1)
    gx = None if ffdnet else F.conv2d(dc, _transposed(T(stack[0][0].weight)), padding=1)
    return [t for layer in per_layer for t in layer], gx


def plan_param_grads_train_bn(net, x, v, sigma=None, masks=None, input_grad=False):
    """(dD/dtheta)^T v of a net param_eligibility(net, train_bn=True) accepts, at x, in x's dtype - the host statement of what
    DenoiserParamGrads(..., train_bn=True).grads runs: one train-mode forward (plan_forward_train_bn's, the buffers left alone) keeps each
    layer's input, c and xhat; walking back, per layer with a BatchNorm and gm the gradient masked by its ReLU: dbeta = sum gm,
    dgamma = sum gm xhat, dc = gamma / sqrt(var + eps) (gm - dbeta / P - xhat dgamma / P), dW = conv2d_weight(input, dc), and dc goes down
    through the UNFOLDED transposed weight.  masks: those of another forward pass (the device's, unpack_masks).  Returns (gradients in
    grad_parameters(net, train_bn=True) order, masks) - with input_grad=True (gradients, masks, J_D(x)^T v: the true input product,
    statistic terms included; None for FFDNet, which detaches its input)."""
    stack, ffdnet, _, tape = _train_bn_walk("plan_param_grads_train_bn", net, x, sigma, masks, False)
    grads, gx = _train_bn_backward(stack, ffdnet, tape, v)
    used = [t[4] for t in tape[:-1]]
    return (grads, used, gx) if input_grad else (grads, used)


# ----------------------------------------------------------------------------- FFDNet, differentiated through its input
def ffdnet_plan(net):
    """Grayscale FFDNet in eval mode as [(weight, bias or None, relu)]: (64,5,3,3) first, 13 x (64,64,3,3) with the BatchNorm folded
    (layers.conv_stack), (4,64,3,3) last.  Functional: ffdnet_plan_forward does not detach its input.  Usable on the CPU."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if not isinstance(net, FFDNet) or net.num_input_channels != 1:
        raise ValueError("ffdnet_plan: a grayscale FFDNet is required")
    mods = net.intermediate_dncnn.itermediate_dncnn
    if any(isinstance(m, RealSNConv2d) for m in mods):
        raise ValueError("ffdnet_plan: RealSNConv2d where FFDNet has a Conv2d")
    layers, why = conv_stack(mods)
    if layers is None:
        raise ValueError(f"ffdnet_plan: {why}")
    shapes = [tuple(w.shape) for w, _, _ in layers]
    if (len(layers) < 3 or shapes[0] != (64, 5, 3, 3) or shapes[-1] != (4, 64, 3, 3) or any(s != (64, 64, 3, 3) for s in shapes[1:-1])
            or not all(r for _, _, r in layers[:-1]) or layers[-1][2] or layers[0][1] is not None or layers[-1][1] is not None):
        raise ValueError(f"ffdnet_plan: layer shapes {shapes} are not the grayscale network's")
    return layers


def _even(x, what):
    if x.dim() != 4 or x.shape[1] != 1 or x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError(f"{what}: FFDNet needs a (n,1,even,even) image (its first layer is a 2x2 pixel-unshuffle), got {tuple(x.shape)}")


def _sigma_map(sigma, x):
    n, _, H, W = x.shape
    s = torch.as_tensor(sigma, dtype=x.dtype, device=x.device).reshape(-1)
    return (s.expand(n) if s.numel() == 1 else s).reshape(n, 1, 1, 1).expand(n, 1, H // 2, W // 2)


def ffdnet_plan_forward(layers, x, sigma):
    """(noise, masks) of FFDNet at (x, sigma) in x's dtype, through the input (no detach): masks[i] is the ReLU decision behind layer i."""
    _even(x, "ffdnet_plan_forward")
    h, masks = masked_forward(layers, torch.cat((_sigma_map(sigma, x), F.pixel_unshuffle(x, 2)), 1))
    return F.pixel_shuffle(F.conv2d(h, layers[-1][0].to(x), padding=1), 2), masks


def ffdnet_plan_jvp(layers, x, sigma, v, masks=None):
    """J_D(x; sigma) v of FFDNet through its input (sigma a constant: its channel of the first layer carries no tangent).  -> (jvp, masks)"""
    _even(x, "ffdnet_plan_jvp")
    masks = ffdnet_plan_forward(layers, x, sigma)[1] if masks is None else masks
    return masked_jvp(layers, masks, v, FFDNET_EDGES), masks


def ffdnet_plan_vjp(layers, x, sigma, v, masks=None):
    """J_D(x; sigma)^T v of FFDNet through its input.  -> (vjp, masks)"""
    _even(x, "ffdnet_plan_vjp")
    masks = ffdnet_plan_forward(layers, x, sigma)[1] if masks is None else masks
    return masked_vjp(layers, masks, v, FFDNET_EDGES), masks


def unpack_masks(words):
    """relu_mask_pack's (n,H,W) int64 words -> the (n,64,H,W) bool mask the host plans take (bit c = channel c)."""
    bits = torch.arange(64, device=words.device, dtype=torch.int64).view(1, 64, 1, 1)
    return ((words.unsqueeze(1) >> bits) & 1).bool()


FFDNET_THROUGH_INPUT = "FFDNet: through the input"          # jacobian_eligibility's reason for the one net that is not a plain stack


def jacobian_eligibility(net):
    """(ok, reason): whether DenoiserJacobian can linearise `net`.  eligibility's refusals; FFDNet is differentiated through its input.  CPU-safe."""
    ok, why = eligibility(net)
    if ok and why == _FFDNET_OK:
        return True, FFDNET_THROUGH_INPUT
    return ok, why


# ----------------------------------------------------------------------------- the device: one masked stack
class _MaskedStack:
    """The layers of a plan linearised at the fp32 GPU image x, on the HIP kernels.  One forward pass at x (first layer stencil, Winograd
    F(2x2,3x3) with the folded BN bias) builds the ReLU masks (.masks: relu_mask_pack's words per layer); jvp and vjp are then linear in v:
    masked layers enqueued on the current stream with no host synchronisation, no pack made twice.  sigma: FFDNet's (1,) or (n,) fp32
    noise levels on x's device - its plan (ffdnet_plan), read through the 2x2 pixel-unshuffle: csrc/jacobian.hip's masked first layer
    serves the linearised head and the transposed tail, deqsci_ffdnet_tail_f32 without bias the linearised tail and the transposed head.
    None: a 1 -> 64 -> ... -> 64 -> 1 stack (host_plan).  keep: hold every post-ReLU activation of the forward pass (.acts[i] = the input
    of layer i + 1, (k-1) n 64 H W 4 bytes in all) - what the weight gradients are formed from (DenoiserParamGrads)."""

    def __init__(self, layers, x, sigma=None, keep=False):
        x = _hip.f32c(x.detach())
        f32 = lambda t: t.to(x.device, torch.float32)
        self.ffdnet = sigma is not None
        with torch.no_grad():
            w0, wt = f32(layers[0][0]), f32(layers[-1][0])
            mid = [f32(w) for w, _, _ in layers[1:-1]]
            if self.ffdnet:
                win = w0[:, 1:5]                                    # (channel 0 is sigma's: it carries no tangent)
                self.head_f = _hip.pack_head_masked_weights(win.contiguous())
                self.tail_f = _hip.pack_tail_weights(wt)
                self.tail_t = _hip.pack_head_masked_weights(_transposed(wt))
                self.head_t = _hip.pack_tail_weights(_transposed(win))
                h = _hip.ffdnet_head(x, _hip.pack_head_weights(w0), sigma)
            else:
                self.head_f = _hip.pack_c1_to_64_weights(w0)
                self.tail_f = _hip.pack_c64_to_1_weights(wt)
                self.tail_t = _hip.pack_c1_to_64_weights(_transposed(wt))
                self.head_t = _hip.pack_c64_to_1_weights(_transposed(w0))
                h = _hip.conv3x3_c1_to_64(x, self.head_f, relu=True)
            self.mid_f = [_hip.pack_winograd_weights(w) for w in mid]
            self.mid_t = [_hip.pack_winograd_weights(_transposed(w)) for w in mid]
            self.masks = [_hip.relu_mask_pack(h)]
            self.acts = [h] if keep else None
            for u, (_, b, _) in zip(self.mid_f, layers[1:-1]):
                h = _hip.conv3x3_c64_winograd(h, u, None if b is None else f32(b).contiguous(), True)
                self.masks.append(_hip.relu_mask_pack(h))
                if keep:
                    self.acts.append(h)

    def jvp(self, v):
        first = _hip.ffdnet_head_masked if self.ffdnet else _hip.conv3x3_c1_to_64_masked
        t = first(_hip.f32c(v), self.head_f, self.masks[0])
        for i, u in enumerate(self.mid_f):
            t = _hip.conv3x3_c64_winograd_masked(t, u, self.masks[i + 1])
        return _hip.ffdnet_tail(t, self.tail_f) if self.ffdnet else _hip.conv3x3_c64_to_1(t, self.tail_f)

    def vjp(self, v):
        first = _hip.ffdnet_head_masked if self.ffdnet else _hip.conv3x3_c1_to_64_masked
        g = first(_hip.f32c(v), self.tail_t, self.masks[-1])
        for i in range(len(self.mid_t) - 1, -1, -1):           # layer i + 1 transposed, masked by the ReLU in front of it
            g = _hip.conv3x3_c64_winograd_masked(g, self.mid_t[i], self.masks[i])
        return _hip.ffdnet_tail(g, self.head_t) if self.ffdnet else _hip.conv3x3_c64_to_1(g, self.head_t)


def _image(x, who):
    if x.dim() != 4 or x.shape[1] != 1 or not x.is_cuda:
        raise _hip.DeqsciHipError(f"{who}: x must be a (n,1,H,W) GPU image, got {tuple(x.shape)} on {x.device}")
    return tuple(x.shape)


class DenoiserJacobian:
    """v -> J_D(x) v (.jvp) and v -> J_D(x)^T v (.vjp) for a (n,1,H,W) fp32 GPU image x and v of its shape, on the HIP kernels
    (_MaskedStack; .masks are its ReLU masks): a diagnostic of the map the iteration applies, so FFDNet (grayscale, eval mode) is
    differentiated through its input at the noise level sigma, a constant of the linearisation.  Raises ValueError for a net
    jacobian_eligibility refuses and for an FFDNet image with an odd side, before any launch."""

    def __init__(self, net, x, sigma=None):
        ok, why = jacobian_eligibility(net)
        if not ok:
            raise ValueError(f"DenoiserJacobian: {why}")
        self.shape = _image(x, "DenoiserJacobian")
        if why == FFDNET_THROUGH_INPUT:
            _even(x, "DenoiserJacobian")
            if sigma is None:
                raise ValueError("DenoiserJacobian: FFDNet is linearised at a noise level: sigma is required")
            layers = ffdnet_plan(net)
            sigma = torch.as_tensor(sigma, dtype=torch.float32, device=x.device).reshape(-1).contiguous()
            if sigma.numel() not in (1, x.shape[0]):
                raise ValueError(f"DenoiserJacobian: sigma must have 1 or {x.shape[0]} elements, got {sigma.numel()}")
        else:
            layers, sigma = host_plan(net)[0], None
        self._stack = _MaskedStack(layers, x, sigma)
        self.masks = self._stack.masks

    def _v(self, v, what):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"DenoiserJacobian.{what}: v must have the shape {self.shape} of x, got {tuple(v.shape)}")
        return v

    def jvp(self, v):
        return self._stack.jvp(self._v(v, "jvp"))

    def vjp(self, v):
        return self._stack.vjp(self._v(v, "vjp"))


class DenoiserVJP:
    """v -> J_D(x)^T v for a (n,1,H,W) fp32 GPU image x and v of its shape: _MaskedStack.vjp, k-1 masked transposed layers and the 64 -> 1
    stencil per call, enqueued on the current stream with no host synchronisation (safe to capture).  sigma: FFDNet's noise level (unused:
    its input is detached, the product is zero - no launches, no masks).  Raises ValueError with eligibility()'s reason for a net it
    cannot differentiate."""

    def __init__(self, net, x, sigma=None):
        ok, why = eligibility(net)
        if not ok:
            raise ValueError(f"DenoiserVJP: {why}")
        self.shape = _image(x, "DenoiserVJP")
        self.zero = why == _FFDNET_OK
        self._stack = None if self.zero else _MaskedStack(host_plan(net)[0], x)
        self.masks = [] if self.zero else self._stack.masks

    def __call__(self, v):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"DenoiserVJP: v must have the shape {self.shape} of x, got {tuple(v.shape)}")
        return torch.zeros_like(v) if self.zero else self._stack.vjp(v)


class DenoiserParamGrads:
    """The denoiser's weight gradients on the device, for a (n,1,H,W) fp32 GPU image x: one forward pass on _MaskedStack's kernels
    (1 -> 64 stencil, Winograd F(2x2,3x3), relu_mask_pack) that keeps the post-ReLU activations - (k-1) n 64 H W 4 bytes - and the masks;
    .noise = D(x) from that pass (the 64 -> 1 stencil), .masks, .shape.  .grads(v) -> [dW_0 .. dW_{k-1}] = (dD/dtheta)^T v, one tensor per
    conv weight (conv_weights(net)): the masked transposed layers of .vjp carry the gradient down, csrc/wgrad.hip's W1 serves the two edge
    layers and W0 every 64 -> 64 layer.  need: one bool per weight - the walk stops below the lowest layer asked for, the others are None.
    .vjp(v) is the input product J_D(x)^T v.  .release() drops the activations.  Everything is enqueued on the current stream with no host
    synchronisation.  Raises ValueError with param_eligibility()'s reason.

    frozen_bn=True: the nets param_eligibility(net, frozen_bn=True) accepts, the BatchNorm folded into the forward and the walk as in
    _MaskedStack; .grads answers for grad_parameters(net) in its order (per layer dW, then dgamma, dbeta) and `need` has one bool per
    parameter.  A 64 -> 64 layer with a BatchNorm runs csrc/wgrad_bn.hip's W0-BN (dW = s R, dbeta, and sum W R for dgamma, from one pass).
    FFDNet (sigma: its (1,) or (n,) noise levels, required) reads both edge layers through the pixel-(un)shuffle with W2, .noise is
    ffdnet_tail's, and .vjp is zero: its input is detached.

    train_bn=True: the nets param_eligibility(net, train_bn=True) accepts - the BatchNorms in TRAIN mode, as the reference trains them.  The
    forward runs per layer the raw convolution (Winograd F(2x2,3x3), no bias, no ReLU), csrc/bn_train.hip's T1 (batch statistics; the
    module's running_mean / running_var / num_batches_tracked are updated IN PLACE on the device, exactly once per construction) and T2
    (normalise + ReLU + the mask words in one pass), and keeps per BatchNorm layer the convolution output c AND the post-ReLU activation:
    (2 (k-2) + 1) n 64 H W 4 bytes for k layers (FFDNet: 27 activations at half resolution), twice the frozen mode's.  .grads answers for
    grad_parameters(net, train_bn=True): T3 (dgamma, dbeta) -> T4 (dc, in place) -> W0 on dc -> the masked transposed Winograd layer with
    the plain (unfolded) transposed weight.  .vjp(v) is the true input product, the statistic terms included (FFDNet: zero)."""

    def __init__(self, net, x, sigma=None, frozen_bn=False, train_bn=False):
        self._train = None
        if train_bn:
            if frozen_bn:
                raise ValueError("DenoiserParamGrads: frozen_bn and train_bn exclude one another")
            self._init_train_bn(net, x, sigma)
            return
        ok, why = param_eligibility(net, frozen_bn=frozen_bn)
        if not ok:
            raise ValueError(f"DenoiserParamGrads: {why}")
        self.shape = _image(x, "DenoiserParamGrads")
        self._x = _hip.f32c(x.detach())
        n, _, H, W = self.shape
        self.ffdnet = why == _FROZEN_FFDNET_OK
        self._sigma, self._bn, self._ws_bn = None, None, None
        if self.ffdnet:
            _even(x, "DenoiserParamGrads")
            if sigma is None:
                raise ValueError("DenoiserParamGrads: FFDNet is evaluated at a noise level: sigma is required")
            self._sigma = torch.as_tensor(sigma, dtype=torch.float32, device=x.device).reshape(-1)
            if self._sigma.numel() not in (1, n):
                raise ValueError(f"DenoiserParamGrads: sigma must have 1 or {n} elements, got {self._sigma.numel()}")
            if self._sigma.numel() > 1 and self._sigma.stride(0) not in (0, 1):
                self._sigma = self._sigma.contiguous()
            self._stack = _MaskedStack(ffdnet_plan(net), self._x, self._sigma, keep=True)
            self.noise = _hip.ffdnet_tail(self._stack.acts[-1], self._stack.tail_f)
            H, W = H // 2, W // 2
        else:
            self._stack = _MaskedStack(host_plan(net)[0], self._x, keep=True)
            self.noise = _hip.conv3x3_c64_to_1(self._stack.acts[-1], self._stack.tail_f)
        self.masks = self._stack.masks
        plain = True
        if frozen_bn:
            stack = _frozen_bn_stack(net)[0]
            dev = lambda t, dt=torch.float32: t.detach().to(x.device, dt).contiguous()
            self._bn = []                                                    # per layer None, or (w, s fp32; mean, 1 / sqrt(var + eps) float64)
            for conv, bn, _ in stack:
                if bn is None:
                    self._bn.append(None)
                else:
                    inv = 1.0 / torch.sqrt(dev(bn.running_var, torch.float64) + bn.eps)
                    self._bn.append((dev(conv.weight), (dev(bn.weight, torch.float64) * inv).float(), dev(bn.running_mean, torch.float64), inv))
            if self.ffdnet or any(b is not None for b in self._bn):
                self._ws_bn = _hip.wgrad_bn_workspace(n, H, W, self._x.device)
            plain = not self.ffdnet or any(b is None for b in self._bn[1:-1])
        self._ws = _hip.wgrad_workspace(n, H, W, self._x.device) if plain else None

    def _v(self, v, what):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"DenoiserParamGrads.{what}: v must have the shape {self.shape} of x, got {tuple(v.shape)}")
        return _hip.f32c(v)

    def _init_train_bn(self, net, x, sigma):
        stack, ffdnet, why = _bn_stack(net, True)
        if stack is None:
            raise ValueError(f"DenoiserParamGrads: {why}")
        self.shape = _image(x, "DenoiserParamGrads")
        self._x = _hip.f32c(x.detach())
        n, _, H, W = self.shape
        self.ffdnet, self._sigma = ffdnet, None
        if ffdnet:
            _even(x, "DenoiserParamGrads")
            if sigma is None:
                raise ValueError("DenoiserParamGrads: FFDNet is evaluated at a noise level: sigma is required")
            self._sigma = torch.as_tensor(sigma, dtype=torch.float32, device=x.device).reshape(-1)
            if self._sigma.numel() not in (1, n):
                raise ValueError(f"DenoiserParamGrads: sigma must have 1 or {n} elements, got {self._sigma.numel()}")
            if self._sigma.numel() > 1 and self._sigma.stride(0) not in (0, 1):
                self._sigma = self._sigma.contiguous()
            H, W = H // 2, W // 2
        if n * H * W < 2:
            raise ValueError(f"DenoiserParamGrads: expected more than 1 value per channel when training, got {n * H * W}")
        dev = lambda t: t.detach().to(x.device, torch.float32).contiguous()
        t = self._train = type("_TrainBN", (), {})()
        with torch.no_grad():
            w0, wt = dev(stack[0][0].weight), dev(stack[-1][0].weight)
            if ffdnet:
                t.tail_f, t.tail_t, t.head_t = _hip.pack_tail_weights(wt), _hip.pack_head_masked_weights(_transposed(wt)), None
                h = _hip.ffdnet_head(self._x, _hip.pack_head_weights(w0), self._sigma)
            else:
                t.tail_f, t.tail_t = _hip.pack_c64_to_1_weights(wt), _hip.pack_c1_to_64_weights(_transposed(wt))
                t.head_t = _hip.pack_c64_to_1_weights(_transposed(w0))
                h = _hip.conv3x3_c1_to_64(self._x, _hip.pack_c1_to_64_weights(w0), relu=True)
            t.ws = _hip.bn_train_workspace(n * H * W, x.device)
            self.masks, t.acts, t.layers = [_hip.relu_mask_pack(h)], [h], []        # layers[i - 1] of 64 -> 64 layer i: (transposed pack, bn state)
            for conv, bn, _ in stack[1:-1]:
                w = dev(conv.weight)
                u, ut = _hip.pack_winograd_weights(w), _hip.pack_winograd_weights(_transposed(w))
                if bn is None:
                    h = _hip.conv3x3_c64_winograd(h, u, None, True)
                    self.masks.append(_hip.relu_mask_pack(h))
                    t.layers.append((ut, None))
                else:
                    c = _hip.conv3x3_c64_winograd(h, u, None, False)
                    rec = _hip.bn_train_stats(c, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, workspace=t.ws)
                    gamma = dev(bn.weight)
                    h, mk = _hip.bn_train_apply(c, rec, gamma, dev(bn.bias), bn.eps, relu=True, want_mask=True)
                    self.masks.append(mk)
                    t.layers.append((ut, (c, rec, gamma, float(bn.eps))))
                t.acts.append(h)
            self.noise = (_hip.ffdnet_tail if ffdnet else _hip.conv3x3_c64_to_1)(h, t.tail_f)
        self._ws = _hip.wgrad_workspace(n, H, W, x.device)
        self._ws_bn = _hip.wgrad_bn_workspace(n, H, W, x.device) if ffdnet else None

    def _walk_train_bn(self, v, need, want_input):
        """The walk back in train mode: (gradients in grad_parameters(net, train_bn=True) order - None where not needed, the input product or None)."""
        t = self._train
        if t.acts is None:
            raise RuntimeError("DenoiserParamGrads.grads: the activations were released")
        k = len(t.layers) + 2
        counts = [1] + [1 if bn is None else 3 for _, bn in t.layers] + [1]
        first = [sum(counts[:i]) for i in range(k)]
        total = sum(counts)
        need = [False] * total if need is None else [bool(b) for b in need]
        if len(need) != total:
            raise ValueError(f"DenoiserParamGrads.grads: need has {len(need)} entries for {total} parameters")
        out = [None] * total
        if not any(need) and not want_input:
            return out, None
        wanted = [any(need[first[i]:first[i] + counts[i]]) for i in range(k)]
        lowest = -1 if want_input else wanted.index(True)
        if wanted[k - 1]:
            out[first[k - 1]] = (_hip.wgrad_shuffle(v, t.acts[-1], 1, None, self._ws_bn) if self.ffdnet
                                 else _hip.wgrad_c1_c64(v, t.acts[-1], 1, self._ws))
        if lowest == k - 1:
            return out, None
        g = (_hip.ffdnet_head_masked if self.ffdnet else _hip.conv3x3_c1_to_64_masked)(v, t.tail_t, self.masks[-1])
        for i in range(k - 2, 0, -1):
            ut, bn = t.layers[i - 1]
            got = [None] * counts[i]
            if bn is not None:
                c, rec, gamma, eps = bn
                got[1], got[2], grec = _hip.bn_train_grad_stats(g, c, rec, eps, t.ws)
                g = _hip.bn_train_grad_apply(g, c, rec, grec, gamma, eps, out=g)         # dc, statistic terms included, in place
            if need[first[i]]:
                got[0] = _hip.wgrad_c64_c64(t.acts[i - 1], g, self._ws)
            for j, tensor in enumerate(got):
                out[first[i] + j] = tensor if need[first[i] + j] else None
            if i == lowest:
                return out, None
            g = _hip.conv3x3_c64_winograd_masked(g, ut, self.masks[i - 1])
        if need[0]:
            out[0] = _hip.wgrad_shuffle(self._x, g, 0, self._sigma, self._ws_bn) if self.ffdnet else _hip.wgrad_c1_c64(self._x, g, 0, self._ws)
        return out, (_hip.conv3x3_c64_to_1(g, t.head_t) if want_input else None)

    def vjp(self, v):
        v = self._v(v, "vjp")
        if self.ffdnet:
            return torch.zeros_like(v)
        return self._walk_train_bn(v, None, True)[1] if self._train is not None else self._stack.vjp(v)

    def _middle(self, i, g):
        """[dW] of 64 -> 64 layer i, or [dW, dgamma, dbeta] where it has a BatchNorm, from its input and the masked gradient g behind it."""
        st = self._stack
        bn = None if self._bn is None else self._bn[i]
        if bn is None:
            return [_hip.wgrad_c64_c64(st.acts[i - 1], g, self._ws)]
        w, s, mean, inv = bn
        dw, dsum, ddot = _hip.wgrad_c64_c64_bn(st.acts[i - 1], g, w, s, self._ws_bn)
        return [dw, ((ddot.double() - mean * dsum.double()) * inv).float(), dsum]

    def grads(self, v, need=None):
        if self._train is not None:
            total = 2 + sum(1 if bn is None else 3 for _, bn in self._train.layers)
            return self._walk_train_bn(self._v(v, "grads"), [True] * total if need is None else need, False)[0]
        st = self._stack
        if st.acts is None:
            raise RuntimeError("DenoiserParamGrads.grads: the activations were released")
        k = len(st.mid_t) + 2
        counts = [1] * k if self._bn is None else [1 if b is None else 3 for b in self._bn]      # parameters per layer
        first = [sum(counts[:i]) for i in range(k)]
        total = sum(counts)
        need = [True] * total if need is None else [bool(b) for b in need]
        if len(need) != total:
            raise ValueError(f"DenoiserParamGrads.grads: need has {len(need)} entries for {total} parameters")
        v = self._v(v, "grads")
        out = [None] * total
        if not any(need):
            return out
        wanted = [any(need[first[i]:first[i] + counts[i]]) for i in range(k)]
        lowest = wanted.index(True)
        if wanted[k - 1]:
            out[first[k - 1]] = (_hip.wgrad_shuffle(v, st.acts[-1], 1, None, self._ws_bn) if self.ffdnet
                                 else _hip.wgrad_c1_c64(v, st.acts[-1], 1, self._ws))
        if lowest == k - 1:
            return out
        # the gradient behind layer k-2, masked by its ReLU
        g = (_hip.ffdnet_head_masked if self.ffdnet else _hip.conv3x3_c1_to_64_masked)(v, st.tail_t, st.masks[-1])
        for i in range(k - 2, 0, -1):
            if wanted[i]:
                for j, t in enumerate(self._middle(i, g)):
                    out[first[i] + j] = t if need[first[i] + j] else None
            if i == lowest:
                return out
            g = _hip.conv3x3_c64_winograd_masked(g, st.mid_t[i - 1], st.masks[i - 1])
        out[0] = _hip.wgrad_shuffle(self._x, g, 0, self._sigma, self._ws_bn) if self.ffdnet else _hip.wgrad_c1_c64(self._x, g, 0, self._ws)
        return out

    def release(self):
        if self._train is not None:
            self._train.acts = None
            self._train.layers = [(ut, None if bn is None else (None,) + bn[1:]) for ut, bn in self._train.layers]
        else:
            self._stack.acts = None
