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

The weight gradients (dD/dtheta)^T v come from ONE walk in every mode, stated once on the host (_taped_forward, _walk_back) and once on
the device (_MaskedStack's forward, DenoiserParamGrads._walk): a forward that keeps each layer's input, then the transposed masked layers
carry v down and every layer forms its gradients from its input and the masked gradient gm behind it.  What a layer is - how it runs
forward, what it forms, what it hands down and through which transposed weight - is its RULE; the edge layers, plain or FFDNet's, come
from PLAIN_EDGES / FFDNET_EDGES.

There are four MODES, and GRAD_MODES states each of them once, as a GradMode:
    name           parameter_backward     serves (in order)               engine option            nets (its stack)       host rule      device rule
    plain          "device"               plain                           -                        bn_stack(net, None)    _PlainRule     _Conv64
    train_realsn   "device+realsn"        plain, train_realsn             train_realsn="device"    realsn_stack(net)      _RealSNRule    _RealSN64
    frozen_bn      "device+bn"            plain, frozen_bn                -                        bn_stack(net, False)   _FrozenRule    _Frozen64
    train_bn       "device+bn-train"      plain, frozen_bn, train_bn      train_bn="device"        bn_stack(net, True)    _TrainRule     _Train64
(a layer without a BatchNorm is _PlainRule / _Conv64 in every mode).  The name is the public keyword that asks for the mode: grad_mode
resolves frozen_bn= / train_bn= / train_realsn= to one, once, at the first line of every public entry point, and switch_modes a
parameter_backward string to the modes it serves.  Everything else - the solver's _param_mode, DEQFixedPoint._taped_call,
training.configure_training, engine._Denoiser's train-mode f-calls, the host statements plan_* and DenoiserParamGrads - reads the record: a
new mode is a new row.  _structure_refusal says what shape a mode's nets must have.  What the four compute:

No BatchNorm - a bias-free conv + ReLU stack, DEQFixedPoint.parameter_backward = "device", param_eligibility(net): dW = wgrad(x, gm), the
correlation of the layer's input with the masked gradient behind it (csrc/wgrad.hip: W0 for a 64 -> 64 layer, W1 for the two edge
layers), and gm goes down through W^T.

A frozen (eval-mode) BatchNorm behind the conv - FFDNet, a conv + BN + ReLU DnCNN; parameter_backward = "device+bn",
param_eligibility(net, frozen_bn=True) - the layer is y = relu(s c + t), c = conv(x, W), s = gamma / sqrt(var + eps), t = beta - mean s, and
with R = wgrad(x, gm), gm going down through (s W)^T:

    dW = s R        dbeta = sum_p gm        dgamma = (sum_{ci,tap} W R - mean dbeta) / sqrt(var + eps)

(sum_p gm c = sum W R: no stored pre-activation and no division by gamma, exact for gamma = 0 and gamma < 0; csrc/wgrad_bn.hip's W0-BN gives
the three sums from one pass).  FFDNet's edge layers are read through the 2x2 pixel-(un)shuffle by W2 of the same file, sigma's channel of
the first weight included.

The BatchNorm in TRAIN mode - what the reference trains: it calls .eval() under --inference only; parameter_backward =
"device+bn-train", param_eligibility(net, train_bn=True) - the layer is y = relu(gamma xhat + beta), xhat = (c - mean) / sqrt(var + eps) with
the mean and the biased variance of c = conv(x, W) over the batch's P = n H W pixels, and:

    dbeta = sum_p gm        dgamma = sum_p gm xhat        dc = gamma / sqrt(var + eps) (gm - dbeta / P - xhat dgamma / P)        dW = wgrad(x, dc)

(csrc/bn_train.hip: T1 statistics and the running buffers' update, T2 apply + mask, T3 the two sums, T4 dc; dc goes down through the UNFOLDED
transposed weight).  The statistic terms reach the pixels the ReLU masked too.

Spectral normalisation in TRAIN mode - RealSN_SimpleCNN as the reference trains it; parameter_backward / implicit_backward =
"device+realsn", the engine's train_realsn="device", param_eligibility(net, train_realsn=True); realsn_stack says which nets qualify - the
layer's parameter is weight_orig and its weight = weight_orig / cur_sigma * sigma changes at every call (csrc/realsn.hip R1).  The packs the
kernels read are therefore made on the device, by R3 of the same file, from the weight R1 just wrote; the walk above then runs on the
normalised weights, and R2 turns each layer's gradient G into weight_orig's, (sigma / cur_sigma) (G - (sum(G W) / cur_sigma) C).  The
implicit backward reads J_D at the weights the last call f0 = f(z0) left in the modules, as the reference's hook does.
"""
import functools
import typing

import torch
import torch.nn.functional as F

from . import _hip
from .layers import conv_bn_stack, conv_stack, folded

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


_FFDNET_COLOUR = "FFDNet with 3 channels (the HIP kernels cover the grayscale network only)"


def _structure_refusal(stack, ffdnet):
    """What the kernels cover, stated once for eligibility, bn_stack (so param_eligibility and grad_parameters) and ffdnet_plan: None, or
    why the layers `stack` = [(conv or its weight, what sits behind it - a BatchNorm2d or its folded bias - or None, relu)] are not
    1 -> 64 -> ... -> 64 -> 1 (ffdnet: 5 -> 64 -> ... -> 64 -> 4) with a ReLU behind every layer but the last and nothing else behind the
    two edge layers."""
    shapes = [tuple(getattr(c, "weight", c).shape) for c, _, _ in stack]
    first, last = ((64, 5, 3, 3), (4, 64, 3, 3)) if ffdnet else ((64, 1, 3, 3), (1, 64, 3, 3))
    if len(shapes) < 2 or shapes[0] != first or shapes[-1] != last or any(s != (64, 64, 3, 3) for s in shapes[1:-1]):
        return f"layer shapes {shapes}: the kernels cover {first[1]} -> 64 -> ... -> 64 -> {last[0]}"
    if not all(r for _, _, r in stack[:-1]) or stack[-1][2]:
        return "ReLU pattern other than after every layer but the last"
    if stack[0][1] is not None or stack[-1][1] is not None:
        return "BatchNorm2d behind the first or the last layer (the edge kernels have no scale)"
    return None


def _plugin_refusal(net, what):
    """Why `net` is no 'denoiser' plugin made of a module sequence .dncnn, or None."""
    if getattr(net, "tag", None) != "denoiser":
        return f"nonlinear_op tag {getattr(net, 'tag', None)!r}: only 'denoiser' and 'ffdnet' plugins have {what}"
    if not isinstance(net, _modules()[0]):
        return f"not a conv [+BN] + ReLU stack: {type(net).__name__}"
    return None


def eligibility(net, train_realsn=False):
    """(ok, reason): whether DenoiserVJP (and DEQFixedPoint.implicit_backward = "device") can differentiate through `net`.  train_realsn=True
    (implicit_backward = "device+realsn"): all of that, and a net with a train-mode RealSNConv2d that realsn_stack accepts - such a net is
    answered by realsn_stack's verdict.  CPU-safe."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if train_realsn:
        ok, why = eligibility(net)
        if ok or not (isinstance(net, torch.nn.Module) and any(isinstance(m, RealSNConv2d) and m.training for m in net.modules())):
            return ok, why
        return GRAD_MODE["train_realsn"].eligibility(net)
    if isinstance(net, FFDNet):
        if net.num_input_channels != 1:
            return False, _FFDNET_COLOUR
        if any(isinstance(m, torch.nn.BatchNorm2d) and m.training for m in net.modules()):
            return False, "FFDNet with BatchNorm2d in train mode"
        return True, _FFDNET_OK
    why = _plugin_refusal(net, "a device VJP")
    layers, why = (None, why) if why else host_plan(net)
    why = _structure_refusal(layers, False) if layers is not None else why
    return (True, "conv [+BN-eval] + ReLU stack") if why is None else (False, why)


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


# ----------------------------------------------------------------------------- the weight gradients: one walk, a layer rule per mode
# A layer rule is what one convolution of the stack is on the host, in its weight W's dtype: .forward(h) -> (y in front of the ReLU, what
# the way back needs of it), .backward(input, kept, gm) -> ([the gradients of the layer's parameters], the gradient behind the convolution)
# for gm the gradient masked by the layer's ReLU, and .down, the weight whose transpose carries that gradient to the layer below.
# A mode's rule (GradMode.host_rule) is made from the layer, Rule(conv, bn, like, update, who); a Conv2d without a BatchNorm is a _PlainRule.
class _PlainRule:
    """y = conv(x, W) [+ bias]:  dW = wgrad(x, gm), gm goes down through W^T."""

    def __init__(self, W, bias=None):
        self.W, self.bias, self.down = W, bias, W

    def forward(self, h):
        return F.conv2d(h, self.W, self.bias, padding=1), None

    def backward(self, inp, kept, gm):
        return [torch.nn.grad.conv2d_weight(inp, self.W.shape, gm, padding=1)], gm


class _FrozenRule:
    """y = s conv(x, W) + t of an eval-mode BatchNorm:  R = wgrad(x, gm), dW = s R, dgamma = (sum W R - mean dbeta) / sqrt(var + eps),
    dbeta = sum gm; gm goes down through (s W)^T."""

    def __init__(self, conv, bn, like, update=False, who=None):
        self.W = W = conv.weight.detach().to(like)
        self.s, self.mean, self.inv = _bn_scale(bn, W)
        self.shift, self.down = bn.bias.detach().to(W) - self.mean * self.s, W * self.s.view(-1, 1, 1, 1)

    def forward(self, h):
        return F.conv2d(h, self.W, padding=1) * self.s.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1), None

    def backward(self, inp, kept, gm):
        R = torch.nn.grad.conv2d_weight(inp, self.W.shape, gm, padding=1)
        dbeta = gm.sum((0, 2, 3))
        return [self.s.view(-1, 1, 1, 1) * R, ((self.W * R).sum((1, 2, 3)) - self.mean * dbeta) * self.inv, dbeta], gm


class _TrainRule:
    """y = gamma xhat + beta of a train-mode BatchNorm, xhat = (c - mean) / sqrt(var + eps) by the batch's statistics of c = conv(x, W):
    dbeta = sum gm, dgamma = sum gm xhat, dc = gamma / sqrt(var + eps) (gm - dbeta / P - xhat dgamma / P), dW = wgrad(x, dc); dc goes down
    through W^T.  update: the forward moves the module's running buffers as torch does."""

    def __init__(self, conv, bn, like, update, who):
        self.W = self.down = W = conv.weight.detach().to(like)
        self.bn, self.update, self.who = bn, update, who
        self.gamma, self.beta = bn.weight.detach().to(W), bn.bias.detach().to(W)

    def forward(self, h):
        c, bn = F.conv2d(h, self.W, padding=1), self.bn
        P = c.numel() // c.shape[1]
        if P < 2:
            raise ValueError(f"{self.who}: expected more than 1 value per channel when training, got input size {list(c.shape)}")
        mean, var = c.mean((0, 2, 3)), c.var((0, 2, 3), unbiased=False)
        inv = 1.0 / torch.sqrt(var + bn.eps)
        xhat = (c - mean.view(1, -1, 1, 1)) * inv.view(1, -1, 1, 1)
        if self.update:
            with torch.no_grad():
                m = bn.momentum
                bn.running_mean.copy_((1.0 - m) * bn.running_mean.to(mean) + m * mean)
                bn.running_var.copy_((1.0 - m) * bn.running_var.to(var) + m * (var * (P / (P - 1))))
                bn.num_batches_tracked += 1
        return xhat * self.gamma.view(1, -1, 1, 1) + self.beta.view(1, -1, 1, 1), (xhat, inv, P)

    def backward(self, inp, kept, gm):
        xhat, inv, P = kept
        dbeta, dgamma = gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))
        dc = (self.gamma * inv).view(1, -1, 1, 1) * (gm - (dbeta / P).view(1, -1, 1, 1) - xhat * (dgamma / P).view(1, -1, 1, 1))
        return [torch.nn.grad.conv2d_weight(inp, self.W.shape, dc, padding=1), dgamma, dbeta], dc


class _RealSNRule(_PlainRule):
    """A RealSNConv2d in train mode: one realsn.power_iteration from the module's weight_u (weight = weight_orig / cur_sigma * sigma; u, v constants)
    in front of _PlainRule on that weight, realsn.weight_grad turning its G into weight_orig's behind it.  update: the module gets the new weight_u and weight."""

    def __init__(self, conv, bn, like, update, who=None):
        from . import realsn
        W = conv.weight_orig.detach()
        weight, u, v, cur_sigma = realsn.power_iteration(W, conv.weight_u, conv.sigma, conv.n_power_iterations, conv.eps)
        if update:
            with torch.no_grad():
                conv.weight_u.copy_(u)
                conv.weight.copy_(weight)
        super().__init__(weight.to(like))
        self.grad_of, self.step = realsn.weight_grad, (W, u, v, cur_sigma, conv.sigma)

    def backward(self, inp, kept, gm):
        (G,), g = super().backward(inp, kept, gm)
        return [self.grad_of(G.to(self.step[0]), *self.step).to(G)], g


def _first_input(who, edges, x, sigma):
    """What the first layer reads of the image x: x itself, or FFDNet's pixel-unshuffle of it behind the noise-level map."""
    if edges is PLAIN_EDGES:
        return x
    _even(x, who)
    if sigma is None:
        raise ValueError(f"{who}: FFDNet is evaluated at a noise level: sigma is required")
    return torch.cat((_sigma_map(sigma, x), edges[0](x)), 1)


def _taped_forward(rules, relus, h, masks=None):
    """The forward that keeps the tape: every layer but the last on the first layer's input h.  -> (tape, masks): tape[i] = (layer i's
    input, what its rule kept), masks[i] the ReLU decision behind layer i - those handed in, else the ones at h - or None without a ReLU."""
    tape, used = [], []
    for i, (rule, relu) in enumerate(zip(rules[:-1], relus)):
        y, kept = rule.forward(h)
        m = (masks[i] if masks is not None else y > 0) if relu else None
        tape.append((h, kept))
        used.append(m)
        h = y if m is None else y * m
    return tape + [(h, None)], used


def _walk_back(rules, tape, used, v, edges, want_input=False):
    """The walk back from the gradient v of the stack's output: each rule forms its layer's gradients, and what it hands down goes through
    the transposed weight and the ReLU mask of the layer below.  -> (the gradients layer by layer in one list, J^T v or None)."""
    read, cin, write = edges
    per_layer, g = [None] * len(rules), read(v)
    for i in range(len(rules) - 1, -1, -1):
        per_layer[i], g = rules[i].backward(*tape[i], g)
        if i > 0:
            g = F.conv2d(g, _transposed(rules[i].down), padding=1)
            if used[i - 1] is not None:
                g = g * used[i - 1]
    gx = write(F.conv2d(g, _transposed(rules[0].down[:, cin]), padding=1)) if want_input else None
    return [t for layer in per_layer for t in layer], gx


def plan_param_grads(layers, x, v, masks=None):
    """(dD/dtheta)^T v of the stack `layers` at x, one tensor per conv weight, in x's dtype - the host statement of what
    DenoiserParamGrads.grads runs, next to plan_vjp: the taped forward keeps each layer's input, the layers are walked backwards with
    masked_vjp's steps, and dW_i comes from layer i's input and the masked gradient behind it.  masks: those of another forward pass (the
    device's, unpack_masks) in place of the decisions at x.  Returns ([dW_0 .. dW_{k-1}], masks)."""
    rules = [_PlainRule(w.to(x), None if b is None else b.to(x)) for w, b, _ in layers]
    tape, used = _taped_forward(rules, [relu for _, _, relu in layers], x, masks)
    return _walk_back(rules, tape, used, v, PLAIN_EDGES)[0], used


class _Refusal(str):
    """Why a mode refuses a net, with .other the name of the mode the net belongs to instead, or None (EquilibriumProxGradSCI._param_mode)."""

    def __new__(cls, text, other=None):
        self = super().__new__(cls, text)
        self.other = other
        return self


def _bn_refusal(mods):
    """Why a BatchNorm2d of `mods` is not a fixed affine map with parameters of its own, or None."""
    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            if not m.track_running_stats or m.running_mean is None or m.running_var is None:
                return _Refusal("BatchNorm2d without running statistics (track_running_stats=False: it normalises by the batch's)",
                                "train_bn" if m.training else None)
            if m.training:
                return _Refusal("BatchNorm2d in train mode (batch statistics have no device kernel)", "train_bn")
            if not m.affine or m.weight is None or m.bias is None:
                return "BatchNorm2d without affine parameters (affine=False)"
    return None


def _train_bn_refusal(mods):
    """Why a BatchNorm2d of `mods` is not a train-mode BatchNorm the batch-statistics kernels serve, or None."""
    for m in mods:
        if isinstance(m, torch.nn.BatchNorm2d):
            if not m.training:
                return _Refusal('BatchNorm2d in eval mode (frozen statistics: that is parameter_backward = "device+bn")', "frozen_bn")
            if not m.affine or m.weight is None or m.bias is None:
                return "BatchNorm2d without affine parameters (affine=False)"
            if not m.track_running_stats or m.running_mean is None or m.running_var is None or m.num_batches_tracked is None:
                return "BatchNorm2d without running statistics (track_running_stats=False: the kernels update them)"
            if m.momentum is None:
                return "BatchNorm2d with momentum=None (the cumulative moving average has no device kernel)"
            if isinstance(m.momentum, bool) or not isinstance(m.momentum, float):
                return f"BatchNorm2d with momentum={m.momentum!r}: a float is required"
    return None


def _no_bn_refusal(mods):
    if any(isinstance(m, torch.nn.BatchNorm2d) for m in mods):
        return _Refusal("BatchNorm2d (its gamma / beta gradients, and the batch statistics in train mode, have no device kernel)", "frozen_bn")
    return None


def _bn_stack(net, bn_refusal, batch_stats=False, ffdnet_too=True):
    """bn_stack for one mode: what it asks of the BatchNorms, whether they normalise by the batch, whether FFDNet is served."""
    DnCNN, FFDNet, RealSNConv2d = _modules()
    ffdnet = isinstance(net, FFDNet)
    if ffdnet and not ffdnet_too:
        return None, None, _Refusal("FFDNet: its 5 -> 64 / 64 -> 4 edge layers and BatchNorm2d parameters have no device weight gradient", "frozen_bn")
    why = (_FFDNET_COLOUR if net.num_input_channels != 1 else None) if ffdnet else _plugin_refusal(net, "device weight gradients")
    if why is not None:
        return None, None, why
    mods = list(net.intermediate_dncnn.itermediate_dncnn if ffdnet else net.dncnn)
    if any(isinstance(m, RealSNConv2d) for m in mods):
        return None, None, _Refusal("RealSNConv2d (its parameter is weight_orig behind the spectral normalisation)", "train_realsn")
    why = bn_refusal(mods)
    if why is not None:
        return None, None, _Refusal(("FFDNet: " if ffdnet else "") + why, getattr(why, "other", None))
    stack, why = conv_bn_stack(mods, train_bn=batch_stats)
    why = _structure_refusal(stack, ffdnet) if stack is not None else why
    if why is None and not all(isinstance(c.weight, torch.nn.Parameter) for c, _, _ in stack):
        why = "a conv weight that is not an nn.Parameter"
    return (stack, ffdnet, None) if why is None else (None, None, why)


def bn_stack(net, train):
    """(stack, ffdnet, reason): layers.conv_bn_stack of a net the device weight gradients serve - [(conv, bn or None, relu)] and whether its
    edge layers are FFDNet's - or (None, None, why not).  train: the stack of the mode frozen_bn (False: every BatchNorm in eval mode), train_bn
    (True) or plain (None: no BatchNorm, no FFDNet).  Refused in this order: tag and type, RealSN, the BatchNorms' state, conv_bn_stack's, the shape."""
    return GRAD_MODE[{None: "plain", False: "frozen_bn", True: "train_bn"}[train]].stack(net)


_REALSN_OK = "train-mode RealSN conv + ReLU stack"


def realsn_stack(net):
    """(stack, reason): the layers [(conv, None, relu)] of a net whose TRAIN-mode f-call, implicit backward and weight gradients run on the
    device with the spectral normalisation in it (engine train_realsn="device", implicit_backward / parameter_backward = "device+realsn") -
    or (None, why not).  A DnCNN plugin in train mode; every convolution a RealSNConv2d (its parameter is weight_orig, renormalised by one
    power step per call: csrc/realsn.hip) or a plain bias-free Conv2d; no BatchNorm; 1 -> 64 -> ... -> 64 -> 1 with a ReLU behind every
    layer but the last; fp32.  Decided here and nowhere else.  CPU-safe."""
    from .layers import _conv_ok
    DnCNN, FFDNet, RealSNConv2d = _modules()
    if isinstance(net, FFDNet):
        return None, "FFDNet: it has no spectrally normalised convolution, and its BatchNorm2d layers belong to train_bn"
    why = _plugin_refusal(net, "a train-mode RealSN device path")
    if why is not None:
        return None, why
    if not net.training:
        return None, "the net is in eval mode (a RealSNConv2d uses its stored weight there: the plain device paths serve it)"
    mods, stack, i = list(net.dncnn), [], 0
    if any(isinstance(m, torch.nn.BatchNorm2d) for m in mods):
        return None, "BatchNorm2d next to RealSNConv2d (RealSN_DnCNN: the spectral normalisation of a BatchNorm has no device kernel)"
    while i < len(mods):
        conv = mods[i]
        if isinstance(conv, RealSNConv2d):
            u = conv.weight_u
            if int(conv.n_power_iterations) < 1:
                return None, f"RealSNConv2d with n_power_iterations = {conv.n_power_iterations}"
            if u.dim() != 4 or u.shape[0] != 1 or u.shape[1] != conv.weight_orig.shape[0] or u.shape[2] * u.shape[3] > (1 << 20):
                return None, f"RealSNConv2d whose weight_u {tuple(u.shape)} is not a (1, C_out, h, w) map of at most 2^20 pixels"
            if not isinstance(conv.weight_orig, torch.nn.Parameter):
                return None, "a weight_orig that is not an nn.Parameter"
        elif isinstance(conv, torch.nn.Conv2d):
            if not _conv_ok(conv):
                return None, "Conv2d other than 3x3, stride 1, padding 1"
            if conv.bias is not None:
                return None, "Conv2d with a bias"
            if not isinstance(conv.weight, torch.nn.Parameter):
                return None, "a conv weight that is not an nn.Parameter"
        else:
            return None, f"unknown module {type(conv).__name__} where a convolution was expected"
        i += 1
        relu = i < len(mods) and isinstance(mods[i], torch.nn.ReLU)
        if relu:
            i += 1
        elif i < len(mods) and not isinstance(mods[i], (torch.nn.Conv2d, RealSNConv2d)):
            return None, f"unknown module {type(mods[i]).__name__}"
        stack.append((conv, None, relu))
    why = _structure_refusal(stack, False)
    if why is None and not all(t.dtype == torch.float32 for t in list(net.parameters()) + list(net.buffers()) if t.is_floating_point()):
        why = "parameters or buffers that are not fp32"
    return (stack, None) if why is None else (None, why)


def _realsn_mode_stack(net):                                    # (realsn_stack as a mode's stack function answers)
    stack, why = realsn_stack(net)
    return (None, None, why) if stack is None else (stack, False, None)


def conv_weights(net):
    """The conv weights of a net param_eligibility accepts, in layer order: the parameters DenoiserParamGrads.grads answers for."""
    return [m.weight for m in net.dncnn if isinstance(m, torch.nn.Conv2d)]


class GradMode(typing.NamedTuple):
    """One way to form the denoiser's weight gradients on the device: what differs between the ways, and nothing else (the module's docstring)."""
    name: str                       # the public keyword that asks for it ("plain": none)
    switch: str                     # the DEQFixedPoint.parameter_backward string that asks for it
    serves: tuple                   # the names of the modes that switch serves, in the order tried
    engine_option: typing.Any       # (DEQSCIEngine keyword, value) that moves the solve's train-mode f-calls to the device, or None
    stack: typing.Callable          # net -> (stack [(conv, bn or None, relu)], ffdnet, None) of a net the mode serves, or (None, None, why not)
    accepted: tuple                 # eligibility's reason for a net it serves: (a DnCNN plugin, FFDNet)
    host_rule: type                 # the host rule of a layer that is more than a plain convolution
    device_rule: type               # the device rule of a 64 -> 64 layer with a BatchNorm (Rule.build: DenoiserParamGrads' _MaskedStack)

    def eligibility(self, net):
        """(ok, reason): whether the mode serves `net`."""
        stack, ffdnet, why = self.stack(net)
        return (False, why) if stack is None else (True, self.accepted[bool(ffdnet)])

    def parameters(self, net):
        """The nn.Parameters of a net the mode serves that .grads answers for, in its order: per layer the conv weight - a RealSNConv2d's
        weight_orig - then its BatchNorm's weight (gamma) and bias (beta)."""
        stack, _, why = self.stack(net)
        if stack is None:
            raise ValueError(f"grad_parameters: {why}")
        RealSNConv2d = _modules()[2]
        return [p for conv, bn, _ in stack
                for p in [conv.weight_orig if isinstance(conv, RealSNConv2d) else conv.weight] + ([] if bn is None else [bn.weight, bn.bias])]


def grad_mode(who, frozen_bn=False, train_bn=False, train_realsn=False):
    """The GradMode the three public keywords ask for; who: the entry point, for the error."""
    if train_realsn and (frozen_bn or train_bn):
        raise ValueError(f"{who}: train_realsn excludes frozen_bn and train_bn")
    if train_bn and frozen_bn:
        raise ValueError(f"{who}: frozen_bn and train_bn exclude one another")
    asked = {"frozen_bn": frozen_bn, "train_bn": train_bn, "train_realsn": train_realsn}
    return next((m for m in GRAD_MODES if asked.get(m.name)), GRAD_MODE["plain"])


def switch_modes(parameter_backward):
    """The GradModes a DEQFixedPoint.parameter_backward string serves, in the order tried - or None for a string that is no mode's switch."""
    return next((tuple(GRAD_MODE[name] for name in m.serves) for m in GRAD_MODES if m.switch == parameter_backward), None)


def param_eligibility(net, frozen_bn=False, train_bn=False, train_realsn=False):
    """(ok, reason): whether DenoiserParamGrads can form the weight gradients of `net` in the mode the keywords name (GRAD_MODES; the
    module's docstring says what each serves).  No keyword: a bias-free conv + ReLU stack 1 -> 64 -> ... -> 64 -> 1 whose conv weights are
    nn.Parameters - SimpleCNN, DnCNN(..., lip=0.0, no_bn=True) of any depth >= 2.  frozen_bn / train_bn: in addition an affine BatchNorm2d
    with running statistics behind every 64 -> 64 conv, in eval / in TRAIN mode (a float momentum; an eval-mode BatchNorm is refused), and
    the grayscale FFDNet: bn_stack decides.  train_realsn: a DnCNN in TRAIN mode whose convolutions are RealSNConv2d or plain bias-free
    Conv2d, without BatchNorm: realsn_stack decides.  CPU-safe."""
    return grad_mode("param_eligibility", frozen_bn, train_bn, train_realsn).eligibility(net)


def grad_parameters(net, train_bn=False, train_realsn=False):
    """The nn.Parameters DenoiserParamGrads.grads answers for, in its order, for a net the mode accepts - frozen_bn without a keyword: per
    layer the conv weight (a RealSNConv2d's weight_orig), then its BatchNorm's weight (gamma) and bias (beta)."""
    return grad_mode("grad_parameters", not (train_bn or train_realsn), train_bn and not train_realsn, train_realsn).parameters(net)


def _bn_scale(bn, like):
    """(s, mean, 1 / sqrt(var + eps)) of a frozen BatchNorm in like's dtype and device."""
    T = lambda p: p.detach().to(like)
    inv = 1.0 / torch.sqrt(T(bn.running_var) + bn.eps)
    return T(bn.weight) * inv, T(bn.running_mean), inv


def _net_rules(who, net, mode, like, update=False):
    """mode.stack(net) as the host walk takes it, in like's dtype: (one rule per layer, the ReLU flags, the edges, ffdnet)."""
    stack, ffdnet, why = mode.stack(net)
    if stack is None:
        raise ValueError(f"{who}: {why}")
    rules = [_PlainRule(conv.weight.detach().to(like)) if bn is None and isinstance(conv, torch.nn.Conv2d) else mode.host_rule(conv, bn, like, update, who)
             for conv, bn, _ in stack]
    return rules, [relu for _, _, relu in stack], FFDNET_EDGES if ffdnet else PLAIN_EDGES, ffdnet


def _net_param_grads(who, net, mode, x, v, sigma, masks, want_input=False, update=False):
    """The host walk of a net: -> (gradients in mode.parameters' order, masks, J_D(x)^T v or None)."""
    rules, relus, edges, ffdnet = _net_rules(who, net, mode, x, update)
    tape, used = _taped_forward(rules, relus, _first_input(who, edges, x, sigma), masks)
    grads, gx = _walk_back(rules, tape, used, v, edges, want_input and not ffdnet)          # (FFDNet detaches its input)
    return grads, used, gx


def plan_param_grads_frozen_bn(net, x, v, sigma=None, masks=None):
    """(dD/dtheta)^T v of a net param_eligibility(net, frozen_bn=True) accepts, at x, in x's dtype - the host statement of what
    DenoiserParamGrads(..., frozen_bn=True).grads runs: plan_param_grads' walk with _FrozenRule where a layer has a BatchNorm.  FFDNet goes
    through FFDNET_EDGES at the noise level sigma (1 or n values; sigma's channel of the first weight included) and differentiates nothing
    through its input.  masks: those of another forward pass (the device's, unpack_masks).  Returns (gradients in grad_parameters order, masks)."""
    return _net_param_grads("plan_param_grads_frozen_bn", net, GRAD_MODE["frozen_bn"], x, v, sigma, masks)[:2]


def plan_forward_train_bn(net, x, sigma=None, update=True):
    """One train-mode forward of a net param_eligibility(net, train_bn=True) accepts, restated in x's dtype: per BatchNorm layer the mean and
    the biased variance of c = conv(x, W) over the batch, y = gamma (c - mean) / sqrt(var + eps) + beta, the ReLU; FFDNet at the noise level
    sigma through its pixel-(un)shuffle.  update=True moves the module's buffers as torch does: running_mean <- (1 - m) running_mean + m mean,
    running_var <- (1 - m) running_var + m var P / (P - 1), num_batches_tracked += 1.  -> (noise, masks)."""
    rules, relus, edges, _ = _net_rules("plan_forward_train_bn", net, GRAD_MODE["train_bn"], x, update)
    tape, used = _taped_forward(rules, relus, _first_input("plan_forward_train_bn", edges, x, sigma))
    return edges[2](rules[-1].forward(tape[-1][0])[0]), used


def plan_param_grads_train_bn(net, x, v, sigma=None, masks=None, input_grad=False):
    """(dD/dtheta)^T v of a net param_eligibility(net, train_bn=True) accepts, at x, in x's dtype - the host statement of what
    DenoiserParamGrads(..., train_bn=True).grads runs: plan_param_grads' walk with _TrainRule where a layer has a BatchNorm - the
    forward is plan_forward_train_bn's with the buffers left alone, and dc goes down through the UNFOLDED transposed weight.  masks: those
    of another forward pass (the device's, unpack_masks).  Returns (gradients in grad_parameters(net, train_bn=True) order, masks) - with
    input_grad=True (gradients, masks, J_D(x)^T v: the true input product, statistic terms included; None for FFDNet, which detaches its
    input)."""
    out = _net_param_grads("plan_param_grads_train_bn", net, GRAD_MODE["train_bn"], x, v, sigma, masks, input_grad)
    return out if input_grad else out[:2]


def plan_param_grads_realsn(net, x, v, masks=None, input_grad=False, update=False):
    """(dD/dtheta)^T v of a net param_eligibility(net, train_realsn=True) accepts, at x, in x's dtype - the host statement of what
    DenoiserParamGrads(..., train_realsn=True).grads runs: plan_param_grads' walk with _RealSNRule where a layer is a RealSNConv2d; a plain
    Conv2d's G_i is its gradient.  update=True writes the new weight_u and weight into the module as its own forward would; otherwise the
    module is left alone.  masks: those of another forward pass.  Returns (gradients in grad_parameters(net, train_realsn=True) order,
    masks) - with input_grad=True (gradients, masks, J_D(x)^T v)."""
    with torch.no_grad():
        out = _net_param_grads("plan_param_grads_realsn", net, GRAD_MODE["train_realsn"], x, v, None, masks, input_grad, update)
    return out if input_grad else out[:2]


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
    why = _structure_refusal(layers, True) if layers is not None else why
    if why is not None:
        raise ValueError(f"ffdnet_plan: {why}")
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
    of layer i + 1, (k-1) n 64 H W 4 bytes in all) and run the last layer on the last of them (.noise) - what the weight gradients are
    formed from (DenoiserParamGrads).  It is the forward of every BatchNorm mode: rules are the 64 -> 64 layers as device rules (below) in
    place of _Conv64 of `layers`' own.  through_input=False (FFDNet under DenoiserParamGrads: its input is detached, nothing is carried
    through the first layer) builds no head_f / head_t."""

    def __init__(self, layers, x, sigma=None, keep=False, rules=None, through_input=True, edges=None):
        x = _hip.f32c(x.detach())
        f32 = lambda t: t.to(x.device, torch.float32)
        self.ffdnet = sigma is not None
        pack_in, pack_out, self._first, self._last = _FFDNET_KERNELS if self.ffdnet else _PLAIN_KERNELS
        with torch.no_grad():
            if edges is not None:           # (a plain stack whose packs csrc/realsn.hip's R3 made on the device: layers is not read)
                self.head_f, self.head_t, self.tail_f, self.tail_t = edges
                w0 = None
            else:
                w0, wt = f32(layers[0][0]), f32(layers[-1][0])
                win = w0[:, 1:5] if self.ffdnet else w0                 # (FFDNet's channel 0 is sigma's: it carries no tangent)
                self.head_f, self.head_t = (pack_in(win.contiguous()), pack_out(_transposed(win))) if through_input else (None, None)
                self.tail_f, self.tail_t = pack_out(wt), pack_in(_transposed(wt))
            self.rules = [_Conv64(f32(w), b) for w, b, _ in layers[1:-1]] if rules is None else rules
            h = _hip.ffdnet_head(x, _hip.pack_head_weights(w0), sigma) if self.ffdnet else _hip.conv3x3_c1_to_64(x, self.head_f, relu=True)
            self.masks = [_hip.relu_mask_pack(h)]
            self.acts = [h] if keep else None
            for rule in self.rules:
                h, mask = rule.forward(h)
                self.masks.append(mask)
                if keep:
                    self.acts.append(h)
            self.noise = self._last(h, self.tail_f) if keep else None
            for rule in self.rules:         # (the way back's BatchNorm state comes last: the host prepares it while the device runs the forward)
                rule.after_forward()
            self.mid_f, self.mid_t = [r.u for r in self.rules], [r.ut for r in self.rules]

    def jvp(self, v):
        t = self._first(_hip.f32c(v), self.head_f, self.masks[0])
        for i, u in enumerate(self.mid_f):
            t = _hip.conv3x3_c64_winograd_masked(t, u, self.masks[i + 1])
        return self._last(t, self.tail_f)

    def vjp(self, v):
        g = self._first(_hip.f32c(v), self.tail_t, self.masks[-1])
        for i in range(len(self.mid_t) - 1, -1, -1):           # layer i + 1 transposed, masked by the ReLU in front of it
            g = _hip.conv3x3_c64_winograd_masked(g, self.mid_t[i], self.masks[i])
        return self._last(g, self.head_t)


# The device kernels of a family's edge layers: (the pack of a k -> 64 weight, the pack of a 64 -> k weight, the masked k -> 64 kernel, the
# 64 -> k kernel), k = 1 or FFDNet's 4 channels of the 2x2 pixel-unshuffle.
_PLAIN_KERNELS = (_hip.pack_c1_to_64_weights, _hip.pack_c64_to_1_weights, _hip.conv3x3_c1_to_64_masked, _hip.conv3x3_c64_to_1)
_FFDNET_KERNELS = (_hip.pack_head_masked_weights, _hip.pack_tail_weights, _hip.ffdnet_head_masked, _hip.ffdnet_tail)


# A device rule is what one 64 -> 64 layer of _MaskedStack is: .u / .ut its weight and its transposed weight - the one the gradient goes
# down through - as Winograd packs, .count its parameters, .forward(h) -> (the post-ReLU activation, its mask words), .after_forward(),
# which makes what only the way back needs - no pack: a pack copies from the host, and the stream would wait - behind the whole forward, and
# .backward(input, g, need) -> ([one gradient or None per parameter], the gradient behind the convolution) for g the gradient masked by the
# layer's ReLU and need one bool per parameter.  .ws: the scratch buffer of the rule's weight-gradient kernel, which its owner assigns.
# GradMode.device_rule is the rule of a layer with a BatchNorm, Rule(w, bias, conv, bn, ws_bn) - one without is a _Conv64 - and Rule.build(stack, x,
# sigma) -> (the _MaskedStack that keeps its activations, the edge layers' realsn steps, R1 / R2's workspace) builds DenoiserParamGrads in every mode.
class _Conv64:
    """conv [+ folded bias] + ReLU: Winograd F(2x2,3x3) with the bias and the ReLU, relu_mask_pack; W0 if the weight is asked for."""
    count, bn_workspace, batch_stats = 1, False, False

    def __init__(self, w, bias=None, conv=None, bn=None, ws_bn=None):
        self.u, self.ut, self.ws = _hip.pack_winograd_weights(w), _hip.pack_winograd_weights(_transposed(w)), None
        self.bias = None if bias is None else bias.to(w.device, torch.float32).contiguous()

    @classmethod
    def build(cls, stack, x, sigma):
        ffdnet = sigma is not None
        P = x.shape[0] * x.shape[2] * x.shape[3] // (4 if ffdnet else 1)             # pixels per channel at the 64 -> 64 layers
        if cls.batch_stats and P < 2:
            raise ValueError(f"DenoiserParamGrads: expected more than 1 value per channel when training, got {P}")
        ws_bn = _hip.bn_train_workspace(P, x.device) if cls.batch_stats and any(bn is not None for _, bn, _ in stack[1:-1]) else None
        layers = [(conv.weight.detach(), None, relu) for conv, _, relu in stack] if cls.batch_stats else folded(stack)
        f32 = lambda t: t.to(x.device, torch.float32)
        with torch.no_grad():
            rules = [(_Conv64 if bn is None else cls)(f32(w), b, conv, bn, ws_bn) for (conv, bn, _), (w, b, _) in zip(stack[1:-1], layers[1:-1])]
        return _MaskedStack(layers, x, sigma, keep=True, rules=rules, through_input=not ffdnet), None, None

    def forward(self, h):
        h = _hip.conv3x3_c64_winograd(h, self.u, self.bias, True)
        return h, _hip.relu_mask_pack(h)

    def after_forward(self):
        pass

    def backward(self, inp, g, need):
        return [_hip.wgrad_c64_c64(inp, g, self.ws) if need[0] else None], g

    def release(self):
        pass


class _Frozen64(_Conv64):
    """The same forward and transposed pack with the eval-mode BatchNorm folded in (w = s W, bias = t); W0-BN and the float64 dgamma line
    if any of W, gamma, beta is asked for.  W, s fp32 and mean, 1 / sqrt(var + eps) float64 are the unfolded layer's."""
    count, bn_workspace = 3, True

    def __init__(self, w, bias, conv, bn, ws_bn=None):
        super().__init__(w, bias)
        self.conv, self.bn = conv, bn

    def after_forward(self):
        dev = lambda t, dt=torch.float32: t.detach().to(self.u.device, dt).contiguous()
        self.inv = 1.0 / torch.sqrt(dev(self.bn.running_var, torch.float64) + self.bn.eps)
        self.s, self.mean = (dev(self.bn.weight, torch.float64) * self.inv).float(), dev(self.bn.running_mean, torch.float64)
        self.W = dev(self.conv.weight)

    def backward(self, inp, g, need):
        if not any(need):
            return [None] * 3, g
        dw, dsum, ddot = _hip.wgrad_c64_c64_bn(inp, g, self.W, self.s, self.ws)
        return [dw, ((ddot.double() - self.mean * dsum.double()) * self.inv).float(), dsum], g


class _Train64(_Conv64):
    """Train-mode BatchNorm: the raw Winograd convolution c, T1 (batch statistics; the module's running buffers move, once), T2 (normalise +
    ReLU + the mask words); c is kept.  Back: T3 (dgamma, dbeta), T4 (dc, in place), W0 on dc if the weight is asked for; dc goes down
    through the UNFOLDED transposed weight.  ws_bn: bn_train_workspace's buffer."""
    count, batch_stats = 3, True

    def __init__(self, w, bias, conv, bn, ws_bn):
        super().__init__(w)
        self.bn, self.ws_bn, self.eps = bn, ws_bn, float(bn.eps)
        self.gamma = bn.weight.detach().to(w.device, torch.float32).contiguous()

    def forward(self, h):
        bn = self.bn
        self.c = _hip.conv3x3_c64_winograd(h, self.u, None, False)
        self.rec = _hip.bn_train_stats(self.c, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, workspace=self.ws_bn)
        return _hip.bn_train_apply(self.c, self.rec, self.gamma, bn.bias.detach().to(self.gamma).contiguous(), self.eps, relu=True, want_mask=True)

    def backward(self, inp, g, need):
        if self.c is None:
            raise RuntimeError(_RELEASED)
        dgamma, dbeta, grec = _hip.bn_train_grad_stats(g, self.c, self.rec, self.eps, self.ws_bn)
        g = _hip.bn_train_grad_apply(g, self.c, self.rec, grec, self.gamma, self.eps, out=g)         # dc, statistic terms included, in place
        return [_hip.wgrad_c64_c64(inp, g, self.ws) if need[0] else None, dgamma, dbeta], g

    def release(self):
        self.c = None


class _RealSN64(_Conv64):
    """A 64 -> 64 layer of a realsn_stack: its two F(2x2,3x3) packs come from csrc/realsn.hip's R3 on the device (no host packer: the weight
    changes at every call); step = (W, u, v, record, sigma) of the power step that made the weight - W0's G is then the gradient of the
    NORMALISED weight and R2 turns it into weight_orig's - or None for a plain Conv2d, whose G is its gradient.  rws: R1 / R2's workspace."""

    def __init__(self, u, ut, step, rws):
        self.u, self.ut, self.ws, self.bias, self.step, self.rws = u, ut, None, None, step, rws

    @classmethod
    def build(cls, stack, x, sigma):
        return _realsn_device_stack(stack, x, True, True)

    def backward(self, inp, g, need):
        if not need[0]:
            return [None], g
        G = _hip.wgrad_c64_c64(inp, g, self.ws)
        return [G if self.step is None else _realsn_grad(G, self.step, self.rws)], g


def _realsn_grad(G, step, rws):
    W, u, v, record, sigma = step
    return _hip.realsn_grad(G, W, u, v, record, sigma, workspace=rws)


def realsn_power_in_place(conv, workspace=None, v=None, record=None):
    """One train-mode call's power step of a RealSNConv2d on the device, R1 writing weight_u and weight IN PLACE into the module's own
    buffers (the kernels of the module's own forward: the same bits).  -> (W = weight_orig as R1 read it, weight, u, v, record)."""
    W, u, weight = _hip.f32c(conv.weight_orig.detach()), conv.weight_u, conv.weight
    if not (u.is_contiguous() and weight.is_contiguous() and u.dtype == weight.dtype == torch.float32):
        raise _hip.DeqsciHipError("RealSNConv2d: weight_u and weight must be contiguous fp32 buffers to be updated in place")
    weight, u, v, record = _hip.realsn_power(W, u, conv.n_power_iterations, conv.sigma, conv.eps, workspace=workspace, weight=weight, v=v, record=record)
    return W, weight, u, v, record


def _realsn_workspace(stack, device):
    """One workspace for R1 / R2 of every RealSNConv2d of the stack (the largest asked for), or None without one."""
    RealSNConv2d = _modules()[2]
    sizes = [_hip.load().deqsci_realsn_workspace_bytes(c.weight_orig.shape[1], c.weight_orig.shape[0], c.weight_u.shape[2], c.weight_u.shape[3])
             for c, _, _ in stack if isinstance(c, RealSNConv2d)]
    if not sizes:
        return None
    if min(sizes) == 0:
        raise _hip.DeqsciHipError("realsn: a RealSNConv2d whose sizes the kernels refuse")
    return _hip._partials(max(sizes), device)


def _realsn_device_stack(stack, x, keep, step):
    """_MaskedStack of a realsn_stack at x with every pack made by R3.  step=True: each RealSNConv2d first takes its power step (R1, in
    place in the module) and the steps are kept for the way back; False: the `weight` buffers are packed as they stand (what the last
    call left behind).  -> (the _MaskedStack, [per layer (W, u, v, record, sigma) or None], R1 / R2's workspace or None)."""
    RealSNConv2d = _modules()[2]
    dev = x.device
    rws = _realsn_workspace(stack, dev) if step else None
    steps, packs = [], []
    with torch.no_grad():
        for conv, _, _ in stack:
            if isinstance(conv, RealSNConv2d):
                if step:
                    W, weight, u, v, record = realsn_power_in_place(conv, rws)
                    steps.append((W, u.clone(), v, record, float(conv.sigma)))      # (weight_u moves again with the next call)
                else:
                    weight = conv.weight
                    steps.append(None)
            else:
                weight = conv.weight.detach()
                steps.append(None)
            weight = _hip.f32c(weight)
            if weight.device != dev:
                raise _hip.DeqsciHipError(f"realsn: the net's weights are on {weight.device}, the image on {dev}")
            cout, cin = weight.shape[:2]
            pack, _, pack_t = _hip.realsn_pack(weight, *_hip.realsn_pack_buffers(cin, cout, dev, pack44=False))
            packs.append((pack, pack_t))
    rules = [_RealSN64(p, pt, st, rws) for (p, pt), st in zip(packs[1:-1], steps[1:-1])]
    edges = (packs[0][0], packs[0][1], packs[-1][0], packs[-1][1])
    return _MaskedStack(None, x, keep=keep, rules=rules, edges=edges), steps, rws


# ----------------------------------------------------------------------------- the modes, stated once, in the order configure_training tries them
GRAD_MODES = (
    GradMode("plain", "device", ("plain",), None, functools.partial(_bn_stack, bn_refusal=_no_bn_refusal, ffdnet_too=False),
             ("bias-free conv + ReLU stack", None), _PlainRule, _Conv64),
    GradMode("train_realsn", "device+realsn", ("plain", "train_realsn"), ("train_realsn", "device"), _realsn_mode_stack,
             (_REALSN_OK, None), _RealSNRule, _RealSN64),
    GradMode("frozen_bn", "device+bn", ("plain", "frozen_bn"), None, functools.partial(_bn_stack, bn_refusal=_bn_refusal),
             ("bias-free conv [+ frozen BN] + ReLU stack", "FFDNet with its BatchNorm frozen"), _FrozenRule, _Frozen64),
    GradMode("train_bn", "device+bn-train", ("plain", "frozen_bn", "train_bn"), ("train_bn", "device"),
             functools.partial(_bn_stack, bn_refusal=_train_bn_refusal, batch_stats=True),
             ("bias-free conv [+ train-mode BN] + ReLU stack", "FFDNet with its BatchNorm in train mode"), _TrainRule, _Train64),
)
GRAD_MODE = {m.name: m for m in GRAD_MODES}


_RELEASED = "DenoiserParamGrads.grads: the activations were released"


def _image(who, x, sigma=None, ffdnet=False):
    """The checks of a (n,1,H,W) GPU image x and, for FFDNet, of its noise levels.  -> (x's shape, sigma as a (1,) or (n,) fp32 vector on x's
    device that the kernels can stride - None without FFDNet)."""
    if x.dim() != 4 or x.shape[1] != 1 or not x.is_cuda:
        raise _hip.DeqsciHipError(f"{who}: x must be a (n,1,H,W) GPU image, got {tuple(x.shape)} on {x.device}")
    if not ffdnet:
        return tuple(x.shape), None
    _even(x, who)
    if sigma is None:
        raise ValueError(f"{who}: FFDNet is evaluated at a noise level: sigma is required")
    sigma = torch.as_tensor(sigma, dtype=torch.float32, device=x.device).reshape(-1)
    if sigma.numel() not in (1, x.shape[0]):
        raise ValueError(f"{who}: sigma must have 1 or {x.shape[0]} elements, got {sigma.numel()}")
    if sigma.numel() > 1 and sigma.stride(0) not in (0, 1):
        sigma = sigma.contiguous()
    return tuple(x.shape), sigma


class DenoiserJacobian:
    """v -> J_D(x) v (.jvp) and v -> J_D(x)^T v (.vjp) for a (n,1,H,W) fp32 GPU image x and v of its shape, on the HIP kernels
    (_MaskedStack; .masks are its ReLU masks): a diagnostic of the map the iteration applies, so FFDNet (grayscale, eval mode) is
    differentiated through its input at the noise level sigma, a constant of the linearisation.  Raises ValueError for a net
    jacobian_eligibility refuses and for an FFDNet image with an odd side, before any launch."""

    def __init__(self, net, x, sigma=None):
        ok, why = jacobian_eligibility(net)
        if not ok:
            raise ValueError(f"DenoiserJacobian: {why}")
        ffdnet = why == FFDNET_THROUGH_INPUT
        self.shape, sigma = _image("DenoiserJacobian", x, sigma, ffdnet)
        self._stack = _MaskedStack(ffdnet_plan(net) if ffdnet else host_plan(net)[0], x, sigma)
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
    cannot differentiate.  train_realsn=True (implicit_backward = "device+realsn") serves in addition a net in train mode that
    param_eligibility(net, train_realsn=True) accepts: J_D is read at the `weight` buffers as the LAST call left them (the reference's hook
    differentiates that call's graph), packed here by csrc/realsn.hip's R3 into buffers of this object's own, which no later call changes."""

    def __init__(self, net, x, sigma=None, train_realsn=False):
        ok, why = eligibility(net, train_realsn)
        if not ok:
            raise ValueError(f"DenoiserVJP: {why}")
        self.shape = _image("DenoiserVJP", x)[0]
        self.zero = why == _FFDNET_OK
        if why == _REALSN_OK:
            self._stack = _realsn_device_stack(realsn_stack(net)[0], _hip.f32c(x.detach()), False, False)[0]
        else:
            self._stack = None if self.zero else _MaskedStack(host_plan(net)[0], x)
        self.masks = [] if self.zero else self._stack.masks

    def __call__(self, v):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"DenoiserVJP: v must have the shape {self.shape} of x, got {tuple(v.shape)}")
        return torch.zeros_like(v) if self.zero else self._stack.vjp(v)


class DenoiserParamGrads:
    """The denoiser's weight gradients on the device, for a (n,1,H,W) fp32 GPU image x: one forward pass of _MaskedStack that keeps the
    post-ReLU activations - (k-1) n 64 H W 4 bytes - and the masks; .noise = D(x) from that pass, .masks, .shape, .ffdnet.  .grads(v) ->
    (dD/dtheta)^T v, one tensor per parameter, and .vjp(v) -> the input product J_D(x)^T v are ONE walk back: the masked transposed layers
    carry the gradient down, csrc/wgrad.hip's W1 serves the two edge layers, and every 64 -> 64 layer does what its rule says.  need: one
    bool per parameter - the walk stops below the lowest layer asked for, the others are None.  .release() drops the activations.
    Everything is enqueued on the current stream with no host synchronisation.  Raises ValueError with param_eligibility()'s reason.

    The keywords name the mode (GRAD_MODES): it serves the nets param_eligibility accepts under the same keywords, and .grads answers for
    the mode's parameters in their order - conv_weights(net) by default (every 64 -> 64 layer is _Conv64: W0), else grad_parameters'.

    frozen_bn=True: a 64 -> 64 layer with a BatchNorm is _Frozen64: the BatchNorm folded into the forward and into the walk,
    csrc/wgrad_bn.hip's W0-BN (dW = s R, dbeta, and sum W R for dgamma, from one pass) - skipped where none of the three is asked for.
    FFDNet (sigma: its (1,) or (n,) noise levels, required) reads both edge layers through the pixel-(un)shuffle with W2, .noise is
    ffdnet_tail's, and .vjp is zero: its input is detached.

    train_bn=True - the BatchNorms in TRAIN mode, as the reference trains them: a 64 -> 64 layer with a BatchNorm is _Train64:
    csrc/bn_train.hip's T1 updates the module's running_mean / running_var / num_batches_tracked IN PLACE on the device, exactly once per
    construction, and the layer keeps its convolution output c beside the post-ReLU activation: (2 (k-2) + 1) n 64 H W 4 bytes for k
    layers (FFDNet: 27 activations at half resolution), twice the frozen mode's.  T3 and T4 run wherever the walk passes, asked for or
    not: dc is what goes down, through the plain (unfolded) transposed weight, so .vjp(v) is the true input product (FFDNet: zero).

    train_realsn=True: per RealSNConv2d R1 (the module's weight_u and weight move IN PLACE, exactly once, as its own forward moves them; W,
    the new u, v and the record are kept as autograd._RealSNWeight keeps them), R3 (both packs, on the device), then the masked stack.
    Back: W0 / W1 give the NORMALISED weight's gradient and R2 turns it into weight_orig's; a plain Conv2d's is its own.  No atomics."""

    def __init__(self, net, x, sigma=None, frozen_bn=False, train_bn=False, train_realsn=False, *, mode=None):
        mode = mode or grad_mode("DenoiserParamGrads", frozen_bn, train_bn, train_realsn)          # (mode: a caller's GradMode in hand)
        stack, self.ffdnet, why = mode.stack(net)
        if stack is None:
            raise ValueError(f"DenoiserParamGrads: {why}")
        self.shape, self._sigma = _image("DenoiserParamGrads", x, sigma, self.ffdnet)
        self._x = _hip.f32c(x.detach())
        self._stack, self._steps, self._rws = mode.device_rule.build(stack, self._x, self._sigma)
        rules = self._stack.rules
        self._counts = [1] + [r.count for r in rules] + [1]                 # parameters per layer
        self.masks, self.noise = self._stack.masks, self._stack.noise
        # the scratch buffers of the walk's kernels, behind the forward's activations: W1 and W0 share one, W2 and W0-BN the other
        n, H, W = (self.shape[0], self.shape[2] // 2, self.shape[3] // 2) if self.ffdnet else (self.shape[0],) + self.shape[2:]
        self._ws = _hip.wgrad_workspace(n, H, W, x.device) if not self.ffdnet or not all(r.bn_workspace for r in rules) else None
        self._ws_bn = _hip.wgrad_bn_workspace(n, H, W, x.device) if self.ffdnet or any(r.bn_workspace for r in rules) else None
        for rule in rules:
            rule.ws = self._ws_bn if rule.bn_workspace else self._ws

    def _v(self, v, what):
        if tuple(v.shape) != self.shape:
            raise _hip.DeqsciHipError(f"DenoiserParamGrads.{what}: v must have the shape {self.shape} of x, got {tuple(v.shape)}")
        return _hip.f32c(v)

    def _edge(self, img, t, which):
        """The weight gradient of the first (which = 0) or the last (1) layer from the image side img and the 64-channel side t."""
        if self.ffdnet:
            return _hip.wgrad_shuffle(img, t, which, None if which else self._sigma, self._ws_bn)
        G = _hip.wgrad_c1_c64(img, t, which, self._ws)
        step = None if self._steps is None else self._steps[-1 if which else 0]
        return G if step is None else _realsn_grad(G, step, self._rws)

    def _walk(self, v, need, want_input):
        """The walk back from the gradient v of the noise.  -> (one gradient per parameter - None where `need` is false -, J_D(x)^T v if
        want_input, else None).  Nothing asked for launches nothing."""
        st, counts = self._stack, self._counts
        k, total = len(counts), sum(counts)
        first = [sum(counts[:i]) for i in range(k)]
        need = [bool(b) for b in need]
        if len(need) != total:
            raise ValueError(f"DenoiserParamGrads.grads: need has {len(need)} entries for {total} parameters")
        out = [None] * total
        if not any(need) and not want_input:
            return out, None
        acts = st.acts if st.acts is not None else [None] * (k - 1)
        wanted = [any(need[first[i]:first[i] + counts[i]]) for i in range(k)]
        lowest = -1 if want_input else wanted.index(True)
        if wanted[k - 1]:
            out[first[k - 1]] = self._edge(v, acts[-1], 1)
        if lowest == k - 1:
            return out, None
        g = st._first(v, st.tail_t, st.masks[-1])                          # the gradient behind layer k-2, masked by its ReLU
        for i in range(k - 2, 0, -1):
            mine = slice(first[i], first[i] + counts[i])
            got, g = st.rules[i - 1].backward(acts[i - 1], g, need[mine])
            out[mine] = [t if b else None for t, b in zip(got, need[mine])]
            if i == lowest:
                return out, None
            g = _hip.conv3x3_c64_winograd_masked(g, st.mid_t[i - 1], st.masks[i - 1])
        if need[0]:
            out[0] = self._edge(self._x, g, 0)
        return out, (st._last(g, st.head_t) if want_input else None)

    def grads(self, v, need=None):
        if self._stack.acts is None:
            raise RuntimeError(_RELEASED)
        return self._walk(self._v(v, "grads"), [True] * sum(self._counts) if need is None else need, False)[0]

    def vjp(self, v):
        v = self._v(v, "vjp")
        return torch.zeros_like(v) if self.ffdnet else self._walk(v, [False] * sum(self._counts), True)[1]

    def release(self):
        self._stack.acts = None
        for rule in self._stack.rules:
            rule.release()
