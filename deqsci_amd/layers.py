"""What a "conv stack" is, decided once: a denoiser's module sequence (conv -> optional BatchNorm -> optional ReLU, repeated) as
[(weight, bias or None, relu)] with eval-mode BatchNorm folded into the convolution.  The engine's f-call (engine._Denoiser), the implicit
backward and the Jacobian diagnostics (vjp.host_plan, vjp.ffdnet_plan) all run this list.  conv_bn_stack is the same walk unfolded -
[(conv, bn or None, relu)], the modules themselves - for what needs the BatchNorm's own parameters: vjp.bn_stack, and behind it
vjp.grad_parameters and the one backward walk of the weight gradients with its three layer rules (no BatchNorm, frozen, train mode);
`folded` turns that list into conv_stack's.  CPU-safe."""
import torch


def _fold_bn(conv_w, bn):
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return (conv_w * scale.view(-1, 1, 1, 1)).contiguous(), (bn.bias - bn.running_mean * scale).contiguous()


def _conv_ok(conv):
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.padding) == (1, 1) and tuple(conv.stride) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros")


def conv_bn_stack(mods, train_bn=False):
    """(stack, reason): the module sequence `mods` as [(conv module, BatchNorm2d module or None, relu)] - or (None, why not), by the rules
    of conv_stack (which folds this list): 3x3, stride-1, pad-1 convolutions without bias, each followed by an optional eval-mode
    BatchNorm2d and an optional ReLU.  train_bn=True: the same walk for a net whose BatchNorm2d layers normalise by the batch (nothing to
    fold: vjp.param_eligibility(net, train_bn=True) says what they must be)."""
    from .networks.simplecnn import RealSNConv2d
    mods = list(mods)
    stack, i = [], 0
    while i < len(mods):
        conv = mods[i]
        if isinstance(conv, RealSNConv2d):
            # in eval mode = conv2d with its stored, already normalised `weight` buffer (networks/provable/model/conv_sn_chen.py:65-67)
            if conv.training:
                return None, "RealSNConv2d in train mode (its weight is renormalised by the power iteration)"
        elif isinstance(conv, torch.nn.Conv2d):
            if not _conv_ok(conv):
                return None, "Conv2d other than 3x3, stride 1, padding 1"
            if conv.bias is not None:
                return None, "Conv2d with a bias"
        else:
            return None, f"unknown module {type(conv).__name__} where a convolution was expected"
        bn = None
        i += 1
        if i < len(mods) and isinstance(mods[i], torch.nn.BatchNorm2d):
            bn = mods[i]
            if not train_bn and (bn.training or not bn.track_running_stats):
                return None, "BatchNorm2d in train mode (batch statistics: its Jacobian is not a fixed scale)"
            i += 1
        relu = i < len(mods) and isinstance(mods[i], torch.nn.ReLU)
        if relu:
            i += 1
        elif i < len(mods) and not isinstance(mods[i], (torch.nn.Conv2d, RealSNConv2d)):
            return None, f"unknown module {type(mods[i]).__name__}"
        stack.append((conv, bn, relu))
    return stack, None


def conv_stack(mods):
    """(layers, reason): the module sequence `mods` (net.dncnn, FFDNet's itermediate_dncnn) as [(weight, bias or None, relu)], detached,
    BatchNorm folded (weight * s, bias = beta - mean * s) - or (None, why not) when it is anything but 3x3, stride-1, pad-1 convolutions
    without bias, each followed by an optional eval-mode BatchNorm2d and an optional ReLU."""
    stack, why = conv_bn_stack(mods)
    return (None, why) if stack is None else (folded(stack), None)


def folded(stack):
    """conv_bn_stack's list as conv_stack's: [(weight, bias or None, relu)], detached, every (eval-mode) BatchNorm folded."""
    layers = []
    for conv, bn, relu in stack:
        w, b = conv.weight.detach(), None
        if bn is not None:
            w, b = (t.detach() for t in _fold_bn(w, bn))
        layers.append((w, b, relu))
    return layers
