"""DEQ-SCI reconstruction engine: the whole GAP/prox-grad fixed-point loop on one MI355X.

What the reference does per measurement (solvers/new_equilibrium_utils_yaping.py:153-189,249-281
driving solvers/equilibrium_solvers_yaping.py:397-425) as ~90 ATen launches, two permute copies
and three host syncs per iteration, this engine does as

    [K7+K3 mix_gap] -> denoiser (torch.nn on PyTorch-ROCm) -> [K4 residual_store] -> [K5+K6 solve]

on a batch of independent measurements, with

  * the loop state kept PLANAR (bsz,B,H,W) - the denoiser's (bsz*B,1,H,W) layout - so both
    per-iteration transposes of the reference disappear; only Phi / x0 in and the reconstruction out
    cross the (bsz,H,W,B) API layout, through the LDS-staged transpose kernels;
  * the history stored as F and G = F - X, Gram matrix updated one row per iteration;
  * the FFDNet sigma schedule (60/255 * 0.971^call, fp32 repeated multiply, ibid. :408-413) read
    from a device table by call index - no `self.y != y.mean()` host sync per call;
  * the relative residual polled one iteration late from pinned memory, so the host never drains
    the GPU queue (the iterate ping-pongs between two buffers, which makes the one speculative
    extra iteration harmless when the tolerance test fires);
  * for small batches, where a conv layer is a few tens of microseconds and the ~3400 launches of a reconstruction are
    what the GPU waits for, the WHOLE reconstruction (x0, every f-call, the output transpose) replayed as ONE hipGraph
    captured on the second call of a shape: same kernels, same arguments, bit-identical output.  The graph always runs
    max_iter iterations; the residual table is read afterwards and, should the tolerance test have fired earlier (it never
    does on the reference's data), the call is redone on the eager path, which stops where the reference stops.

Semantics are the reference's (same slots k % m, same bordered system, residual over the whole
batch as at :184, returned iterate = f(X_last)).  Deliberate deviations, all result-neutral for the
reference's own usage: sigma restarts at every reconstruct() call (the reference restarts when
y.mean() changes); the dead second f-call of DEQFixedPoint.forward (:271-272, only feeds the
backward hook) is skipped unless `extra_call=True` - or the denoiser has a train-mode RealSNConv2d,
whose every call advances module state (weight_u, weight): such a net gets all max_iter + 2 calls and
runs eagerly, never as a captured graph.  The same holds for a net whose train-mode BatchNorms run on
the device (train_bn="device": csrc/bn_train.hip moves running_mean / running_var /
num_batches_tracked at every f-call, as the module's own forward does).  train_realsn="device" puts the
f-calls of a train-mode RealSN_SimpleCNN on the HIP kernels too: the power step in place in the module's
buffers, csrc/realsn.hip's R3 from the new weight to the packs, the fp32 kernels (path "train realsn per layer").
"""
import math
import numpy as np

import torch
import torch.nn.functional as F

from . import _hip
from ._hip import LAYOUT_BHW, LAYOUT_HWB
from .layers import _fold_bn, conv_stack                    # noqa: F401  (engine._fold_bn stays importable)

SIGMA0 = 60 / 255
SIGMA_DECAY = 0.971


def sigma_schedule(n):
    """sigma used by f-call c (0-based): fp32(60/255) multiplied c times by fp32(0.971) in fp32."""
    out = np.empty(n, dtype=np.float32)
    s = np.float32(SIGMA0)
    d = np.float32(SIGMA_DECAY)
    for i in range(n):
        out[i] = s
        s = np.float32(s * d)
    return out


def _exhaust(gen):
    """Run a generator to its end and return its return value (the plain-call form of the *_steps generators below)."""
    while True:
        try:
            next(gen)
        except StopIteration as done:
            return done.value


def check_snapshots(snapshots, max_iter, iterator="anderson"):
    """The `snapshots=` request of DEQSCIEngine.reconstruct as a tuple of ints (None: no snapshot), or ValueError: every entry an
    integer iteration count, strictly increasing, smaller than max_iter, and one the iterator can stop at (Anderson: at least 3 - a
    run with max_iter <= 2 raises in the reference; Picard: at least 1)."""
    if snapshots is None:
        return None
    if isinstance(snapshots, (str, bytes)) or not hasattr(snapshots, "__iter__"):
        raise ValueError(f"snapshots={snapshots!r}: expected a sequence of iteration counts")
    out = []
    for k in snapshots:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"snapshots={snapshots!r}: {k!r} is not an integer iteration count")
        out.append(int(k))
    if not out:
        return None
    lo = 3 if iterator == "anderson" else 1
    for a, b in zip(out, out[1:]):
        if b <= a:
            raise ValueError(f"snapshots={tuple(out)}: must be strictly increasing")
    if out[0] < lo:
        raise ValueError(f"snapshots={tuple(out)}: the smallest horizon of the {iterator} iteration is {lo}")
    if out[-1] >= max_iter:
        raise ValueError(f"snapshots={tuple(out)}: every horizon must be smaller than max_iter={max_iter} (the run's own result is the last one)")
    return tuple(out)


class _Edges:
    """The first and last layer of a conv + BN + ReLU denoiser as an f-call runs them - what differs between FFDNet (div = 2: its 64->64
    layers run at half resolution, its first layer takes sigma and the range of the image, its last layer ends in a pixel shuffle) and a
    plain network (div = 1: SimpleCNN, DnCNN-17, plugins), described once.  head_w / tail_w: the packs of the fp32 stencil kernels
    (csrc/ffdnet_edges.hip), None where that layer has no HIP kernel; head_w16 / tail_w16: those of the kernels that write / read the
    Sp16 and P32 layouts of the 64->64 layers (a plain first layer has one pack for all three)."""
    __slots__ = ("div", "ffdnet", "relu", "head_w", "tail_w", "head_w16", "tail_w16")

    def __init__(self, div=1, relu=True):
        self.div, self.ffdnet, self.relu = div, div == 2, relu
        self.head_w = self.tail_w = self.head_w16 = self.tail_w16 = None

    def head(self, x, sigma, act=None, out=None, in_rng=None, out_rng=None, out_exp=_hip.SP16_DEFAULT_EXP, track=None):
        """The first layer on x (n,1,H,W) as fp32 channels_last (act=None) or in the layout act (_hip.Sp16 / _hip.P32) with the range
        (out_rng, out_exp); sigma and in_rng (the slots holding max |image|) are FFDNet's, track the slots of a measuring launch."""
        if not self.ffdnet:
            return _hip.conv3x3_c1_to_64(x, self.head_w, relu=self.relu, out=out, sp16=act is _hip.Sp16, p32=act is _hip.P32,
                                         out_rng=out_rng, out_exp=out_exp, track=track)
        if act is None:
            return _hip.ffdnet_head(x, self.head_w, sigma)
        if act is _hip.P32:
            return _hip.ffdnet_head_p32(x, self.head_w16, sigma, out, in_rng, out_rng=out_rng, out_exp=out_exp)
        return _hip.ffdnet_head_split16(x, self.head_w16, sigma, out, in_rng, out_rng=out_rng, out_exp=out_exp, track=track)

    def tail(self, h, out=None, in_bias=None):
        """The last layer (FFDNet: + pixel shuffle) on h in any of the three layouts; in_bias: the bias + ReLU the layer in front of an
        fp32 h left to this one."""
        if isinstance(h, _hip.P32):
            return _hip.ffdnet_tail_p32(h, self.tail_w16, out)
        if isinstance(h, _hip.Sp16):
            return _hip.tail_split16(h, self.tail_w16, out)
        return (_hip.ffdnet_tail if self.ffdnet else _hip.conv3x3_c64_to_1)(h.contiguous(memory_format=torch.channels_last), self.tail_w, out, in_bias)


class _Denoiser:
    """Adapter from a reference-style denoiser plugin (nn.Module with .tag) to
    `run(z1_planar, call) -> (tensor (bsz,B,H,W), is_noise)`; dispatch as at
    solvers/equilibrium_solvers_yaping.py:402-425."""

    def __init__(self, net, fold_bn=True, channels_last=None, fused_epilogue=True, fused_edges=True, winograd=True, conv64="fast",
                 act_range="data", blk32=True, stack=True, stack_kernel="w16", train_bn="module", train_realsn="module"):
        from .networks import FFDNet
        self.net = net
        # what runs an f-call of a net in TRAIN mode - "module" (default): the plugin's own forward (MIOpen); "device": the kernels, for a net the
        # option's mode of vjp.GRAD_MODES serves (_refresh_train).  A net it cannot serve keeps "module"; train_why says why.
        #   train_bn (batch statistics; the reference trains FFDNet so): head kernel -> per layer [fp32 Winograd raw convolution -> T1 statistics
        #     + buffer update -> T2 normalise + ReLU] -> tail kernel (csrc/bn_train.hip)
        #   train_realsn (one power step per RealSNConv2d and call): per layer R1 in place in the module's weight_u / weight buffers, R3 into
        #     pack buffers allocated once here, then the fp32 kernels on those packs (csrc/realsn.hip)
        for option, value in (("train_bn", train_bn), ("train_realsn", train_realsn)):
            if value not in ("module", "device"):
                raise ValueError(f"{option}={value!r}: expected 'module' or 'device'")
            setattr(self, option, value)
        self._bn_ws = {}
        # stack_kernel: which kernel a stack launch of FFDNet's run runs - "w16" (default): the split-fp16 arithmetic under Winograd F(2,3) x
        # direct (csrc/conv_w16.hip: a third fewer matrix-core products, p32 activations between FFDNet's first and last layer); "s16": the
        # split-fp16 direct convolution (csrc/conv_s16.hip).  The measuring f-call keeps the direct kernel; SimpleCNN's two middle layers (a run
        # shorter than STACK_MIN_LAYERS) go out as single launches of the chosen kernel.
        if stack_kernel not in ("w16", "s16"):
            raise ValueError(f"stack_kernel={stack_kernel!r}: expected 'w16' or 's16'")
        self.stack_kernel = stack_kernel
        self.gate = None                                            # (_StackGate of a grouped reconstruction: one stack launch on the device at a time)
        # set by the engine while it keeps off the stack launches after a time-out: FFDNet's run as ONE LAUNCH PER LAYER of the same Winograd
        # kernel - bit-identical to the stack launch (test_wino16_stack_is_bit_identical_to_single_launches), so that the calls behind a
        # time-out return the bits of ordinary calls.  (A caller's own stack=False keeps its documented meaning: the direct kernel per layer.)
        self.per_layer_w16 = False
        self.last_path = None                                       # what the last f-call's run of 64->64 layers went out as (last_info["denoiser_path"])
        self._wstacks = {}                                          # first layer of a run -> _hip.Wino16Stack
        # stack: a run of split-fp16 64->64 layers (FFDNet's 13, SimpleCNN's 2) as ONE launch per slice of the batch
        # (_hip.conv3x3_c64_split16_stack: tiles synchronised by per-tile progress words instead of kernel boundaries, slices that keep
        # their activations in the Infinity Cache); bit-identical to the per-layer launches, which the measuring f-call keeps
        self.stack = bool(stack)
        self.stack_per_launch = None                                # images per stack launch (None: _hip.split16_stack_per_launch; an A/B of the tools)
        self.slice_edges = True                                     # FFDNet: first layer -> run -> last layer slice by slice (False: an A/B of the tools)
        self._stacks = {}                                           # first layer of a run -> _hip.Split16Stack
        self.stack_launches = 0
        self.fused_edges = fused_edges
        self.winograd = winograd
        self.conv64 = conv64                                        # _hip.conv64_kernel_for policy: "fast" | "fast32" | "f22" | "f44" | "s16"
        self.f22_calls = None                                       # f-calls [0, f22_calls) run F(2x2,3x3) whatever the policy (DEQSCIEngine)
        self._policy = conv64
        self.blk32 = bool(blk32)                                    # blk32 activations between F(4x4,3x3) layers (False: an A/B of the tools)
        # The scales of the split-fp16 layers' activations: "data" = every activation's power-of-two scale follows max |activation| as
        # measured ON THE DEVICE during the first f-call of a reconstruction (run(..., calibrate=True): each layer is run once to measure,
        # once to write - fp32 is scale-free, fp16 is not; see _hip.act_exp); "fixed" = 2^8 throughout (activations of a few units).
        if act_range not in ("data", "fixed"):
            raise ValueError(f"act_range={act_range!r}: expected 'data' or 'fixed'")
        self.act_range = act_range
        self.ranges = None                                          # (len(layers) + 1, images) fp32 on the device: [i, j] = max |input of layer i, image j|
        self._calibrating = False
        self._stale = True                                          # the ranges have not been measured on the current input yet
        # channels_last is what the HIP Winograd / edge kernels consume.  Without them (winograd=False) it is a
        # MIOpen trade-off measured on MI355X (profiles/r01_denoiser_variants.jsonl): 8 % faster for FFDNet's
        # 128x128x64 layers, 11 % slower for SimpleCNN's 256x256x64 ones.
        self.channels_last = (winograd or isinstance(net, FFDNet)) if channels_last is None else bool(channels_last)
        self.fused_epilogue = fused_epilogue
        self.tag = getattr(net, "tag", None)
        if self.tag not in ("conv2d", "conv3d", "ffdnet", "denoiser", "3d_denoiser"):
            raise NotImplementedError(f"unknown nonlinear_op tag {self.tag!r}")
        self.sigma_table = None
        self.fold_bn = fold_bn
        self.fast = None
        self._wkey = None
        self._refresh()

    # the edge layers' packs (self.edges), under the names tools and tests read
    head_w, tail_w, head_w16, tail_w16 = (property(lambda self, k=k: getattr(self.edges, k)) for k in ("head_w", "tail_w", "head_w16", "tail_w16"))

    def _weights_key(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.net.parameters()) + list(self.net.buffers()))

    def _refresh(self):
        """(Re)build the BN-folded functional FFDNet whenever the module's tensors changed
        (e.g. load_state_dict after the engine was created)."""
        from .networks import DnCNN, FFDNet
        net = self.net
        key = (self._weights_key(), net.training)
        if key == self._wkey:
            return
        self._wkey = key
        self.fast = None
        self.wino = None
        self.edges = e = _Edges(2 if isinstance(net, FFDNet) else 1)
        self._refresh_train(e)
        seq = None
        if isinstance(net, FFDNet) and not net.training and net.num_input_channels == 1 and self.fold_bn:
            seq = net.intermediate_dncnn.itermediate_dncnn
        elif isinstance(net, DnCNN) and not net.training and self.fold_bn:
            seq = net.dncnn                       # SimpleCNN / RealSN_SimpleCNN / DnCNN-17: conv [+BN] + ReLU blocks
        # a sequence the walker refuses (a bias, a kernel other than 3x3 pad 1, BatchNorm in train mode, ...) keeps fast = None: _route
        # answers "module" and the plugin's own forward runs
        layers = None if seq is None else conv_stack(seq)[0]
        if layers is not None:
            layers = [(w.contiguous(memory_format=torch.channels_last) if self.channels_last else w.contiguous(), b, relu)
                      for w, b, relu in layers]
            self.fast = layers
            # 64->64 layers: Winograd on the fp32 matrix cores with bias+ReLU fused: F(4x4,3x3) (csrc/winograd44.hip) when the
            # launch has more than a wave of block tiles, F(2x2,3x3) (csrc/winograd.hip) below that - _hip.conv3x3_c64 picks
            # (the split-fp16 pack costs a host sync: made here, never inside a hipGraph capture, whenever the policy can pick that kernel)
            s16 = self.conv64 in ("fast", "s16")
            self.wino = [(_hip.pack_conv64_weights(w, s16=s16) if (self.winograd and self.channels_last and w.is_cuda
                                                                      and tuple(w.shape) == (64, 64, 3, 3)) else None)
                         for w, _, _ in layers]
            self.ranges = None
            self._stacks = {}
            self._wstacks = {}
            (w0, b0, e.relu), (wl, bl, relu_l) = layers[0], layers[-1]
            if self.fused_edges and self.channels_last and w0.is_cuda and bl is None and not relu_l and tuple(wl.shape) == (e.div ** 2, 64, 3, 3):
                # the last layer (FFDNet: + upsamplefeatures) as one HIP stencil kernel (csrc/ffdnet_edges.hip), and for an sp16 / p32 input (MFMA form)
                e.tail_w = (_hip.pack_tail_weights if e.ffdnet else _hip.pack_c64_to_1_weights)(wl)
                e.tail_w16 = _hip.TailSplit16Weights(wl)
            if self.fused_edges and self.channels_last and w0.is_cuda and b0 is None:
                if e.ffdnet and e.tail_w is not None and e.relu and tuple(w0.shape) == (64, 5, 3, 3):
                    # concatenate_input_noise_map + first conv + ReLU likewise, and writing sp16 / p32 (f16 matrix-core form)
                    e.head_w, e.head_w16 = _hip.pack_head_weights(w0), _hip.HeadSplit16Weights(w0)
                elif not e.ffdnet and tuple(w0.shape) == (64, 1, 3, 3):
                    e.head_w = e.head_w16 = _hip.pack_c1_to_64_weights(w0)      # (one stencil kernel, three output layouts)

    # option (the name of its mode in vjp.GRAD_MODES, whose stack says which nets it serves) -> (the path of an f-call it serves, what packs the
    # net's layers, the f-call, what an option that is not served says of a net in eval mode), in the order the options are tried
    TRAIN_OPTIONS = {"train_bn": ("train bn per layer", "_pack_train_bn", "_train_bn_call", "its BatchNorm is folded into the convolutions"),
                     "train_realsn": ("train realsn per layer", "_pack_train_realsn", "_train_realsn_call", "a RealSNConv2d uses its stored weight")}

    def _refresh_train(self, e):
        """train_mode = the first option asked for ("device") whose mode serves the net as it stands, with the net's layers packed for it
        (self.train or self.rsn, the edge kernels' packs in e) - or None and train_why, the first reason a net in train mode stays on its module."""
        from . import vjp
        net = self.net
        self.train, self.rsn, self.train_why, self.train_mode = None, None, None, None
        if not (isinstance(net, torch.nn.Module) and net.training):
            return
        for option, (_, pack, _, _) in self.TRAIN_OPTIONS.items():
            if getattr(self, option) != "device":
                continue
            stack, _, why = vjp.GRAD_MODE[option].stack(net)
            if stack is not None and not all(t.is_cuda and t.dtype == torch.float32 for t in list(net.parameters()) + list(net.buffers()) if t.is_floating_point()):
                stack, why = None, "the net's parameters and buffers are not fp32 tensors on the GPU"
            if stack is not None:
                getattr(self, pack)(e, stack)
                self.train_mode = option
                return
            self.train_why = self.train_why or why

    def _pack_train_bn(self, e, stack):
        """train_bn="device": the UNFOLDED layers of a net in train mode - self.train = [(Conv64Weights, BatchNorm2d or None)] for the 64->64
        layers, the edge kernels' packs in e."""
        w0, wl = stack[0][0].weight.detach(), stack[-1][0].weight.detach()
        if e.ffdnet:
            e.head_w, e.tail_w = _hip.pack_head_weights(w0), _hip.pack_tail_weights(wl)
        else:
            e.head_w, e.tail_w = _hip.pack_c1_to_64_weights(w0), _hip.pack_c64_to_1_weights(wl)
        e.relu = True
        self.train = [(_hip.pack_conv64_weights(conv.weight.detach(), s16=False), bn) for conv, bn, _ in stack[1:-1]]

    def _train_bn_call(self, x, sg):
        """One f-call with the BatchNorms normalising by the batch: no activation is kept, the module's buffers move once per layer."""
        e = self.edges
        h = e.head(x, sg)
        P = h.shape[0] * h.shape[2] * h.shape[3]
        ws = self._bn_ws.get((P, h.device))
        if ws is None:
            self._bn_ws = {(P, h.device): (_hip.bn_train_workspace(P, h.device), torch.empty(128, dtype=torch.float64, device=h.device))}
            ws = self._bn_ws[(P, h.device)]
        for weights, bn in self.train:
            if bn is None:
                h = _hip.conv3x3_c64(h, weights, None, True, policy="fast32")
                continue
            c = _hip.conv3x3_c64(h, weights, None, False, policy="fast32")
            rec = _hip.bn_train_stats(c, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum, record=ws[1], workspace=ws[0])
            h = _hip.bn_train_apply(c, rec, bn.weight.detach(), bn.bias.detach(), bn.eps, relu=True, out=c)
        return e.tail(h)

    def _pack_train_realsn(self, e, stack):
        """train_realsn="device": self.rsn = (per layer (conv, is RealSN, pack, pack44, v, record), R1's workspace, the 64->64 layers'
        Conv64Weights over those packs) with every buffer allocated HERE, once - an f-call allocates none of them and their addresses do
        not move.  A plain Conv2d's packs are made now (its weight does not move between f-calls); a RealSNConv2d's at every call, behind
        its power step."""
        from . import vjp
        from .networks.simplecnn import RealSNConv2d
        dev = stack[0][0].weight.device
        layers = []
        for conv, _, _ in stack:
            cout, cin = conv.weight.shape[:2]
            is_rsn = isinstance(conv, RealSNConv2d)
            pack, pack44, _ = _hip.realsn_pack_buffers(cin, cout, dev, pack_t=False)
            v = torch.empty((1, cin) + tuple(conv.weight_u.shape[2:]), device=dev, dtype=torch.float32) if is_rsn else None
            record = torch.empty(3, device=dev, dtype=torch.float64) if is_rsn else None
            if not is_rsn:
                _hip.realsn_pack(_hip.f32c(conv.weight.detach()), pack, pack44, None)
            layers.append((conv, is_rsn, pack, pack44, v, record))
        mids = [_hip.Conv64Weights(conv.weight, s16=False, f22=pack, f44=pack44) for conv, _, pack, pack44, _, _ in layers[1:-1]]
        e.head_w, e.tail_w, e.relu = layers[0][2], layers[-1][2], True
        self.rsn = (layers, vjp._realsn_workspace(stack, dev), mids)

    def _train_realsn_call(self, x, sg=None):
        """One f-call with every RealSNConv2d renormalised first: R1 moves the module's weight_u and weight in place (the module's own
        kernels: its bits), R3 turns the weight into the packs, and the first-layer stencil, the fp32 64->64 kernels and the last-layer
        kernel run on them.  No host synchronisation, no host -> device copy."""
        from . import vjp
        layers, ws, mids = self.rsn
        for conv, is_rsn, pack, pack44, v, record in layers:
            if is_rsn:
                vjp.realsn_power_in_place(conv, ws, v, record)
                _hip.realsn_pack(conv.weight, pack, pack44, None)
        h = self.edges.head(x, None)
        for weights in mids:
            h = _hip.conv3x3_c64(h, weights, None, True, policy="fast32")
        return self.edges.tail(h)

    def _run_stack(self, h, skip_last=False, skip_first=False, defer_last_epilogue=False, native_out=False):
        """defer_last_epilogue: leave the bias+ReLU of the last executed layer to the consumer (the fused
        FFDNet tail applies it while staging its input) and return (raw conv output, bias) - only when that
        layer runs on MIOpen; the HIP 64->64 kernels apply bias+ReLU in their own epilogue for free.
        native_out: the consumer reads the split-fp16 kernel's sp16 layout directly (the HIP tails do): do not convert back."""
        if self.channels_last and not isinstance(h, _hip.Sp16):
            h = h.contiguous(memory_format=torch.channels_last)
        fused = self.fused_epilogue and h.is_cuda
        lo, hi = (1 if skip_first else 0), (len(self.fast) - 1 if skip_last else len(self.fast))
        idx = list(range(lo, hi))
        if defer_last_epilogue:
            last = idx[-1]
            w, b, relu = self.fast[last]
            if self.wino[last] is not None and h.is_cuda:
                return self._run_layers(h, idx, fused, native_out), None
            assert b is not None and relu
            return F.conv2d(self._run_layers(h, idx[:-1], fused, native_out), w, None, padding=1), b
        return self._run_layers(h, idx, fused, native_out)

    # a run shorter than this keeps its per-layer launches: the stack launch earns its keep over many layers on a cache-resident slice
    # (FFDNet's 13: 138.8 -> 144.8 frames/s); on SimpleCNN's two layers it costs 4 % (180.6 vs 188.7: agent-scope loads re-read the halo
    # overlap from memory instead of the L2, and there is no kernel boundary worth saving between two 100 us launches)
    STACK_MIN_LAYERS = 3
    # a plain conv + BN + ReLU network (tag 'denoiser') with a long run of 64->64 layers - DnCNN-17's 15 - goes slice by slice like FFDNet:
    # 1->64 layer -> the run as ONE stack launch -> 64->1 layer (_sliced).  Set on the instance by a prepare() that is told the f-call's
    # batch (n_img=: the engine's own); a bare prepare(n_calls, device) + run() keeps the launch per layer of the kernels' own tests and tools.
    plain_sliced = False
    # _refresh_train's: the option that serves the net's train-mode f-calls on the device, or None and, where one was asked for and the net is in
    # train mode, the reason; train: _pack_train_bn's layers (train_bn="device"), rsn: _pack_train_realsn's (train_realsn="device"), else None
    train_mode = train_why = train = rsn = None

    def _stack_for(self, idx, device, w16=False):
        """The Split16Stack (w16: Wino16Stack) of the run of layers idx (an H2D copy of its table: built by prepare(), never inside a
        hipGraph capture)."""
        stacks = self._wstacks if w16 else self._stacks
        st = stacks.get(idx[0])
        if st is None or st.n_layers != len(idx) or st.table.device != torch.device(device):
            st = stacks[idx[0]] = (_hip.Wino16Stack if w16 else _hip.Split16Stack)(
                [(self.wino[i].w16 if w16 else self.wino[i].s16, self.fast[i][1], self.fast[i][2]) for i in idx], device)
        return st

    def _middle_run(self):
        """Indices of the run of 64->64 layers between the edge layers, when the whole run can take the split-fp16 kernel."""
        if self.fast is None or self.wino is None or len(self.fast) < 4 or self.conv64 not in ("fast", "s16"):
            return None
        idx = list(range(1, len(self.fast) - 1))
        return idx if all(self.wino[i] is not None for i in idx) else None

    def _has_stack(self, stacks, idx):
        """Whether `stacks` (_stacks or _wstacks) holds a stack built for exactly the run of layers idx."""
        return idx is not None and idx[0] in stacks and stacks[idx[0]].n_layers == len(idx)

    def _route(self, n, H, W, device, policy, cal):
        """The path (_run_gen) of an f-call on n images of H x W under the conv64 `policy`, calibrating (cal) or not, from the attributes as
        they are NOW: tests and tools set them between calls, and the engine turns `stack` off and `per_layer_w16` on behind a time-out."""
        if self.train_mode is not None and self.tag in ("ffdnet", "denoiser") and torch.device(device).type == "cuda":
            return self.TRAIN_OPTIONS[self.train_mode][0]
        if self.fast is None or self.tag not in ("ffdnet", "denoiser"):
            return "module"
        e, cuda = self.edges, torch.device(device).type == "cuda"
        if not e.ffdnet and not (cuda and (e.head_w is not None or e.tail_w is not None)):
            return "layers"
        run = self._middle_run()
        # a run of 64->64 layers on the split-fp16 kernel: the head writes its sp16 layout, the tail reads it - no conversion pass
        # (_middle_run has looked at the packs already where it names a run)
        sp = (cuda and e.head_w is not None and e.tail_w is not None and (run is not None or all(u is not None for u in self.wino[1:-1]))
              and _hip.conv64_kernel_for(n, H // e.div, W // e.div, device, policy) == "s16")
        # the Winograd kernel of a plain network reads the ranges the first f-call measured on the direct kernels (and its time-out
        # fallback, "w16 per layer" below, needs them too); conv64="s16" means the direct kernel there
        w16 = self.stack_kernel == "w16" and (e.ffdnet or (self.conv64 != "s16" and self.ranges is not None))
        if (sp and not cal and self.stack and self.slice_edges and (e.ffdnet or self.plain_sliced) and run is not None
                and len(run) >= self.STACK_MIN_LAYERS and self._has_stack(self._stacks, run)):
            # FFDNet, DnCNN-17: first layer -> the run of 64->64 layers as one stack launch -> last layer, slice by slice
            return "w16 stack launch" if w16 and self._has_stack(self._wstacks, run) else "s16 stack launch"
        # FFDNet behind a stack time-out: the stack launch's kernel and ranges, one launch per layer.  A plain network: the 64->64 layers
        # on the split-fp16 Winograd kernel (csrc/conv_w16.hip: a third fewer matrix-core products) whenever they do not go out as a stack
        # launch - SimpleCNN's two (no run worth one), a long DnCNN-style run of a user plugin or of a bare prepare()
        # (test_plugin_stack_dncnn17_follows_the_data_scale), and behind a time-out
        if (sp and not cal and w16 and self.ranges is not None
                and (not e.ffdnet or (not self.stack and self.per_layer_w16 and self._has_stack(self._wstacks, run)))):
            return "w16 per layer"
        return "sp16 per layer" if sp else "per layer"

    def _slicing(self, path, n, H, W, device):
        """(stack, images per stack launch) of an f-call on a "... stack launch" path, n images of H x W at the 64->64 layers."""
        st = (self._wstacks if path == "w16 stack launch" else self._stacks)[1]       # (_middle_run: layers 1 .. len(fast) - 2)
        return st, self.stack_per_launch or _hip.split16_stack_per_launch(n, H, W, cus=_hip._cus(device), tile=st.TILE)

    def stack_slice(self, bsz, B, H, W, device):
        """Images per stack launch when an f-call of this shape takes a stack launch path under the engine's policy (a calibrating call
        and the first conv64_f22_calls f-calls aside) - else None.  prepare() must have run."""
        path = self._route(bsz * B, H, W, device, self.conv64, False)
        if path not in ("w16 stack launch", "s16 stack launch"):
            return None
        f = self.edges.div                                         # (FFDNet's 64->64 layers run at half resolution)
        return self._slicing(path, bsz * B, H // f, W // f, device)[1]

    def stack_timed_out(self):
        """(host sync) whether a wait inside a stack launch gave up since the last call: its results are invalid."""
        return any([st.timed_out() for st in list(self._stacks.values()) + list(self._wstacks.values())])    # (every stack: the words are rearmed)

    def _run_layers(self, h, idx, fused, native_out):
        if (self.stack and isinstance(h, _hip.Sp16) and len(idx) >= self.STACK_MIN_LAYERS and native_out and not self._calibrating
                and self._has_stack(self._stacks, idx) and (h.rng is None) == (self.ranges is None)):
            # the whole run in one launch (per slice of the batch): sp16 in, sp16 out, ranges of the run = slots idx[0] .. idx[-1] + 1
            self.stack_launches += 1
            return _hip.conv3x3_c64_split16_stack(h, self._stack_for(idx, h.t.device), None if self.ranges is None else self.ranges[idx[0]:idx[-1] + 2],
                                                  per_launch=self.stack_per_launch, check=False)
        for pos, i in enumerate(idx):
            w, b, relu = self.fast[i]
            nxt = idx[pos + 1] if pos + 1 < len(idx) else None
            chain = nxt is not None and self.wino[nxt] is not None          # the next layer is a 64->64 layer too: keep the kernel's own layout
            native = isinstance(h, (_hip.Sp16, _hip.Blk32))
            if self.wino[i] is not None and (native or (h.is_cuda and h.is_contiguous(memory_format=torch.channels_last))):
                # 64->64 layer on one of the three HIP kernels; between two such layers the activation stays in the kernel's own layout
                # (sp16 for the split-fp16 direct convolution, blk32 for F(4x4,3x3)); the layer's kind is fixed by the FIRST layer of a run
                kind = ("s16" if isinstance(h, _hip.Sp16) else "f44" if isinstance(h, _hip.Blk32) else
                        _hip.conv64_kernel_for(h.shape[0], h.shape[2], h.shape[3], h.device, self._policy))
                if kind == "s16":
                    if not isinstance(h, _hip.Sp16):
                        if self._calibrating:
                            _hip.absmax(h, self._slot(i))
                            self._measured = True
                        h = _hip.to_split16(h, rng=self._slot(i))
                    sp_out = chain or (nxt is None and native_out)
                    if sp_out and self._calibrating:               # measure max |output| of this layer, then write it with that range
                        _hip.conv3x3_c64_split16(h, self.wino[i].s16, b, relu, track=self._slot(i + 1))
                        self._measured = True
                    h = _hip.conv3x3_c64_split16(h, self.wino[i].s16, b, relu, out_f32=not sp_out, out_rng=self._slot(i + 1) if sp_out else None)
                elif kind == "f44":
                    h = _hip.conv3x3_c64_winograd44(h, self.wino[i].f44, b, relu, out_blk=bool(self.blk32 and chain))
                else:
                    h = _hip.conv3x3_c64_winograd(h, self.wino[i].f22, b, relu)
            elif fused and b is not None:
                # Conv-BN-ReLU = MIOpen conv with folded weights + ONE in-place bias+ReLU pass (HIP)
                h = _hip.bias_relu_(F.conv2d(h, w, None, padding=1), b, relu)
            else:
                h = F.conv2d(h, w, b, padding=1)
                if relu:
                    h = F.relu_(h)
        return h

    def _slot(self, i):
        """Range slots (one per image) of the input of layer i (= the output of layer i - 1), or None under act_range="fixed"."""
        return None if self.ranges is None else self.ranges[i]

    def _alloc_ranges(self, n_img, device):
        if self.fast is not None and self.act_range == "data" and (self.ranges is None or self.ranges.device != torch.device(device)
                                                                    or self.ranges.shape[1] != n_img):
            # kept across calls of a shape: a captured hipGraph carries this tensor's address in its conv nodes (a new batch size is a
            # new graph, captured after an eager call)
            self.ranges = torch.zeros((len(self.fast) + 1, n_img), dtype=torch.float32, device=device)
            self._stale = True

    def prepare(self, n_calls, device, n_img=None):
        self._refresh()
        if n_img is not None:
            self._alloc_ranges(n_img, device)
        run = self._middle_run() if (self.stack and torch.device(device).type == "cuda") else None
        if run is not None and len(run) >= self.STACK_MIN_LAYERS and self.wino[run[0]].s16.packed.is_cuda:
            self._stack_for(run, device)
            e = self.edges
            # the sliced f-call needs both edge layers in the stack's layout; a plain network takes it once prepare() knows the batch
            if e.head_w16 is not None and e.tail_w16 is not None and (e.ffdnet or n_img is not None):
                if not e.ffdnet:
                    self.plain_sliced = True
                if self.stack_kernel == "w16" and (e.ffdnet or self.conv64 != "s16"):
                    self._stack_for(run, device, w16=True)
        if self.tag == "ffdnet":
            t = self.sigma_table
            if t is None or t.numel() < n_calls or t.device != torch.device(device):
                # kept across calls: a captured hipGraph carries this tensor's address in its FFDNet-head nodes
                self.sigma_table = torch.from_numpy(sigma_schedule(n_calls)).to(device)

    def run(self, z1, call, calibrate=False):
        return _exhaust(self.run_steps(z1, call, calibrate))

    def run_steps(self, z1, call, calibrate=False):
        """calibrate: a new input (the engine: the first f-call of a reconstruction) - the ranges of the split-fp16 activations measured
        last are stale.  They are measured by the next call that takes the split-fp16 path (this one, unless the policy runs its first
        f-calls on another kernel) and kept from then on."""
        bsz, B, H, W = z1.shape
        x = z1.view(bsz * B, 1, H, W)
        self._policy = "f22" if (self.f22_calls is not None and call < self.f22_calls) else self.conv64
        if x.is_cuda:
            self._alloc_ranges(bsz * B, x.device)
        if calibrate:
            self._stale = True
        self._calibrating = cal = self._stale and self.ranges is not None and x.is_cuda
        self._measured = False                                      # set by the first measuring launch of this call
        if cal:
            self.ranges.zero_()
        try:
            out = yield from self._run_gen(z1, x, call, cal)
            if self._measured:                                      # (only a call that ran to its end has measured every layer)
                self._stale = False
            return out
        finally:
            self._calibrating = False

    def _run_gen(self, z1, x, call, cal):
        """(generator) the f-call's denoiser on the path _route picks; yields "stack" behind every stack launch when a gate is set - where
        a grouped reconstruction switches to its other half (DEQSCIEngine._reconstruct_grouped) - and returns (output, is_noise)."""
        bsz, B, H, W = z1.shape
        path = self._route(bsz * B, H, W, x.device, self._policy, cal)
        if self.tag in ("ffdnet", "denoiser"):
            sg = self.sigma_table[call:call + 1] if self.tag == "ffdnet" else None      # (a plain network takes no sigma)
            if self.train_mode is not None and path == self.TRAIN_OPTIONS[self.train_mode][0]:
                self.last_path = path
                out = getattr(self, self.TRAIN_OPTIONS[self.train_mode][2])(x, sg)
            elif path == "module":
                out = self.net(x) if sg is None else self.net(x, sg.expand(bsz * B))
            elif path == "layers":
                self.last_path = "per layer"
                out = self._run_stack(x)
            elif path in ("w16 stack launch", "s16 stack launch"):
                out = yield from self._sliced(x, sg, path)
                self.last_path = path
            elif path == "w16 per layer":
                # (behind a stack time-out: the stack launch's kernel and ranges, one launch per layer - its bits)
                self.last_path = "w16 per layer (behind a stack time-out)" if self.per_layer_w16 else path
                h = self.edges.head(x, sg, _hip.P32, in_rng=self._slot(0), out_rng=self._slot(1))
                for i in range(1, len(self.fast) - 1):
                    h = _hip.conv3x3_c64_wino16(h, self.wino[i].w16, self.fast[i][1], self.fast[i][2], out_rng=self._slot(i + 1))
                out = self.edges.tail(h)
            else:
                self.last_path = "per layer"
                out = self._per_layer(x, sg, cal, path == "sp16 per layer")
            return out.reshape(bsz, B, H, W), True
        if self.tag == "conv2d":
            return self.net(x).reshape(bsz, B, H, W), False
        x5 = z1.view(bsz, 1, B, H, W)
        return self.net(x5).reshape(bsz, B, H, W), self.tag == "3d_denoiser"

    def _sliced(self, x, sg, path):
        """(generator) The f-call slice by slice on the kernels of the path's stack: the first layer writes the slice's input buffer in that
        stack's layout (p32 / sp16) with the range slots of its images, the run of 64->64 layers is one stack launch, the last layer reads
        the buffer the run wrote - each handing its output to the next through the Infinity Cache (a slice's activation is at most
        128 MiB).  The kernels, weights and ranges of the per-layer paths: their bits."""
        e = self.edges
        n, H, W = x.shape[0], x.shape[2] // e.div, x.shape[3] // e.div
        st, per = self._slicing(path, n, H, W, x.device)
        bufs, hbuf = st.state(min(per, n), H, W), st.head_buffer(min(per, n), H, W)
        rows = None if self.ranges is None else self.ranges[1:len(self.fast)]     # (the run's slots: its input's first)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        for a in range(0, n, per):
            m = min(per, n - a)
            hin = hbuf if m == hbuf.n else st.ACT(hbuf.t[:m], m, H, W)
            in_rng, out_rng = (None, None) if self.ranges is None else (self._slot(0)[a:a + m], self._slot(1)[a:a + m])
            hs = e.head(x[a:a + m], sg, st.ACT, out=hin, in_rng=in_rng, out_rng=out_rng)
            if self.gate is not None:
                self.gate.acquire()
            ys = st.launch(hs, st, rows, per_launch=m, rng_offset=a, out_bufs=bufs, check=False)
            if self.gate is not None:
                self.gate.release()
                yield "stack"
            e.tail(ys, out=out[a:a + m])
        self.stack_launches += 1
        return out

    def _per_layer(self, x, sg, cal, sp):
        """The f-call layer by layer.  sp: the first layer writes sp16 and the last reads it (a calibrating call measures their ranges first)."""
        e = self.edges
        first = e.head_w is not None and x.is_cuda
        if first and sp:
            if cal:                                    # FFDNet: max |image| (the head adds sigma itself); then max |the head's own output|
                self._measured = True
                if e.ffdnet:
                    _hip.absmax(x, self._slot(0))
                e.head(x, sg, _hip.Sp16, in_rng=self._slot(0), out_exp=0, track=self._slot(1))
            h = e.head(x, sg, _hip.Sp16, in_rng=self._slot(0), out_rng=self._slot(1))
        elif first:
            h = e.head(x, sg)
        elif e.ffdnet:                                 # no HIP first layer: FFDNet's concatenate in torch; a plain network's stays on _run_stack
            n, _, H, W = x.shape
            h = torch.cat((sg.expand(n).view(-1, 1, 1, 1).expand(n, 1, H // 2, W // 2), F.pixel_unshuffle(x, 2)), 1)
        else:
            h = x
        if e.tail_w is not None and h.is_cuda:
            # FFDNet's fp32 tail takes the bias + ReLU of the layer in front of it; a plain network does not defer them
            defer = e.ffdnet and self.fused_epilogue and self.fast[-2][1] is not None and self.fast[-2][2]
            raw = self._run_stack(h, skip_last=True, skip_first=first, defer_last_epilogue=defer, native_out=sp)
            raw, b = raw if defer else (raw, None)
            return e.tail(raw, in_bias=b)
        h = self._run_stack(h, skip_first=first)       # (no HIP last layer: it runs with the others, FFDNet's pixel shuffle in torch)
        return F.pixel_shuffle(h, 2) if e.ffdnet else h


class _StackTimeout(Exception):
    """A wait inside a stack launch gave up (seen behind the first stack f-call of an eager reconstruction)."""


class _StackGate:
    """One stack launch on the device at a time, whatever stream it is on.  The workgroups of a stack launch wait for one another, so all of
    them have to be resident; two such launches dispatched side by side from two streams can each hold part of the CUs and starve the other
    until the waits give up.  Every stack launch of a grouped reconstruction therefore waits (on the device: a stream-side event wait, the
    host goes on) for the stack launch issued before it - a chain in issue order, no cycle."""

    def __init__(self):
        self.ev = None

    def acquire(self):
        if self.ev is not None:
            torch.cuda.current_stream().wait_event(self.ev)

    def release(self):
        self.ev = torch.cuda.Event()
        self.ev.record()


class DEQSCIEngine:
    GRAPH_AUTO_PIXELS = 4 * 256 * 256
    STACK_RETRY_CALLS = 16        # reconstructions on per-layer launches after a stack launch timed out, before the stack launch is tried again

    def __init__(self, denoiser, iterator="anderson", m=5, beta=1.0, lam=1e-2, max_iter=180, tol=1e-5,
                 fold_bn=True, extra_call=False, poll_residual=True, channels_last=None, fused_epilogue=True,
                 fused_edges=True, winograd=True, use_graph="auto", conv64="auto", conv64_f22_calls=None, act_range="data", blk32=True, anderson_arith="reference",
                 stack=True, stack_kernel="w16", groups=1, train_bn="module", train_realsn="module"):
        if iterator not in ("anderson", "picard"):
            raise ValueError(iterator)
        if not (groups == "auto" or (isinstance(groups, int) and 1 <= groups <= 2)):
            raise ValueError(f"groups={groups!r}: expected 'auto', 1 or 2")
        # groups: 2 (or "auto") = a batch of at least two stack slices (FFDNet: 2 x 32 images = 8 measurements of 256 x 256 x 8) is reconstructed
        # as TWO independent half batches, each on its own stream, issued alternately up to every stack launch (_reconstruct_grouped).
        # Measurements are independent problems and every kernel of the path is per measurement, so the result is bit-identical; what
        # changes is what the device overlaps: a stack launch holds every CU, but the dozen short kernels around it (first / last layer, K4,
        # the Gram kernels, the 6 x 6 solve, K7+K3 - a seventh of an f-call) of one half run beside the other half's.  MEASURED, and NOT the
        # default (1 = one stream): the short kernels are HBM- or latency-bound and run at the clock the power-capped stack launch leaves
        # behind; side by side they gain 50 us per f-call, the stack launches lose 13-36 us each waiting for CUs the other half's short
        # kernels still hold, and the outcome is between -4 % and +1.3 % from box to box and configuration to configuration
        # (profiles/r06_groups_*.txt).
        self.groups = groups
        self._ctor = dict(iterator=iterator, m=m, beta=beta, lam=lam, max_iter=max_iter, tol=tol, fold_bn=fold_bn, extra_call=extra_call,
                          channels_last=channels_last, fused_epilogue=fused_epilogue, fused_edges=fused_edges, winograd=winograd, conv64=conv64,
                          conv64_f22_calls=conv64_f22_calls, act_range=act_range, blk32=blk32, anderson_arith=anderson_arith, stack=stack,
                          stack_kernel=stack_kernel, train_bn=train_bn, train_realsn=train_realsn)
        self._net = denoiser
        self._kids, self._gate, self._grouped = None, None, False
        if anderson_arith not in ("float64", "reference"):
            raise ValueError(f"anderson_arith={anderson_arith!r}: expected 'reference' or 'float64'")
        # How alpha is computed.  "reference" (the default of every entry point: this class, the drop-in DEQFixedPoint / andersonexp, the CLI,
        # bench.py): the reference's own arithmetic for that step, solvers/new_equilibrium_utils_yaping.py:177-180 - G G^T as ONE fp32 torch.bmm
        # over the N = H W B elements, fp32 LU - by the build's own kernels: the new Gram row in the summation ORDER of that GEMM on the CPU
        # behind tests/golden (MKL sgemm on the build host's AVX-512 CPU: 16 interleaved FMA chains per entry, csrc/anderson.hip; no GEMM
        # library, capturable), the system formed and factorised in fp32 by K6 as sgesv does.  It exists because that order is not neutral on
        # BASELINE config 2: a 2^15-step chain absorbs the many small products of the heavy-tailed residuals, the diagonal of the Gram matrix
        # comes out 3-7e-6 too small, and that bias is what puts the reference's 180-iteration ensemble means where they are (DESIGN section
        # 5, "Config 2").  Another BLAS build or CPU orders the sum differently: "the reference's fp32 Gram" is a property of the machine the
        # reference ran on, and this is the build host's.  "float64": the Gram row accumulated in float64 from the fp32 block partials of K4,
        # the bordered system solved in float64 (K5+K6) - alpha to ~1e-8, 2-4 % faster at eight measurements per call, ~10 % at one; every
        # well-conditioned configuration is indifferent.  (Round 4's rocBLAS torch.bmm form lives in tools/config2_anderson_arith.py.)
        self.anderson_arith = anderson_arith
        if conv64 not in ("auto", "fast", "fast32", "f22", "f44", "s16"):
            raise ValueError(f"conv64={conv64!r}: expected 'auto', 'fast', 'fast32', 'f22', 'f44' or 's16'")
        # Which kernel runs the 64->64 layers (_hip.conv64_kernel_for): "fast" (= "auto") the faster of the split-fp16 direct convolution
        # on the f16 matrix cores and Winograd F(2x2,3x3) on the f32 ones, per launch; "fast32" fp32 MFMA arithmetic only (F(4x4,3x3) /
        # F(2x2,3x3)); "f22" / "f44" / "s16" one kernel always.  `conv64_f22_calls=K` additionally runs the first K f-calls on F(2x2,3x3).
        # What the choice does to the result was measured where it can matter - FFDNet under Anderson beyond ~30 iterations is chaotic
        #  - as 25-start ensembles over the six traffic measurements (tools/config2_ensemble.py,
        # profiles/r03_config2_ensembles.json; mean PSNR, standard error 0.004): reference 21.434 +- 0.004 (as it is 21.439 +- 0.005); F(2x2,3x3)
        # 21.420; split-fp16 21.428; F(2x2,3x3) for 40 f-calls then F(4x4,3x3) 21.417; MIOpen's direct fp32 convolution 21.410;
        # F(4x4,3x3) throughout 21.395.  Single measurements move by up to 0.09 dB under ANY change of arithmetic (the reference's own two
        # Gram variants: RMS 0.065 dB), so only the pooled mean separates kernels; it puts split-fp16 and F(2x2,3x3) together, nearest
        # the reference, which is why "auto" uses exactly those two.  Well-conditioned configurations (SimpleCNN, Picard, <= 30
        # iterations) agree to 1e-5 under every policy.
        self.conv64 = conv64
        self.conv64_policy = "fast" if conv64 == "auto" else conv64
        self.conv64_f22_calls = None if conv64_f22_calls is None else int(conv64_f22_calls)
        # act_range: "data" (default) = the power-of-two scales of the split-fp16 activations follow the data, measured on the device at
        # the first f-call of every reconstruction (fp32, the reference's arithmetic at equilibrium_solvers_yaping.py:397-420, is
        # scale-free; fp16 pieces are not); "fixed" = 2^8 throughout, the round-3 behaviour (activations of a few units).
        self.den = _Denoiser(denoiser, fold_bn=fold_bn, channels_last=channels_last, fused_epilogue=fused_epilogue,
                             fused_edges=fused_edges, winograd=winograd, conv64=self.conv64_policy, act_range=act_range, blk32=blk32, stack=stack,
                             stack_kernel=stack_kernel, train_bn=train_bn, train_realsn=train_realsn)
        self.train_bn = train_bn
        self.train_realsn = train_realsn
        self._solve_only = False
        self.den.f22_calls = self.conv64_f22_calls
        self.iterator = iterator
        self.m, self.beta, self.lam = int(m), float(beta), float(lam)
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.extra_call = extra_call
        self.poll_residual = poll_residual
        # True / False / "auto": replay a captured hipGraph when one reconstruction is at most GRAPH_AUTO_PIXELS
        # measurement-pixels (4 measurements of 256x256), i.e. when launch gaps are a visible share of the run
        self.use_graph = use_graph
        self._eager = True                # (False while a hipGraph capture records the launches: no host sync then)
        self._early_check = True          # (False in the halves of a grouped reconstruction: the parent looks at the time-out words once, at the end)
        self._stack_wanted, self._stack_off_for, self.stack_timeouts_total = bool(stack), 0, 0
        self._ws = {}
        self._graph = None
        self._snaps, self._trace, self._gt = None, False, None      # the options of the reconstruct() call in progress
        self.last_info = None

    # ------------------------------------------------------------------ buffers
    def _workspace(self, bsz, H, W, B, device):
        key = (bsz, H, W, B, str(device), self.iterator, self.m, self.max_iter, self._snaps, self._trace and self._gt is not None)
        ws = self._ws.get(key)
        if ws is None:
            m = self.m if self.iterator == "anderson" else 1
            rows = self.max_iter + 2
            ws = _hip.AndersonWorkspace(bsz, H * W * B, m, device, res_rows=rows)
            ws.xbuf = [torch.empty((bsz, B, H, W), device=device, dtype=torch.float32) for _ in range(2)]
            ws.z1 = torch.empty((bsz, B, H, W), device=device, dtype=torch.float32)
            ws.host_res = torch.full((rows, 1 + bsz), float('inf'), dtype=torch.float32).pin_memory()   # unfinished copy != converged
            # snapshots: one output buffer per horizon (a replayed hipGraph writes them in place; they are cloned out as rec is)
            ws.snap = {K: torch.empty((bsz, H, W, B), device=device, dtype=torch.float32) for K in (self._snaps or ())}
            ws.sq = ws.sq_ws = ws.gt = None
            if self._trace and self._gt is not None:
                # trace with a ground truth: sum of squared errors of every f-call's output, row = the f-call's residual row
                ws.sq = torch.zeros((rows, bsz), device=device, dtype=torch.float64)
                ws.sq_ws = _hip.sqerr_workspace(bsz, H * W * B, device)
                ws.gt = torch.empty((bsz, B, H, W), device=device, dtype=torch.float32)
            self._ws = {key: ws}          # one live shape at a time: history is bsz*m*N*8 bytes
        return ws

    # ------------------------------------------------------------------ one f-call = GAP -> denoise -> store -> solve
    def _denoise_steps(self, z1, call, calibrate=False):
        """(generator) den.run_steps where a gate is set (a half of a grouped reconstruction: it yields behind every stack launch), else
        den.run - which tests and tools wrap to see every f-call."""
        if self.den.gate is not None:
            return (yield from self.den.run_steps(z1, call, calibrate=calibrate))
        return self.den.run(z1, call, calibrate=calibrate)

    def _store_solve_steps(self, ws, x_in, call, slot, n_filled, n_solve, x_next, eps, res_row):
        out, is_noise = yield from self._denoise_steps(ws.z1, call, calibrate=(call == 0))     # (the first f-call measures the activations' ranges)
        if call == 1 and self._eager and self._early_check and self.den.stack and self.den.stack_launches and self.den.stack_timed_out():
            # the FIRST stack launch of the reconstruction: a wait that gave up (its workgroups were not all resident: somebody else holds CUs)
            # is seen here, one f-call in - not after 180 f-calls on invalid data.  One host sync per reconstruction (~0.1 ms of queue refill).
            raise _StackTimeout()
        out = _hip.f32c(out)
        ref = self.anderson_arith == "reference"               # the reference's fp32 Gram formed by K4 + K5 themselves (no GEMM library)
        if is_noise:
            _hip.residual_store(ws, ws.z1, out, x_in, slot, n_filled, x_next, ref=ref)
        else:
            _hip.residual_store(ws, out, None, x_in, slot, n_filled, x_next, ref=ref)
        _hip.anderson_solve(ws, slot, n_filled, n_solve, self.lam, eps, res_row, ref=ref)    # (+ lam I and the fp32 LU of :178-180 in K6)
        if ws.sq is not None:
            # trace: |clamp(F_k) - gt|^2 per measurement from the history slot K4 just wrote (csrc/trace.hip), into row k of the table
            _hip.sqerr_rows(ws.F[:, slot], ws.gt.view(ws.bsz, ws.N), out=ws.sq[res_row], clamp_x=True, workspace=ws.sq_ws)

    def _snapshot_steps(self, ws, x_last, call, phi, y, ps, K):
        """(generator) the result of the run with max_iter=K, formed as _enqueue_steps forms the final z = f(z*): f(x_last) as f-call
        number `call`, into ws.snap[K].  Advances nothing the main run reads later: sigma is indexed by `call`, the activation ranges
        are those of f-call 0, ws.z1 is rewritten by the next iteration, the history is untouched."""
        stale = self.den._stale
        _hip.gap_update(x_last, phi, y, ps, LAYOUT_BHW, out=ws.z1)
        out, is_noise = yield from self._denoise_steps(ws.z1, call)
        out = _hip.f32c(out)
        if is_noise:
            _hip.residual_out(ws.z1, out, LAYOUT_HWB, out=ws.snap[K])
        else:
            _hip.transpose(out, LAYOUT_HWB, out=ws.snap[K])
        if stale:                                             # (conv64_f22_calls: the ranges are measured by the main run's own first split-fp16 call)
            self.den._stale = True

    def _poll(self, ws, row):
        ws.host_res[row].copy_(ws.res[row], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def reconstruct(self, y, Phi, Phi_sum=None, initial_point=None, *, snapshots=None, trace=False, gt=None):
        """y (bsz,H,W), Phi (bsz|1,H,W,B) or (H,W,B) fp32 on the GPU -> reconstruction (bsz,H,W,B).
        `self.last_info` holds res (whole batch), per-sample res, iterations and f-call count.

        snapshots=(K1, K2, ...): also the reconstruction at those iteration horizons (strictly increasing, each smaller than max_iter)
        from this ONE run, one extra f-call each: last_info["snapshots"][K] = {"rec" (bsz,H,W,B), "res", "res_per_sample"} is what an
        engine with max_iter=K returns and reports, bit for bit (if the tolerance test stops the run before K, the run's own result).
        trace=True: last_info["trace"] = {"res" (n_calls,), "res_per_sample" (n_calls,bsz), "psnr" (n_calls,bsz) or None}, float64 numpy:
        the residual rows of the f-calls of the iteration (f-call k = row k; the closing z = f(z*) and the snapshots' f-calls have no
        row), copied back once at the end; with gt= (the ground truth, (bsz,H,W,B) on the device) also the PSNR of every f-call's output
        against it, per measurement, by harness.psnr's definition (csrc/trace.hip, no host sync).  Both are None when not asked for, and
        neither changes the result.  A call with snapshots or a trace runs ungrouped (groups=2 is ignored for it).  An invalid request
        raises ValueError before anything is launched."""
        snaps = check_snapshots(snapshots, self.max_iter, self.iterator)
        if gt is not None and not trace:
            raise ValueError("gt= is the ground truth of the trace's PSNR: pass trace=True with it")
        if gt is not None and not (isinstance(gt, torch.Tensor) and gt.dim() == 4 and isinstance(y, torch.Tensor) and gt.shape[0] == y.shape[0]
                                   and tuple(gt.shape[1:3]) == tuple(y.shape[1:3]) and gt.shape[3] == Phi.shape[-1]):
            raise ValueError(f"gt must be a (bsz,H,W,B) tensor matching y {tuple(getattr(y, 'shape', ()))} and Phi {tuple(getattr(Phi, 'shape', ()))}")
        if not (isinstance(y, torch.Tensor) and y.is_cuda):
            raise _hip.DeqsciHipError("DEQSCIEngine.reconstruct needs GPU tensors; there is no CPU path")
        if gt is not None and gt.device != y.device:
            raise ValueError(f"gt is on {gt.device}, y on {y.device}")
        self._snaps, self._trace, self._gt = snaps, bool(trace), (None if gt is None else _hip.f32c(gt))
        try:
            return self._reconstruct_checked(y, Phi, Phi_sum, initial_point)
        finally:
            self._snaps, self._trace, self._gt = None, False, None

    def _reconstruct_checked(self, y, Phi, Phi_sum, initial_point):
        with torch.cuda.device(y.device):          # events, stream sync and launches all on y's device
            if self._stack_off_for > 0:            # (a stack launch timed out a while ago: per-layer launches for STACK_RETRY_CALLS calls, then try again)
                self._stack_off_for -= 1
                if self._stack_off_for == 0 and self._stack_wanted:
                    self.den.stack, self.den.per_layer_w16, self._graph = True, False, None
            timed_out = 0
            try:
                rec = self._reconstruct(y, Phi, Phi_sum, initial_point)
                if self.den.stack and self.den.stack_launches and self._stack_timed_out():
                    raise _StackTimeout()          # (a replayed hipGraph, a grouped call, or a wait that gave up later than the first stack f-call)
            except _StackTimeout:
                # a stack launch waits for its own workgroups only - all resident when the device is ours.  A wait that gave up means it is
                # not (another process holds CUs): that result is invalid; redo it with a launch per layer, and stay there for a while
                import warnings
                warnings.warn("deqsci_amd: a wait inside a split-fp16 stack launch timed out (the device's CUs are shared with other work); "
                              f"redoing this call with one launch per layer and keeping that for the next {self.STACK_RETRY_CALLS} calls of this engine",
                              RuntimeWarning)
                self._stack_timed_out()            # (rearm every stack's words)
                self.den.stack = False
                self.den.per_layer_w16 = True      # (FFDNet under the Winograd kernel: per-layer launches of THAT kernel, the stack launch's bits)
                self.den.stack_launches = 0
                self._graph = None
                self._stack_off_for = self.STACK_RETRY_CALLS
                self.stack_timeouts_total += 1
                timed_out = 1
                rec = self._reconstruct(y, Phi, Phi_sum, initial_point)
            self.last_info["stack_launches"], self.den.stack_launches = self.den.stack_launches, 0
            self.last_info["stack_timeouts"] = timed_out     # 1: a stack launch of THIS call timed out (the result below is the per-layer redo)
            # what the run of 64->64 layers of the LAST f-call went out as (the kernel actually used, for every call)
            self.last_info["denoiser_path"] = (self._kids[0].den.last_path if (self._grouped and self._kids) else self.den.last_path)
            for option, (_, _, _, in_eval) in _Denoiser.TRAIN_OPTIONS.items():
                if getattr(self, option) == "device":
                    # what the option did for this call: "device" where the f-calls ran its kernels, else "module" and why
                    served = self.train_mode_on_device() == option
                    self.last_info[option] = "device" if served else "module"
                    self.last_info[option + "_reason"] = None if served else (self.den.train_why or f"the denoiser is not in train mode (net.eval(): {in_eval})")
            fallback = None
            if self.conv64 == "auto" and not math.isfinite(self.last_info["res"]) and bool(torch.isfinite(y).all()):
                # conv64="auto" promises the reference's fp32 range: a non-finite residual under the split-fp16 layers (already warned
                # about) is redone on the fp32 MFMA kernels - THIS call only (eagerly; a captured hipGraph and the policy of later,
                # unrelated inputs are left alone; every rank of a sharded job decides for its own call) - and last_info says so.  A run
                # that diverges by itself comes back non-finite again and is returned as it is.
                first = self.last_info.get("snapshots")
                saved = (self.conv64_policy, self.den.conv64, self.use_graph)
                self.conv64_policy = self.den.conv64 = self.den._policy = "fast32"
                self.use_graph = False
                try:
                    rec = self._reconstruct(y, Phi, Phi_sum, initial_point)
                finally:
                    self.conv64_policy, self.den.conv64, self.use_graph = saved
                    self.den._policy = saved[1]
                fallback = "fast32"
                if first:
                    # a run with max_iter=K is redone on fp32 only if ITS residual is not finite: a horizon whose residual was still finite
                    # in the first pass keeps that pass's snapshot (what the separate run returns), the others come from the redo
                    snaps = self.last_info["snapshots"]
                    for K, v in first.items():
                        if math.isfinite(v["res"]):
                            snaps[K] = v
            self.last_info["conv64_fallback"] = fallback
            # what the first f-call measured: max |activation| in front of every layer of the denoiser's stack, here the maximum over the
            # batch's images (the kernels use one range per image: den.ranges; 0 where no split-fp16 layer ran)
            rng = self._all_ranges()
            self.last_info["act_ranges"] = None if (rng is None or fallback) else rng.max(dim=1).values.tolist()
            return rec

    def _stack_timed_out(self):
        """(host sync) whether a wait inside a stack launch of this engine or of the halves of a grouped call gave up; rearms the words."""
        dens = [self.den] + [k.den for k in (self._kids or [])]
        return any([d.stack_timed_out() for d in dens])

    def _all_ranges(self):
        """(layers + 1, images) range slots of the last call (a grouped call: its halves' side by side)."""
        if self._grouped and self._kids:
            parts = [k.den.ranges for k in self._kids]
            return None if any(p is None for p in parts) else torch.cat(parts, dim=1)
        return self.den.ranges

    def _reconstruct(self, y, Phi, Phi_sum, initial_point):
        y = _hip.f32c(y)
        bsz, H, W = y.shape
        Phi4 = _hip.f32c(Phi if Phi.dim() == 4 else Phi.unsqueeze(0))
        B = Phi4.shape[3]
        if Phi4.shape[0] not in (1, bsz) or tuple(Phi4.shape[1:3]) != (H, W):
            raise _hip.DeqsciHipError(f"Phi {tuple(Phi.shape)} does not match y {tuple(y.shape)}")
        if Phi_sum is not None and Phi_sum.numel() == Phi4.shape[0] * H * W:
            Phi_sum = _hip.f32c(Phi_sum).view(Phi4.shape[0], H, W)
        else:
            Phi_sum = None
        if initial_point is not None:
            initial_point = _hip.f32c(initial_point)
        graph = self.use_graph if self.use_graph != "auto" else bsz * H * W <= self.GRAPH_AUTO_PIXELS
        self.den._refresh()
        # an f-call that moves module state - the BatchNorms' running buffers (and the batch statistics are those of the WHOLE f-call's batch),
        # a RealSNConv2d's weight_u and weight - is not replayed from a graph, which would not carry that state from call to call
        for moves, what in ((self.train_mode_on_device() == "train_bn", "train_bn='device' runs the denoiser's train-mode BatchNorm2d layers on the device, "
                             "and every f-call moves their running_mean / running_var / num_batches_tracked; such a net runs eagerly "
                             "(use_graph='auto' or False, or net.eval())"),
                            (self._train_mode_realsn(), "the denoiser has a train-mode RealSNConv2d, whose every call runs a power-iteration step on "
                             "its weight_u and weight buffers; such a net runs eagerly (use_graph='auto' or False, or net.eval())")):
            if moves and self.use_graph is True:
                raise ValueError("use_graph=True: " + what)
            graph = graph and not moves
        self._grouped = False
        extras = self._snaps is not None or self._trace
        plan = None if (graph or extras or self._solve_only or self.train_mode_on_device()) else self._group_plan(bsz, H, W, B, y.device)
        if plan is not None:
            rec = self._reconstruct_grouped(plan, y, Phi4, Phi_sum, initial_point)
            if rec is not None:
                return rec
        ws = self._workspace(bsz, H, W, B, y.device)
        self.den.prepare(self.max_iter + 4, y.device, n_img=bsz * B)
        if graph:
            rec = self._replay(ws, y, Phi4, Phi_sum, initial_point)
            if rec is not None:
                return rec
        rec, call, last, res_row = self._enqueue(ws, y, Phi4, Phi_sum, initial_point, self.poll_residual, self._gt)
        if extras:
            ws.host_res.copy_(ws.res, non_blocking=True)      # the whole residual table, once
        torch.cuda.current_stream().synchronize()
        r = ws.host_res[res_row]
        self.last_info = {"res": float(r[0]), "res_per_sample": r[1:].tolist(), "iterations": last,
                          "f_calls": call, "iterator": self.iterator, "graph": False}
        self._add_extras(ws, rec, last, res_row)
        self._warn_if_not_finite()
        return rec

    def train_mode_on_device(self):
        """The option ("train_bn", "train_realsn") under which the f-calls run a net in train mode on the device - each moves the module's
        buffers, the BatchNorms' running statistics or the RealSNConv2ds' weight_u and weight - or None."""
        return self.den.train_mode

    @torch.no_grad()
    def solve(self, y, Phi, Phi_sum=None, initial_point=None):
        """The iteration ALONE: z*, the iterate the reference's solver returns (new_equilibrium_utils_yaping.py:189, :222) - not f(z*), no
        closing call - as (bsz,H,W,B); last_info as reconstruct leaves it, "f_calls" = the calls of the loop.  What a training step's
        no-tape solve needs (DEQFixedPoint with engine_options["train_bn"] = "device"): the taped call f(z*) is the caller's."""
        self._solve_only = True
        try:
            return self.reconstruct(y, Phi, Phi_sum, initial_point)
        finally:
            self._solve_only = False

    def _train_mode_realsn(self):
        """True where an f-call mutates the denoiser: a RealSNConv2d in train mode (deqsci_amd.networks.simplecnn)."""
        from .networks.simplecnn import RealSNConv2d
        return isinstance(self._net, torch.nn.Module) and any(isinstance(m, RealSNConv2d) and m.training for m in self._net.modules())

    def _add_extras(self, ws, rec, last, res_row):
        """last_info["snapshots"] / ["trace"] of the call in progress from the workspace (the stream is synchronised and ws.host_res holds
        the whole table when either was asked for).  The f-calls behind the snapshots count in "f_calls"."""
        info = self.last_info
        info["snapshots"] = info["trace"] = None
        if self._snaps is not None:
            snaps = {}
            for K in self._snaps:
                k_last = K - 1                                # `last` of the run with max_iter=K (both iterators)
                if last < k_last:                             # the tolerance test stopped the run first: that run stops there too
                    snaps[K] = {"rec": rec, "res": info["res"], "res_per_sample": list(info["res_per_sample"])}
                    continue
                r = ws.host_res[k_last if self.iterator == "anderson" else K]
                snaps[K] = {"rec": ws.snap[K].clone(), "res": float(r[0]), "res_per_sample": r[1:].tolist()}
                info["f_calls"] += 1
            info["snapshots"] = snaps
        if self._trace:
            n = res_row + 1
            table = ws.host_res[:n].numpy().astype(np.float64)
            psnr = None
            if ws.sq is not None:
                with np.errstate(divide="ignore"):
                    psnr = 10.0 * np.log10(1.0 / (ws.sq[:n].cpu().numpy() / float(ws.N)))
            info["trace"] = {"res": table[:, 0].copy(), "res_per_sample": table[:, 1:].copy(), "psnr": psnr}

    # ------------------------------------------------------------------ two half batches on two streams
    def _group_plan(self, bsz, H, W, B, device):
        """[(lo, hi), (lo, hi)]: the measurements of the two halves of a grouped reconstruction, or None (groups=1; a batch of less than two
        stack slices; a denoiser whose f-call is not the sliced stack path).  A half is a whole number of stack slices."""
        if self.groups == 1 or bsz < 2:
            return None
        self.den.prepare(self.max_iter + 4, device)
        per = self.den.stack_slice(bsz, B, H, W, device)
        if per is None or per % B or bsz * B < 2 * per:
            return None
        mps = per // B                                        # measurements per stack slice
        first = (-(-(-(-bsz // mps)) // 2)) * mps             # ceil(slices / 2) slices
        return [(0, first), (first, bsz)]

    def _make_kids(self, n, device):
        if self._kids is None or len(self._kids) != n or self._kids[0].stream.device != torch.device(device):
            self._gate = _StackGate()
            self._kids = []
            for _ in range(n):
                kid = DEQSCIEngine(self._net, use_graph=False, groups=1, poll_residual=False, **self._ctor)
                kid.den.gate = self._gate
                kid._early_check = False
                kid.stream = torch.cuda.Stream(device=device)
                self._kids.append(kid)
        for kid in self._kids:                                # (what callers set on an engine after building it)
            for name in ("m", "beta", "lam", "max_iter", "tol", "extra_call", "iterator", "anderson_arith", "conv64", "conv64_policy", "conv64_f22_calls"):
                setattr(kid, name, getattr(self, name))
            for name in ("stack", "stack_per_launch", "slice_edges", "f22_calls", "conv64", "stack_kernel", "blk32"):
                setattr(kid.den, name, getattr(self.den, name))
        return self._kids

    def _reconstruct_grouped(self, plan, y, Phi4, Phi_sum, initial_point):
        """The batch as independent half batches (plan), each on its own stream with its own workspace and activation buffers, their
        f-calls issued alternately; the stack launches of the two streams are chained by events (_StackGate).  Bit-identical to the
        one-stream path (every kernel of the path is per measurement).  The tolerance test of new_equilibrium_utils_yaping.py:184-186 is
        over the WHOLE batch: the halves run max_iter iterations, and if any half's own residual ever fell below tol (then, and only then,
        the whole batch's might have: sqrt(sum g) / (eps + sqrt(sum f)) >= tol whenever that holds for every half) the call is redone on
        the one-stream path, which stops where the reference stops -> None.  Never on the reference's data."""
        bsz, H, W = y.shape
        B = Phi4.shape[3]
        dev = y.device
        kids = self._make_kids(len(plan), dev)
        main = torch.cuda.current_stream()
        gens, wss = [], []
        try:
            for kid, (lo, hi) in zip(kids, plan):
                kid.stream.wait_stream(main)
                with torch.cuda.stream(kid.stream):
                    ws = kid._workspace(hi - lo, H, W, B, dev)
                    # K4 and the reference Gram's first pass stay TWO launches here: the blocks of the fused launch wait for one another inside
                    # it (a bounded look-back), and a stack launch of the other half that takes the CUs in the middle of its dispatch leaves
                    # them spinning on blocks that cannot start - measured: stack launches 1017 -> 1053 us, the grouped step slower than one stream
                    ws.ref_fusable = False
                    kid.den.prepare(self.max_iter + 4, dev, n_img=(hi - lo) * B)
                    kid.den.stack_launches = 0
                    wss.append(ws)
                    gens.append(kid._enqueue_steps(ws, y[lo:hi], Phi4 if Phi4.shape[0] == 1 else Phi4[lo:hi],
                                                   None if Phi_sum is None else (Phi_sum if Phi_sum.shape[0] == 1 else Phi_sum[lo:hi]),
                                                   None if initial_point is None else initial_point[lo:hi], False))
            # One ROUND = every half issued up to (and including) its next stack launch; then every half that launched one makes its stream
            # wait for the LAST stack launch of the round before it goes on.  Without that wait the order on the device is a race at every
            # stack's end - the finished half's own short kernels (next in ITS stream) against the other half's stack launch (released by an
            # event) - and it locks into the pattern stack A | A's short kernels | stack B | B's short kernels: nothing overlaps, and the
            # halved launches make it SLOWER than one stream (443 against 426 ms per step).  With it: stack A | stack B | the short
            # kernels of both halves side by side | stack A | ...
            done = [None] * len(kids)
            alive = list(range(len(kids)))
            while alive:
                stacked = []
                for i in list(alive):
                    with torch.cuda.stream(kids[i].stream):
                        try:
                            while next(gens[i]) != "stack":
                                pass
                            stacked.append(i)
                        except StopIteration as fin:
                            done[i] = fin.value
                            alive.remove(i)
                if stacked and self._gate.ev is not None:
                    for i in stacked:
                        kids[i].stream.wait_event(self._gate.ev)
            rec = torch.empty((bsz, H, W, B), dtype=torch.float32, device=dev)
            norms = []
            for kid, ws, (lo, hi), (r, call, last, res_row) in zip(kids, wss, plan, done):
                with torch.cuda.stream(kid.stream):
                    ws.host_res.copy_(ws.res, non_blocking=True)
                    norms.append(ws.gram[:(hi - lo) * 80].view(hi - lo, 80)[:, 64:66].to("cpu", non_blocking=True))     # |F_k|^2, |G_k|^2 of the last solve (fp64)
                main.wait_stream(kid.stream)
                rec[lo:hi].copy_(r)
                r.record_stream(main)
            main.synchronize()
        except BaseException:
            for g in gens:
                g.close()
            torch.cuda.synchronize(dev)
            raise
        _, call, last, res_row = done[0]
        first = 2 if self.iterator == "anderson" else 1
        for ws in wss:
            if bool((ws.host_res[first:res_row, 0] < self.tol).any()):
                return None
        # the whole batch's residual of the last iteration, as K6's last block folds it: the samples' float64 norms added in sample order
        sf = sg = 0.0
        for nm in norms:
            for k in range(nm.shape[0]):
                sf += float(nm[k, 0])
                sg += float(nm[k, 1])
        eps = float(np.float32(1e-5 if self.iterator == "anderson" else 1e-7))     # (K6 takes eps as a float)
        res = float(np.float32(math.sqrt(sg) / (eps + math.sqrt(sf))))
        self._grouped = True
        self.den.stack_launches += max(k.den.stack_launches for k in kids)
        self.last_info = {"res": res, "res_per_sample": [v for ws in wss for v in ws.host_res[res_row, 1:].tolist()], "iterations": last,
                          "f_calls": call, "iterator": self.iterator, "graph": False, "groups": [list(p) for p in plan]}
        self._add_extras(None, rec, last, res_row)            # (never asked for on this path: both keys None)
        self._warn_if_not_finite()
        return rec

    def _warn_if_not_finite(self):
        """A non-finite residual is what an fp16 overflow inside the split-fp16 layers (activations beyond |x| = 255.9: csrc/conv_s16.hip keeps
        it inf / NaN all the way to the output on purpose) looks like from here - as does a genuinely diverging run.  Say so, loudly."""
        import warnings
        if not math.isfinite(self.last_info["res"]) and self.conv64_policy in ("fast", "s16"):
            what = ("redoing this call with conv64='fast32' (fp32 MFMA kernels, no such limit; last_info['conv64_fallback'])" if self.conv64 == "auto"
                    else "rerun with conv64='fast32' (fp32 MFMA kernels, no such limit)")
            how = ("16 x the largest activation of the first f-call, which set the scales" if self.den.act_range == "data" and self.den.ranges is not None
                   else "|x| >= 255.9 under act_range='fixed'; inputs are expected in [0, 1]")
            warnings.warn("DEQSCIEngine: the reconstruction's residual is not finite.  If the iteration itself is not diverging, an activation of "
                          f"the denoiser has left fp16's range inside the split-fp16 64->64 layers ({how}): " + what + ".", RuntimeWarning, stacklevel=4)

    def _enqueue(self, ws, y, Phi4, Phi_sum, initial_point, poll, gt=None):
        """Every launch of one reconstruction on the current stream.  poll: True = lagged residual read-back with early stop,
        False = one read-back at the end, None = no host traffic at all (what a hipGraph capture records)."""
        return _exhaust(self._enqueue_steps(ws, y, Phi4, Phi_sum, initial_point, poll, gt))

    def _enqueue_steps(self, ws, y, Phi4, Phi_sum, initial_point, poll, gt=None):
        """_enqueue as a generator that yields behind every f-call (a grouped reconstruction issues the f-calls of its halves alternately);
        returns what _enqueue returns.  gt: the trace's ground truth (bsz,H,W,B), transposed once to the loop's planar order."""
        self._eager = poll is not None
        if ws.gt is not None:
            _hip.transpose(gt, LAYOUT_BHW, out=ws.gt)
        phi = _hip.transpose(Phi4, LAYOUT_BHW)
        ps = Phi_sum if Phi_sum is not None else _hip.phi_sum(phi, LAYOUT_BHW)
        if initial_point is None:
            _hip.sci_adjoint(y, phi, LAYOUT_BHW, out=ws.xbuf[0])
        else:
            _hip.transpose(initial_point, LAYOUT_BHW, out=ws.xbuf[0])
        if self.iterator == "anderson":
            x_last, call, last = yield from self._anderson(ws, y, phi, ps, poll)
        else:
            x_last, call, last = yield from self._picard(ws, y, phi, ps, poll)
        res_row = last
        if self._solve_only:
            return _hip.transpose(x_last, LAYOUT_HWB), call, last, res_row
        # z = f(z*)  (new_equilibrium_utils_yaping.py:268)
        _hip.gap_update(x_last, phi, y, ps, LAYOUT_BHW, out=ws.z1)
        out, is_noise = yield from self._denoise_steps(ws.z1, call)
        out = _hip.f32c(out)
        rec = _hip.residual_out(ws.z1, out, LAYOUT_HWB) if is_noise else _hip.transpose(out, LAYOUT_HWB)
        call += 1
        # dead f0 = f(z) of :271-272 - not dead for a train-mode RealSNConv2d: the call advances weight_u, as it does in the reference
        if self.extra_call or self._train_mode_realsn() or self.train_mode_on_device():
            yield "fcall"
            zt = _hip.transpose(rec, LAYOUT_BHW)
            _hip.gap_update(zt, phi, y, ps, LAYOUT_BHW, out=ws.z1)
            yield from self._denoise_steps(ws.z1, call)
            call += 1
        return rec, call, last, res_row

    # ------------------------------------------------------------------ hipGraph replay of a whole reconstruction
    def _replay(self, ws, y, Phi4, Phi_sum, initial_point):
        """-> reconstruction, or None when this call has to take the eager path (first call of a shape: it warms every
        kernel up; or the tolerance test fired inside the replayed run)."""
        key = (tuple(y.shape), tuple(Phi4.shape), Phi_sum is not None, initial_point is not None, self.den._wkey, self.extra_call, self._solve_only,
               None if self.den.sigma_table is None else self.den.sigma_table.data_ptr(), self._snaps, self._trace and self._gt is not None)
        g = self._graph
        if g is None or g["key"] != key or g["ws"] is not ws:
            # (the graph holds the workspace it was captured on: its nodes carry that workspace's raw pointers)
            self._graph = {"key": key, "ws": ws, "graph": None}
            return None                                       # eager now, capture on the next call with this key
        if g["graph"] is None:
            g["y"], g["Phi4"] = y.clone(), Phi4.clone()
            g["ps"] = None if Phi_sum is None else Phi_sum.clone()
            g["x0"] = None if initial_point is None else initial_point.clone()
            g["gt"] = None if ws.gt is None else self._gt.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            c0 = self.den.stack_launches
            with torch.cuda.graph(graph):
                g["rec"], g["call"], g["last"], g["res_row"] = self._enqueue(ws, g["y"], g["Phi4"], g["ps"], g["x0"], None, g["gt"])
            g["graph"], g["stack_n"] = graph, self.den.stack_launches - c0
        else:
            self.den.stack_launches += g["stack_n"]
            g["y"].copy_(y)
            g["Phi4"].copy_(Phi4)
            if Phi_sum is not None:
                g["ps"].copy_(Phi_sum)
            if initial_point is not None:
                g["x0"].copy_(initial_point)
            if g["gt"] is not None:
                g["gt"].copy_(self._gt)
        g["graph"].replay()
        rec = g["rec"].clone()
        ws.host_res.copy_(ws.res, non_blocking=True)          # the whole residual table, once
        torch.cuda.current_stream().synchronize()
        first = 2 if self.iterator == "anderson" else 1
        table = ws.host_res[first:g["res_row"], 0]
        if bool((table < self.tol).any()):                    # the reference would have stopped earlier: redo it eagerly
            return None
        r = ws.host_res[g["res_row"]]
        self.last_info = {"res": float(r[0]), "res_per_sample": r[1:].tolist(), "iterations": g["last"],
                          "f_calls": g["call"], "iterator": self.iterator, "graph": True}
        self._add_extras(ws, rec, g["last"], g["res_row"])
        self._warn_if_not_finite()
        return rec

    # ------------------------------------------------------------------ Anderson (new_equilibrium_utils_yaping.py:153-189)
    def _anderson(self, ws, y, phi, ps, poll):
        m, max_iter = self.m, self.max_iter
        if m < 2:
            raise IndexError("index 1 is out of bounds for dimension 1 with size %d" % m)   # X[:, 1] at :163
        xb = ws.xbuf
        # f-calls 1, 2 fill slots 0, 1 (:162-163)
        _hip.gap_update(xb[0], phi, y, ps, LAYOUT_BHW, out=ws.z1)
        yield from self._store_solve_steps(ws, xb[0], 0, 0, 1, 0, xb[1], 1e-5, 0)
        yield "fcall"
        _hip.gap_update(xb[1], phi, y, ps, LAYOUT_BHW, out=ws.z1)
        yield from self._store_solve_steps(ws, xb[1], 1, 1, 2, 2, None, 1e-5, 1)
        yield "fcall"
        if max_iter <= 2:
            raise UnboundLocalError("local variable 'res' referenced before assignment")      # :189 with the loop skipped
        last, prev_ev = None, None
        for k in range(2, max_iter):
            n = min(k, m)
            x = xb[k % 2]
            _hip.anderson_mix_gap(ws, self.beta, n, phi, y, ps, x, ws.z1, LAYOUT_BHW)
            nf = min(k + 1, m)
            yield from self._store_solve_steps(ws, x, k, k % m, nf, nf, None, 1e-5, k)
            last = k
            yield "fcall"
            if k + 1 in ws.snap:                              # X_k is overwritten two iterations on: the horizon k + 1 result now, as f-call k + 1
                yield from self._snapshot_steps(ws, x, k + 1, phi, y, ps, k + 1)
                yield "fcall"
            if poll:
                ev = self._poll(ws, k)
                if prev_ev is not None:
                    prev_ev.synchronize()
                    if float(ws.host_res[k - 1, 0]) < self.tol:
                        last = k - 1
                        break
                prev_ev = ev
        if poll is not None and (not poll or last == max_iter - 1):
            ws.host_res[last].copy_(ws.res[last], non_blocking=True)
        return xb[last % 2], last + 1, last

    # ------------------------------------------------------------------ Picard (new_equilibrium_utils_yaping.py:213-222)
    def _picard(self, ws, y, phi, ps, poll):
        xb = ws.xbuf
        _hip.gap_update(xb[0], phi, y, ps, LAYOUT_BHW, out=ws.z1)
        yield from self._store_solve_steps(ws, xb[0], 0, 0, 1, 0, xb[1], 1e-7, 0)           # f0 = f(x0)
        yield "fcall"
        if self.max_iter <= 0:
            if poll is not None:
                ws.host_res[0].copy_(ws.res[0], non_blocking=True)
            return xb[1], 1, 0
        last, prev_ev = None, None
        for k in range(self.max_iter):
            x, nxt = xb[(k + 1) % 2], xb[k % 2]
            _hip.gap_update(x, phi, y, ps, LAYOUT_BHW, out=ws.z1)
            yield from self._store_solve_steps(ws, x, k + 1, 0, 1, 0, nxt, 1e-7, k + 1)
            last = k
            yield "fcall"
            if k + 1 in ws.snap:                              # the run with max_iter = k + 1 returns f(nxt) as f-call k + 2
                yield from self._snapshot_steps(ws, nxt, k + 2, phi, y, ps, k + 1)
                yield "fcall"
            if poll:
                ev = self._poll(ws, k + 1)
                if prev_ev is not None:
                    prev_ev.synchronize()
                    if float(ws.host_res[k, 0]) < self.tol:
                        last = k - 1
                        break
                prev_ev = ev
        if poll is not None and (not poll or last == self.max_iter - 1):
            ws.host_res[last + 1].copy_(ws.res[last + 1], non_blocking=True)
        return xb[last % 2], last + 2, last + 1
