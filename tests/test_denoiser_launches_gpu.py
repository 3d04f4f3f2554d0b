"""What an f-call of engine._Denoiser sends to the device, pinned launch by launch: the C entry points of _hip.SIGNATURES with their
arguments, in order, recorded on the loaded library object itself - below every layer of the Python that picks them (_route, the
edge-layer record, _sliced, _per_layer), so that a change of that Python which keeps these lists keeps the f-call.

Per launch: the entry's name, every integer argument (n, H, W, relu, exponents, n_layers, strides) and, for every pointer, None (a null
pointer; the default stream), "r+<bytes>" (a range slot: its offset from den.ranges) or "p" (any other address: activations, weights,
tables - not noted).  PINNED is what run_case() recorded for every case on the commit before the edge layers of the two families were
merged into one description (printed entry by entry, pasted here), and has not been touched since.

The shapes are the smallest that still slice and are ragged against both block tiles (16 x 32 of the direct kernel, 8 x 64 of the
Winograd one): three images - stack_per_launch=2 makes the second slice one image at an offset into the batch and its range slots -
with 64->64 layers of 24 x 40 pixels.  Shapes this small take F(2x2,3x3) under the default policy, so the cases pin the split-fp16
kernels with _hip.FORCE_CONV64 as tests/test_dncnn17_gpu.py does, unless they say otherwise.  Nothing waits and nothing times out here:
the state behind a stack time-out is set by hand.

The three train-mode cases (train_bn="device" on FFDNet and on DnCNN-17, train_realsn="device" on RealSN_SimpleCNN; no kernel pinned:
_hip.FORCE_CONV64 would override their policy "fast32") were pinned later, on the commit before the engine's two train-mode refreshes
and routes were gathered into one - what THAT commit recorded, never what the code behind it records.  Each gets a net of its own: these
f-calls move the module's buffers."""
import contextlib
import functools
import os

import pytest
import torch

from deqsci_amd import _hip, checkpoint
from deqsci_amd.cli import build_pipeline
from deqsci_amd.engine import DEQSCIEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
DNCNN17 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dncnn_noise15.npz")
# family -> (build_pipeline's denoiser, weights, shape of z: FFDNet's 64->64 layers run at half resolution)
FAMILIES = {"ffdnet": ("ffdnet", checkpoint.shipped("ffdnet_gray"), (1, 3, 48, 80)),
            "dncnn17": ("DnCNN", DNCNN17, (1, 3, 24, 40)),
            "cnn": ("SimpleCNN", checkpoint.shipped("cnn"), (1, 3, 24, 40)),
            "rsn": ("RealSN_SimpleCNN", checkpoint.shipped("rsn_cnn"), (1, 3, 24, 40))}
TIMED_OUT = {"stack": False, "per_layer_w16": True}                 # (what the engine sets behind a stack time-out)


def case(family, route, last_path, pin="s16", cal=False, n_img=3, ctor=None, after=None, train=False):
    """route: what _Denoiser._route answers for the recorded f-call; last_path: den.last_path behind it; pin: _hip.FORCE_CONV64; cal: the
    recorded f-call is the calibrating one (else the one behind it); n_img: prepare()'s (None: a bare prepare(n_calls, device)); ctor:
    DEQSCIEngine's keywords; after: attributes set on the denoiser after prepare(); train: a fresh net in train mode."""
    return dict(family=family, route=route, last_path=last_path, pin=pin, cal=cal, n_img=n_img, ctor=ctor or {}, after=after or {}, train=train)


CASES = {
    "ffdnet-calibrating": case("ffdnet", "sp16 per layer", "per layer", cal=True),
    "ffdnet-w16-stack": case("ffdnet", "w16 stack launch", "w16 stack launch"),
    "ffdnet-s16-stack": case("ffdnet", "s16 stack launch", "s16 stack launch", ctor={"stack_kernel": "s16"}),
    "ffdnet-no-stack": case("ffdnet", "sp16 per layer", "per layer", ctor={"stack": False}),
    "ffdnet-timed-out": case("ffdnet", "w16 per layer", "w16 per layer (behind a stack time-out)", after=TIMED_OUT),
    "ffdnet-unsliced-stack": case("ffdnet", "sp16 per layer", "per layer", after={"slice_edges": False}),
    "ffdnet-no-pin": case("ffdnet", "per layer", "per layer", pin=None),
    "ffdnet-torch-edges": case("ffdnet", "per layer", "per layer", ctor={"fused_edges": False}),
    "dncnn17-calibrating": case("dncnn17", "sp16 per layer", "per layer", cal=True),
    "dncnn17-w16-stack": case("dncnn17", "w16 stack launch", "w16 stack launch"),
    "dncnn17-s16-stack": case("dncnn17", "s16 stack launch", "s16 stack launch", ctor={"stack_kernel": "s16"}),
    "dncnn17-timed-out": case("dncnn17", "w16 per layer", "w16 per layer (behind a stack time-out)", after=TIMED_OUT),
    "dncnn17-bare-prepare": case("dncnn17", "w16 per layer", "w16 per layer", n_img=None),
    "cnn-w16-per-layer": case("cnn", "w16 per layer", "w16 per layer"),
    "cnn-s16": case("cnn", "sp16 per layer", "per layer", ctor={"stack_kernel": "s16"}),
    "cnn-min-layers-2": case("cnn", "w16 per layer", "w16 per layer", after={"STACK_MIN_LAYERS": 2}),
    "cnn-no-pin": case("cnn", "per layer", "per layer", pin=None),
    "cnn-torch-edges": case("cnn", "layers", "per layer", ctor={"fused_edges": False}),
    "ffdnet-train-bn": case("ffdnet", "train bn per layer", "train bn per layer", pin=None, ctor={"train_bn": "device"}, train=True),
    "dncnn17-train-bn": case("dncnn17", "train bn per layer", "train bn per layer", pin=None, ctor={"train_bn": "device"}, train=True),
    "rsn-train-realsn": case("rsn", "train realsn per layer", "train realsn per layer", pin=None, ctor={"train_realsn": "device"}, train=True),
}


@functools.lru_cache(maxsize=None)
def _net(family):
    kind, weights, _ = FAMILIES[family]
    return build_pipeline(kind, weights, 8)[0].nonlinear_op


@contextlib.contextmanager
def recording(den):
    """Every call of an entry of _hip.SIGNATURES on the loaded library, noted as described above and then made."""
    lib, log, saved = _hip.load(), [], {}

    def note(arg, kind):
        if kind in (_hip._int, _hip._i64):
            return int(arg)
        if kind is _hip._f32 or kind is _hip._f64:
            return float(arg)
        if not arg:
            return None
        base = None if den.ranges is None else den.ranges.data_ptr()
        if base is not None and isinstance(arg, int) and base <= arg < base + 4 * den.ranges.numel():
            return f"r+{arg - base}"
        return "p"

    def wrapper(name, fn, kinds):
        def call(*args):
            log.append((name,) + tuple(note(a, k) for a, k in zip(args, kinds)))
            return fn(*args)
        return call

    for name, kinds in _hip.SIGNATURES.items():
        saved[name] = getattr(lib, name)
        setattr(lib, name, wrapper(name, saved[name], kinds))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def run_case(name):
    """-> (the launches of the case's f-call, its output, the denoiser, the route of that f-call)."""
    c = CASES[name]
    net, shape = (_net.__wrapped__(c["family"]).train() if c["train"] else _net(c["family"])), FAMILIES[c["family"]][2]
    z = torch.rand(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(sum(shape)))
    old, _hip.FORCE_CONV64 = _hip.FORCE_CONV64, c["pin"]
    try:
        den = DEQSCIEngine(net, max_iter=8, use_graph=False, **c["ctor"]).den
        if c["n_img"] is None:
            den.prepare(16, DEV)
        else:
            den.prepare(16, DEV, n_img=c["n_img"])
        den.stack_per_launch = 2
        for k, v in c["after"].items():
            setattr(den, k, v)
        if not c["cal"]:
            den.run(z, 0, calibrate=True)                           # (the first f-call of a reconstruction: it measures the ranges)
        with recording(den) as log:
            out = den.run(z, 0, calibrate=True)[0] if c["cal"] else den.run(z, 1)[0]
        route = den._route(shape[0] * shape[1], shape[2], shape[3], z.device, den.conv64, c["cal"])
        assert not den.stack_timed_out()
        return log, out, den, route
    finally:
        _hip.FORCE_CONV64 = old


@pytest.mark.parametrize("name", list(CASES))
def test_fcall_launches_are_pinned(name):
    log, out, den, route = run_case(name)
    for entry in log:
        print(entry)
    assert route == CASES[name]["route"] and den.last_path == CASES[name]["last_path"]
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert log == PINNED[name]


PINNED = {
    'ffdnet-calibrating': [
        ('deqsci_absmax_f32', 'p', 3, 3840, 'r+0', None),
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 3, 24, 40, 14, 'r+0', 8, None, 0, 'r+12', None),
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 3, 24, 40, 14, 'r+0', 8, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 12, 'r+12', 8, None, 0, 'r+24', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+24', 8, None, 0, 'r+36', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+24', 8, 'r+36', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+36', 8, None, 0, 'r+48', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+36', 8, 'r+48', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+48', 8, None, 0, 'r+60', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 12, 'r+60', 8, None, 0, 'r+72', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+60', 8, 'r+72', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+72', 8, None, 0, 'r+84', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+72', 8, 'r+84', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+84', 8, None, 0, 'r+96', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+84', 8, 'r+96', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 12, 'r+96', 8, None, 0, 'r+108', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+96', 8, 'r+108', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+108', 8, None, 0, 'r+120', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+108', 8, 'r+120', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+120', 8, None, 0, 'r+132', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+120', 8, 'r+132', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+132', 8, None, 0, 'r+144', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+132', 8, 'r+144', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+144', 8, None, 0, 'r+156', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+144', 8, 'r+156', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+156', 8, None, 0, 'r+168', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+156', 8, 'r+168', 8, None, 0, None, None, None),
        ('deqsci_ffdnet_tail_split16', 'p', 'p', 'p', 3, 24, 40, 15, 'r+168', 8, None),
    ],
    'ffdnet-w16-stack': [
        ('deqsci_ffdnet_head_p32', 'p', 'p', 'p', 0, 'p', 2, 24, 40, 14, 'r+0', 8, 'r+12', 8, None),
        ('deqsci_conv3x3_c64_wino16_stack', 'p', 'p', 'p', 'p', 13, 2, 24, 40, 'r+12', 3, 8, 8, 'p', None, None, None),
        ('deqsci_ffdnet_tail_p32', 'p', 'p', 'p', 2, 24, 40, 15, 'r+168', 8, None),
        ('deqsci_ffdnet_head_p32', 'p', 'p', 'p', 0, 'p', 1, 24, 40, 14, 'r+8', 8, 'r+20', 8, None),
        ('deqsci_conv3x3_c64_wino16_stack', 'p', 'p', 'p', 'p', 13, 1, 24, 40, 'r+20', 3, 8, 8, 'p', None, None, None),
        ('deqsci_ffdnet_tail_p32', 'p', 'p', 'p', 1, 24, 40, 15, 'r+176', 8, None),
    ],
    'ffdnet-s16-stack': [
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 2, 24, 40, 14, 'r+0', 8, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 13, 2, 24, 40, 'r+12', 3, 8, 8, 'p', None, None, None),
        ('deqsci_ffdnet_tail_split16', 'p', 'p', 'p', 2, 24, 40, 15, 'r+168', 8, None),
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 1, 24, 40, 14, 'r+8', 8, 'r+20', 8, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 13, 1, 24, 40, 'r+20', 3, 8, 8, 'p', None, None, None),
        ('deqsci_ffdnet_tail_split16', 'p', 'p', 'p', 1, 24, 40, 15, 'r+176', 8, None),
    ],
    'ffdnet-no-stack': [
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 3, 24, 40, 14, 'r+0', 8, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+24', 8, 'r+36', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+36', 8, 'r+48', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+60', 8, 'r+72', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+72', 8, 'r+84', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+84', 8, 'r+96', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+96', 8, 'r+108', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+108', 8, 'r+120', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+120', 8, 'r+132', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+132', 8, 'r+144', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+144', 8, 'r+156', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+156', 8, 'r+168', 8, None, 0, None, None, None),
        ('deqsci_ffdnet_tail_split16', 'p', 'p', 'p', 3, 24, 40, 15, 'r+168', 8, None),
    ],
    'ffdnet-timed-out': [
        ('deqsci_ffdnet_head_p32', 'p', 'p', 'p', 0, 'p', 3, 24, 40, 14, 'r+0', 8, 'r+12', 8, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+24', 8, 'r+36', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+36', 8, 'r+48', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+60', 8, 'r+72', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+72', 8, 'r+84', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+84', 8, 'r+96', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+96', 8, 'r+108', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+108', 8, 'r+120', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+120', 8, 'r+132', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+132', 8, 'r+144', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+144', 8, 'r+156', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+156', 8, 'r+168', 8, None, None, None),
        ('deqsci_ffdnet_tail_p32', 'p', 'p', 'p', 3, 24, 40, 15, 'r+168', 8, None),
    ],
    'ffdnet-unsliced-stack': [
        ('deqsci_ffdnet_head_split16', 'p', 'p', 'p', 0, 'p', 3, 24, 40, 14, 'r+0', 8, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 13, 2, 24, 40, 'r+12', 3, 8, 8, 'p', None, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 13, 1, 24, 40, 'r+20', 3, 8, 8, 'p', None, None, None),
        ('deqsci_ffdnet_tail_split16', 'p', 'p', 'p', 3, 24, 40, 15, 'r+168', 8, None),
    ],
    'ffdnet-no-pin': [
        ('deqsci_ffdnet_head_f32', 'p', 'p', 'p', 0, 'p', 3, 24, 40, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_ffdnet_tail_f32', 'p', 'p', None, 'p', 3, 24, 40, None),
    ],
    'ffdnet-torch-edges': [
        ('deqsci_f32_to_split16', 'p', 'p', 3, 24, 40, 'r+12', 8, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+24', 8, 'r+36', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+36', 8, 'r+48', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+60', 8, 'r+72', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+72', 8, 'r+84', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+84', 8, 'r+96', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 12, 'r+96', 8, 'r+108', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+108', 8, 'r+120', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+120', 8, 'r+132', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+132', 8, 'r+144', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+144', 8, 'r+156', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+156', 8, None, 8, None, 1, None, None, None),
    ],
    'dncnn17-calibrating': [
        ('deqsci_conv3x3_c1_to_64_sp16', 'p', 'p', 'p', 3, 24, 40, 1, None, 0, 'r+12', None),
        ('deqsci_conv3x3_c1_to_64_sp16', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+12', 8, None, 0, 'r+24', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+12', 8, 'r+24', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 13, 'r+24', 8, None, 0, 'r+36', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+24', 8, 'r+36', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+36', 8, None, 0, 'r+48', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+36', 8, 'r+48', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+48', 8, None, 0, 'r+60', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 14, 'r+60', 8, None, 0, 'r+72', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+60', 8, 'r+72', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+72', 8, None, 0, 'r+84', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+72', 8, 'r+84', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+84', 8, None, 0, 'r+96', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+84', 8, 'r+96', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+96', 8, None, 0, 'r+108', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+96', 8, 'r+108', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+108', 8, None, 0, 'r+120', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+108', 8, 'r+120', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+120', 8, None, 0, 'r+132', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+120', 8, 'r+132', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+132', 8, None, 0, 'r+144', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+132', 8, 'r+144', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+144', 8, None, 0, 'r+156', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+144', 8, 'r+156', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+156', 8, None, 0, 'r+168', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+156', 8, 'r+168', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 15, 'r+168', 8, None, 0, 'r+180', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+168', 8, 'r+180', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', None, 3, 24, 40, 1, 16, 'r+180', 8, None, 0, 'r+192', 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 16, 'r+180', 8, 'r+192', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_to_1_split16', 'p', 'p', 'p', 3, 24, 40, 16, 'r+192', 8, None),
    ],
    'dncnn17-w16-stack': [
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 2, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_wino16_stack', 'p', 'p', 'p', 'p', 15, 2, 24, 40, 'r+12', 3, 8, 8, 'p', None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 2, 24, 40, 16, 'r+192', 8, None),
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 1, 24, 40, 1, 'r+20', 8, None, None),
        ('deqsci_conv3x3_c64_wino16_stack', 'p', 'p', 'p', 'p', 15, 1, 24, 40, 'r+20', 3, 8, 8, 'p', None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 1, 24, 40, 16, 'r+200', 8, None),
    ],
    'dncnn17-s16-stack': [
        ('deqsci_conv3x3_c1_to_64_sp16', 'p', 'p', 'p', 2, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 15, 2, 24, 40, 'r+12', 3, 8, 8, 'p', None, None, None),
        ('deqsci_conv3x3_c64_to_1_split16', 'p', 'p', 'p', 2, 24, 40, 16, 'r+192', 8, None),
        ('deqsci_conv3x3_c1_to_64_sp16', 'p', 'p', 'p', 1, 24, 40, 1, 'r+20', 8, None, None),
        ('deqsci_conv3x3_c64_split16_stack', 'p', 'p', 'p', 'p', 15, 1, 24, 40, 'r+20', 3, 8, 8, 'p', None, None, None),
        ('deqsci_conv3x3_c64_to_1_split16', 'p', 'p', 'p', 1, 24, 40, 16, 'r+200', 8, None),
    ],
    'dncnn17-timed-out': [
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+12', 8, 'r+24', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+24', 8, 'r+36', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+36', 8, 'r+48', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+60', 8, 'r+72', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+72', 8, 'r+84', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+84', 8, 'r+96', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+96', 8, 'r+108', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+108', 8, 'r+120', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+120', 8, 'r+132', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+132', 8, 'r+144', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+144', 8, 'r+156', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+156', 8, 'r+168', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+168', 8, 'r+180', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 16, 'r+180', 8, 'r+192', 8, None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 3, 24, 40, 16, 'r+192', 8, None),
    ],
    'dncnn17-bare-prepare': [
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+12', 8, 'r+24', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 13, 'r+24', 8, 'r+36', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+36', 8, 'r+48', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+48', 8, 'r+60', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+60', 8, 'r+72', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+72', 8, 'r+84', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+84', 8, 'r+96', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+96', 8, 'r+108', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 14, 'r+108', 8, 'r+120', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+120', 8, 'r+132', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+132', 8, 'r+144', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+144', 8, 'r+156', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+156', 8, 'r+168', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 15, 'r+168', 8, 'r+180', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', 'p', 'p', 3, 24, 40, 1, 16, 'r+180', 8, 'r+192', 8, None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 3, 24, 40, 16, 'r+192', 8, None),
    ],
    'cnn-w16-per-layer': [
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+24', 8, 'r+36', 8, None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 3, 24, 40, 16, 'r+36', 8, None),
    ],
    'cnn-s16': [
        ('deqsci_conv3x3_c1_to_64_sp16', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+24', 8, 'r+36', 8, None, 0, None, None, None),
        ('deqsci_conv3x3_c64_to_1_split16', 'p', 'p', 'p', 3, 24, 40, 16, 'r+36', 8, None),
    ],
    'cnn-min-layers-2': [
        ('deqsci_conv3x3_c1_to_64_p32', 'p', 'p', 'p', 3, 24, 40, 1, 'r+12', 8, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+12', 8, 'r+24', 8, None, None, None),
        ('deqsci_conv3x3_c64_wino16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+24', 8, 'r+36', 8, None, None, None),
        ('deqsci_conv3x3_c64_to_1_p32', 'p', 'p', 'p', 3, 24, 40, 16, 'r+36', 8, None),
    ],
    'cnn-no-pin': [
        ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 3, 24, 40, None),
    ],
    'cnn-torch-edges': [
        ('deqsci_f32_to_split16', 'p', 'p', 3, 24, 40, 'r+24', 8, None),
        ('deqsci_conv3x3_c64_split16', 'p', 'p', None, 'p', 3, 24, 40, 1, 12, 'r+24', 8, None, 8, None, 1, None, None, None),
    ],
    'ffdnet-train-bn': [
        ('deqsci_ffdnet_head_f32', 'p', 'p', 'p', 0, 'p', 3, 24, 40, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_ffdnet_tail_f32', 'p', 'p', None, 'p', 3, 24, 40, None),
    ],
    'dncnn17-train-bn': [
        ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 0, None),
        ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 2880, 'p', None),
        ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', None, 1, 2880, None),
        ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 3, 24, 40, None),
    ],
    'rsn-train-realsn': [
        ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 1, 64, 40, 40, 'p', None),
        ('deqsci_realsn_pack_f32', 'p', 'p', None, None, 1, 64, None),
        ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 64, 40, 40, 'p', None),
        ('deqsci_realsn_pack_f32', 'p', 'p', 'p', None, 64, 64, None),
        ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 64, 40, 40, 'p', None),
        ('deqsci_realsn_pack_f32', 'p', 'p', 'p', None, 64, 64, None),
        ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 1, 40, 40, 'p', None),
        ('deqsci_realsn_pack_f32', 'p', 'p', None, None, 64, 1, None),
        ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 3, 24, 40, 1, None),
        ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 3, 24, 40, None),
    ],
}
