"""What vjp.DenoiserParamGrads sends to the device, pinned launch by launch in every BatchNorm mode: the C entry points of _hip.SIGNATURES
with their integer arguments, in order, recorded as tests/test_denoiser_launches_gpu.py records an f-call (its `recording`; there are no
range slots here, so every pointer is None or "p").  Per case the phases are the construction, grads(v), grads with one middle layer's
gamma alone (its weight where the layer has no BatchNorm), grads with the last weight alone, grads with nothing asked for - which must
launch nothing - and vjp(v).  PINNED is what record() gave for every case on the commit before the three backward walks of
deqsci_amd/vjp.py were merged into one (printed entry by entry, pasted here), and has not been touched since: a change of that Python
which keeps these lists keeps the device's work.

The images are (2,1,12,20): ragged against the 16 x 16 tile of the F(2x2,3x3) kernel; FFDNet's 64 -> 64 layers run at 6 x 10.  Beside
the launches: a train-mode construction moves every BatchNorm's buffers exactly once and the walks move nothing, a second grads(v) is
bit-equal to the first, and the SHA-256 of every result is printed (not asserted) so that two commits can be compared by eye.

The two train_realsn cases (a four-layer all-RealSNConv2d net in train mode, and the same net with a plain bias-free Conv2d in the
middle) were pinned later, on the commit before the training modes were gathered into vjp.GRAD_MODES - what THAT commit recorded, printed
and pasted in the same way, never what the code behind it records.  There the construction takes every RealSNConv2d's power step in the
module's weight_u / weight exactly once - the buffers equal those of a twin whose own forward ran once - and the walks move nothing."""
import copy
import hashlib
import types

import pytest
import torch

from deqsci_amd import vjp
from deqsci_amd.networks import DnCNN, FFDNet
from deqsci_amd.networks.simplecnn import RealSNConv2d
from test_denoiser_launches_gpu import recording
from test_wgrad_bn_host import seeded_bn_dncnn, seeded_ffdnet

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 1, 12, 20)
PHASES = ("construct", "grads", "grads-middle", "grads-last", "vjp")


def _plain():
    g = torch.Generator().manual_seed(11)
    net = DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="denoiser")
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / (9 * m.weight.shape[1])) ** 0.5
    return net.eval()


def _mixed():
    net = seeded_bn_dncnn(5, 6)
    bns = [i for i, m in enumerate(net.dncnn) if isinstance(m, torch.nn.BatchNorm2d)]
    del net.dncnn[bns[1]]
    return net


def _realsn(mixed=False):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(13)                 # weight_orig; every weight_u comes from a generator of its module's own, seeded by the layer
        net = DnCNN(1, num_of_layers=4, lip=1.0, no_bn=True, tag="denoiser")
        if mixed:
            net.dncnn[2] = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False)
    return net.train()


# case -> (the net, DenoiserParamGrads' keywords)
CASES = {
    "plain": (lambda: _plain(), {}),
    "plain-under-frozen": (lambda: _plain(), {"frozen_bn": True}),
    "frozen-dncnn": (lambda: seeded_bn_dncnn(5, 6).eval(), {"frozen_bn": True}),
    "frozen-ffdnet": (lambda: seeded_ffdnet(4).eval(), {"frozen_bn": True}),
    "frozen-mixed": (lambda: _mixed().eval(), {"frozen_bn": True}),
    "train-dncnn": (lambda: seeded_bn_dncnn(5, 6).train(), {"train_bn": True}),
    "train-ffdnet": (lambda: seeded_ffdnet(4).train(), {"train_bn": True}),
    "train-mixed": (lambda: _mixed().train(), {"train_bn": True}),
    "realsn": (lambda: _realsn(), {"train_realsn": True}),
    "realsn-mixed": (lambda: _realsn(mixed=True), {"train_realsn": True}),
}


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def record(name):
    """-> (phase -> launches, what grads with nothing asked for launched, name -> digest)."""
    make, kw = CASES[name]
    net = make().to(DEV)
    ffdnet = isinstance(net, FFDNet)
    g = torch.Generator().manual_seed(sum(SHAPE))
    x = torch.rand(SHAPE, generator=g).to(DEV)
    v = torch.randn(SHAPE, generator=g).to(DEV)
    sigma = torch.tensor([0.1, 0.235], device=DEV) if ffdnet else None
    realsn = bool(kw.get("train_realsn"))
    params = (vjp.grad_parameters(net, train_realsn=True) if realsn else
              vjp.grad_parameters(net, train_bn=bool(kw.get("train_bn"))) if kw else vjp.conv_weights(net))
    convs = [m for m in (net.intermediate_dncnn.itermediate_dncnn if ffdnet else net.dncnn) if isinstance(m, (torch.nn.Conv2d, RealSNConv2d))]
    weight_of = lambda c: c.weight_orig if isinstance(c, RealSNConv2d) else c.weight
    first = [next(j for j, p in enumerate(params) if p is weight_of(c)) for c in convs]
    mid = len(convs) // 2
    has_bn = first[mid + 1] - first[mid] == 3
    only = lambda j: [i == j for i in range(len(params))]
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    rsn = lambda of: [m for m in of.modules() if isinstance(m, RealSNConv2d)]
    buffers = lambda of=net: ([b.clone() for m in bns for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
                              + [b.clone() for m in rsn(of) for b in (m.weight_u, m.weight)])
    assert all(int(m.num_batches_tracked) == 0 for m in bns)
    before, twin = buffers(), copy.deepcopy(net)
    if realsn:
        assert len(rsn(net)) == (len(convs) - 1 if name == "realsn-mixed" else len(convs)) == len(before) // 2
        with torch.no_grad():
            twin(x)                           # the module's own train-mode forward: one power step per RealSNConv2d, on the same kernels
    den, logs = types.SimpleNamespace(ranges=None), {}
    with recording(den) as log:
        pg = vjp.DenoiserParamGrads(net, x, sigma, **kw)
    logs["construct"] = list(log)
    moved = 1 if kw.get("train_bn") else 0
    assert all(int(m.num_batches_tracked) == moved for m in bns)
    after = buffers()
    if realsn:                                # every weight_u and weight moved, and exactly once
        assert all(not torch.equal(a, b) for a, b in zip(after, before))
        assert all(torch.equal(a, b) for a, b in zip(after, buffers(twin)))
    with recording(den) as log:
        grads = pg.grads(v)
    logs["grads"] = list(log)
    with recording(den) as log:
        middle = pg.grads(v, need=only(first[mid] + (1 if has_bn else 0)))
    logs["grads-middle"] = list(log)
    with recording(den) as log:
        last = pg.grads(v, need=only(first[-1]))
    logs["grads-last"] = list(log)
    with recording(den) as log:
        nothing = pg.grads(v, need=[False] * len(params))
    none = list(log)
    with recording(den) as log:
        gx = pg.vjp(v)
    logs["vjp"] = list(log)
    # the walks move no buffer; asking for less gives the same tensors and nothing else; a second walk is bit-equal
    assert all(torch.equal(a, b) for a, b in zip(buffers(), after))
    assert len(grads) == len(params) and all(a.shape == p.shape for a, p in zip(grads, params))
    assert all(t is None for t in nothing)
    for part in (middle, last):
        assert sum(t is not None for t in part) == 1
        assert all(t is None or torch.equal(t, a) for t, a in zip(part, grads))
    assert all(torch.equal(a, b) for a, b in zip(pg.grads(v), grads))
    assert gx.shape == x.shape and pg.shape == SHAPE and pg.ffdnet == ffdnet
    digests = {"noise": _digest(pg.noise), "vjp": _digest(gx)}
    digests.update({f"mask{i}": _digest(m) for i, m in enumerate(pg.masks)})
    digests.update({f"grad{i}": _digest(t) for i, t in enumerate(grads)})
    pg.release()
    with pytest.raises(RuntimeError, match="released"):
        pg.grads(v)
    return logs, none, digests


@pytest.mark.parametrize("name", list(CASES))
def test_backward_launches_are_pinned(name):
    logs, none, digests = record(name)
    for phase in PHASES:
        print(f"{name} {phase}: {len(logs[phase])} entries")
        for entry in logs[phase]:
            print("   ", entry)
    print(name, "sha256:", hashlib.sha256(repr(sorted(digests.items())).encode()).hexdigest()[:16], digests)
    assert none == []
    for phase in PHASES:
        assert logs[phase] == PINNED[name][phase], phase


PINNED = {
    'plain': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'plain-under-frozen': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'frozen-dncnn': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'frozen-ffdnet': {
        'construct': [
            ('deqsci_ffdnet_head_f32', 'p', 'p', 'p', 1, 'p', 2, 6, 10, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 6, 10, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_ffdnet_tail_f32', 'p', 'p', None, 'p', 2, 6, 10, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_shuffle_f32', 'p', None, 0, 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_ffdnet_head_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_shuffle_f32', 'p', 'p', 1, 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_ffdnet_head_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 6, 10, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_shuffle_f32', 'p', None, 0, 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
        ],
    },
    'frozen-mixed': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_bn_f32', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'train-dncnn': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 480, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 480, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 480, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'train-ffdnet': {
        'construct': [
            ('deqsci_ffdnet_head_f32', 'p', 'p', 'p', 1, 'p', 2, 6, 10, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 6, 10, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 120, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 120, None),
            ('deqsci_ffdnet_tail_f32', 'p', 'p', None, 'p', 2, 6, 10, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_shuffle_f32', 'p', None, 0, 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_ffdnet_head_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 6, 10, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_wgrad3x3_shuffle_f32', 'p', 'p', 1, 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_ffdnet_head_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 6, 10, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 120, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 120, None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_shuffle_f32', 'p', None, 0, 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
        ],
    },
    'train-mixed': {
        'construct': [
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 480, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 0, None),
            ('deqsci_bn_train_stats_f32', 'p', 'p', 'p', 'p', 'p', 0.1, 480, 'p', None),
            ('deqsci_bn_train_apply_f32', 'p', 'p', 'p', 'p', 1e-05, 'p', 'p', 1, 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_bn_train_grad_stats_f32', 'p', 'p', 'p', 1e-05, 'p', 'p', 'p', 480, 'p', None),
            ('deqsci_bn_train_grad_apply_f32', 'p', 'p', 'p', 'p', 'p', 1e-05, 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'realsn': {
        'construct': [
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 1, 64, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 1, 64, None),
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 64, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 64, None),
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 64, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 64, None),
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 1, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 1, None),
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 1, 40, 40, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 64, 40, 40, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 64, 40, 40, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 1, 64, 40, 40, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 64, 40, 40, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 1, 40, 40, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
    'realsn-mixed': {
        'construct': [
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 1, 64, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 1, 64, None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 64, None),
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 64, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 64, None),
            ('deqsci_realsn_power_f32', 'p', 'p', 'p', 'p', 'p', 1, 1.0, 1e-12, 64, 1, 40, 40, 'p', None),
            ('deqsci_realsn_pack_f32', 'p', 'p', None, 'p', 64, 1, None),
            ('deqsci_conv3x3_c1_to_64_f32', 'p', 'p', 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_winograd_f32', 'p', 'p', None, 'p', 2, 12, 20, 1, None),
            ('deqsci_relu_mask_pack_f32', 'p', 'p', 480, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
        'grads': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 1, 40, 40, 'p', None),
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 64, 40, 40, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 0, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 1, 64, 40, 40, 'p', None),
        ],
        'grads-middle': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_wgrad3x3_c64_c64_f32', 'p', 'p', 'p', 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 64, 40, 40, 'p', None),
        ],
        'grads-last': [
            ('deqsci_wgrad3x3_c1_c64_f32', 'p', 'p', 'p', 1, 2, 12, 20, 'p', None),
            ('deqsci_realsn_grad_f32', 'p', 'p', 'p', 'p', 'p', 'p', 1.0, 64, 1, 40, 40, 'p', None),
        ],
        'vjp': [
            ('deqsci_conv3x3_c1_to_64_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_winograd_masked_f32', 'p', 'p', 'p', 'p', 2, 12, 20, None),
            ('deqsci_conv3x3_c64_to_1_f32', 'p', 'p', None, 'p', 2, 12, 20, None),
        ],
    },
}
