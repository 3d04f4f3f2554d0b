"""DE-GAP-CNN denoiser ("SimpleCNN") with the reference's module API
(networks/provable/model/SimpleCNN_models.py:6-61): `DnCNN(channels, num_of_layers, lip, no_bn,
adaptive, tag)` with the layers in `self.dncnn`, so `cnn.ckpt` keys `dncnn.{0,2,4,6}.weight` load
unchanged.  `lip > 0` selects real-spectral-norm convolutions (conv_sn_chen.py:16-93); in eval mode
those use their stored, already normalised `weight` buffer, which is all inference needs
(`rsn_cnn.ckpt` keys `weight_orig / weight / weight_u`).  In train mode every forward runs one
power-iteration step on `weight_u` and renormalises `weight_orig` by the estimated operator norm
(deqsci_amd.realsn; csrc/realsn.hip on the device), as the reference's forward pre-hook does.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import autograd as _ag


class RealSNConv2d(nn.Module):
    """Stand-in for conv_spectral_norm(nn.Conv2d(..., bias=False)): same state-dict entries.
    Eval mode: conv2d with the stored normalised weight (conv_sn_chen.py:65-67).
    Train mode (conv_sn_chen.py:29-50,60-64), at every forward, under torch.no_grad() too: n_power_iterations steps of the power
    iteration from `weight_u`, weight = weight_orig / cur_sigma * sigma (differentiable in weight_orig; autograd.realsn_weight), the new
    left vector copied into `weight_u` and the detached weight into `weight`, both in place - so a later .eval() uses the last
    train-mode weight and state_dict() carries it - and conv2d with that weight.
    A fresh module's `weight_u` is a unit-norm normal draw (conv_sn_chen.py:80) from a generator of the module's own (seed: the layer's
    shape, or `seed`): the global random stream is left to the weight's initialisation alone."""

    n_power_iterations = 1
    eps = 1e-12

    def __init__(self, cin, cout, sigma=1.0, seed=None):
        super().__init__()
        self.sigma = sigma
        w = torch.empty(cout, cin, 3, 3)
        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
        self.weight_orig = nn.Parameter(w)
        self.register_buffer("weight", w.detach().clone())
        g = torch.Generator().manual_seed(1000 * cin + cout if seed is None else int(seed))
        u = torch.randn(1, 1 if cout == 1 else 64, 40, 40, generator=g)
        self.register_buffer("weight_u", u / u.norm().clamp_min(self.eps))

    def forward(self, x):
        if self.training:
            weight, u = _ag.realsn_weight(self.weight_orig, self.weight_u, self.sigma, self.n_power_iterations, self.eps)
            with torch.no_grad():
                self.weight_u.copy_(u)
                self.weight.copy_(weight)
            return F.conv2d(x, weight, padding=1)
        return F.conv2d(x, self.weight, padding=1)


class DnCNN(nn.Module):
    def __init__(self, channels, num_of_layers=17, lip=1.0, no_bn=False, adaptive=False, tag='denoiser'):
        super().__init__()
        self.tag = tag
        features = 64
        sigmas = [pow(lip, 1.0 / num_of_layers) if lip > 0.0 else 0.0 for _ in range(num_of_layers)]
        if adaptive:
            sigmas = [5.0, 2.0, 1.0, 0.681, 0.464, 0.316]
            if len(sigmas) != num_of_layers:
                raise AssertionError(f"adaptive spectral-norm schedule has {len(sigmas)} entries, the network {num_of_layers} layers")

        def conv_layer(cin, cout, sigma, index=0):
            if sigma > 0.0:
                return RealSNConv2d(cin, cout, sigma, seed=index)
            return nn.Conv2d(cin, cout, kernel_size=3, padding=1, bias=False)

        layers = [conv_layer(channels, features, sigmas[0]), nn.ReLU(inplace=True)]
        for i in range(1, num_of_layers - 1):
            layers.append(conv_layer(features, features, sigmas[i], i))
            if not no_bn:
                layers.append(nn.BatchNorm2d(features))
            layers.append(nn.ReLU(inplace=True))
        layers.append(conv_layer(features, channels, sigmas[-1], num_of_layers - 1))
        self.dncnn = nn.Sequential(*layers)

    def forward(self, x):
        return self.dncnn(x)
