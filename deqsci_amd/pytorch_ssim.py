"""Drop-in for the reference's pytorch_ssim (pytorch_ssim/__init__.py): `ssim(img1, img2, window_size=11, size_average=True)` and
`SSIM(window_size=11, size_average=True)` on NCHW tensors - the structural similarity of Wang et al. (2004) with a Gaussian window of
sigma 1.5, zero padding of window_size//2, C1 = 0.01^2 and C2 = 0.03^2, every channel of every image on its own.

    size_average=True    the mean of the SSIM map over everything (a 0-d tensor)
    size_average=False   the mean over C, H, W per image (an (N,) tensor)

Tensors on a HIP device go through the kernel of csrc/ssim.hip (fp64 after the load, deterministic); CPU tensors through `ssim_float64`,
a float64 torch restatement of the same formula.  Both return float32, like the reference on fp32 input.  An evaluation metric only:
there is no backward, and asking for one raises instead of returning a detached value.  window_size must be odd and in 3..15.
"""
import math

import torch

from . import _hip

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def gaussian_taps(window_size, sigma=1.5):
    """The reference's window: exp values rounded to fp32, normalised by their fp32 sum (pytorch_ssim.gaussian)."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    s = torch.zeros((), dtype=torch.float32)
    for v in g:                                   # left to right in fp32, as the kernel's host code sums them
        s = s + v
    return g / s


def ssim_map_float64(img1, img2, window_size=11):
    """The SSIM map of two NCHW tensors in float64 (zero padding, 'same' size), on the tensors' device."""
    g = gaussian_taps(window_size).double().to(img1.device)
    C = img1.shape[1]
    w = torch.outer(g, g).expand(C, 1, window_size, window_size).contiguous()
    a, b = img1.double(), img2.double()
    pad = window_size // 2

    def conv(t):
        return torch.nn.functional.conv2d(t, w, padding=pad, groups=C)
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu12
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))


def ssim_float64(img1, img2, window_size=11, size_average=True):
    """CPU path: the float64 restatement, reduced like the reference."""
    m = ssim_map_float64(img1, img2, window_size)
    return m.mean() if size_average else m.mean(dim=(1, 2, 3))


def _check(img1, img2, window_size):
    if not _hip.ssim_window_ok(window_size):
        raise ValueError(f"window_size must be an odd integer in 3..15, got {window_size!r}")
    if img1.dim() != 4 or tuple(img1.shape) != tuple(img2.shape):
        raise ValueError(f"ssim expects two NCHW tensors of one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.device != img2.device:
        raise ValueError(f"img1 is on {img1.device}, img2 on {img2.device}")
    if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad):
        raise RuntimeError("deqsci_amd.pytorch_ssim is an evaluation metric, no backward: call it under torch.no_grad() or on detached "
                           "tensors")


def ssim(img1, img2, window_size=11, size_average=True):
    _check(img1, img2, window_size)
    if img1.is_cuda:
        per = _hip.ssim_frames(_hip.f32c(img1), _hip.f32c(img2), _hip.LAYOUT_BHW, window_size)       # (N, C): NCHW is BHW
        out = per.mean() if size_average else per.mean(dim=1)
    else:
        out = ssim_float64(img1, img2, window_size, size_average)
    return out.float()


class SSIM(torch.nn.Module):
    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        if not _hip.ssim_window_ok(window_size):
            raise ValueError(f"window_size must be an odd integer in 3..15, got {window_size!r}")
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)
