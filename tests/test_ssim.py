"""SSIM: the kernel of csrc/ssim.hip through the C ABI, _hip.ssim_frames, the pytorch_ssim drop-in, the harness and the CLI.

Yardsticks: (a) a float64 restatement in this file (separable shifted sums, zero padding) - the kernel is held to 2e-6 per frame;
(b) tests/golden/ssim.npz, the reference's own fp32 pytorch_ssim (tests/golden/make_ssim_golden.py) - held to 2e-5, the size of
the reference's fp32 error on these inputs."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

HWB, BHW = 0, 1
C1, C2 = 0.01 ** 2, 0.03 ** 2
PAIR_SHAPES = [(1, 1, 7, 9), (2, 1, 37, 53), (1, 3, 64, 64), (4, 1, 256, 256)]
REC_KEYS = [("SimpleCNN_anderson_180", "drop8"), ("SimpleCNN_anderson_180", "runner8"), ("SimpleCNN_anderson_180", "traffic"),
            ("ffdnet_anderson_30", "traffic")]


def taps(window):
    g = np.array([np.exp(-(k - window // 2) ** 2 / (2 * 1.5 ** 2)) for k in range(window)]).astype(np.float32)
    s = np.float32(0)
    for v in g:
        s = np.float32(s + v)
    return (g / s).astype(np.float64)


def ssim_planes_f64(x, y, window, mode="same"):
    """float64 restatement: x, y (N,H,W) planes (torch, any device) -> (N,) mean SSIM per plane."""
    g = taps(window)
    R = window // 2
    x, y = x.double(), y.double()
    N, H, W = x.shape

    def blur(t):
        t = torch.nn.functional.pad(t, (R, R, R, R))
        h = sum(float(g[k]) * t[:, :, k:k + W] for k in range(window))
        return sum(float(g[k]) * h[:, k:k + H, :] for k in range(window))
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    if mode == "valid":
        m = m[:, R:H - R, R:W - R]
    return m.mean(dim=(1, 2))


def golden():
    return np.load(os.path.join(GOLDEN, "ssim.npz"))


def pair(i, gd=None):
    """Seeded NCHW pair i of ssim.npz (the inputs are not stored: the same recipe as tests/golden/make_ssim_golden.py, numpy's
    fixed RandomState stream and float64 arithmetic, checked against the stored hash) -> two float32 torch tensors on the CPU."""
    shape = PAIR_SHAPES[i]
    rs = np.random.RandomState(20261015 + i)
    x = rs.random_sample(shape)
    nb = sum(np.roll(np.roll(x, dy, axis=2), dx, axis=3) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    y = np.clip(0.7 * x + 0.3 * nb + 0.05 * rs.standard_normal(shape), 0.0, 1.0)
    x, y = x.astype(np.float32), y.astype(np.float32)
    gd = golden() if gd is None else gd
    assert hashlib.sha256(x.tobytes() + y.tobytes()).hexdigest()[:16] == str(gd[f"pair{i}_sha"]), "ssim.npz inputs not reproduced"
    return torch.from_numpy(x), torch.from_numpy(y)


def gt_frames(clip):
    from deqsci_amd.harness import load_test_data
    return load_test_data(os.path.join(ROOT, "data", "test_gray", f"{clip}_cacti.mat"))["gt"]


# ----------------------------------------------------------------------------- CPU
def test_ssim_exports():
    from deqsci_amd import _hip
    lib = ctypes.CDLL(_hip.lib_path())
    for name in ("deqsci_ssim_f32", "deqsci_ssim_workspace_bytes"):
        assert hasattr(lib, name)
        assert name in _hip.SIGNATURES or name in _hip.OTHER_EXPORTS


def test_ssim_argument_validation_without_a_gpu():
    from deqsci_amd import _hip
    lib = _hip.load()
    assert lib.deqsci_ssim_workspace_bytes(8, 256, 256, 8, HWB) == 8 * 8 * (16 * 8) * 8          # one fp64 per (measurement, frame, 32x16 tile)
    assert lib.deqsci_ssim_workspace_bytes(0, 256, 256, 8, HWB) == 0
    assert lib.deqsci_ssim_workspace_bytes(1, 0, 256, 8, HWB) == -2
    assert lib.deqsci_ssim_workspace_bytes(1, 7, 9, 1, 5) == -4
    buf = (ctypes.c_double * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    x, y, out, ws = p, p + 8192, p + 16384, p + 20480                                            # disjoint host buffers: nothing is launched

    def call(x=x, y=y, out=out, ws=ws, M=1, H=16, W=16, B=2, layout=HWB, window=11, valid=0, clamp=0):
        return lib.deqsci_ssim_f32(x, y, out, M, H, W, B, layout, window, valid, clamp, ws, None)
    assert call(x=None) == -1 and call(y=None) == -1 and call(out=None) == -1 and call(ws=None) == -1
    assert call(H=0) == -2 and call(W=-1) == -2 and call(M=-1) == -2 and call(B=-3) == -2
    assert call(window=10) == -2 and call(window=1) == -2 and call(window=17) == -2 and call(window=2) == -2
    assert call(H=7, W=9, window=11, valid=1) == -2 and call(H=16, W=10, window=11, valid=1) == -2            # empty valid region
    assert call(layout=2) == -4
    assert call(M=0) == 0 and call(B=0) == 0                                                     # no-op
    assert call(x=x + 2) == -3 and call(out=out + 4) == -3
    assert call(out=x) == -4 and call(ws=y + 64) == -4 and call(ws=out) == -4                    # aliasing
    with pytest.raises(ValueError):
        _hip.ssim_frames(torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, 1), window=9, mode="full")


@pytest.mark.parametrize("i", range(len(PAIR_SHAPES)))
def test_restatement_reproduces_the_golden(i):
    """Checks this file's float64 restatement against the reference's fp32 values."""
    gd = golden()
    x, y = pair(i, gd)
    N, C, H, W = x.shape
    for ws in (7, 11):
        per = ssim_planes_f64(x.reshape(N * C, H, W), y.reshape(N * C, H, W), ws).reshape(N, C)
        assert abs(float(per.mean()) - float(gd[f"pair{i}_w{ws}_avg"])) < 2e-5
        assert np.abs(per.mean(dim=1).numpy() - gd[f"pair{i}_w{ws}_img"]).max() < 2e-5
    # ... and on the reference's reconstructions
    if i == 0:
        for tag, clip in REC_KEYS:
            rec = torch.from_numpy(np.load(os.path.join(GOLDEN, f"e2e_{tag}_rec.npz"))[f"{clip}_m0"][0]).clamp(0, 1)
            gt = torch.from_numpy(gt_frames(clip)[..., :8])
            per = ssim_planes_f64(rec.permute(2, 0, 1), gt.permute(2, 0, 1), 11)
            assert np.abs(per.numpy() - gd[f"rec_{tag}_{clip}_m0"]).max() < 2e-5


def test_pytorch_ssim_cpu_path_vs_golden():
    from deqsci_amd import pytorch_ssim
    gd = golden()
    for i in range(len(PAIR_SHAPES)):
        x, y = pair(i, gd)
        for ws in (7, 11):
            a = pytorch_ssim.ssim(x, y, window_size=ws)
            assert a.dtype == torch.float32 and a.dim() == 0 and abs(float(a) - float(gd[f"pair{i}_w{ws}_avg"])) < 2e-5
            b = pytorch_ssim.SSIM(window_size=ws, size_average=False)(x, y)
            assert b.shape == (x.shape[0],) and np.abs(b.numpy() - gd[f"pair{i}_w{ws}_img"]).max() < 2e-5
    x = pair(1, gd)[0]
    for bad in (10, 1, 17):
        with pytest.raises(ValueError):
            pytorch_ssim.ssim(x, x, window_size=bad)
        with pytest.raises(ValueError):
            pytorch_ssim.SSIM(window_size=bad)
    with pytest.raises(RuntimeError, match="no backward"):
        pytorch_ssim.ssim(x.clone().requires_grad_(), x)
    with torch.no_grad():
        assert float(pytorch_ssim.ssim(x.clone().requires_grad_(), x)) == pytest.approx(1.0, abs=1e-6)


def test_harness_frame_ssim_on_the_host():
    from deqsci_amd.harness import ssim
    gd = golden()
    rec = np.load(os.path.join(GOLDEN, "e2e_SimpleCNN_anderson_180_rec.npz"))["drop8_m0"][0].clip(0, 1)
    gt = gt_frames("drop8")
    assert abs(ssim(rec[..., 3], gt[..., 3]) - float(gd["rec_SimpleCNN_anderson_180_drop8_m0"][3])) < 2e-5


def test_cli_ssim_flags_parse_and_default_off():
    from deqsci_amd.cli import parser
    a = parser().parse_args([])
    assert a.ssim is False and a.ssim_mode is None
    a = parser().parse_args(["--ssim", "--ssim_mode", "valid"])
    assert a.ssim is True and a.ssim_mode == "valid"
    assert parser().parse_args(["--ssim_mode", "same"]).ssim_mode == "same"
    with pytest.raises(SystemExit):
        parser().parse_args(["--ssim_mode", "full"])


# ----------------------------------------------------------------------------- GPU
DEV = "cuda"
# (M, B, H, W): every M in {1, 5, 64}, B in {1, 3, 8, 16}, H x W in {7x9, 37x53, 256x256, 512x512} appears
SHAPES_A = [(1, 1, 7, 9), (5, 3, 7, 9), (64, 16, 7, 9), (5, 8, 37, 53), (64, 3, 37, 53), (1, 16, 37, 53),
            (1, 8, 256, 256), (5, 3, 256, 256), (64, 1, 256, 256), (1, 16, 512, 512), (5, 1, 512, 512)]


def _case(M, B, H, W, seed, clamp):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.rand(M, B, H, W, device=DEV, generator=g)
    if clamp:
        x = x * 1.4 - 0.2                                                          # outside [0,1]: the clamp matters
    y = (0.8 * torch.rand(M, B, H, W, device=DEV, generator=g) + 0.2 * x).clamp(0, 1)
    x[:, :, : H // 3, : W // 3] = 0.5                                              # a flat region: the cancellation of E[x^2] - mu^2
    y[:, :, : H // 3, : W // 3] = 0.5 + 1e-3 * y[:, :, : H // 3, : W // 3]
    return x, y


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [HWB, BHW])
@pytest.mark.parametrize("window", [3, 7, 11, 15])
@pytest.mark.parametrize("mode", ["same", "valid"])
@pytest.mark.parametrize("clamp", [False, True])
def test_kernel_vs_float64_restatement(layout, window, mode, clamp):
    """(a) <= 2e-6 absolute per frame against the float64 restatement; a valid region that is empty is refused."""
    from deqsci_amd import _hip
    for si, (M, B, H, W) in enumerate(SHAPES_A):
        x, y = _case(M, B, H, W, 100 * window + si, clamp)
        xl, yl = (x, y) if layout == BHW else (x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous())
        if mode == "valid" and (H < window or W < window):
            with pytest.raises(_hip.DeqsciHipError, match="code -2"):
                _hip.ssim_frames(xl, yl, layout, window, mode, clamp)
            continue
        got = _hip.ssim_frames(xl, yl, layout, window, mode, clamp)
        assert got.shape == (M, B) and got.dtype == torch.float64
        xs = x.clamp(0, 1) if clamp else x
        want = ssim_planes_f64(xs.reshape(M * B, H, W), y.reshape(M * B, H, W), window, mode).reshape(M, B)
        err = float((got - want).abs().max())
        assert err <= 2e-6, (M, B, H, W, err)


@pytest.mark.gpu
def test_kernel_vs_reference_golden():
    """(b) the reference's fp32 values: synthetic pairs through the drop-in, its reconstructions through clip_ssim / ssim_frames."""
    from deqsci_amd import _hip, pytorch_ssim
    from deqsci_amd.harness import clip_ssim
    gd = golden()
    for i in range(len(PAIR_SHAPES)):
        x, y = (t.to(DEV) for t in pair(i, gd))
        for ws in (7, 11):
            a = pytorch_ssim.ssim(x, y, window_size=ws)
            assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 0
            assert abs(float(a) - float(gd[f"pair{i}_w{ws}_avg"])) < 2e-5
            b = pytorch_ssim.SSIM(window_size=ws, size_average=False)(x, y)
            assert b.shape == (x.shape[0],) and np.abs(b.cpu().numpy() - gd[f"pair{i}_w{ws}_img"]).max() < 2e-5
    for tag, clip in REC_KEYS:
        rec = torch.from_numpy(np.load(os.path.join(GOLDEN, f"e2e_{tag}_rec.npz"))[f"{clip}_m0"]).to(DEV)        # (1,H,W,8), unclamped
        gt = gt_frames(clip)
        want = gd[f"rec_{tag}_{clip}_m0"]
        per = _hip.ssim_frames(rec, torch.from_numpy(gt[None, ..., :8]).contiguous().to(DEV), HWB, 11, "same", clamp_x=True)
        assert np.abs(per[0].cpu().numpy() - want).max() < 2e-5
        assert abs(clip_ssim(rec, gt, [0])[0] - float(np.mean(want, dtype=np.float64))) < 2e-5


@pytest.mark.gpu
def test_kernel_is_deterministic():
    """(c) two calls on the same inputs are bit-identical."""
    from deqsci_amd import _hip
    x, y = _case(5, 8, 256, 256, 7, True)
    xh, yh = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
    for mode in ("same", "valid"):
        a = _hip.ssim_frames(xh, yh, HWB, 11, mode, True)
        b = _hip.ssim_frames(xh, yh, HWB, 11, mode, True)
        assert torch.equal(a, b)
        assert torch.equal(_hip.ssim_frames(x, y, BHW, 11, mode, True), _hip.ssim_frames(x, y, BHW, 11, mode, True))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [HWB, BHW])
def test_nan_reaches_exactly_its_frame(layout):
    """(d) a NaN pixel (in x, clamped or not, or in y; at a corner in valid mode) gives NaN for its frame and no other."""
    from deqsci_amd import _hip
    for mode, clamp, which, (h, w) in (("same", False, "x", (100, 37)), ("same", True, "x", (0, 0)), ("valid", True, "x", (0, 0)),
                                       ("valid", False, "y", (255, 255))):
        x, y = _case(3, 8, 256, 256, 11, clamp)
        (x if which == "x" else y)[1, 5, h, w] = float("nan")
        if layout == HWB:
            x, y = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
        got = _hip.ssim_frames(x, y, layout, 11, mode, clamp)
        nan = torch.isnan(got)
        assert bool(nan[1, 5]) and int(nan.sum()) == 1, (mode, clamp, which)


@pytest.mark.gpu
def test_device_path_does_not_call_the_host_fallback(monkeypatch):
    """(e) device tensors never reach the float64 CPU restatement."""
    from deqsci_amd import harness, pytorch_ssim

    def boom(*a, **k):
        raise AssertionError("host fallback called for device tensors")
    monkeypatch.setattr(pytorch_ssim, "ssim_float64", boom)
    monkeypatch.setattr(pytorch_ssim, "ssim_map_float64", boom)
    gd = golden()
    x, y = (t.to(DEV) for t in pair(2, gd))
    assert abs(float(pytorch_ssim.ssim(x, y)) - float(gd["pair2_w11_avg"])) < 2e-5
    assert abs(float(pytorch_ssim.SSIM(7)(x, y)) - float(gd["pair2_w7_avg"])) < 2e-5
    assert harness.ssim(x[0, 0], y[0, 0].cpu()) == pytest.approx(float(ssim_planes_f64(x[0, :1], y[0, :1], 11)[0]), abs=2e-6)
    with pytest.raises(AssertionError):                                     # (the patch is live: the CPU path does hit it)
        pytorch_ssim.ssim(x.cpu(), y.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [False, True, "all"])
def test_evaluate_with_ssim_end_to_end(batch):
    """(f) evaluate(..., ssim=True), SimpleCNN @180 over the three shipped clips: each ClipResult.ssim is clip_ssim of its own rec, and
    on m0 the SSIM is within 1e-3 of the reference's SSIM of the reference's reconstruction."""
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import build_pipeline
    from deqsci_amd.harness import SCITestDataset, clip_ssim, evaluate
    _, deq = build_pipeline("SimpleCNN", checkpoint.shipped("cnn"), 180)
    clips = list(SCITestDataset(os.path.join(ROOT, "data", "test_gray")))
    avg, results = evaluate(deq, clips, batch=batch, ssim=True)
    _, plain = evaluate(deq, clips[:1], batch=batch)
    assert plain[0].ssim is None and plain[0].mean_ssim is None
    gd = golden()
    by_name = {c["file"]: c for c in clips}
    assert [r.name for r in results] == ["drop8_cacti.mat", "runner8_cacti.mat", "traffic_cacti.mat"]
    for r in results:
        ids = r.info["measurements"]
        assert len(r.ssim) == len(ids) and r.ssim == clip_ssim(r.rec, by_name[r.name]["gt"], ids)
        assert r.mean_ssim == pytest.approx(sum(r.ssim) / len(r.ssim))
        want = float(np.mean(gd[f"rec_SimpleCNN_anderson_180_{r.name.split('_')[0]}_m0"], dtype=np.float64))
        assert abs(r.ssim[0] - want) < 1e-3, (r.name, r.ssim[0], want)


def _cli(tmp_path, *extra):
    env = dict(os.environ)
    env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, "-m", "deqsci_amd.cli", "--denoiser", "SimpleCNN", "--and_maxiters", "10", "--testpath",
           os.path.join(ROOT, "data", "test_gray") + "/", "--savepath", str(tmp_path) + "/"] + list(extra)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


@pytest.mark.gpu
def test_cli_ssim_output(tmp_path):
    """(g) --ssim adds '  SSIM: x' to the clip lines and a 'Total Average SSIM' line; without it the lines are today's."""
    plain = _cli(tmp_path / "a")
    with_ssim = _cli(tmp_path / "b", "--ssim")
    assert not any("SSIM" in ln for ln in plain)
    clip_lines = [ln for ln in plain if ln.startswith("['")]
    assert len(clip_lines) == 3 and all(ln.endswith(" dB") and "  PSNR: " in ln for ln in clip_lines)
    assert sum(ln.startswith("--------------------------------- Total Average PSNR: ") for ln in plain) == 1
    total = [ln for ln in with_ssim if "Total Average SSIM" in ln]
    assert len(total) == 1 and 0.0 < float(total[0].split(": ")[-1]) <= 1.0
    # with the SSIM parts taken out, the same lines (the timing line aside)
    assert all("   SSIM: " in ln for ln in with_ssim if ln.startswith("['"))
    stripped = [ln.split("   SSIM: ")[0] for ln in with_ssim if "Total Average SSIM" not in ln]
    assert [ln for ln in stripped if "frames/s" not in ln] == [ln for ln in plain if "frames/s" not in ln]
