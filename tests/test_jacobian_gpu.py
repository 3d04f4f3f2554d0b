"""GPU: the Jacobian diagnostics on the device - csrc/jacobian.hip's masked FFDNet head (J1) and power step (J2), DenoiserJacobian in both
directions for the three shipped denoisers, power_report against its float64 host twin, and the harness option end to end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, rel_l2

pytestmark = pytest.mark.gpu

KINDS = {"SimpleCNN": "cnn", "RealSN_SimpleCNN": "rsn_cnn", "ffdnet": "ffdnet_gray"}
CASES = {"SimpleCNN": "SimpleCNN", "RealSN_SimpleCNN": "RealSN_SimpleCNN", "ffdnet_s0": "ffdnet", "ffdnet_s1": "ffdnet"}


def _pipeline(kind, iters=30):
    from deqsci_amd import checkpoint
    from deqsci_amd.cli import build_pipeline
    return build_pipeline(kind, checkpoint.shipped(KINDS[kind]), and_maxiters=iters)


def _host_op(solver, op, z, y, Phi, Phi_sum, sigma, **kw):
    """The float64 host statement of `op` under the DEVICE's masks (or kw's)."""
    import copy
    from deqsci_amd import jacobian, vjp
    net64 = copy.deepcopy(solver.nonlinear_op).cpu().double()
    if "mask_dtype" not in kw and "masks" not in kw:
        kw["masks"] = [vjp.unpack_masks(m).cpu() for m in op.denoiser.masks]
    return jacobian.HostMapJacobian(net64, z.cpu(), y.cpu(), Phi.cpu(), Phi_sum.cpu(), sigma=sigma, **kw)


@pytest.mark.parametrize("n,H2,W2", [(1, 34, 50), (5, 34, 50), (1, 128, 128), (5, 128, 128)])
def test_masked_head_against_float64(n, H2, W2):
    from deqsci_amd import _hip
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 1, H2, W2, generator=g).cuda()
    w = (torch.randn(64, 4, 3, 3, generator=g) * 0.2).cuda()
    act = torch.randn(n, 64, H2 // 2, W2 // 2, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    mask = _hip.relu_mask_pack(act)
    got = _hip.ffdnet_head_masked(x, _hip.pack_head_masked_weights(w), mask)
    want = F.conv2d(F.pixel_unshuffle(x.double(), 2), w.double(), padding=1) * (act > 0)
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert bool((got[~(act > 0)] == 0).all())
    err = rel_l2(got.cpu(), want.cpu())
    print(f"J1 n={n} {H2}x{W2}: rel-L2 vs float64 {err:.3e}")
    assert err <= 1e-5
    with pytest.raises(_hip.DeqsciHipError):
        _hip.ffdnet_head_masked(x[:, :, :-1], _hip.pack_head_masked_weights(w), mask)


@pytest.mark.parametrize("kind", list(KINDS))
def test_denoiser_jacobian_against_host_plans_under_the_devices_masks(kind):
    from deqsci_amd import vjp
    solver, _ = _pipeline(kind)
    net = solver.nonlinear_op
    g = torch.Generator().manual_seed(5)
    x = torch.rand(3, 1, 34, 50, generator=g).cuda()
    v, w = torch.randn(3, 1, 34, 50, generator=g).cuda(), torch.randn(3, 1, 34, 50, generator=g).cuda()
    sigma = 0.2 if kind == "ffdnet" else None
    jd = vjp.DenoiserJacobian(net, x, sigma)
    jv, jtw = jd.jvp(v), jd.vjp(w)
    import copy
    net64 = copy.deepcopy(net).cpu().double()
    masks = [vjp.unpack_masks(m).cpu() for m in jd.masks]
    if kind == "ffdnet":
        L = vjp.ffdnet_plan(net64)
        want_jv = vjp.ffdnet_plan_jvp(L, x.cpu().double(), sigma, v.cpu().double(), masks)[0]
        want_jtw = vjp.ffdnet_plan_vjp(L, x.cpu().double(), sigma, w.cpu().double(), masks)[0]
        with pytest.raises(ValueError, match="even"):
            vjp.DenoiserJacobian(net, x[:, :, :-1], sigma)
        with pytest.raises(ValueError, match="sigma"):
            vjp.DenoiserJacobian(net, x)
    else:
        L, _ = vjp.host_plan(net64)
        want_jv = vjp.plan_jvp(L, x.cpu().double(), v.cpu().double(), masks)[0]
        want_jtw = vjp.plan_vjp(L, x.cpu().double(), w.cpu().double(), masks)[0]
        assert torch.equal(jtw, vjp.DenoiserVJP(net, x)(w))                 # the hook's product, bit for bit
    e1, e2 = rel_l2(jv.cpu(), want_jv), rel_l2(jtw.cpu(), want_jtw)
    lhs, rhs = float((w.double() * jv.double()).sum()), float((jtw.double() * v.double()).sum())
    adj = abs(lhs - rhs) / float(w.double().norm() * jv.double().norm())
    print(f"{kind}: jvp {e1:.3e} vjp {e2:.3e} adjoint {adj:.3e}")
    assert e1 <= 1e-5 and e2 <= 1e-5 and adj <= 1e-5


@pytest.mark.parametrize("shape", [(3, 24, 20), (1, 1, 1)])
@pytest.mark.parametrize("kind", ["SimpleCNN", "DnCNN17_bn"])
def test_the_hooks_product_is_the_diagnostics_transpose_bit_for_bit(kind, shape):
    """DenoiserVJP and DenoiserJacobian.vjp are one masked stack: equal masks and equal products, at a shape ragged against the 16x16
    Winograd tile in both directions with more than one image, and at the smallest shape the masked kernels accept."""
    from deqsci_amd import vjp
    from deqsci_amd.networks import DnCNN
    if kind == "SimpleCNN":
        net = _pipeline(kind)[0].nonlinear_op
    else:
        torch.manual_seed(7)
        net = DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag="denoiser")
        for mod in net.dncnn:
            if isinstance(mod, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
            elif isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.data.uniform_(0.7, 1.3)
                mod.bias.data.normal_(0, 0.05)
                mod.running_mean.normal_(0, 0.05)
                mod.running_var.uniform_(0.8, 1.2)
        net = net.cuda().eval()
    n, H, W = shape
    g = torch.Generator().manual_seed(13)
    x, v = torch.rand(n, 1, H, W, generator=g).cuda(), torch.randn(n, 1, H, W, generator=g).cuda()
    hook, jd = vjp.DenoiserVJP(net, x), vjp.DenoiserJacobian(net, x)
    assert len(hook.masks) == len(jd.masks) == (3 if kind == "SimpleCNN" else 16)
    assert all(torch.equal(a, b) for a, b in zip(hook.masks, jd.masks))
    got = hook(v)
    assert got.shape == v.shape and torch.equal(got, jd.vjp(v))
    assert bool(got.any()) or n == 1                    # (not two zeros: 1440 pixels x 64 units do not all sit behind a closed ReLU)


@pytest.mark.parametrize("case", list(CASES))
def test_map_jacobian_against_the_reference_golden(case):
    gold = np.load(os.path.join(GOLDEN, "jacobian.npz"))
    solver, _ = _pipeline(CASES[case])
    g = lambda k: torch.from_numpy(np.asarray(gold[f"{case}/a_{k}"], dtype=np.float32)).cuda()
    sigma = float(gold[f"{case}/a_sigma"]) if CASES[case] == "ffdnet" else None
    op = solver.device_jacobian(g("z"), g("y"), g("Phi"), g("Phi_sum"), sigma=sigma)
    e = rel_l2(op.jv(g("v")).cpu(), gold[f"{case}/a_Jv"])
    print(f"{case}: J v vs the reference {e:.3e}")
    assert e <= 5e-4
    if CASES[case] != "ffdnet":
        e = rel_l2(op.jtv(g("w")).cpu(), gold[f"{case}/a_JTw"])
        print(f"{case}: J^T w vs the reference {e:.3e}")
        assert e <= 5e-4


def test_power_step_against_numpy_and_edge_rows():
    from deqsci_amd import _hip
    g = torch.Generator().manual_seed(9)
    for bsz, N in ((3, 4096 * 3 + 5), (2, 1001), (8, 256 * 256 * 8)):
        w, v = torch.randn(bsz, N, generator=g).cuda(), torch.randn(bsz, N, generator=g).cuda()
        row, row2 = (torch.zeros(bsz, 2, dtype=torch.float64, device="cuda") for _ in range(2))
        out, out2 = torch.empty_like(w), torch.empty_like(w)
        _hip.power_step(w, v, out, row)
        _hip.power_step(w, v, out2, row2)
        assert torch.equal(out, out2) and torch.equal(row, row2)              # bit-stable
        a = (w.double() ** 2).sum(1).cpu().numpy()
        b = (w.double() * v.double()).sum(1).cpu().numpy()
        assert np.allclose(row[:, 0].cpu().numpy(), a, rtol=1e-13, atol=0) and np.allclose(row[:, 1].cpu().numpy(), b, rtol=0, atol=1e-12 * np.sqrt(a).max() * float(v.double().norm(dim=1).max()))
        assert rel_l2(out.cpu(), (w.double() / w.double().norm(dim=1, keepdim=True)).cpu()) <= 1e-7
        _hip.power_step(w, None, out2, row2)
        assert torch.equal(out, out2) and torch.equal(row[:, 0], row2[:, 0]) and bool(torch.isnan(row2[:, 1]).all())
        w2 = w.clone()
        _hip.power_step(w2, v, w2, row2)                                      # in place
        assert torch.equal(w2, out)
    w = torch.randn(4, 5000, generator=g).cuda()
    w[1] = 0.0
    w[2, 17] = float("inf")
    w[3, 4999] = float("nan")
    row = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    out = _hip.power_step(w, w.clone(), torch.full_like(w, 7.0), row)
    assert bool(torch.isfinite(row[0]).all()) and bool(torch.isnan(row[1:]).all())
    assert bool((out[1:] == 0).all()) and abs(float(out[0].double().norm()) - 1) < 1e-6


@pytest.mark.parametrize("kind", list(KINDS))
def test_power_report_against_the_float64_host_iteration(kind):
    """lipschitz_*: Rayleigh quotients of a symmetric operator known to 1e-5 per application, and the power iteration damps perturbations
    of the vector: 1e-4 relative.  rho_f: J is not normal, so the yardstick is the float64 host iteration's own sensitivity - to a 1e-6
    relative perturbation of the start vector and to masks taken from an fp32 forward instead of a float64 one; the device gets 4x the
    larger of the two spreads (its differences are of exactly those two kinds), and fails regardless above 1e-2: the number is read to
    two digits against 1."""
    from deqsci_amd import jacobian
    gold = np.load(os.path.join(GOLDEN, "jacobian.npz"))
    case = "ffdnet_s1" if kind == "ffdnet" else kind
    solver, _ = _pipeline(kind)
    g = lambda k: torch.from_numpy(np.asarray(gold[f"{case}/a_{k}"], dtype=np.float32)).cuda()
    z, y, Phi, Phi_sum = g("z"), g("y"), g("Phi"), g("Phi_sum")
    sigma = float(gold[f"{case}/a_sigma"]) if kind == "ffdnet" else None
    op = solver.device_jacobian(z, y, Phi, Phi_sum, sigma=sigma)
    kw = dict(n_iters=30, window=10, seed=0)
    dev = jacobian.power_report(op, tuple(z.shape), **kw)
    host = jacobian.power_report_host(_host_op(solver, op, z, y, Phi, Phi_sum, sigma), tuple(z.shape), **kw)
    for key in ("lipschitz_f", "lipschitz_denoiser"):
        d = abs(dev[key][0] - host[key][0]) / host[key][0]
        print(f"{kind} {key}: device {dev[key][0]:.6f} host {host[key][0]:.6f} rel {d:.3e}")
        assert d <= 1e-4
    # rho_f's yardstick: the host iteration's own sensitivity
    h64 = jacobian.power_report_host(_host_op(solver, op, z, y, Phi, Phi_sum, sigma, mask_dtype=torch.float64), tuple(z.shape), of=("f",), **kw)
    h32 = jacobian.power_report_host(_host_op(solver, op, z, y, Phi, Phi_sum, sigma, mask_dtype=torch.float32), tuple(z.shape), of=("f",), **kw)
    orig = jacobian.start_vector
    try:
        def perturbed(N, seed=0):
            v = orig(N, seed)
            return v * (1 + 1e-6 * torch.randn(v.shape, generator=torch.Generator().manual_seed(77)))
        jacobian.start_vector = perturbed
        hp = jacobian.power_report_host(_host_op(solver, op, z, y, Phi, Phi_sum, sigma, mask_dtype=torch.float64), tuple(z.shape), of=("f",), **kw)
    finally:
        jacobian.start_vector = orig
    spread = max(abs(h32["rho_f"][0] - h64["rho_f"][0]), abs(hp["rho_f"][0] - h64["rho_f"][0])) / h64["rho_f"][0]
    d = abs(dev["rho_f"][0] - host["rho_f"][0]) / host["rho_f"][0]
    print(f"{kind} rho_f: device {dev['rho_f'][0]:.6f} host {host['rho_f'][0]:.6f} rel {d:.3e}; host spread {spread:.3e}")
    # measured on an MI355X (one run; profiles/r08_jacobian.json "test_record" holds these printed figures), relative to the host's rho_f:
    #   SimpleCNN         host spread 2.6e-08, device's difference 3.9e-09
    #   RealSN_SimpleCNN  host spread 9.0e-10, device's difference 1.5e-10
    #   ffdnet            host spread 4.0e-09, device's difference 6.3e-09
    assert d <= 1e-2 and d <= 4 * spread, (d, spread)


def test_harness_option_end_to_end():
    from deqsci_amd import harness
    from oracle import deqsci_oracle as orc
    clip = harness.load_test_data(os.path.join(orc.DATA_DIR, "traffic_cacti.mat"))
    clip["file"] = "traffic_cacti.mat"
    one = dict(clip, meas=clip["meas"][..., :1], gt=clip["gt"][..., :8])
    two = dict(clip, meas=clip["meas"][..., :2], gt=clip["gt"][..., :16])
    opt = dict(n_iters=12, window=4, seed=0)
    solver, deq = _pipeline("SimpleCNN", 30)
    _, plain = harness.evaluate(deq, [one])
    _, withj = harness.evaluate(deq, [one], jacobian=opt)
    assert plain[0].jacobian is None and plain[0].psnr == withj[0].psnr and torch.equal(plain[0].rec, withj[0].rec)
    j = withj[0].jacobian
    assert set(j) == {"lipschitz_f", "rho_f", "lipschitz_denoiser", "histories"} and len(j["rho_f"]) == 1
    # ... equals a direct call at the reconstruction
    Phi = torch.as_tensor(clip["mask"]).cuda()[None].contiguous()
    y = torch.as_tensor(one["meas"]).cuda().permute(2, 0, 1).contiguous()
    from deqsci_amd import operators
    direct = deq.jacobian_report(y, Phi, operators.phi_sum(Phi), withj[0].rec, **opt)
    for k in ("lipschitz_f", "rho_f", "lipschitz_denoiser"):
        assert j[k][0] == float(direct[k][0]), k
        assert np.isfinite(j[k][0]) and j[k][0] > 0
    print("traffic m0 SimpleCNN @30:", {k: j[k][0] for k in ("lipschitz_f", "rho_f", "lipschitz_denoiser")})
    # batching two measurements: per-sample values equal to the separate calls
    _, both = harness.evaluate(deq, [two], jacobian=opt)
    second = dict(clip, meas=clip["meas"][..., 1:2], gt=clip["gt"][..., 8:16])
    _, sep = harness.evaluate(deq, [second], jacobian=opt, batch=False)
    for k in ("lipschitz_f", "rho_f", "lipschitz_denoiser"):
        assert both[0].jacobian[k][0] == j[k][0] and both[0].jacobian[k][1] == sep[0].jacobian[k][0], k
    recs = []
    harness.test_solver_sci(deq, [one], save_image=False, verbose=False, records=recs, jacobian=opt)
    assert recs[0]["jacobian"]["rho_f"] == j["rho_f"][0]
    with pytest.raises(ValueError, match="gaptv"):
        harness.evaluate(None, [one], method="gaptv", jacobian=opt)


@pytest.mark.parametrize("snapshots", [None, (5, 8)])
def test_ffdnet_report_linearises_at_the_sigma_of_the_call_that_made_the_reconstruction(snapshots):
    """An Anderson run of M iterations issues f-calls 0 .. M-1 inside the loop and call M, z = f(z*), whose result is the reconstruction;
    FFDNet's call k runs at row k of the sigma schedule.  So the report of a 12-iteration forward is power_report on
    device_jacobian(sigma=sigma_schedule(13)[12]), whether or not snapshots (whose extra f-calls come behind, at rows of their own) were
    taken - and not the report at the row before."""
    from deqsci_amd import harness, jacobian, operators
    from deqsci_amd.engine import sigma_schedule
    from oracle import deqsci_oracle as orc
    M = 12
    clip = harness.as_clip(dict(harness.load_test_data(os.path.join(orc.DATA_DIR, "traffic_cacti.mat")), file="traffic_cacti.mat"))
    Phi = clip["mask"].cuda()[None].contiguous()
    y = clip["meas"].cuda().permute(2, 0, 1)[:2].contiguous()
    Phi_sum = operators.phi_sum(Phi)
    solver, deq = _pipeline("ffdnet", M)
    deq.snapshots = snapshots
    with torch.no_grad():
        rec = deq.forward(y, Phi, Phi_sum, initial_point=operators.initial_point(y, Phi, Phi_sum, None), train_flag=False).detach()
    info = deq._engine[1].last_info
    assert info["iterations"] == M - 1                                  # the tolerance test did not end the run early
    assert info["f_calls"] == M + 1 + len(snapshots or ())
    assert (info["snapshots"] is None) == (snapshots is None)
    kw = dict(n_iters=8, window=4, seed=0)
    got = deq.jacobian_report(y, Phi, Phi_sum, rec, **kw)
    table = sigma_schedule(M + 1)
    want = jacobian.power_report(solver.device_jacobian(rec, y, Phi, Phi_sum, sigma=float(table[M])), tuple(rec.shape), **kw)
    before = jacobian.power_report(solver.device_jacobian(rec, y, Phi, Phi_sum, sigma=float(table[M - 1])), tuple(rec.shape), **kw)
    for k in ("lipschitz_f", "rho_f", "lipschitz_denoiser"):
        print(f"ffdnet @{M} snapshots={snapshots} {k}: report {got[k]} at row {M} {want[k]} at row {M - 1} {before[k]}")
        assert np.array_equal(got[k], want[k]), k
        assert not np.array_equal(got[k], before[k]), k
