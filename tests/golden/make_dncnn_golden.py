#!/usr/bin/env python3
"""Generate the DnCNN-17 goldens by IMPORTING the reference on the CPU (tests/golden/ref_shims.py) and running its own code.

    python tests/golden/make_dncnn_golden.py weights     # dncnn_noise15.npz (+ .part1 / .part2): the checkpoint as plain tensor archives
    python tests/golden/make_dncnn_golden.py golden      # dncnn17.npz, and the growth curve on stdout (profiles/dncnn17.md)

Runs only where the reference is mounted.  Nothing of the reference's text is stored: only its pretrained tensors (data), inputs cut
from the shipped clip, and the numbers its modules compute from them.

weights   networks/provable/Pretrained_models/DnCNN_noise15.pth is a bare DataParallel state dict (92 keys `module.dncnn.N.*`, 557 967
          values).  It is re-serialised key by key, values untouched, as np.savez_compressed archives; one archive would be 2.0 MB, over
          the repository's limit for a committed file, so the keys go in checkpoint order into dncnn_noise15.npz, .part1.npz and .part2.npz,
          and the first names the others in `__parts__` (deqsci_amd.checkpoint.read_state_dict follows it and refuses a part that is
          missing or repeats a key).

golden    the problem: traffic measurement 0, rows 96:160, columns 64:128, 8 frames (the crop of trace_*.npz).
  (a)     x = the GAP step of the reference's solver on its initial point, as the (8,1,64,64) batch the denoiser sees; D(x) = one forward
          of the reference's DnCNN (networks/provable/model/models.py, eval mode) with the noise-15 weights; keys = its state-dict names.
  (b)     the reference's DEQFixedPoint(EquilibriumProxGradSCI, andersonexp m=5 beta=1 lam=1e-2 tol=1e-5) at max_iter = 10 and = K:
          the reconstruction, forward_res, and the residual of every f-call of the Anderson loop (the expression of
          new_equilibrium_utils_yaping.py:184 evaluated on the tensors the reference fed to and got from f; calls 0 and 1, which the
          reference does not score, included).
  K       the reference is run twice to 100 iterations, the second time from x0 * (1 + 1e-7 randn(seed 1)) (the perturbation of
          make_golden.py g10).  A run with max_iter = k returns what f returned at call k - 1 of the longer run (the loop is a prefix,
          f has no state for tag 'denoiser'), so d(k) = rel-L2 between the two runs' results at every horizon k comes out of the two
          runs.  K = the largest k <= 100 with d(k) <= 1e-5.  d is stored (growth) and printed.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

from networks.provable.model.models import DnCNN  # noqa: E402
from solvers.equilibrium_solvers_yaping import EquilibriumProxGradSCI  # noqa: E402
from solvers import new_equilibrium_utils_yaping as eq_utils  # noqa: E402
from utils.cg_utils import A_torch_, At_torch_, initial_point  # noqa: E402
from utils.sci_dataloader import load_test_data  # noqa: E402

REF = ref_shims.REFERENCE_ROOT
PTH = REF + "/networks/provable/Pretrained_models/DnCNN_noise15.pth"
PART_BYTES = 800 << 10            # raw tensor bytes per archive (the limit for a committed file is 1 MiB)
HORIZON_MAX = 100
GROWTH_TOL = 1e-5


def state_dict():
    sd = torch.load(PTH, map_location="cpu", weights_only=False)
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def weights():
    sd = torch.load(PTH, map_location="cpu", weights_only=False)
    parts, size = [{}], 0
    for k, v in sd.items():
        a = v.numpy()
        if size and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    names = ["dncnn_noise15.npz"] + [f"dncnn_noise15.part{i}.npz" for i in range(1, len(parts))]
    for i, (name, part) in enumerate(zip(names, parts)):
        extra = {"__parts__": np.array(names[1:])} if i == 0 else {}
        np.savez_compressed(os.path.join(HERE, name), **extra, **part)
        print("weights ->", name, len(part), "keys", os.path.getsize(os.path.join(HERE, name)), "bytes")


def build(iters):
    net = DnCNN(channels=1, num_of_layers=17, tag="denoiser")
    net.load_state_dict(state_dict())
    net.eval()
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    deq = eq_utils.DEQFixedPoint(solver, eq_utils.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=iters, tol=1e-5)
    return net, solver, deq


def problem():
    d = load_test_data(REF + "/data/test_gray/traffic_cacti.mat")
    sl = (slice(96, 160), slice(64, 128))
    Phi = torch.from_numpy(np.ascontiguousarray(d["mask"][sl]))[None]
    y = torch.from_numpy(np.ascontiguousarray(d["meas"][sl][..., 0]))[None]
    gt = torch.from_numpy(np.ascontiguousarray(d["gt"][sl][..., :8]))[None]
    Phi_sum = torch.sum(Phi, axis=3)
    Phi_sum[Phi_sum == 0] = 1
    return y, Phi, Phi_sum, gt


def run(iters, y, Phi, Phi_sum, x0):
    """-> (rec, forward_res, residual per f-call of the Anderson loop, what f returned at every call)"""
    _, solver, deq = build(iters)
    fed, ret = [], []
    orig = solver.forward

    def traced(z, yy, P, Ps):
        r = orig(z, yy, P, Ps)
        fed.append(z.detach().clone())
        ret.append(r.detach().clone())
        return r
    solver.forward = traced
    rec = deq.forward(y, Phi, Phi_sum, initial_point=x0, train_flag=False).detach()
    n_loop = len(fed) - 2                                   # (the closing z = f(z*) and the hook's f0 are not the loop's)
    res = [float((r - z).norm().item() / (1e-5 + r.norm().item())) for z, r in zip(fed[:n_loop], ret[:n_loop])]
    assert abs(res[-1] - deq.forward_res) <= 1e-12 + 1e-6 * deq.forward_res, (res[-1], deq.forward_res)
    return rec, float(deq.forward_res), np.array(res), ret[:n_loop]


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def golden():
    torch.manual_seed(0)
    y, Phi, Phi_sum, gt = problem()
    x0 = initial_point(y, Phi, Phi_sum, gt)
    net, _, _ = build(10)
    # (a) the GAP step on x0, in the denoiser's batch layout, and one forward
    z1 = x0 + At_torch_((y - A_torch_(x0, Phi)) / Phi_sum, Phi)
    x = z1.permute(0, 3, 1, 2).contiguous().view(8, 1, 64, 64)
    with torch.no_grad():
        Dx = net(x)
    # K: two runs to HORIZON_MAX, the second from a perturbed x0
    g = torch.Generator().manual_seed(1)
    x0p = x0 * (1 + 1e-7 * torch.randn(x0.shape, generator=g))
    _, _, res_a, ret_a = run(HORIZON_MAX, y, Phi, Phi_sum, x0)
    _, _, res_b, ret_b = run(HORIZON_MAX, y, Phi, Phi_sum, x0p)
    n = min(len(ret_a), len(ret_b))
    growth = np.array([rel(ret_b[k - 1], ret_a[k - 1]) for k in range(1, n + 1)])      # growth[k - 1] = d(k)
    ok = [k for k in range(3, n + 1) if growth[k - 1] <= GROWTH_TOL]
    if not ok:
        raise RuntimeError("no horizon at which the perturbed run stays within 1e-5")
    K = max(ok)
    print(f"x0 perturbation: rel-L2 {rel(x0p, x0):.3e}; f-calls of the two runs {len(ret_a)} / {len(ret_b)}")
    print("horizon k | d(k) = rel-L2 of the perturbed run's result | residual of the unperturbed run")
    for k in range(1, n + 1):
        print(f"{k:4d} | {growth[k - 1]:.3e} | {res_a[k - 1]:.3e}")
    print("K =", K)
    out = {"keys": np.array(list(net.state_dict().keys())), "y": y.numpy(), "Phi": Phi.numpy(), "Phi_sum": Phi_sum.numpy(), "gt": gt.numpy(),
           "x0": x0.numpy(), "a_x": x.numpy(), "a_out": Dx.numpy(), "K": np.int64(K), "growth": growth, "growth_res": res_a[:n],
           "x0_perturbation": np.float64(rel(x0p, x0))}
    for iters in (10, K):
        rec, fres, res, ret = run(iters, y, Phi, Phi_sum, x0)
        assert torch.equal(rec, ret[-1]) and torch.equal(ret[-1], ret_a[iters - 1]), "a shorter run is not a prefix of the longer one"
        mse = float(((torch.clamp(rec, 0, 1) - gt) ** 2).mean())
        out.update({f"b{iters}_rec": rec.numpy(), f"b{iters}_res": np.float64(fres), f"b{iters}_res_list": res,
                    f"b{iters}_psnr": np.float64(10 * np.log10(1.0 / mse))})
        print(f"(b) max_iter {iters}: f-calls in the loop {len(res)}  forward_res {fres:.4e}  PSNR {out[f'b{iters}_psnr']:.3f} dB")
    fn = os.path.join(HERE, "dncnn17.npz")
    np.savez_compressed(fn, **out)
    print("->", fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    for what in sys.argv[1:] or ["golden"]:
        {"weights": weights, "golden": golden}[what]()
