#!/usr/bin/env python3
"""Generate tests/golden/mask_grad.npz by IMPORTING the reference on the CPU (tests/golden/ref_shims.py) and running its own code: the
gradient of the training loss with respect to the MASK.  The reference's operators are plain torch, so its training-mode DEQFixedPoint
fills Phi.grad whenever Phi requires a gradient; this file records what it fills.

    python tests/golden/make_mask_grad_golden.py

The problem is make_golden.py's g8 - shape (2,24,20,4), seed 2024, Anderson m=5 beta=1 lam=1e-2, 12 iterations, tol 1e-9, MSE loss - with
a grey mask, 0.1 + 0.9 U(0,1), Phi[:, 0, :2, :] = 0 (two pixels whose Phi_sum is replaced by 1: no gradient reaches the mask through
Phi_sum there).  y = A(gt, Phi) and Phi_sum are formed from Phi under the tape, so the gradient has all three routes.  Cases:

    {SimpleCNN (cnn.ckpt), ffdnet (net_gray.pth)}  x  {ps: one mask per sample, sh: one (1,H,W,B) mask expanded over the batch}
                                                   x  {train: every denoiser parameter requires a gradient, frozen: none does}

Stored per case `<kind>.<ps|sh>.<train|frozen>.`: grad.Phi (the mask's own shape), rec, loss, forward_res, backward_res; sigma_after
for ffdnet; for the trainable cases the parameter gradients - whole (`grad.<name>`) where a parameter has at most 4096 elements, the
first two output channels (`gradslice.<name>` = grad[:2]) of the 64 -> 64 convolutions, which keeps the file at a few hundred KB (the
whole gradients are checked against a run with the mask as data, which tests/golden/backward*.npz hold to the reference).
`conditioning`: per case, the largest relative L2 by which grad.Phi moves when x0 moves by 1e-7 relative (seeds 1 .. 4, as in
make_wgrad_bn_golden.py); the file is not written unless every figure is below 1e-5.

Runs only where the reference is mounted.  Nothing of the reference's text is stored: inputs and the numbers its modules compute.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

from networks.ffdnet.models import FFDNet  # noqa: E402
from networks.provable.model.SimpleCNN_models import DnCNN  # noqa: E402
from solvers.equilibrium_solvers_yaping import EquilibriumProxGradSCI  # noqa: E402
from solvers import new_equilibrium_utils_yaping as eq_utils  # noqa: E402
from utils.cg_utils import A_torch_, At_torch_, initial_point  # noqa: E402

REF = ref_shims.REFERENCE_ROOT
ITERS = 12
SEEDS = (1, 2, 3, 4)
CONDITIONING_TOL = 1e-5
SMALL = 4096
KINDS, MASKS, PARAMS = ("SimpleCNN", "ffdnet"), ("ps", "sh"), ("train", "frozen")


def build_solver(kind):
    """make_golden.py's build_solver for the two denoisers with shipped weights."""
    if kind == "ffdnet":
        net = FFDNet(num_input_channels=1, tag="ffdnet")
        sd = torch.load(REF + "/networks/ffdnet/models/net_gray.pth", map_location="cpu", weights_only=False)
        net.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    else:
        net = DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="denoiser")
    net.eval()
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    if kind == "SimpleCNN":
        sd = torch.load(REF + "/models/cnn.ckpt", map_location="cpu", weights_only=False)["solver_state_dict"]
        solver.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    return solver


def problem():
    g = torch.Generator().manual_seed(2024)
    bsz, H, W, B = 2, 24, 20, 4
    Phi = 0.1 + 0.9 * torch.rand(bsz, H, W, B, generator=g)
    Phi[:, 0, :2, :] = 0
    gt = torch.rand(bsz, H, W, B, generator=g)
    return {"ps": Phi, "sh": Phi[:1].clone()}, gt


def run(kind, Phi_data, gt, trainable, perturb=None):
    bsz = gt.shape[0]
    leaf = Phi_data.clone().requires_grad_(True)
    Phi = leaf.expand(bsz, -1, -1, -1)
    y = A_torch_(gt, Phi)
    Phi_sum = torch.sum(Phi, axis=3)
    Phi_sum[Phi_sum == 0] = 1
    solver = build_solver(kind)
    for p in solver.parameters():
        p.requires_grad_(trainable)
    deq = eq_utils.DEQFixedPoint(solver, eq_utils.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=ITERS, tol=1e-9)
    x0 = initial_point(y, Phi, Phi_sum, gt).detach()
    if perturb is not None:
        x0 = x0 * (1 + 1e-7 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(perturb)))
    rec = deq(y, Phi, Phi_sum, initial_point=x0)
    loss = torch.nn.MSELoss()(rec, gt)
    solver.zero_grad()
    loss.backward()
    out = {"grad.Phi": leaf.grad.detach().clone(), "rec": rec.detach(), "loss": loss.detach().double(),
           "forward_res": torch.tensor(deq.forward_res, dtype=torch.float64), "backward_res": torch.tensor(deq.backward_res, dtype=torch.float64)}
    if kind == "ffdnet":
        out["sigma_after"] = solver.noise_sigma.detach().clone()
    if trainable:
        for name, p in solver.named_parameters():
            if p.numel() <= SMALL:
                out["grad." + name] = p.grad.detach().clone()
            else:
                out["gradslice." + name] = p.grad.detach()[:2].clone()
    return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    masks, gt = problem()
    out = {"Phi.ps": masks["ps"], "Phi.sh": masks["sh"], "gt": gt, "iters": torch.tensor(ITERS)}
    cases, cond = [], []
    for kind in KINDS:
        for mask in MASKS:
            for params in PARAMS:
                tag = f"{kind}.{mask}.{params}"
                res = run(kind, masks[mask], gt, params == "train")
                moved = max(rel(run(kind, masks[mask], gt, params == "train", seed)["grad.Phi"], res["grad.Phi"]) for seed in SEEDS)
                print(f"{tag}: loss {float(res['loss']):.6e} |grad.Phi| {float(res['grad.Phi'].norm()):.4e} forward res {float(res['forward_res']):.3e} "
                      f"backward res {float(res['backward_res']):.3e}; grad.Phi moves {moved:.3e} under x0 (1 + 1e-7 randn)")
                cases.append(tag)
                cond.append(moved)
                for k, v in res.items():
                    out[f"{tag}.{k}"] = v
    if max(cond) >= CONDITIONING_TOL:
        raise RuntimeError(f"grad.Phi moves by {max(cond):.3e} >= {CONDITIONING_TOL}: not a golden")
    out["conditioning"] = torch.tensor(cond, dtype=torch.float64)
    fn = os.path.join(HERE, "mask_grad.npz")
    np.savez_compressed(fn, cases=np.array(cases), **{k: v.numpy() for k, v in out.items()})
    print("->", fn, os.path.getsize(fn), "bytes; conditioning", max(cond))


if __name__ == "__main__":
    main()
