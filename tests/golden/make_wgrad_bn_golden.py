#!/usr/bin/env python3
"""Generate tests/golden/backward_dncnn_bn.npz by IMPORTING the reference on the CPU (tests/golden/ref_shims.py) and running its own code:
the training-mode DEQFixedPoint of make_golden.py's g8 - shape (2,24,20,4), seed 2024, Anderson m=5 beta=1 lam=1e-2, 12 iterations,
tol 1e-9, MSE loss - on the reference's conv + BatchNorm + ReLU denoiser, DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False) in eval mode.

    python tests/golden/make_wgrad_bn_golden.py

Runs only where the reference is mounted.  Nothing of the reference's text is stored: the seeded weights and BatchNorm state written
here, the inputs, and the numbers its modules compute from them.

The network has no shipped weights, so they are seeded (generator 77) and stored under their state-dict names (`state.*`):
  conv     N(0, 1) * scale * sqrt(2 / (9 cin))
  gamma    0.5 + U(0,1), entry 3 exactly 0, entries 7, 20 and 41 negated          beta    0.2 N(0,1), entry 3 = 0.3 (the gamma = 0 unit is live)
  mean     0.3 N(0,1)                                                            var     0.5 + U(0,1)
scale is the best conditioned of SCALES: at each, the reference is run again from x0 * (1 + 1e-7 randn(seed)) for the seeds 1 .. 4 (seed 1
is the perturbation of make_golden.py g10; one seed alone can miss a ReLU that sits on its threshold) and the figure is the largest
relative L2 by which a parameter's gradient moves in any of them; the smallest figure wins and must be below 1e-5.  It is stored (`conditioning`, per parameter; `scale`) and printed for profiles/wgrad.md.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

from networks.provable.model.SimpleCNN_models import DnCNN  # noqa: E402
from solvers.equilibrium_solvers_yaping import EquilibriumProxGradSCI  # noqa: E402
from solvers import new_equilibrium_utils_yaping as eq_utils  # noqa: E402
from utils.cg_utils import A_torch_, At_torch_, initial_point  # noqa: E402

SCALES = (1.0, 0.7, 0.5, 0.35, 0.25, 0.18, 0.1, 0.07, 0.05)
ITERS = 12
SEEDS = (1, 2, 3, 4)
CONDITIONING_TOL = 1e-5


def build(scale):
    net = DnCNN(1, num_of_layers=5, lip=0.0, no_bn=False, tag="denoiser")
    g = torch.Generator().manual_seed(77)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (scale * (2.0 / (9 * m.weight.shape[1])) ** 0.5)
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = 0.5 + torch.rand(64, generator=g)
            m.weight.data[3] = 0.0
            m.weight.data[[7, 20, 41]] *= -1.0
            m.bias.data = 0.2 * torch.randn(64, generator=g)
            m.bias.data[3] = 0.3
            m.running_mean.copy_(0.3 * torch.randn(64, generator=g))
            m.running_var.copy_(0.5 + torch.rand(64, generator=g))
    net.eval()
    return EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)


def problem():
    g = torch.Generator().manual_seed(2024)
    bsz, H, W, B = 2, 24, 20, 4
    Phi = (torch.rand(bsz, H, W, B, generator=g) < 0.5).float()
    Phi[:, 0, :2, :] = 0
    gt = torch.rand(bsz, H, W, B, generator=g)
    y = A_torch_(gt, Phi)
    Phi_sum = torch.sum(Phi, axis=3)
    Phi_sum[Phi_sum == 0] = 1
    return Phi, gt, y, Phi_sum


def run(scale, Phi, gt, y, Phi_sum, x0):
    solver = build(scale)
    for p in solver.parameters():
        p.requires_grad_(True)
    deq = eq_utils.DEQFixedPoint(solver, eq_utils.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=ITERS, tol=1e-9)
    rec = deq(y, Phi, Phi_sum, initial_point=x0)
    loss = torch.nn.MSELoss()(rec, gt)
    solver.zero_grad()
    loss.backward()
    return solver, deq, rec.detach(), loss.detach(), {name: p.grad.detach().clone() for name, p in solver.named_parameters()}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    Phi, gt, y, Phi_sum = problem()
    x0 = initial_point(y, Phi, Phi_sum, gt)
    x0ps = [x0 * (1 + 1e-7 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(seed))) for seed in SEEDS]
    best = None
    for scale in SCALES:
        result = run(scale, Phi, gt, y, Phi_sum, x0)
        deq, rec, grads = result[1], result[2], result[4]
        moved, rec_moved = {k: 0.0 for k in grads}, 0.0
        for x0p in x0ps:
            _, _, recp, _, gradsp = run(scale, Phi, gt, y, Phi_sum, x0p)
            moved = {k: max(moved[k], rel(gradsp[k], grads[k])) for k in grads}
            rec_moved = max(rec_moved, rel(recp, rec))
        print(f"scale {scale}: x0 perturbed by {rel(x0ps[0], x0):.3e} -> rec moves {rec_moved:.3e}, gradients move at most {max(moved.values()):.3e}"
              f" (forward res {deq.forward_res:.3e}, backward res {deq.backward_res:.3e})")
        if best is None or max(moved.values()) < max(best[2].values()):
            best = (scale, result, moved)
    scale, (solver, deq, rec, loss, grads), moved = best
    if max(moved.values()) >= CONDITIONING_TOL:
        raise RuntimeError(f"no scale of {SCALES} is well conditioned at {ITERS} iterations")
    print(f"chosen: scale {scale}, gradients move at most {max(moved.values()):.3e}")
    out = {"Phi": Phi, "gt": gt, "y": y, "Phi_sum": Phi_sum, "rec": rec, "loss": loss.double(),
           "forward_res": torch.tensor(deq.forward_res, dtype=torch.float64), "backward_res": torch.tensor(deq.backward_res, dtype=torch.float64),
           "scale": torch.tensor(scale, dtype=torch.float64), "iters": torch.tensor(ITERS),
           "conditioning": torch.tensor([moved[k] for k in grads], dtype=torch.float64)}
    for name, t in solver.nonlinear_op.state_dict().items():
        out["state." + name] = t.detach()
    for name, t in grads.items():
        out["grad." + name] = t
    fn = os.path.join(HERE, "backward_dncnn_bn.npz")
    np.savez_compressed(fn, **{k: v.numpy() for k, v in out.items()})
    print("->", fn, os.path.getsize(fn), "bytes; loss", float(loss), {k: float(v.norm()) for k, v in grads.items()})


if __name__ == "__main__":
    main()
