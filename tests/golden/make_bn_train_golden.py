#!/usr/bin/env python3
"""Generate tests/golden/bn_train.npz by IMPORTING the reference on the CPU (tests/golden/ref_shims.py) and running its own code with the
BatchNorm2d layers in TRAIN mode - what the reference's training script runs: it calls learned_component.eval() under --inference only.

    python tests/golden/make_bn_train_golden.py

The arrays go, in order, into bn_train.npz, bn_train.part1.npz, ... - a new archive whenever the next array would take one past the
repository's limit for a committed file; a reader loads all of them and merges.  Runs only where the reference is mounted.  Nothing of the
reference's text is stored: inputs, seeded state and the numbers its modules compute from them.

a.  FFDNet (net_gray.pth; the same weights ship as deqsci_amd/weights/ffdnet_gray.npz and are NOT stored again) in .train() on
    make_golden.py's g8 problem - shape (2,24,20,4), seed 2024, Anderson m=5 beta=1 lam=1e-2, 12 iterations, tol 1e-9, MSE loss: one
    training step of the reference's DEQFixedPoint.  Stored: rec, loss, the 41 gradients (`a.grad.*`), every BatchNorm buffer after the step
    (`a.buffer.*`: 13 x running_mean, running_var, num_batches_tracked = 14 = 12 + 2 f-calls), sigma_after, the residuals.  The step is run
    again from x0 * (1 + 1e-7 randn(seed)) for the seeds 1 .. 4; the largest relative L2 by which each quantity moves in any of them is its
    conditioning figure (`a.conditioning.*`), and every one of them must stay below 1e-5 - the script fails otherwise.
b.  The seeded 5-layer conv + BN + ReLU DnCNN of make_wgrad_bn_golden.py (its build(), at the scale stored in backward_dncnn_bn.npz; gamma
    with an exact zero and three negative entries) in .train(): ONE f-call, no DEQ - through the DEQ this family is not well conditioned
    in train mode (its first-layer gradient moves 5e-4 .. 2e-3 at every scale).  x = the problem's x0 in planar form (8,1,24,20), v seeded:
    noise = net(x), (noise * v).sum().backward().  Stored: x, v, the state before (`b.state.*`), noise, every gradient (`b.grad.*`), the
    input gradient, the buffers after (`b.buffer.*`).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()

import make_wgrad_bn_golden as bn_golden  # noqa: E402  (the seeded DnCNN and the g8 problem)
from networks.ffdnet.models import FFDNet  # noqa: E402
from solvers.equilibrium_solvers_yaping import EquilibriumProxGradSCI  # noqa: E402
from solvers import new_equilibrium_utils_yaping as eq_utils  # noqa: E402
from utils.cg_utils import A_torch_, At_torch_, initial_point  # noqa: E402

ITERS = 12
SEEDS = (1, 2, 3, 4)
CONDITIONING_TOL = 1e-5


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def ffdnet_solver():
    net = FFDNet(num_input_channels=1, tag="ffdnet")
    sd = torch.load(ref_shims.REFERENCE_ROOT + "/networks/ffdnet/models/net_gray.pth", map_location="cpu", weights_only=False)
    net.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    net.train()
    return EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)


def step(Phi, gt, y, Phi_sum, x0):
    solver = ffdnet_solver()
    for p in solver.parameters():
        p.requires_grad_(True)
    deq = eq_utils.DEQFixedPoint(solver, eq_utils.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=ITERS, tol=1e-9)
    rec = deq(y, Phi, Phi_sum, initial_point=x0)
    loss = torch.nn.MSELoss()(rec, gt)
    solver.zero_grad()
    loss.backward()
    out = {"rec": rec.detach(), "loss": loss.detach().double()}
    for name, p in solver.nonlinear_op.named_parameters():
        out["grad." + name] = p.grad.detach().clone()
    for name, b in solver.nonlinear_op.named_buffers():
        out["buffer." + name] = b.detach().clone()
    extra = {"sigma_after": solver.noise_sigma.detach().clone(), "forward_res": torch.tensor(deq.forward_res, dtype=torch.float64),
             "backward_res": torch.tensor(deq.backward_res, dtype=torch.float64)}
    return out, extra


def case_a(out):
    Phi, gt, y, Phi_sum = bn_golden.problem()
    x0 = initial_point(y, Phi, Phi_sum, gt)
    base, extra = step(Phi, gt, y, Phi_sum, x0)
    moved = {k: 0.0 for k in base if k != "loss" and not k.endswith("num_batches_tracked")}
    for seed in SEEDS:
        x0p = x0 * (1 + 1e-7 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(seed)))
        got, _ = step(Phi, gt, y, Phi_sum, x0p)
        for k in moved:
            moved[k] = max(moved[k], rel(got[k], base[k]))
        for k in base:
            if k.endswith("num_batches_tracked"):
                assert int(got[k]) == int(base[k]) == ITERS + 2, (k, got[k], base[k])
    worst = {kind: max(v for k, v in moved.items() if k.startswith(kind)) for kind in ("rec", "grad.", "buffer.")}
    print("a. FFDNet in train mode, seeds", SEEDS, ": rec moves", f"{worst['rec']:.2e}", "gradients at most", f"{worst['grad.']:.2e}",
          "buffers at most", f"{worst['buffer.']:.2e}", "| forward res", float(extra["forward_res"]), "backward res", float(extra["backward_res"]))
    if max(moved.values()) >= CONDITIONING_TOL:
        raise RuntimeError(f"case a. is not well conditioned: {max(moved, key=moved.get)} moves {max(moved.values()):.3e} >= {CONDITIONING_TOL}")
    out.update({"a.Phi": Phi, "a.gt": gt, "a.y": y, "a.Phi_sum": Phi_sum, "a.x0": x0, "a.iters": torch.tensor(ITERS)})
    out.update({"a." + k: v for k, v in base.items()})
    out.update({"a." + k: v for k, v in extra.items()})
    out.update({"a.conditioning." + k: torch.tensor(v, dtype=torch.float64) for k, v in moved.items()})


def case_b(out):
    scale = float(np.load(os.path.join(HERE, "backward_dncnn_bn.npz"))["scale"])
    net = bn_golden.build(scale).nonlinear_op
    net.train()
    Phi, gt, y, Phi_sum = bn_golden.problem()
    x0 = initial_point(y, Phi, Phi_sum, gt)
    bsz, H, W, B = x0.shape
    x = x0.permute(0, 3, 1, 2).reshape(bsz * B, 1, H, W).contiguous().requires_grad_(True)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(99))
    out.update({"b.state." + k: t.detach().clone() for k, t in net.state_dict().items()})
    noise = net(x)
    net.zero_grad()
    (noise * v).sum().backward()
    out.update({"b.x": x.detach(), "b.v": v, "b.noise": noise.detach(), "b.grad_input": x.grad.detach(), "b.scale": torch.tensor(scale, dtype=torch.float64)})
    out.update({"b.grad." + k: p.grad.detach() for k, p in net.named_parameters()})
    out.update({"b.buffer." + k: t.detach().clone() for k, t in net.named_buffers()})
    print("b. DnCNN-5 + BN in train mode at scale", scale, ": |noise|", float(noise.detach().norm()), "|grad_input|", float(x.grad.norm()),
          {k: float(p.grad.norm()) for k, p in net.named_parameters()})


PART_BYTES = 900_000        # raw bytes per archive: a committed file stays below 1 MiB


def main():
    out = {}
    case_a(out)
    case_b(out)
    # the arrays in order, a new archive whenever the next one would not fit: bn_train.npz, bn_train.part1.npz, ... (load all, merge)
    parts, size = [{}], 0
    for k, v in out.items():
        a = v.numpy()
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    for old in os.listdir(HERE):
        if old.startswith("bn_train.") and old.endswith(".npz"):
            os.remove(os.path.join(HERE, old))
    for i, part in enumerate(parts):
        fn = os.path.join(HERE, "bn_train.npz" if i == 0 else f"bn_train.part{i}.npz")
        np.savez_compressed(fn, **part)
        print("->", fn, os.path.getsize(fn), "bytes,", len(part), "arrays")


if __name__ == "__main__":
    main()
