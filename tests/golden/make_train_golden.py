#!/usr/bin/env python3
"""Generate tests/golden/train_simplecnn.npz by IMPORTING the reference on the CPU and running its own training loop: its
train_solver_sci, SCITrainingDatasetSubset, DEQFixedPoint and andersonexp, on the tiny training set of tests/train_cases.py.

    python tests/golden/make_train_golden.py

SimpleCNN from the reference's cnn.ckpt in .train(), torch.optim.Adam lr 1e-4, nn.MSELoss, batch 2, and_maxiters 12, 2 epochs of 2 steps,
the samples drawn in train_cases.ORDER through a sampler.  Stored: the per-step loss and PSNR, the first step's four gradients, the four
weights after step 4, the sample order, and `update_spread`:

Adam's first steps move every weight by about lr whatever the gradient's size, so an entry whose gradient is within rounding of zero
can go either way.  The loop is therefore run again with every gradient of every step moved by Gaussian noise of 1e-4 of the gradient's
L2 norm (g + 1e-4 |g| n / sqrt(numel), n ~ N(0, 1): the tolerance this project holds one training step to), under 3 seeds; the largest
relative L2 deviation of an update w_4 - w_0 from the unperturbed run's is `update_spread`, and a test allows 4 x that.  The three runs
must lie within 2 x their mean, or the file is not written (the case would be ill-posed: lengthen and_maxiters).

Shims of this generator (ref_shims.py's, plus): a recording torch.utils.tensorboard.SummaryWriter, tqdm as the identity, PIL where it
is absent, and the reference's end-of-epoch / periodic evaluation switched off (it evaluates a test set this run has none of; SimpleCNN
has no buffers an evaluation would move).  Runs only where the reference is mounted.  Nothing of the reference's text is stored: seeds
and the numbers its code computes.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                      # tests/train_cases.py
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the package
import ref_shims  # noqa: E402

ref_shims.install()


class _Writer:
    """torch.utils.tensorboard.SummaryWriter: keeps what the loop logs"""
    log = []

    def __init__(self, *a, **k):
        pass

    def add_scalar(self, name, value, global_step=None, walltime=None):
        _Writer.log.append((name, float(value), global_step))

    def flush(self):
        pass


sys.modules["torch.utils.tensorboard"].SummaryWriter = _Writer
try:
    import tqdm  # noqa: F401
except ImportError:
    import importlib.machinery
    _tqdm = types.ModuleType("tqdm")
    _tqdm.__spec__ = importlib.machinery.ModuleSpec("tqdm", None)
    _tqdm.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = _tqdm
try:
    import PIL.Image  # noqa: F401
except ImportError:
    _pil = types.ModuleType("PIL")
    _pil.Image = types.ModuleType("PIL.Image")
    sys.modules["PIL"], sys.modules["PIL.Image"] = _pil, _pil.Image

from networks.provable.model.SimpleCNN_models import DnCNN  # noqa: E402
from solvers.equilibrium_solvers_yaping import EquilibriumProxGradSCI  # noqa: E402
from solvers import new_equilibrium_utils_yaping as eq_utils  # noqa: E402
from training import sci_equilibrium_training as ref_training  # noqa: E402
from utils.cg_utils import A_torch_, At_torch_  # noqa: E402
from utils.sci_dataloader import SCITrainingDatasetSubset  # noqa: E402

import train_cases as tc  # noqa: E402
from deqsci_amd import checkpoint  # noqa: E402

ref_training.test_solver_sci = lambda **k: (0.0, {})            # no test set in this run
ref_training.tqdm = lambda it, *a, **k: it                      # no progress bar in the log
REF = ref_shims.REFERENCE_ROOT
NOISE, SEEDS = 1e-4, (1, 2, 3)


def build_solver():
    net = DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag="denoiser")
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    sd = torch.load(REF + "/models/cnn.ckpt", map_location="cpu", weights_only=False)["solver_state_dict"]
    solver.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})
    shipped, _ = checkpoint.read_state_dict(checkpoint.shipped("cnn"))          # the test starts from the shipped archive: the same weights
    for k, v in solver.state_dict().items():
        assert torch.equal(v, shipped[k]), k
    net.train()
    return solver


class _Adam(torch.optim.Adam):
    """The reference's optimizer, watched: keeps the first step's gradients and, for the spread runs, moves every gradient first."""

    def __init__(self, params, lr, noise_seed=None):
        super().__init__(params, lr=lr)
        self.first_grads = None
        self.gen = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)

    def step(self, closure=None):
        ps = [p for g in self.param_groups for p in g["params"]]
        if self.first_grads is None:
            self.first_grads = [p.grad.detach().clone() for p in ps]
        if self.gen is not None:
            for p in ps:
                n = torch.randn(p.grad.shape, generator=self.gen)
                p.grad.add_(n * (NOISE * float(p.grad.norm()) / p.grad.numel() ** 0.5))
        return super().step(closure)


def run(directory, noise_seed=None):
    solver = build_solver()
    start = [p.detach().clone() for p in solver.parameters()]
    dataset = SCITrainingDatasetSubset(directory + "gt/", directory + "measurement/", directory + "mask.mat")
    loader = torch.utils.data.DataLoader(dataset=dataset, batch_size=tc.BATCH, sampler=tc.RecordedSampler(), drop_last=True)
    optimizer = _Adam(solver.parameters(), tc.LR, noise_seed)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer=optimizer, step_size=10, gamma=0.9)
    deq = eq_utils.DEQFixedPoint(solver, eq_utils.andersonexp, m=5, beta=1.0, lam=1e-2, max_iter=tc.ITERS, tol=1e-5)
    _Writer.log = []
    ref_training.train_solver_sci(solver, loader, optimizer, directory + "model/", torch.nn.MSELoss(reduction='mean'), tc.EPOCHS, deq,
                                  scheduler=scheduler, print_every_n_steps=1, save_every_n_steps=1000, tflog_path=None)
    log = _Writer.log
    return {"loss": np.array([v for n, v, _ in log if n == "main/loss"]), "psnr": np.array([v for n, v, _ in log if n == "main/PSNR"]),
            "grads": optimizer.first_grads, "weights": [p.detach().clone() for p in solver.parameters()],
            "updates": [p.detach().double() - s.double() for p, s in zip(solver.parameters(), start)],
            "names": [n for n, _ in solver.named_parameters()]}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        directory = tc.write(tmp)
        os.makedirs(directory + "model/", exist_ok=True)
        base = run(directory)
        assert len(base["loss"]) == len(base["psnr"]) == tc.EPOCHS * tc.STEPS_PER_EPOCH and np.isfinite(base["loss"]).all()
        spreads = []
        for seed in SEEDS:
            other = run(directory, seed)
            spreads.append(max(float((o - b).norm() / b.norm()) for o, b in zip(other["updates"], base["updates"])))
    mean = sum(spreads) / len(spreads)
    print("loss per step", base["loss"], "PSNR per step", base["psnr"])
    print(f"update spread under {NOISE:g} gradient noise, seeds {SEEDS}: {['%.3e' % s for s in spreads]}; mean {mean:.3e}")
    if max(spreads) > 2 * mean:
        raise RuntimeError("the spread runs do not lie within 2 x their mean: ill-posed case, lengthen and_maxiters")
    out = {"loss": base["loss"], "psnr": base["psnr"], "order": np.array(tc.ORDER), "names": np.array(base["names"]),
           "update_spread": np.float64(max(spreads)), "spreads": np.array(spreads), "iters": np.int64(tc.ITERS), "lr": np.float64(tc.LR)}
    for i, (g, w) in enumerate(zip(base["grads"], base["weights"])):
        out[f"grad.{i}"] = g.numpy()
        out[f"weight.{i}"] = w.numpy()
    fn = os.path.join(HERE, "train_simplecnn.npz")
    np.savez_compressed(fn, **out)
    print("->", fn, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
