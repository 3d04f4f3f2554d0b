"""Checkpoint loading with the reference's conventions (video_sci_proxgrad.py:210-227):
pickle dict {'solver_state_dict', 'epoch', ...} whose keys are `nonlinear_op.<net keys>`, optional
DataParallel 'module.' prefixes; bare FFDNet state dicts (`net_gray.pth`, keys under 'module.');
and the plain `.npz` tensor archives shipped in deqsci_amd/weights/.  Unlike the reference, a
missing path is an error (the reference silently keeps random weights, :211)."""
import os

import numpy as np
import torch

WEIGHTS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights")


def _strip(k, prefixes=("module.",)):
    for p in prefixes:
        if k.startswith(p):
            k = k[len(p):]
    return k


def read_state_dict(path):
    """-> (state_dict with 'module.' stripped, epoch or None)"""
    if not os.path.exists(path):
        raise FileNotFoundError(f"checkpoint {path!r} not found (the reference would silently run with "
                                "random weights here; this build refuses)")
    if path.endswith(".npz"):
        arc = np.load(path)
        sd = {k: torch.from_numpy(arc[k]) for k in arc.files if not k.startswith("__")}
        epoch = int(arc["__epoch__"]) if "__epoch__" in arc.files else None
        # an archive split over several files (each within the size limit of a committed file: tests/golden/dncnn_noise15.npz): the
        # first names the others, which lie next to it
        for name in ([str(n) for n in arc["__parts__"]] if "__parts__" in arc.files else []):
            part = os.path.join(os.path.dirname(path), name)
            if os.path.basename(name) != name or not os.path.exists(part):
                raise FileNotFoundError(f"checkpoint {path!r} names the part {name!r}, which is not next to it")
            parc = np.load(part)
            for k in parc.files:
                if k in sd:
                    raise KeyError(f"checkpoint part {part!r} repeats the key {k!r}")
                if not k.startswith("__"):
                    sd[k] = torch.from_numpy(parc[k])
    else:
        obj = torch.load(path, map_location="cpu", weights_only=False)
        epoch = obj.get("epoch") if isinstance(obj, dict) else None
        sd = obj["solver_state_dict"] if isinstance(obj, dict) and "solver_state_dict" in obj else obj
    return {_strip(k): v for k, v in sd.items()}, epoch


def load_solver(solver, path):
    """solver.load_state_dict for a solver checkpoint; a bare denoiser state dict (no 'nonlinear_op.'
    prefix) is loaded into solver.nonlinear_op instead."""
    sd, epoch = read_state_dict(path)
    if all(k.startswith("nonlinear_op.") for k in sd):
        solver.load_state_dict(sd)
    else:
        solver.nonlinear_op.load_state_dict(sd)
    return epoch


def save_training(path, solver, epoch, optimizer, scheduler=None):
    """The reference's training checkpoint (training/sci_equilibrium_training.py:126-130, :143-147): a pickle of {'solver_state_dict',
    'epoch', 'optimizer_state_dict', 'scheduler_state_dict'} - the solver's parameters AND buffers (BatchNorm's running statistics, a
    RealSNConv2d's weight_u), which load_solver reads back.  scheduler=None stores None."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({'solver_state_dict': solver.state_dict(),
                'epoch': epoch,
                'optimizer_state_dict': optimizer.state_dict(),
                'scheduler_state_dict': None if scheduler is None else scheduler.state_dict()}, path)


def load_training(path, solver, optimizer=None, scheduler=None):
    """Resume from a save_training checkpoint (or one of the reference's): the solver as load_solver loads it and, where given and
    stored, the optimizer's and the scheduler's state -> the stored epoch (resume at epoch + 1, video_sci_proxgrad.py:216)."""
    epoch = load_solver(solver, path)
    if optimizer is None and scheduler is None:
        return epoch
    obj = torch.load(path, map_location="cpu", weights_only=False)
    for what, key in ((optimizer, 'optimizer_state_dict'), (scheduler, 'scheduler_state_dict')):
        if what is not None:
            if not isinstance(obj, dict) or obj.get(key) is None:
                raise KeyError(f"checkpoint {path!r} holds no {key!r}")
            what.load_state_dict(obj[key])
    return epoch


def shipped(name):
    """Path of a shipped archive: 'cnn', 'rsn_cnn' (reference models/*.ckpt) or 'ffdnet_gray'
    (networks/ffdnet/models/net_gray.pth - substitute for the reference's missing ffdnet.ckpt)."""
    return os.path.join(WEIGHTS_DIR, name + ".npz")
