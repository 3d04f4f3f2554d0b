"""The reference's training loop (training/sci_equilibrium_training.py:28-150) and training data set (utils/sci_dataloader.py:163-239).

    train_solver_sci(...)        the reference's signature and control flow; what this build adds is keyword-only
    SCITrainingDatasetSubset     mask.mat + gt/*.mat + measurement/*.mat -> {'gt', 'mask', 'meas'} per item
    configure_training(deq, backend)   DEQFixedPoint's three switches (engine_options, implicit_backward, parameter_backward) in one place

Deviations from the reference, all of them where it could not run here or would crash:
  - TensorBoard is absent: `tflog_path` gets the same four scalars per step as JSON lines (scalars.jsonl in that directory).
  - the tensors go to the device of the solver's parameters instead of .cuda() (so the loop also runs on the CPU, for the tests).
  - with `test_dataloader=None` the evaluations (every save_every_n_steps steps, end of epoch) are skipped; the reference would raise.
  - evaluation is harness.evaluate (PSNR per clip as the reference's test_solver_sci), PNG export left to the command line.
  - `scheduler=None` is tolerated (no step, None in the checkpoint).
  - after a NaN or blown-up loss the reference reloads `save_model_path` itself, which under its own command line is a directory
    prefix and cannot be loaded: here a `save_model_path` that is a file is loaded as the reference would, otherwise the last checkpoint
    this run wrote (none yet: FileNotFoundError).
loss_function="device" (this build's): deqsci_amd.autograd.mse_loss_stats - loss, gradient, NaN check and the batch PSNR out of ONE pass
over the reconstruction and ONE read-back of three float64 words per step; nothing else copies the reconstruction to the host.
clip_grad_norm=MAX (this build's, off by default; the reference trains without clipping): the global gradient norm is clipped to MAX and a
step whose gradient holds a NaN or an Inf is skipped (deqsci_amd.optim), at the cost of one second read-back of three words per step.
"""
import json
import math
import os
import time
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import autograd as _ag
from . import checkpoint, harness, operators
from . import optim as _optim
from . import vjp as _vjp

TrainStep = namedtuple("TrainStep", "epoch step loss psnr lr nonfinite")
TrainingConfig = namedtuple("TrainingConfig", "backend engine_options implicit_backward parameter_backward reasons")

_GT_KEYS = ("patch_save", "p1", "p2", "p3")


def load_mat(path, key):
    """utils/sci_dataloader.py:163-214: key 'gt' (the first of patch_save / p1 / p2 / p3 the file has, / 255), 'meas' (/ 255) or 'mask',
    as float32.  MATLAB v7.3 (HDF5) files need h5py, as harness.load_test_data: NotImplementedError without it."""
    import scipy.io as sio
    if key not in ("gt", "meas", "mask"):
        raise ValueError(f"load_mat: unknown key {key!r} (expected 'gt', 'meas' or 'mask')")
    try:
        f = sio.loadmat(path)
        transpose = False
    except NotImplementedError as e:                      # MATLAB v7.3 = HDF5 (utils/sci_dataloader.py:188-210)
        try:
            import h5py
        except ImportError:
            raise NotImplementedError(f"{path}: MATLAB v7.3 files need h5py, which is not installed") from e
        f = h5py.File(path, 'r')
        transpose = True                                  # HDF5 keeps MATLAB's column-major order: transpose back
    if key == "gt":
        name = next((k for k in _GT_KEYS if k in f), None)
        if name is None:
            raise KeyError(f"{path}: none of {_GT_KEYS} found")
        data = np.float32(np.asarray(f[name]) / 255)
    elif key == "meas":
        data = np.float32(np.asarray(f["meas"]) / 255)
    else:
        data = np.float32(np.asarray(f["mask"]))
    return data.transpose() if transpose else data


class SCITrainingDatasetSubset(torch.utils.data.Dataset):
    """utils/sci_dataloader.py:218-239.  The directories are joined to the file names as strings, as in the reference: they end in '/'."""

    def __init__(self, gt_directory, meas_directory, mask_location):
        training_data = harness.directory_filelist(gt_directory)
        self.full_gt_filelist = [gt_directory + f for f in training_data]
        self.full_meas_filelist = [meas_directory + f for f in training_data]
        self.mask = load_mat(mask_location, 'mask')

    def __len__(self):
        return len(self.full_gt_filelist)

    def __getitem__(self, item):
        return {'gt': load_mat(self.full_gt_filelist[item], 'gt'), 'mask': self.mask, 'meas': load_mat(self.full_meas_filelist[item], 'meas')}


# ----------------------------------------------------------------------------- the backend switches
_CUSTOM_OPS = "custom A / At: the device paths use the HIP GAP projection"


def configure_training(deq, backend="device"):
    """Set deq.engine_options (its train_bn / train_realsn entries), deq.implicit_backward and deq.parameter_backward for a training run
    -> TrainingConfig(backend, engine_options, implicit_backward, parameter_backward, reasons).  backend="autograd": the defaults
    ("autograd" for both, the solve's f-calls on the torch module).  backend="device": per switch the first device mode that serves the
    denoiser as it stands (its train / eval mode included) - the weight gradients by the modes of vjp.GRAD_MODES in its order ("device",
    "device+realsn", "device+bn", "device+bn-train"), the implicit backward by vjp.eligibility in the order "device", "device+realsn" -
    with the engine's train-mode f-calls where the mode has them; a switch nothing serves stays "autograd" and reasons[switch] says why
    (reasons is empty when both run on the device)."""
    if backend not in ("device", "autograd"):
        raise ValueError(f"backend={backend!r}: expected 'device' or 'autograd'")
    options = {k: v for k, v in dict(deq.engine_options).items() if k not in {m.engine_option[0] for m in _vjp.GRAD_MODES if m.engine_option}}
    implicit = parameter = "autograd"
    reasons = {}
    if backend == "device":
        f = deq.f.module if isinstance(deq.f, torch.nn.DataParallel) else deq.f
        net = getattr(f, "nonlinear_op", None)
        custom = not (getattr(f, "A", None) is operators.A_torch_ and getattr(f, "At", None) is operators.At_torch_)
        tag = "ffdnet" if isinstance(net, _vjp._modules()[1]) else "denoiser"
        why = _CUSTOM_OPS if custom else None
        for mode in (() if custom else _vjp.GRAD_MODES):
            ok, why = mode.eligibility(net)
            if ok and getattr(net, "tag", None) != tag:
                ok, why = False, f"{type(net).__name__} under nonlinear_op tag {getattr(net, 'tag', None)!r}: the device call serves it under {tag!r} only"
            if ok:
                parameter = mode.switch
                options.update([mode.engine_option] if mode.engine_option else [])
                break
        if parameter == "autograd":
            reasons["parameter_backward"] = why
        why = _CUSTOM_OPS if custom else None
        for mode, realsn in (() if custom else (("device", False), ("device+realsn", True))):
            ok, why = _vjp.eligibility(net, train_realsn=realsn)
            if ok:
                implicit = mode
                break
        if implicit == "autograd":
            reasons["implicit_backward"] = why
    deq.engine_options = options
    deq.implicit_backward, deq.parameter_backward = implicit, parameter
    return TrainingConfig(backend, dict(options), implicit, parameter, reasons)


# ----------------------------------------------------------------------------- the loop
def _tflog(tflog_path):
    if tflog_path is None:
        return None
    path = tflog_path if str(tflog_path).endswith(".jsonl") else os.path.join(tflog_path, "scalars.jsonl")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    return open(path, "a")


def _to(t, device):
    return (t if isinstance(t, torch.Tensor) else torch.as_tensor(t)).to(device)


def train_solver_sci(single_iterate_solver, train_dataloader, optimizer,
                     save_model_path, loss_function, n_epochs, deep_eq_module,
                     use_dataparallel=False, scheduler=None,
                     print_every_n_steps=100, save_every_n_steps=1000, start_epoch=0,
                     test_dataloader=None, train_img_path=None, test_img_path=None, best_img_path=None,
                     tflog_path=None, *, max_steps=None, on_step=None, clip_grad_norm=None):
    """training/sci_equilibrium_training.py:28-150 (see the module's docstring for the deviations).  loss_function: a callable
    (rec, gt) -> loss, as nn.MSELoss() - loss.item() and the PSNR on the host, as the reference - or the string "device"
    (autograd.mse_loss_stats).  max_steps: stop after that many steps in all (the epoch it falls in ends there, with the epoch's
    bookkeeping).  on_step: called with a TrainStep after every optimizer step.  clip_grad_norm: None, or the largest global gradient
    norm - with a DeviceAdam its max_grad_norm is set (norm, clipping and step on the device, the statistics read back AFTER
    optimizer.step()); with any other optimizer optim.clip_grad_norm_ runs before the step and optimizer.step() is not called where the
    gradient is not finite.  The jsonl row then gains main/grad_norm and main/skipped, the print line the norm, the epoch's end the
    count of skipped steps.  -> the list of the TrainSteps."""
    if use_dataparallel:
        raise NotImplementedError("train_solver_sci: training is single-device in this build (use_dataparallel=True)")
    if isinstance(loss_function, str) and loss_function != "device":
        raise ValueError(f"loss_function={loss_function!r}: a callable, or the string 'device'")
    device_loss = isinstance(loss_function, str)
    fused_clip = clip_grad_norm is not None and isinstance(optimizer, _optim.DeviceAdam)
    if fused_clip:
        optimizer.max_grad_norm = float(clip_grad_norm)
    device = next(single_iterate_solver.parameters()).device
    start_time = time.time()
    cur_nimg = 0
    log = _tflog(tflog_path)
    history = []
    previous_loss = 10.0
    reset_flag = False
    best_psnr = 0
    loss_value = float("nan")
    steps_done = 0

    last_saved = [None]

    def save(name, epoch):
        checkpoint.save_training(save_model_path + name, single_iterate_solver, epoch, optimizer, scheduler)
        last_saved[0] = save_model_path + name

    def reload():
        # :46-49 loads `save_model_path` itself: a checkpoint file where the caller passes one; under the command line's directory
        # prefix (where the reference's torch.load would raise) the last checkpoint this run wrote.  Solver and optimizer, not the scheduler.
        path = save_model_path if os.path.isfile(save_model_path) else last_saved[0]
        if path is None:
            raise FileNotFoundError(f"the loss blew up and there is no checkpoint to go back to: {save_model_path!r} is no file and this run "
                                    "has saved none yet")
        checkpoint.load_training(path, single_iterate_solver, optimizer)

    try:
        for epoch in range(start_epoch, n_epochs):
            if reset_flag:
                reload()
            reset_flag = False
            psnr_sum = 0
            skipped_steps = 0
            for ii, sample_batch in enumerate(train_dataloader):
                cur_nimg += sample_batch['gt'].size(0)
                optimizer.zero_grad()
                gt_batch = _to(sample_batch['gt'], device)
                y = _to(sample_batch['meas'], device)
                Phi = _to(sample_batch['mask'], device)
                Phi_sum = torch.sum(Phi, axis=3)
                Phi_sum[Phi_sum == 0] = 1
                with torch.no_grad():
                    # (At(y, Phi); on CPU tensors - the host tests - the same products in torch)
                    initial_point = operators.initial_point(y, Phi, Phi_sum, gt_batch) if y.is_cuda else y.unsqueeze(3) * Phi
                reconstruction = deep_eq_module.forward(y, Phi, Phi_sum, initial_point=initial_point)
                total = reconstruction.numel()
                if device_loss:
                    loss, stats = _ag.mse_loss_stats(reconstruction, gt_batch)
                    host = stats.cpu()                                    # the step's ONE read-back: loss, NaN check, PSNR
                    loss_value, nonfinite = float(host[0]) / total, int(host[2])
                else:
                    loss = loss_function(reconstruction, gt_batch)
                    loss_value, nonfinite = loss.item(), None
                if np.isnan(loss_value):
                    print('Loss is nan!')
                    reset_flag = True
                    break
                loss.backward()
                grad_norm, skipped = None, False
                if clip_grad_norm is None:
                    optimizer.step()
                elif fused_clip:
                    optimizer.step()
                    grad_host = optimizer.last_grad_stats[:3].cpu()       # the step's second read-back, behind the Adam launch
                    grad_norm, skipped = float(grad_host[0]), float(grad_host[2]) > 0
                else:
                    params = [p for group in optimizer.param_groups for p in group["params"]]
                    grad_host = _optim.clip_grad_norm_(params, clip_grad_norm, return_stats=True)[:3].cpu()
                    grad_norm, skipped = float(grad_host[0]), float(grad_host[2]) > 0
                    if not skipped:
                        optimizer.step()
                skipped_steps += int(skipped)
                if ii == 0:
                    previous_loss = loss_value
                if device_loss:
                    sq = float(host[1])
                    PSNR = 10.0 * math.log10(total / sq) if sq > 0 else float("inf")
                else:
                    PSNR = harness.psnr(reconstruction.clip(0, 1).cpu().detach().numpy(), gt_batch.cpu().detach().numpy())
                psnr_sum += PSNR
                lr = optimizer.param_groups[0]['lr']
                stats_dict = OrderedDict([('main/PSNR', PSNR), ('main/loss', loss_value), ('config/lr', lr), ('main/best_PSNR', best_psnr)])
                if clip_grad_norm is not None:
                    stats_dict['main/grad_norm'], stats_dict['main/skipped'] = grad_norm, int(skipped)
                if log is not None:
                    log.write(json.dumps({"global_step": int(cur_nimg), "walltime": time.time() - start_time, **stats_dict}) + "\n")
                    log.flush()
                if ii % print_every_n_steps == 0:
                    print("Epoch: " + str(epoch) + " Step: " + str(ii) + " Loss: " + str(np.float32(loss_value)) + " PSNR: %2.2f dB" % PSNR +
                          " best PSNR (test): %2.2f dB" % best_psnr + " lr: %.8f" % lr +
                          ("" if clip_grad_norm is None else " grad norm: %.4e" % grad_norm + (" (not finite: step skipped)" if skipped else "")), flush=True)
                step = TrainStep(epoch, ii, loss_value, PSNR, lr, nonfinite)
                history.append(step)
                steps_done += 1
                if on_step is not None:
                    on_step(step)
                if (ii + 1) % save_every_n_steps == 0 and test_dataloader is not None:
                    cur_psnr, _ = harness.evaluate(deep_eq_module, test_dataloader, device=device, batch=False)
                    if cur_psnr > best_psnr:
                        best_psnr = cur_psnr
                        print('saving best model')
                        save('best.ckpt', epoch)
                if max_steps is not None and steps_done >= max_steps:
                    break
            avg_psnr = psnr_sum / len(train_dataloader)
            print('avg PSNR in epoch %d: %.2f dB' % (epoch, avg_psnr))
            if clip_grad_norm is not None:
                print('skipped steps (gradient not finite) in epoch %d: %d' % (epoch, skipped_steps))
            if (previous_loss - loss_value) / previous_loss < -10.0 or np.isnan(loss_value):
                reset_flag = True
            if scheduler is not None:
                scheduler.step()
            if not reset_flag:
                save('epoch_%d.ckpt' % epoch, epoch)
                print('dict saved!')
            if test_dataloader is not None:
                avg, _ = harness.evaluate(deep_eq_module, test_dataloader, device=device, batch=False)
                print('---------------------------------', 'Total Average PSNR: %.2f dB' % avg)
            if max_steps is not None and steps_done >= max_steps:
                break
    finally:
        if log is not None:
            log.close()
    return history
