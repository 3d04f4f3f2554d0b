"""Command-line driver with the reference's flags (video_sci_proxgrad.py:23-49): inference, and training with `--inference False`.

    python -m deqsci_amd.cli --denoiser ffdnet --loadpath deqsci_amd/weights/ffdnet_gray.npz \\
        --testpath data/test_gray/ --and_maxiters 180 --inference True [--gpu_ids 0,1,2,3]

Every flag of the reference parses (so its test_*.sh and train_*.sh command lines run unchanged); --etainit and --sigma are accepted and
ignored.  `--inference False` trains (deqsci_amd.training.train_solver_sci, the reference's loop): --trainpath DIR/ holds mask.mat, gt/ and
measurement/; --n_epochs --batch_size --lr --lr_gamma --sched_step --print_every_n_steps --save_every_n_steps as in the reference; resumed
from --loadpath (a missing file is an error; without the flag: random weights), checkpoints under --savepath + 'model/'.  Single device.  `--train_backend device|autograd`,
`--seed`, `--max_steps` and `--clip_grad_norm` are this build's ("Training").
`--trainvideos DIR --trainmask FILE` (this build's) train from raw video in place of --trainpath: patches of --patch_size x --patch_size x
--frames are cut out of the videos, turned (--augment) and measured on the device, --patches_per_epoch per epoch (deqsci_amd.synth).

    python -m deqsci_amd.cli --inference False --denoiser SimpleCNN --loadpath deqsci_amd/weights/cnn.npz --trainpath data/train/ \\
        --savepath save/cnn/ --and_maxiters 30 --batch_size 8 --lr 1e-4 --n_epochs 80

`--gpu_ids a,b,..` with more than one id is this build's addition: one process per listed GPU, every clip's
measurements sharded over them (deqsci_amd.distributed), rank 0 prints and writes the PNGs.
`--ssim` (also this build's) adds the per-clip SSIM and a 'Total Average SSIM' line (window 11, `--ssim_mode same|valid`).
`--init_point gaptv` starts the DEQ from GAP-TV (the reference's commented-out initial point) instead of At(y, Phi); `--baseline gaptv`
reconstructs by GAP-TV alone, with no DEQ (both this build's; deqsci_amd.gaptv).
`--snapshots 10,30,100` (this build's) also scores the clips at those iteration horizons out of the SAME run (one extra f-call each) and
prints one '[and_maxiters K] Total Average PSNR' line per horizon after the usual lines; `--trace FILE.json` writes the PSNR and the
residual of every f-call, per clip and measurement.
`--jacobian [N_ITERS]` (this build's) adds the local Lipschitz constant and spectral radius of f and the Lipschitz constant of the noise
predictor at every reconstruction (deqsci_amd.jacobian) to each clip line and one 'Total Average' line per quantity after the totals;
`--jacobian_json FILE` writes the per-measurement values and the iterations' histories.
`--solver broyden` (this build's) solves the fixed point with Broyden's method (deqsci_amd.broyden, the reference's
broyd_equilibrium_utils.broyden on the device) instead of Anderson acceleration: `--broyden_threshold` steps at most (default:
--and_maxiters), stopped when |f(z) - z| over the batch falls below `--broyden_eps`.  It runs on the generic solver path, so
--snapshots / --trace (the engine's) are refused with it.
`--solver epsilon2` (this build's) solves it with the vector epsilon-algorithm (deqsci_amd.epsilon2, the reference's epsilon2 on the
device): --and_maxiters iterations of two f-calls at most, stopped when |x_new - x| / |x_new| over the batch falls below `--eps2_tol`;
`--eps2_lam` is the regulariser of its denominator.  The generic solver path too: --snapshots / --trace are refused.
`--solver picard` (this build's) runs the plain iteration z <- f(z) (forward_iteration) on the engine, --and_maxiters iterations at most;
--snapshots / --trace work with it.
`--meas_noise_sigma S --meas_noise_gain G --meas_bits N --meas_full_scale F --noise_seed K` (this build's) put read noise (S grey levels),
shot noise and an N-bit ADC on the measurements (deqsci_amd.noise): the test measurements in inference - one line says so -, the
synthesised training measurements with --inference False --trainvideos; refused with --trainpath (python -m deqsci_amd.synth write makes
a noisy directory).  The reference's --sigma stays ignored.
"""
import argparse
import os
import sys
import time

import torch

from . import checkpoint, distributed
from .harness import (SCITestDataset, clip_line, evaluate, jacobian_document, png_payloads, print_horizons, print_jacobian_totals,
                      solver_line, trace_document, write_png)
from .networks import DnCNN, FFDNet
from .noise import add_noise_arguments, noise_from_arguments
from .operators import A_torch_, At_torch_
from .broyden import broyden_fixed_point
from .epsilon2 import epsilon2
from .solvers import DEQFixedPoint, EquilibriumProxGradSCI, andersonexp, forward_iteration

SHIPPED = {'ffdnet': 'ffdnet_gray', 'SimpleCNN': 'cnn', 'RealSN_SimpleCNN': 'rsn_cnn'}
# --train_backend's default: decided by the measurement in profiles/train.md (tools/train_bench.py)
TRAIN_BACKEND_DEFAULT = 'device'
# denoisers the reference's command line names and has weights for, but none trained for SCI: no shipped default, --loadpath names the checkpoint
NO_DEFAULT = {'DnCNN': "the Provable-PnP DnCNN of 17 layers (a Gaussian denoiser: networks/provable/Pretrained_models/DnCNN_noise{5,15,40}.pth of the "
                       "reference, or tests/golden/dncnn_noise15.npz of this repository)"}


def default_loadpath(denoiser, loadpath=''):
    """--loadpath as given, else the shipped archive of the denoiser; a denoiser without one (NO_DEFAULT) needs the flag: ValueError."""
    if loadpath:
        return loadpath
    if denoiser in NO_DEFAULT:
        raise ValueError(f"--denoiser {denoiser} has no shipped weights: pass --loadpath CHECKPOINT ({NO_DEFAULT[denoiser]})")
    return checkpoint.shipped(SHIPPED[denoiser])


def build_denoiser(name, n_channels=1):
    """Factory of video_sci_proxgrad.py:145-185 restricted to the denoisers with shipped SCI weights, and DnCNN (:172-174: the reference's
    networks/provable/model/models.py:DnCNN - 17 layers, BatchNorm, the same state-dict keys - whose weights --loadpath names)."""
    if name == 'ffdnet':
        return FFDNet(num_input_channels=n_channels, tag='ffdnet')
    if name == 'SimpleCNN':
        return DnCNN(1, num_of_layers=4, lip=0.0, no_bn=True, tag='denoiser')
    if name == 'RealSN_SimpleCNN':
        return DnCNN(1, num_of_layers=4, lip=1.0, no_bn=True, tag='denoiser')
    if name == 'DnCNN':
        return DnCNN(1, num_of_layers=17, lip=0.0, no_bn=False, tag='denoiser')
    raise NotImplementedError('unknown denoiser!')


def build_pipeline(denoiser, loadpath=None, and_maxiters=100, and_m=5, and_beta=1.0, device="cuda", solver_name="anderson", broyden_threshold=None,
                   broyden_eps=1e-5, eps2_tol=1e-2, eps2_lam=1e-4):
    net = build_denoiser(denoiser).eval()
    solver = EquilibriumProxGradSCI(A=A_torch_, At=At_torch_, nonlinear_operator=net, eta=0.2, minval=-1, maxval=1)
    if loadpath:
        checkpoint.load_solver(solver, loadpath)
    solver = solver.to(device)
    if solver_name == "broyden":
        deq = DEQFixedPoint(solver, broyden_fixed_point, threshold=and_maxiters if broyden_threshold is None else broyden_threshold, eps=broyden_eps)
    elif solver_name == "epsilon2":
        deq = DEQFixedPoint(solver, epsilon2, max_iter=and_maxiters, tol=eps2_tol, lam=eps2_lam)
    elif solver_name == "picard":
        deq = DEQFixedPoint(solver, forward_iteration, max_iter=and_maxiters, tol=1e-5)
    elif solver_name == "anderson":
        deq = DEQFixedPoint(solver, andersonexp, m=and_m, beta=and_beta, lam=1e-2, max_iter=and_maxiters, tol=1e-5)
    else:
        raise ValueError(f"solver_name must be 'anderson', 'broyden', 'epsilon2' or 'picard', got {solver_name!r}")
    return solver, deq


def parse_snapshots(text):
    """'10,30,100' -> (10, 30, 100) (argparse type of --snapshots; the engine checks the values against --and_maxiters)."""
    try:
        out = tuple(int(v) for v in str(text).split(',') if v.strip() != '')
    except ValueError:
        raise argparse.ArgumentTypeError(f"--snapshots wants comma-separated iteration counts, got {text!r}")
    if not out:
        raise argparse.ArgumentTypeError("--snapshots wants at least one iteration count")
    return out


def write_trace(path, results):
    """--trace FILE.json: {clip: {measurement: {"psnr": [...], "res": [...]}}}, one value per issued f-call of the iteration."""
    import json
    with open(path, "w") as fh:
        json.dump(trace_document(results), fh)
        fh.write("\n")


def parser():
    p = argparse.ArgumentParser(description="DEQ-SCI inference and training on MI355X")
    p.add_argument('--gpu_ids', default='0')
    p.add_argument('--and_maxiters', default=100, type=int)
    p.add_argument('--and_beta', type=float, default=1.0)
    p.add_argument('--and_m', type=int, default=5)
    p.add_argument('--denoiser', default='ffdnet')
    p.add_argument('--savepath', default="./save/test/")
    p.add_argument('--loadpath', default='')
    p.add_argument('--testpath', default="./data/test_gray/")
    p.add_argument('--inference', default='True')
    p.add_argument('--conv64', default='auto', choices=['auto', 'fast', 'fast32', 'f22', 'f44', 's16'],
                   help="(this build) kernel of the denoiser's 64->64 layers: auto = split-fp16 direct convolution on the f16 matrix cores / "
                        "Winograd F(2x2,3x3), the faster per launch; fast32 = fp32 MFMA arithmetic only")
    p.add_argument('--anderson_arith', default='reference', choices=['reference', 'float64'],
                   help="(this build) how alpha is computed: reference (default) = the reference's own arithmetic - the fp32 Gram of "
                        "new_equilibrium_utils_yaping.py:177-178 in the summation order of its torch.bmm, fp32 LU - which reproduces the reference's "
                        "ensemble statistics on the chaotic FFDNet + Anderson @180 configuration (DESIGN.md section 5); float64 = Gram and solve in "
                        "float64 (exact; 4 %% faster at eight measurements per call, 14 %% at one)")
    p.add_argument('--batch_measurements', nargs='?', const='clip', default=None, choices=['clip', 'all'],
                   help="(this build) clip: a clip's measurements as ONE engine batch instead of the reference's one-by-one schedule (implied by "
                        "more than one --gpu_ids entry, which shards them); all: the measurements of all clips of one frame size as one batch "
                        "(the three shipped clips: one call of eight measurements - what the device is fastest at)")
    p.add_argument('--ssim', action='store_true',
                   help="(this build) also report SSIM (the reference's pytorch_ssim per frame, window 11, on the device): per clip and a "
                        "'Total Average SSIM' line after the PSNR lines")
    p.add_argument('--ssim_mode', default=None, choices=['same', 'valid'],
                   help="(this build) same (default) = the mean over the whole zero-padded SSIM map, as pytorch_ssim; valid = over the "
                        "map values whose window lies inside the frame.  Implies --ssim")
    p.add_argument('--init_point', default='At', choices=['At', 'gaptv'],
                   help="(this build) the DEQ's starting point: At (default) = At(y, Phi), the reference's initial_point; gaptv = GAP-TV, 40 "
                        "iterations, step 1, TV weight 0.3 (the reference's commented-out initialiser), timed as part of the reconstruction")
    p.add_argument('--baseline', default=None, choices=['gaptv'],
                   help="(this build) reconstruct by the classical baseline alone, no DEQ: gaptv = GAP-TV (40 iterations, step 1, TV weight "
                        "0.3).  The same clip lines, totals, PNGs and --ssim handling")
    p.add_argument('--snapshots', default=None, type=parse_snapshots, metavar='K1,K2,..',
                   help="(this build) also score the clips at these iteration horizons (each smaller than --and_maxiters), out of the same run: "
                        "one '[and_maxiters K] Total Average PSNR' line per horizon after the usual lines (with SSIM under --ssim)")
    p.add_argument('--trace', default=None, metavar='FILE.json',
                   help="(this build) write the PSNR and the residual of every f-call, per clip and measurement, to FILE.json")
    p.add_argument('--jacobian', nargs='?', const=30, default=None, type=int, metavar='N_ITERS',
                   help="(this build) also report, at every reconstruction, the local Lipschitz constant Lip(f) and the spectral radius rho(f) of "
                        "the fixed-point map and the Lipschitz constant Lip(D) of the noise predictor (power iterations of N_ITERS steps, "
                        "default 30): per clip and one 'Total Average' line per quantity")
    p.add_argument('--solver', default='anderson', choices=['anderson', 'broyden', 'epsilon2', 'picard'],
                   help="(this build) the fixed-point solver: anderson (default) = Anderson acceleration on the engine; broyden = Broyden's method "
                        "(the reference's broyd_equilibrium_utils.broyden, HIP step kernels) on the generic solver path; epsilon2 = the vector "
                        "epsilon-algorithm (the reference's epsilon2, HIP step kernels) on the generic solver path, --and_maxiters iterations of "
                        "two f-calls at most; picard = the plain iteration z <- f(z) (forward_iteration) on the engine")
    p.add_argument('--broyden_threshold', default=None, type=int,
                   help="(this build) --solver broyden: the largest number of steps (default: --and_maxiters); the history keeps min(threshold, 27) terms")
    p.add_argument('--broyden_eps', default=1e-5, type=float,
                   help="(this build) --solver broyden: stop when |f(z) - z| over the batch of a call falls below this")
    p.add_argument('--eps2_tol', default=1e-2, type=float,
                   help="(this build) --solver epsilon2: stop when |x_new - x| / |x_new| over the batch of a call falls below this")
    p.add_argument('--eps2_lam', default=1e-4, type=float,
                   help="(this build) --solver epsilon2: the regulariser added to |d2|^2 in the extrapolation's denominator")
    p.add_argument('--jacobian_json', default=None, metavar='FILE',
                   help="(this build) write the per-measurement Jacobian values and the histories of their iterations to FILE.  Implies --jacobian")
    train = p.add_argument_group("training (--inference False)")
    train.add_argument('--n_epochs', type=int, default=80)
    train.add_argument('--batch_size', type=int, default=1)
    train.add_argument('--lr', type=float, default=0.0001)
    train.add_argument('--lr_gamma', type=float, default=0.9)
    train.add_argument('--sched_step', type=int, default=10)
    train.add_argument('--trainpath', default="", help="directory with mask.mat, gt/ and measurement/ (joined as strings: end it in '/')")
    train.add_argument('--trainvideos', default="", metavar='DIR',
                       help="(this build) train from raw video instead of --trainpath: a directory of .npy ((T,H,W) or (T,H,W,3) uint8) / .mat (key "
                            "'orig') videos; patches are cut, turned and measured on the device, per batch (deqsci_amd.synth)")
    train.add_argument('--trainmask', default="", metavar='FILE',
                       help="(this build) with --trainvideos: a .mat with key 'mask' (a test clip will do); its leading --patch_size x --patch_size x --frames corner is used")
    train.add_argument('--patches_per_epoch', type=int, default=1024, help="(this build) with --trainvideos: the samples drawn per epoch")
    train.add_argument('--patch_size', type=int, default=256, help="(this build) with --trainvideos: the side of a patch")
    train.add_argument('--frames', type=int, default=8, help="(this build) with --trainvideos: the frames of a measurement")
    train.add_argument('--augment', default='flip,transpose,reverse',
                       help="(this build) with --trainvideos: a comma-separated choice of flip, transpose, reverse (the clip played backwards), or none")
    train.add_argument('--print_every_n_steps', type=int, default=1)
    train.add_argument('--save_every_n_steps', type=int, default=50)
    train.add_argument('--train_backend', default=TRAIN_BACKEND_DEFAULT, choices=['device', 'autograd'],
                       help="(this build) device = the backward, the loss / PSNR / NaN glue and Adam on the HIP kernels, as far as the denoiser "
                            "is served (training.configure_training prints what it chose); autograd = torch's, as the reference")
    train.add_argument('--seed', type=int, default=None, help="(this build) torch.manual_seed before the data loader is built (the shuffle)")
    train.add_argument('--max_steps', type=int, default=None, help="(this build) stop after this many training steps in all")
    train.add_argument('--clip_grad_norm', type=float, default=None,
                       help="(this build) clip the global gradient norm to this value and skip a step whose gradient is not finite "
                            "(deqsci_amd.optim: on the device with --train_backend device); default: no clipping, as the reference")
    add_noise_arguments(p.add_argument_group(
        "sensor noise (this build)",
        "read noise, shot noise and an ADC on the measurements (deqsci_amd.noise, csrc/noise.hip): in inference on the test measurements, "
        "measurement m of clip k under the sequence number (k << 32) | m whatever the batching or the number of GPUs; with --inference False "
        "--trainvideos on the training measurements (the evaluation on --testpath stays clean).  Refused with --trainpath: write a noisy "
        "directory with python -m deqsci_amd.synth write"))
    ignored = p.add_argument_group("accepted for command-line compatibility, unused")
    ignored.add_argument('--etainit', type=float, default=0.9)
    ignored.add_argument('--sigma', type=int, default=0)
    return p


def train(args):
    """--inference False (video_sci_proxgrad.py:98-135, 193-202, 241-270): the denoiser in train mode, Adam + StepLR, MSELoss, a shuffled
    DataLoader over --trainpath, resumed from --loadpath, checkpoints under --savepath + 'model/'."""
    from . import training
    from .optim import DeviceAdam
    _, _, _, dev = distributed.init_from_env("nccl")
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.trainvideos:
        dataloader = None                                             # (built below: its first epoch is the one the checkpoint continues at)
    else:
        dataset = training.SCITrainingDatasetSubset(args.trainpath + 'gt/', args.trainpath + 'measurement/', args.trainpath + 'mask.mat')
        dataloader = torch.utils.data.DataLoader(dataset=dataset, batch_size=args.batch_size, shuffle=True, drop_last=True, pin_memory=True)
    test_dataset = SCITestDataset(args.testpath) if args.testpath and os.path.isdir(args.testpath) else None
    solver, deq = build_pipeline(args.denoiser, None, args.and_maxiters, args.and_m, args.and_beta, device=dev)
    solver.nonlinear_op.train()
    for p in solver.parameters():
        p.requires_grad_(True)
    device = args.train_backend == 'device'
    optimizer = (DeviceAdam if device else torch.optim.Adam)(params=solver.parameters(), lr=args.lr)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer=optimizer, step_size=args.sched_step, gamma=args.lr_gamma)
    start_epoch = 0
    if args.loadpath:
        epoch = checkpoint.load_solver(solver, args.loadpath)         # (the solver alone, as the reference: optimizer and scheduler start afresh)
        start_epoch = 0 if epoch is None else int(epoch) + 1
        print('loaded dict!')
        if start_epoch:
            print(f"the checkpoint's epoch is {epoch}: training continues at epoch {start_epoch} of --n_epochs {args.n_epochs}"
                  + (" - nothing left to do" if start_epoch >= args.n_epochs else ""))
    if dataloader is None:
        from . import synth
        pool = synth.VideoPool(synth.list_videos(args.trainvideos), dev)
        mask = synth.load_mask(args.trainmask, args.patch_size, args.patch_size, args.frames)
        dataloader = synth.SynthTrainLoader(pool, mask, args.batch_size, args.patches_per_epoch, args.patch_size, args.patch_size, args.frames,
                                            seed=0 if args.seed is None else args.seed, start_epoch=start_epoch, noise=noise_from_arguments(args, args.seed),
                                            augment=synth.parse_augment(args.augment))
        print(f"training from {len(pool)} videos ({pool.nbytes / 1e6:.1f} MB on {dev}): {len(dataloader)} batches of {args.batch_size} patches "
              f"{args.patch_size}x{args.patch_size}x{args.frames} per epoch")
        if dataloader.noise is not None:
            print(f"sensor noise on the training measurements: {dataloader.noise.describe(args.frames)}")
    opts = {}
    if args.conv64 != 'auto':
        opts["conv64"] = args.conv64
    if args.anderson_arith != 'reference':
        opts["anderson_arith"] = args.anderson_arith
    deq.engine_options = opts
    cfg = training.configure_training(deq, args.train_backend)
    print(f"train backend {cfg.backend}: implicit_backward={cfg.implicit_backward} parameter_backward={cfg.parameter_backward} "
          f"engine_options={cfg.engine_options}" + "".join(f"\n  {k} stays on autograd: {v}" for k, v in cfg.reasons.items()))
    save_model_path = args.savepath + 'model/'
    for path in (save_model_path, args.savepath + 'img/train/', args.savepath + 'img/test/'):
        os.makedirs(path, exist_ok=True)
    return training.train_solver_sci(
        single_iterate_solver=solver, train_dataloader=dataloader, optimizer=optimizer, save_model_path=save_model_path,
        loss_function="device" if device else torch.nn.MSELoss(reduction='mean'), n_epochs=args.n_epochs, deep_eq_module=deq,
        use_dataparallel=False, scheduler=scheduler, print_every_n_steps=args.print_every_n_steps,
        save_every_n_steps=args.save_every_n_steps, start_epoch=start_epoch, test_dataloader=test_dataset,
        train_img_path=args.savepath + 'img/train/', test_img_path=args.savepath + 'img/test/', best_img_path=args.savepath + 'img/best/',
        tflog_path=args.savepath, max_steps=args.max_steps, clip_grad_norm=args.clip_grad_norm)


def run(args):
    """One rank (or the only process): build, evaluate every clip, rank 0 reports."""
    rank, world, _, dev = distributed.init_from_env("nccl")
    deq = None
    if args.baseline is None:
        loadpath = default_loadpath(args.denoiser, args.loadpath)
        _, deq = build_pipeline(args.denoiser, loadpath, args.and_maxiters, args.and_m, args.and_beta, device=dev, solver_name=args.solver,
                                broyden_threshold=args.broyden_threshold, broyden_eps=args.broyden_eps, eps2_tol=args.eps2_tol, eps2_lam=args.eps2_lam)
        opts = {}
        if args.conv64 != 'auto':
            opts["conv64"] = args.conv64
        if args.anderson_arith != 'reference':
            opts["anderson_arith"] = args.anderson_arith
        if opts:
            deq.engine_options = opts
    if args.baseline is not None and (args.snapshots is not None or args.trace):
        sys.exit("--snapshots / --trace are the DEQ iteration's: not available with --baseline")
    jac = None
    if args.jacobian is not None or args.jacobian_json:
        if args.baseline is not None:
            sys.exit("--jacobian is the DEQ map's: not available with --baseline")
        n_it = 30 if args.jacobian is None else args.jacobian
        jac = {"n_iters": n_it, "window": min(10, n_it)}
    if rank == 0:
        if deq is not None:
            print('loaded dict!')
            if args.solver != 'anderson':
                print(solver_line(deq))
        os.makedirs(args.savepath, exist_ok=True)
    noise = noise_from_arguments(args, args.seed)
    if noise is not None and rank == 0:
        print(f"sensor noise on the test measurements: {noise.describe()}")
    images = {}
    ssim = bool(args.ssim or args.ssim_mode)

    def on_clip(r):
        if rank == 0:
            images.update(png_payloads(r, args.savepath))
            print(*clip_line(r, ssim))
    t0 = time.time()
    avg, results = evaluate(deq, SCITestDataset(args.testpath), device=dev, on_clip=on_clip,
                            batch="all" if args.batch_measurements == "all" else bool(args.batch_measurements or world > 1),
                            ssim=ssim, ssim_mode=args.ssim_mode or "same", init=args.init_point,
                            method="deq" if args.baseline is None else args.baseline,
                            **({"snapshots": args.snapshots, "trace": bool(args.trace)} if (args.snapshots is not None or args.trace) else {}),
                            **({} if jac is None else {"jacobian": jac}), **({} if noise is None else {"noise": noise}))
    dt = time.time() - t0
    if rank == 0:
        print('---------------------------------', 'Total Average PSNR: %.2f dB' % avg)
        if ssim:
            print('---------------------------------', 'Total Average SSIM: %.4f' % (sum(r.mean_ssim for r in results) / len(results)))
        if args.snapshots is not None:
            print_horizons(results)
        print_jacobian_totals(results)
        if args.trace:
            write_trace(args.trace, results)
        if args.jacobian_json:
            import json
            with open(args.jacobian_json, "w") as fh:
                json.dump(jacobian_document(results), fh)
                fh.write("\n")
        for path, img in images.items():
            write_png(path, img)
        n = sum(r.frames for r in results)
        print(f"{n} frames in {dt:.2f} s -> {n / dt:.2f} frames/s on {world} GPU(s) (excl. PNG export)")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return avg


def main(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if args.solver in ('broyden', 'epsilon2') and (args.snapshots is not None or args.trace):
        p.error(f"--snapshots / --trace come out of the engine's Anderson / Picard loop: not available with --solver {args.solver}")
    if args.denoiser not in SHIPPED and args.denoiser not in NO_DEFAULT:
        raise NotImplementedError('unknown denoiser!')
    training = str(args.inference).lower() in ('false', '0', '')
    try:
        noisy = noise_from_arguments(args, args.seed) is not None
    except ValueError as e:
        p.error(f"sensor noise: {e}")
    if training and noisy and not args.trainvideos:
        p.error("the sensor-noise flags act on the samples --trainvideos synthesises; a --trainpath directory holds its measurements already: "
                "write a noisy one with python -m deqsci_amd.synth write --meas_noise_sigma ... and train on that")
    if training:
        if args.trainvideos and args.trainpath:
            p.error("--trainvideos and --trainpath exclude one another: one source of training samples")
        if args.trainvideos:
            if not args.trainmask:
                p.error("--trainvideos needs --trainmask FILE (a .mat with key 'mask')")
            from .synth import parse_augment
            try:
                parse_augment(args.augment)
            except ValueError as e:
                p.error(f"--{e}")
            if args.patches_per_epoch < args.batch_size:
                p.error(f"--patches_per_epoch {args.patches_per_epoch} is less than one batch (--batch_size {args.batch_size})")
        elif not args.trainpath:
            sys.exit("--inference False trains: --trainpath DIR/ (with mask.mat, gt/ and measurement/) or --trainvideos DIR with --trainmask FILE is needed")
        ids = [int(v) for v in str(args.gpu_ids).split(',') if v != '']
        if len(ids) > 1:
            sys.exit(f"--gpu_ids {args.gpu_ids}: training is single-device in this build (data-parallel training is out of scope)")
        if args.loadpath and not os.path.exists(args.loadpath):
            sys.exit(f"--loadpath {args.loadpath}: no such file (the reference would silently train from random weights; omit the flag for that)")
        if args.solver != 'anderson' or args.baseline is not None or args.snapshots is not None or args.trace or args.jacobian is not None \
                or args.jacobian_json or args.init_point != 'At':
            sys.exit("--inference False trains the DEQ with Anderson acceleration from At(y, Phi), as the reference: --solver, --baseline, "
                     "--init_point, --snapshots, --trace and --jacobian are inference's")
    if args.baseline is None and not training:                        # (training looks up no shipped default: --loadpath '' starts from random weights, as the reference)
        try:
            default_loadpath(args.denoiser, args.loadpath)
        except ValueError as e:
            p.error(str(e))
    if args.snapshots is not None:
        from .engine import check_snapshots
        try:
            check_snapshots(args.snapshots, args.and_maxiters, "picard" if args.solver == "picard" else "anderson")
        except ValueError as e:
            sys.exit(f"--snapshots: {e}")
    ids = [int(v) for v in str(args.gpu_ids).split(',') if v != '']
    if distributed.relaunch_needed(len(ids)):
        # the launcher parent never calls into HIP (not even to count devices): visibility variables / KFD topology only
        seen = distributed.visible_gpu_count()
        if seen is not None and seen <= max(ids):
            sys.exit(f"--gpu_ids {args.gpu_ids} but only {seen} GPU(s) are visible")
        cmd = [sys.executable, "-m", "deqsci_amd.cli"] + list(sys.argv[1:] if argv is None else argv)
        sys.exit(distributed.launch_ranks(cmd, len(ids), device_ids=ids))
    if not torch.cuda.is_available():
        sys.exit("deqsci_amd needs an MI355X: there is no CPU path")
    if len(ids) == 1 and "LOCAL_RANK" not in os.environ:
        os.environ["LOCAL_RANK"] = str(ids[0])
    return train(args) if training else run(args)


if __name__ == "__main__":
    main()
