"""DnCNN-17 (the reference's --denoiser DnCNN: networks/provable/model/models.py, 17 layers with BatchNorm) without a GPU: the weights
archive, the module's state-dict names, the folded layer list, one forward against the reference's own (tests/golden/dncnn17.npz,
make_dncnn_golden.py) and the command line's handling of a denoiser without shipped weights."""
import os

import numpy as np
import pytest
import torch

from deqsci_amd import checkpoint, cli, vjp
from deqsci_amd.layers import conv_stack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHTS = os.path.join(GOLDEN, "dncnn_noise15.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "dncnn17.npz"))


@pytest.fixture(scope="module")
def solver():
    return cli.build_pipeline("DnCNN", WEIGHTS, and_maxiters=10, device="cpu")[0]


def test_weights_archive_loads():
    """The three parts (each below the size limit of a committed file) read as ONE state dict: 92 entries, 557 967 values, 'module.' stripped."""
    sd, epoch = checkpoint.read_state_dict(WEIGHTS)
    assert epoch is None and len(sd) == 92 and sum(v.numel() for v in sd.values()) == 557967
    assert all(k.startswith("dncnn.") for k in sd)
    assert tuple(sd["dncnn.0.weight"].shape) == (64, 1, 3, 3) and tuple(sd["dncnn.47.weight"].shape) == (1, 64, 3, 3)
    for name in os.listdir(GOLDEN):
        if name.startswith("dncnn"):
            assert os.path.getsize(os.path.join(GOLDEN, name)) <= 1 << 20, name


def test_state_dict_keys_are_the_references(gold):
    net = cli.build_denoiser("DnCNN")
    assert net.tag == "denoiser"
    assert list(net.state_dict().keys()) == [str(k) for k in gold["keys"]]
    assert list(checkpoint.read_state_dict(WEIGHTS)[0].keys()) == [str(k) for k in gold["keys"]]


def test_conv_stack_folds_fifteen_batchnorms(solver):
    layers = conv_stack(solver.nonlinear_op.eval().dncnn)[0]
    assert len(layers) == 17
    assert sum(b is not None for _, b, _ in layers) == 15 and layers[0][1] is None and layers[-1][1] is None
    assert [relu for _, _, relu in layers] == [True] * 16 + [False]
    assert [tuple(w.shape) for w, _, _ in layers] == [(64, 1, 3, 3)] + [(64, 64, 3, 3)] * 15 + [(1, 64, 3, 3)]
    plan = vjp.host_plan(solver.nonlinear_op)                 # (the implicit backward and the Jacobian diagnostics walk the same list)
    assert len(plan[0]) == 17


def test_cpu_forward_equals_the_references(gold, solver):
    """(a) of the golden: the reference's DnCNN on the GAP output of traffic measurement 0's crop.  The module itself, and the folded
    layers the engine runs, both to 1e-6."""
    x, want = torch.from_numpy(gold["a_x"]), gold["a_out"].astype(np.float64)
    net = solver.nonlinear_op.eval()
    with torch.no_grad():
        got = net(x).double().numpy()
        h = x
        for w, b, relu in conv_stack(net.dncnn)[0]:
            h = torch.nn.functional.conv2d(h, w, b, padding=1)
            h = torch.relu(h) if relu else h
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    err_folded = np.linalg.norm(h.double().numpy() - want) / np.linalg.norm(want)
    print(f"module {err:.3e}  folded layers {err_folded:.3e}")
    assert err <= 1e-6 and err_folded <= 1e-6


def test_bare_pth_loads_through_load_solver_and_partial_loads_are_errors(tmp_path, solver):
    """A bare DataParallel state dict of the reference's shape ('module.dncnn.N.*' in a .pth) loads; one with a key missing or a key too
    many raises instead of loading what fits."""
    sd = {"module." + k: v.clone() for k, v in solver.nonlinear_op.state_dict().items()}
    torch.save(sd, tmp_path / "DnCNN_noise15.pth")
    fresh = cli.build_pipeline("DnCNN", str(tmp_path / "DnCNN_noise15.pth"), device="cpu")[0]
    for (k, a), (_, b) in zip(fresh.nonlinear_op.state_dict().items(), solver.nonlinear_op.state_dict().items()):
        assert torch.equal(a, b), k
    short = dict(sd)
    del short["module.dncnn.24.running_var"]
    torch.save(short, tmp_path / "short.pth")
    with pytest.raises(RuntimeError, match="Missing key"):
        cli.build_pipeline("DnCNN", str(tmp_path / "short.pth"), device="cpu")
    long = dict(sd)
    long["module.dncnn.48.weight"] = torch.zeros(1)
    torch.save(long, tmp_path / "long.pth")
    with pytest.raises(RuntimeError, match="Unexpected key"):
        cli.build_pipeline("DnCNN", str(tmp_path / "long.pth"), device="cpu")
    with pytest.raises(RuntimeError):                          # another denoiser's archive
        cli.build_pipeline("DnCNN", checkpoint.shipped("cnn"), device="cpu")


def test_a_missing_part_of_a_split_archive_is_an_error(tmp_path):
    import shutil
    shutil.copy(WEIGHTS, tmp_path / "dncnn_noise15.npz")
    with pytest.raises(FileNotFoundError, match="part"):
        checkpoint.read_state_dict(str(tmp_path / "dncnn_noise15.npz"))


def test_cli_accepts_the_name_and_wants_a_loadpath(capsys):
    args = cli.parser().parse_args(["--denoiser", "DnCNN", "--loadpath", WEIGHTS])
    assert args.denoiser == "DnCNN" and cli.default_loadpath(args.denoiser, args.loadpath) == WEIGHTS
    assert sorted(cli.SHIPPED) == ["RealSN_SimpleCNN", "SimpleCNN", "ffdnet"] and "DnCNN" in cli.NO_DEFAULT
    with pytest.raises(ValueError, match="--loadpath"):
        cli.default_loadpath("DnCNN", "")
    with pytest.raises(SystemExit):                            # refused by the parser, before any device is looked for
        cli.main(["--denoiser", "DnCNN"])
    assert "--loadpath" in capsys.readouterr().err
    with pytest.raises(NotImplementedError, match="unknown denoiser"):
        cli.main(["--denoiser", "dncnn_norm"])
    for name, path in cli.SHIPPED.items():                     # (the shipped defaults are what they were)
        assert cli.default_loadpath(name) == checkpoint.shipped(path)
