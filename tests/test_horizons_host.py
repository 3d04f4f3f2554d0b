"""CPU: the host side of snapshots= / trace= (several iteration horizons and a quality trace from one DEQ run): the C ABI of
csrc/trace.hip, request validation before any device use, CLI parsing, the trace file's schema, ClipResult defaults, and the
kernel's register budget."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_header_library_and_binding_agree_on_the_sqerr_exports():
    from deqsci_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deqsci_hip.h")).read(), flags=re.S)
    protos = {}
    for name in ("deqsci_sqerr_workspace_bytes", "deqsci_sqerr_rows_f32"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, f"{name} is not declared in include/deqsci_hip.h"
        protos[name] = [a for a in m.group(1).split(",") if a.strip()]
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "deqsci_sqerr_workspace_bytes") and hasattr(lib, "deqsci_sqerr_rows_f32")
    assert len(_hip.SIGNATURES["deqsci_sqerr_rows_f32"]) == len(protos["deqsci_sqerr_rows_f32"]) == 9
    assert "deqsci_sqerr_workspace_bytes" in _hip.OTHER_EXPORTS and len(protos["deqsci_sqerr_workspace_bytes"]) == 2
    lib = _hip.load()
    assert len(lib.deqsci_sqerr_workspace_bytes.argtypes) == 2


def test_sqerr_argument_validation_needs_no_gpu():
    from deqsci_amd import _hip
    lib = _hip.load()
    # one float64 partial per (sample, chunk of 4096 elements)
    assert lib.deqsci_sqerr_workspace_bytes(8, 256 * 256 * 8) == 8 * 128 * 8
    assert lib.deqsci_sqerr_workspace_bytes(3, 5) == 3 * 8 and lib.deqsci_sqerr_workspace_bytes(1, 4097) == 16
    assert lib.deqsci_sqerr_workspace_bytes(0, 100) == 0 and lib.deqsci_sqerr_workspace_bytes(4, 0) == 0
    assert lib.deqsci_sqerr_workspace_bytes(-1, 8) == 0
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.deqsci_sqerr_rows_f32(None, None, None, 1, 8, 8, 1, None, None) == -1
    assert lib.deqsci_sqerr_rows_f32(p, p, p, -1, 8, 8, 1, p, None) == -2
    assert lib.deqsci_sqerr_rows_f32(p, p, p, 2, 8, 4, 1, p, None) == -2          # rows of x closer than N
    assert lib.deqsci_sqerr_rows_f32(p + 2, p, p, 1, 8, 8, 1, p, None) == -3
    assert lib.deqsci_sqerr_rows_f32(p, p, p + 4, 1, 8, 8, 1, p, None) == -3
    # nothing to do: nothing is launched, whatever the pointers
    assert lib.deqsci_sqerr_rows_f32(None, None, None, 0, 8, 8, 1, None, None) == 0
    assert lib.deqsci_sqerr_rows_f32(None, None, None, 4, 0, 0, 1, None, None) == 0


BAD = [("anderson", 40, (3.0, 10)), ("anderson", 40, ("10",)), ("anderson", 40, "10,20"), ("anderson", 40, 10), ("anderson", 40, (True, 10)),
       ("anderson", 40, (10, 10)), ("anderson", 40, (30, 10)), ("anderson", 40, (10, 40)), ("anderson", 40, (10, 41)),
       ("anderson", 40, (2, 10)), ("anderson", 40, (0,)), ("anderson", 40, (-3,)), ("picard", 40, (0, 5)), ("picard", 40, (5, 40)),
       ("picard", 40, (5, 5)), ("picard", 40, (1.5,))]


@pytest.mark.parametrize("iterator,max_iter,snaps", BAD)
def test_invalid_snapshot_requests_raise_before_any_device_use(iterator, max_iter, snaps):
    from deqsci_amd.engine import DEQSCIEngine, check_snapshots
    with pytest.raises(ValueError):
        check_snapshots(snaps, max_iter, iterator)
    net = torch.nn.Conv2d(1, 1, 3, padding=1, bias=False)
    net.tag = "conv2d"
    eng = DEQSCIEngine(net, iterator=iterator, max_iter=max_iter)
    y, Phi = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 4)                     # CPU tensors: a valid request would be refused for THAT
    with pytest.raises(ValueError):
        eng.reconstruct(y, Phi, snapshots=snaps)
    assert eng.last_info is None


def test_valid_requests_and_gt_rules():
    from deqsci_amd import _hip
    from deqsci_amd.engine import DEQSCIEngine, check_snapshots
    assert check_snapshots(None, 40) is None and check_snapshots((), 40) is None
    assert check_snapshots([3, 10, 39], 40) == (3, 10, 39) and check_snapshots((np.int64(5),), 40) == (5,)
    assert check_snapshots((1, 2), 40, "picard") == (1, 2)
    net = torch.nn.Conv2d(1, 1, 3, padding=1, bias=False)
    net.tag = "conv2d"
    eng = DEQSCIEngine(net, max_iter=40)
    y, Phi = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, 4)
    with pytest.raises(ValueError):
        eng.reconstruct(y, Phi, gt=torch.zeros(1, 8, 8, 4))                    # gt without trace
    with pytest.raises(ValueError):
        eng.reconstruct(y, Phi, trace=True, gt=torch.zeros(1, 8, 8, 5))        # wrong shape
    with pytest.raises(_hip.DeqsciHipError):
        eng.reconstruct(y, Phi, snapshots=(3, 10), trace=True)                 # valid request: refused for the CPU tensors, not the options


def test_deqfixedpoint_refuses_the_options_off_the_engine_path():
    import deqsci_amd
    from deqsci_amd.solvers import DEQFixedPoint, andersonexp
    deq = DEQFixedPoint(torch.nn.Identity(), andersonexp, max_iter=10)
    assert deq.snapshots is None and deq.trace is False and deq.trace_gt is None
    assert deq.last_snapshots is None and deq.last_trace is None
    deq.snapshots = (3,)
    with pytest.raises(NotImplementedError, match="engine"):
        deq.forward(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 2), torch.ones(1, 4, 4), train_flag=False)
    assert deqsci_amd.__version__


def test_cli_parses_snapshots_and_trace():
    from deqsci_amd import cli
    a = cli.parser().parse_args([])
    assert a.snapshots is None and a.trace is None
    a = cli.parser().parse_args(["--snapshots", "10,30,100", "--trace", "out.json", "--and_maxiters", "180"])
    assert a.snapshots == (10, 30, 100) and a.trace == "out.json"
    assert cli.parser().parse_args(["--snapshots", "10"]).snapshots == (10,)
    for bad in ("ten", "10,,x", ""):
        with pytest.raises(SystemExit):
            cli.parser().parse_args(["--snapshots", bad])
    with pytest.raises(SystemExit, match="snapshots"):
        cli.main(["--snapshots", "10,200", "--and_maxiters", "180", "--denoiser", "SimpleCNN"])      # before any device use


def test_clipresult_defaults_and_trace_schema(tmp_path):
    from deqsci_amd import cli, harness
    r = harness.ClipResult(name="a.mat", rec=torch.zeros(2, 4, 4, 8), psnr=[20.0, 22.0], res=[0.1, 0.2])
    assert r.snapshots is None and r.trace is None
    assert harness.horizon_means([r]) == {} and harness.trace_document([r]) == {}
    r.info = {"measurements": [0, 3]}
    r.trace = {"psnr": np.array([[10.0, 11.0, 12.0], [13.0, 14.0, 15.0]]), "res": np.array([[0.5, 0.4, 0.3], [0.6, 0.5, 0.4]])}
    r.snapshots = {10: {"psnr": [19.0, 21.0], "res": [0.3, 0.4], "ssim": None}}
    path = tmp_path / "t.json"
    cli.write_trace(str(path), [r])
    doc = json.loads(path.read_text())
    assert list(doc) == ["a.mat"] and list(doc["a.mat"]) == ["0", "3"]
    assert doc["a.mat"]["3"] == {"psnr": [13.0, 14.0, 15.0], "res": [0.6, 0.5, 0.4]}
    assert harness.horizon_means([r]) == {10: (20.0, None)}


def test_harness_refuses_the_options_where_they_cannot_apply():
    from deqsci_amd import harness
    with pytest.raises(ValueError):
        harness._Horizons(None, (10,), False, "gaptv")
    with pytest.raises(NotImplementedError):
        harness._Horizons(torch.nn.Identity(), (10,), False, "deq")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc on this machine")
def test_trace_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "deqsci_amd", "csrc"), "--save-temps", "-c", os.path.join(ROOT, "deqsci_amd", "csrc", "trace.hip"),
           "-o", "trace.o"]
    subprocess.run(cmd, check=True, cwd=tmp_path, capture_output=True)
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert len(asm) == 1
    text = open(os.path.join(tmp_path, asm[0])).read()
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    assert len(scratch) == 2 and scratch == [0, 0]
    assert [int(v) for v in re.findall(r"\.sgpr_spill_count:\s*(\d+)", text)] == [0, 0]
    assert [int(v) for v in re.findall(r"\.vgpr_spill_count:\s*(\d+)", text)] == [0, 0]
    assert "buffer_atomic" not in text and "global_atomic" not in text and "flat_atomic" not in text
