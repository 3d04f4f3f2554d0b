#!/usr/bin/env python3
"""Deliberately wrong builds of csrc/sci_ops.hip, to show that tests/test_sci_ops_gpu.py bites (profiles/sci_ops_tests.md has the table).

    python tools/sci_ops_mutants.py build            # build/mutants/<name>/libdeqsci_hip.so, one per mutant (nothing under build/ is committed)
    python tools/sci_ops_mutants.py run              # on the GPU: the new tests and the two older operator tests against every mutant

Every mutation changes ARITHMETIC only - a flag, the order or fusion of floating-point operations, which value goes to a slot - never an
address, a bound, a clamp or a barrier, so no mutant can fault.  Only sci_ops.hip (with its private copy of common.hpp) is recompiled; the
other sources are compiled once with the shipped flags and linked into every mutant.  The package loads a mutant through DEQSCI_HIP_LIB."""
import argparse
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "mutants")
CSRC = os.path.join(ROOT, "deqsci_amd", "csrc")

FMA4 = "make_float4(fmaf(r.x, pv[b].x, zv[b].x), fmaf(r.y, pv[b].y, zv[b].y), fmaf(r.z, pv[b].z, zv[b].z), fmaf(r.w, pv[b].w, zv[b].w))"
# name -> (file, old text, new text) or, "no_fp_contract_off", a flag change
MUTANTS = {
    "no_fp_contract_off": None,
    "dot4_fma": ("common.hpp", "{ return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }",
                 "{ return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, 0.0f)))); }"),
    "butterfly8_last_step": ("common.hpp", "    if (LP >= 8) v += __shfl_xor(v, 4, WAVE);\n", ""),
    "planar_forward_from_b2": ("sci_ops.hip", "for (int b = 1; b < B; ++b) acc = acc + ldp<POL>(xs + b * P) * ldp<POL>(ps + b * P);",
                               "for (int b = 2; b < B; ++b) acc = acc + ldp<POL>(xs + b * P) * ldp<POL>(ps + b * P);"),
    "phisum_bhw_keeps_zero": ("sci_ops.hip", "    acc.x = acc.x == 0.0f ? 1.0f : acc.x; acc.y = acc.y == 0.0f ? 1.0f : acc.y;\n"
                                             "    acc.z = acc.z == 0.0f ? 1.0f : acc.z; acc.w = acc.w == 0.0f ? 1.0f : acc.w;\n", ""),
    "hwb2bhw_rows_swapped": ("sci_ops.hip", "t[0] = o.x; t[TS] = o.y;", "t[0] = o.y; t[TS] = o.x;"),
    "gap_bhw_fused_update": ("sci_ops.hip", "stp<POL>(os + b * P, zv[b] + r * pv[b]);", f"stp<POL>(os + b * P, {FMA4});"),
}
NEW_TESTS = "tests/test_sci_ops_gpu.py"
OLD_TESTS = ["tests/test_gpu_parity.py::test_ops_vs_oracle_all_layouts", "tests/test_gpu_parity.py::test_ops_reference_golden"]


def makefile_var(name):
    with open(os.path.join(ROOT, "Makefile")) as f:
        m = re.search(rf"^{name}\s*:=\s*(.*)$", f.read(), re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def run(cmd):
    subprocess.run(cmd, check=True, cwd=ROOT)


def build(jobs):
    flags, srcs = makefile_var("HIPFLAGS"), makefile_var("SRCS")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(OUT, "obj")
    os.makedirs(objdir, exist_ok=True)
    others = [s for s in srcs if not s.endswith("sci_ops.hip")]
    objs = [os.path.join(objdir, os.path.basename(s) + ".o") for s in others]
    with ThreadPoolExecutor(jobs) as ex:
        list(ex.map(lambda pair: run([hipcc, *flags, "-c", pair[0], "-o", pair[1]]), zip(others, objs)))      # (always: an object from older sources or flags must not be linked)
    for name, mut in MUTANTS.items():
        d = os.path.join(OUT, name)
        os.makedirs(d, exist_ok=True)
        for f in ("sci_ops.hip", "common.hpp", "rows.hpp"):                # (a quoted #include looks beside the including file first)
            shutil.copy(os.path.join(CSRC, f), d)
        fl = list(flags)
        if mut is None:
            fl.remove("-ffp-contract=off")
        else:
            path = os.path.join(d, mut[0])
            text = open(path).read()
            assert text.count(mut[1]) == 1, (name, "the text to replace must occur exactly once")
            open(path, "w").write(text.replace(mut[1], mut[2]))
        run([hipcc, *fl, "-c", os.path.join(d, "sci_ops.hip"), "-o", os.path.join(d, "sci_ops.hip.o")])
        run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", os.path.join(d, "libdeqsci_hip.so"), os.path.join(d, "sci_ops.hip.o"), *objs])
        print("built", os.path.join(d, "libdeqsci_hip.so"))


def run_tests(select, log_dir):
    """One pytest process per mutant, one at a time, each under its own time limit; anything but 'tests failed' or 'all passed' stops the run."""
    os.makedirs(log_dir, exist_ok=True)
    print("| mutant | caught by the two older tests | caught by tests/test_sci_ops_gpu.py | by which tests |\n|---|---|---|---|")
    for name in MUTANTS:
        lib = os.path.join(OUT, name, "libdeqsci_hip.so")
        env = dict(os.environ, DEQSCI_HIP_LIB=lib)
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-rf", "-p", "no:cacheprovider", NEW_TESTS, *OLD_TESTS] + (["-k", select] if select else [])
        p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        open(os.path.join(log_dir, name + ".log"), "w").write(p.stdout)
        if p.returncode not in (0, 1):
            sys.exit(f"{name}: pytest ended with status {p.returncode}: stopping here (see {log_dir}/{name}.log)")
        failed = re.findall(r"^FAILED (\S+?)::(\w+)", p.stdout, re.M)
        old = sorted({t for f, t in failed if f.endswith("test_gpu_parity.py")})
        new = sorted({t for f, t in failed if f.endswith("test_sci_ops_gpu.py")})
        n_new = sum(1 for f, _ in failed if f.endswith("test_sci_ops_gpu.py"))
        print(f"| `{name}` | {', '.join(old) if old else 'no'} | {'yes, ' + str(n_new) + ' cases' if new else 'NO'} | {', '.join(new)} |", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["build", "run"])
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("-k", default="", help="pytest -k selection for `run`")
    ap.add_argument("--logs", default=os.path.join(OUT, "logs"))
    a = ap.parse_args()
    build(a.j) if a.what == "build" else run_tests(a.k, a.logs)
