#!/usr/bin/env python3
"""Generate tests/golden/epsilon2_toy.npz: the REFERENCE's epsilon2 (solvers/new_equilibrium_utils_yaping.py) on seeded toy maps.

Imports the reference on the CPU with the shims make_golden.py documents (tests/golden/ref_shims.py); stores seeded inputs, the maps'
parameters and the numbers the reference computes from them, none of its text.  Runs only where the reference is mounted.

    python tests/golden/make_epsilon2_golden.py

Cases (tests/epsilon2_f64.py: CASES, on the maps of tests/broyden_f64.py: CASES - the parameters and starting points of
tests/golden/broyden_toy.npz), f(x) = tanh(conv3x3(x) + b) with the B -> B kernel scaled to the spectral norm rho, lam 1e-4:
  a  (2,16,16,8)  rho 0.9   max_iter 12  tol 1e-9   (below the fp32 floor: all 12 iterations, 24 f-calls)
  b  (2,16,16,8)  rho 0.5   max_iter 40  tol 1e-4   (stopped by tol)
  c  (1,12,20,5)  rho 0.9   the defaults: max_iter 50, tol 1e-2   (N = 1200)
  d  (1,12,12,4)  rho 1.25  max_iter 40  tol 1e-4   (bias scale 0.2; stopped by tol)
Per case c: c/x0, c/p0, c/p1 (the map's parameters), c/max_iter, c/tol, c/lam, c/ref_x, c/ref_res, c/ref_f_calls (the reference, fp32),
c/ref_vs_f64 (the relative L2 distance of ref_x to the float64 restatement tests/epsilon2_f64.py), c/f64_f_calls, c/f64_res,
c/f64_res_before (the residual of the iteration before the last; NaN when there is none), c/tol_stop (whether tol ended the float64
run).

Conditions asserted here: the reference and the float64 restatement make the same number of f-calls; where tol ended the run, the
float64 residual at the stopping iteration and at the one before differ from tol by more than 1 % (fp32 noise cannot move the stop).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shims  # noqa: E402

ref_shims.install()

from solvers import new_equilibrium_utils_yaping as ref  # noqa: E402

import epsilon2_f64 as ef  # noqa: E402


def parameters(name):
    kind, shape, seed, rho, _, _ = ef.MAPS[name]
    r = np.random.RandomState(100 + seed)
    p0, p1 = ef.conv_params(seed, shape[-1], rho, bias=0.2 if name == "d" else 0.5)
    return p0, p1, r.randn(*shape).astype(np.float32)


def main():
    out = {}
    for name, (max_iter, tol, lam) in ef.CASES.items():
        p0, p1, x0 = parameters(name)
        out.update({f"{name}/p0": p0, f"{name}/p1": p1, f"{name}/x0": x0, f"{name}/max_iter": np.int64(max_iter), f"{name}/tol": np.float64(tol),
                    f"{name}/lam": np.float64(lam)})
        f32 = ef.case_map(out, name, torch.float32)[0]
        f64 = ef.case_map(out, name, torch.float64)[0]
        calls = [0]

        def counted(x):
            calls[0] += 1
            return f32(x)
        with torch.no_grad():
            ref_x, ref_res = ref.epsilon2(counted, torch.from_numpy(x0), max_iter=max_iter, tol=tol, lam=lam)
        x64, res64, info = ef.epsilon2_f64(ef.as_numpy_map(f64), x0, max_iter, tol, lam)
        dist = float(np.linalg.norm(ref_x.numpy().astype(np.float64) - x64) / np.linalg.norm(x64))
        tr = info["trace"]
        tol_stop = tr[-1] < tol
        before = tr[-2] if len(tr) > 1 else float("nan")
        print(f"{name}: f calls ref {calls[0]} f64 {info['f_calls']}  res ref {ref_res:.6e} f64 {res64:.6e}  ref_vs_f64 {dist:.3e}  "
              f"tol_stop {tol_stop}  last residuals {before:.4e} {tr[-1]:.4e}")
        assert calls[0] == info["f_calls"], name
        if tol_stop:
            assert abs(tr[-1] - tol) > 0.01 * tol and not abs(before - tol) <= 0.01 * tol, name
        out.update({f"{name}/ref_x": ref_x.numpy(), f"{name}/ref_res": np.float64(ref_res), f"{name}/ref_f_calls": np.int64(calls[0]),
                    f"{name}/ref_vs_f64": np.float64(dist), f"{name}/f64_f_calls": np.int64(info["f_calls"]), f"{name}/f64_res": np.float64(res64),
                    f"{name}/f64_res_before": np.float64(before), f"{name}/tol_stop": np.bool_(tol_stop)})
    fn = os.path.join(HERE, "epsilon2_toy.npz")
    np.savez_compressed(fn, **out)
    print("->", fn, os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) <= 1_000_000


if __name__ == "__main__":
    main()
