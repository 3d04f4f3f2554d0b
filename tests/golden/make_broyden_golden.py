#!/usr/bin/env python3
"""Generate tests/golden/broyden_toy.npz: the REFERENCE's broyden (solvers/broyd_equilibrium_utils.py) on seeded toy maps.

Imports the reference on the CPU with the shims make_golden.py documents (tests/golden/ref_shims.py); stores seeded inputs, the maps'
parameters and the numbers the reference computes from them, none of its text.  Runs only where the reference is mounted.

    python tests/golden/make_broyden_golden.py

Cases (tests/broyden_f64.py: CASES), f(x) = tanh(conv3x3(x) + b) with the B -> B kernel scaled to the spectral norm rho, g = f - id:
  a  (2,16,16,8)  rho 0.9  threshold 12  eps 1e-9   (below the fp32 floor: all 12 steps)
  b  (2,16,16,8)  rho 0.5  threshold 40  eps 1e-3   (stopped by eps)
  c  (1,12,20,5)  rho 0.9  threshold  9  eps 1e-5   (N = 1200)
  d  (1,12,12,4)  rho 1.25 threshold 60  eps 4e-4   (bias scale 0.2; 31 steps to eps, so the history wraps: rows 0, 1, 2 are rewritten and
                  used.  A diagonal linear map with a wide spectrum was tried first: its fp32 runs leave the float64 trajectory - the g-call counts
                  differ before the wrap - so it cannot pin a stop)
Per case c: c/x0, c/p0, c/p1 (the map's parameters), c/threshold, c/eps, c/ref_x, c/ref_res, c/ref_g_calls (the reference, fp32),
c/ref_vs_f64 (the relative L2 distance of ref_x to the float64 restatement tests/broyden_f64.py), c/f64_g_calls, c/f64_res,
c/eps_stop (whether eps ended the float64 run).

Conditions asserted here: the reference and the float64 restatement make the same number of g calls; where eps ended the run, the
float64 objective at the stopping step and at the step before differ from eps by more than 1 % (fp32 noise cannot move the stop); case d
takes more than 28 steps (the wrapped row is written and used).
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

from solvers import broyd_equilibrium_utils as ref  # noqa: E402

import broyden_f64 as bf  # noqa: E402


def parameters(name):
    kind, shape, seed, rho, threshold, eps = bf.CASES[name]
    r = np.random.RandomState(100 + seed)
    p0, p1 = bf.conv_params(seed, shape[-1], rho, bias=0.2 if name == "d" else 0.5)
    return p0, p1, r.randn(*shape).astype(np.float32)


def main():
    out = {}
    for name, (kind, shape, seed, rho, threshold, eps) in bf.CASES.items():
        p0, p1, x0 = parameters(name)
        out.update({f"{name}/p0": p0, f"{name}/p1": p1, f"{name}/x0": x0, f"{name}/threshold": np.int64(threshold), f"{name}/eps": np.float64(eps)})
        f32, _, _, _ = bf.case_map(out, name, torch.float32)
        f64, _, _, _ = bf.case_map(out, name, torch.float64)
        calls = [0]
        g32 = bf.as_g(f32, shape)

        def counted(x):
            calls[0] += 1
            return g32(x)
        with torch.no_grad():
            ref_x, ref_res = ref.broyden(counted, torch.from_numpy(x0), threshold=threshold, eps=eps)
        x64, res64, info = bf.broyden_f64(bf.as_g_numpy(f64, shape), x0, threshold, eps)
        dist = float(np.linalg.norm(ref_x.numpy().astype(np.float64) - x64) / np.linalg.norm(x64))
        tr = info["trace"]
        eps_stop = tr[-1] < eps
        print(f"{name}: g calls ref {calls[0]} f64 {info['g_calls']}  res ref {ref_res:.6e} f64 {res64:.6e}  ref_vs_f64 {dist:.3e}  "
              f"eps_stop {eps_stop}  last objectives {tr[-2]:.4e} {tr[-1]:.4e}")
        assert calls[0] == info["g_calls"], name
        if eps_stop:
            assert abs(tr[-1] - eps) > 0.01 * eps and abs(tr[-2] - eps) > 0.01 * eps, name
        if name == "d":
            assert eps_stop and info["nstep"] > bf.MAX_L + 1, (name, info["nstep"])
        out.update({f"{name}/ref_x": ref_x.numpy(), f"{name}/ref_res": np.float64(ref_res), f"{name}/ref_g_calls": np.int64(calls[0]),
                    f"{name}/ref_vs_f64": np.float64(dist), f"{name}/f64_g_calls": np.int64(info["g_calls"]), f"{name}/f64_res": np.float64(res64),
                    f"{name}/eps_stop": np.bool_(eps_stop)})
    fn = os.path.join(HERE, "broyden_toy.npz")
    np.savez_compressed(fn, **out)
    print("->", fn, os.path.getsize(fn), "bytes")
    assert os.path.getsize(fn) <= 1_000_000


if __name__ == "__main__":
    main()
