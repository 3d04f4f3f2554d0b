"""Float64 numpy restatement of the vector epsilon-algorithm as deqsci_amd.epsilon2 computes it - the yardstick of
tests/test_epsilon2_host.py and tests/test_epsilon2_gpu.py - on the seeded toy maps of tests/broyden_f64.py.  Written from the algorithm,
not from any code:

    x of shape (bsz, ...).  For k < max_iter:  f_x = f(x), f_fx = f(f_x);  dx = f_x - x, df = f_fx - f_x, d2 = df - dx;
      per sample a = sum dx^2, b = sum df^2, c = sum d2^2 + lam;   x_new = f_x + (df a - dx b) / c;
      residual = |x_new - x| / |x_new| over the whole batch;  x = x_new;  stop if residual < tol.
"""
import numpy as np

from broyden_f64 import CASES as MAPS, conv_map, conv_params  # noqa: F401  (the maps: kind, shape, seed, rho of each case)

CASES = {      # name: (max_iter, tol, lam) on the map of the same name in tests/broyden_f64.py: CASES
    "a": (12, 1e-9, 1e-4),       # below the fp32 floor: all 12 iterations
    "b": (40, 1e-4, 1e-4),       # stopped by tol
    "c": (50, 1e-2, 1e-4),       # the defaults; N = 1200
    "d": (40, 1e-4, 1e-4),       # rho 1.25: plain iteration does not contract
}


def sums_f64(x, f_x, f_fx):
    """Per sample (sum dx^2, sum df^2, sum d2^2) in float64 for rows (bsz, N) of any float type, and the differences."""
    x, f_x, f_fx = (np.asarray(v, dtype=np.float64) for v in (x, f_x, f_fx))
    dx, df = f_x - x, f_fx - f_x
    d2 = df - dx
    return (dx * dx).sum(1), (df * df).sum(1), (d2 * d2).sum(1), dx, df


def step_f64(x, f_x, f_fx, lam):
    """One extrapolation in float64 on rows (bsz, N) -> (x_new, residual over the whole batch)."""
    a, b, c, dx, df = sums_f64(x, f_x, f_fx)
    with np.errstate(all="ignore"):
        x_new = np.asarray(f_x, dtype=np.float64) + (df * a[:, None] - dx * b[:, None]) / (c + lam)[:, None]
    return x_new, float(np.linalg.norm(x_new - np.asarray(x, dtype=np.float64))) / float(np.linalg.norm(x_new))


def epsilon2_f64(f, x0, max_iter=50, tol=1e-2, lam=1e-4):
    """-> (x shaped like x0, the last residual, info): f maps float64 arrays shaped like x0 to the same shape.  info: iterations, f_calls,
    trace (the residual of every iteration)."""
    x0 = np.asarray(x0, dtype=np.float64)
    bsz = x0.shape[0]
    x = x0.reshape(bsz, -1)
    calls, trace = [0], []

    def call(v):
        calls[0] += 1
        return np.asarray(f(v.reshape(x0.shape)), dtype=np.float64).reshape(bsz, -1)

    for _ in range(max_iter):
        f_x = call(x)
        f_fx = call(f_x)
        x, residual = step_f64(x, f_x, f_fx, lam)
        trace.append(residual)
        if residual < tol:
            break
    return x.reshape(x0.shape), trace[-1], {"iterations": len(trace), "f_calls": calls[0], "trace": trace}


def as_numpy_map(f):
    """A torch map run in float64 on the host, as a numpy float64 -> numpy float64 map for epsilon2_f64."""
    import torch

    def g(x):
        with torch.no_grad():
            return f(torch.from_numpy(np.ascontiguousarray(x))).numpy()
    return g


def case_map(golden, name, dtype, device="cpu"):
    """(f, shape, max_iter, tol, lam) of a stored case, f at the given precision on the given device."""
    f = conv_map(golden[f"{name}/p0"], golden[f"{name}/p1"], dtype, device)
    return f, tuple(golden[f"{name}/x0"].shape), int(golden[f"{name}/max_iter"]), float(golden[f"{name}/tol"]), float(golden[f"{name}/lam"])
