"""Float64 numpy restatement of Broyden's method as deqsci_amd.broyden computes it - the yardstick of tests/test_broyden_host.py and
tests/test_broyden_gpu.py - and the seeded toy maps of tests/golden/broyden_toy.npz.  Written from the algorithm, not from any code:

    x viewed as (bsz, N); L = min(threshold, 27) history rows U_j, V_j; gx = g(x), update = gx, objective = |gx| over the whole batch.
    While objective >= eps and nstep < threshold:
      x += update; gx_new = g(x); dx = update; dg = gx_new - gx; nstep += 1; objective = |gx_new|; remember the lowest iterate;
      stop if objective < eps, or (objective < 3 eps, nstep > 30, max / min of the last 30 objectives < 1.3), or objective > 1e6 x the first;
      with the t = min(nstep - 1, L) filled rows: vT = -dx + sum_j <dx, U_j> V_j,  w = dx + dg - sum_j <V_j, dg> U_j,  u = w / <vT, dg>
      (per sample), NaNs of vT and u -> 0 after d and u are formed, both stored in row (nstep - 1) % L;
      update = gx_new - sum_j <V_j, gx_new> U_j over the min(nstep, L) rows now filled.
"""
import numpy as np

MAX_L = 27


def step_f64(U, V, dx, g0, g1, t, slot, dg=None):
    """One update in float64 on copies of the history U, V (bsz, L, N): -> dict with the coefficients a, b, c (bsz, t), gg, d, c_new (bsz,),
    the new rows vT (NaNs zeroed), w, u (NaNs zeroed), update, and the histories U, V after the step.  c_new is formed from vT before its
    NaNs are zeroed, as the kernels form it.  dg: gx_new - gx_old as the caller formed it (the kernels: in fp32) instead of g1 - g0."""
    U, V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
    dx, g1 = np.asarray(dx, dtype=np.float64), np.asarray(g1, dtype=np.float64)
    dg = g1 - np.asarray(g0, dtype=np.float64) if dg is None else np.asarray(dg, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = np.einsum("bn,bjn->bj", dx, U[:, :t])
        b = np.einsum("bjn,bn->bj", V[:, :t], dg)
        c = np.einsum("bjn,bn->bj", V[:, :t], g1)
        gg = np.einsum("bn,bn->b", g1, g1)
        vT = -dx + np.einsum("bj,bjn->bn", a, V[:, :t])
        w = dx - (np.einsum("bj,bjn->bn", b, U[:, :t]) - dg)
        d = np.einsum("bn,bn->b", vT, dg)
        c_new = np.einsum("bn,bn->b", vT, g1)
        u = w / d[:, None]
        vT0, u0 = np.where(np.isnan(vT), 0.0, vT), np.where(np.isnan(u), 0.0, u)
        U[:, slot], V[:, slot] = u0, vT0
        rows = max(t, slot + 1)
        cc = np.zeros((U.shape[0], rows))
        cc[:, :t] = c
        cc[:, slot] = c_new
        update = g1 - np.einsum("bj,bjn->bn", cc, U[:, :rows])
    return {"a": a, "b": b, "c": c, "gg": gg, "d": d, "c_new": c_new, "vT": vT0, "w": w, "u": u0, "update": update, "U": U, "V": V, "cc": cc}


def broyden_f64(g, x0, threshold=9, eps=1e-5):
    """-> (lowest iterate shaped like x0, its objective, info): g maps float64 (bsz, N, 1) arrays to the same shape.  info: nstep, g_calls,
    trace (the objective after every g call), lowest_step."""
    x0 = np.asarray(x0, dtype=np.float64)
    bsz = x0.shape[0]
    x = x0.reshape(bsz, -1).copy()
    N = x.shape[1]
    L = min(threshold, MAX_L)
    calls = [0]

    def call(v):
        calls[0] += 1
        return np.asarray(g(v.reshape(bsz, N, 1)), dtype=np.float64).reshape(bsz, N)

    U, V = np.zeros((bsz, max(L, 1), N)), np.zeros((bsz, max(L, 1), N))
    gx = call(x)
    update = gx.copy()
    objective = init = float(np.linalg.norm(gx))
    trace = [objective]
    lowest, lowest_x, lowest_step, nstep = objective, x.copy(), 0, 0
    while objective >= eps and nstep < threshold:
        x = x + update
        gx_new = call(x)
        nstep += 1
        objective = float(np.linalg.norm(gx_new))
        trace.append(objective)
        if objective < lowest:
            lowest, lowest_x, lowest_step = objective, x.copy(), nstep
        if objective < eps:
            break
        if objective < 3 * eps and nstep > 30 and max(trace[-30:]) / min(trace[-30:]) < 1.3:
            break
        if objective > init * 1e6:
            break
        st = step_f64(U, V, update, gx, gx_new, min(nstep - 1, L), (nstep - 1) % L)
        U, V, update, gx = st["U"], st["V"], st["update"], gx_new
    return lowest_x.reshape(x0.shape), lowest, {"nstep": nstep, "g_calls": calls[0], "trace": trace, "lowest_step": lowest_step}


# ----------------------------------------------------------------------------- the toy maps of tests/golden/broyden_toy.npz
def conv_spectral_norm(w, n=16):
    """Largest singular value of the circular 3x3 convolution with kernel w (cout, cin, 3, 3) on an n x n grid."""
    k = np.zeros((w.shape[0], w.shape[1], n, n))
    k[:, :, :3, :3] = w
    W = np.fft.fft2(k, axes=(2, 3)).transpose(2, 3, 0, 1)
    return float(np.linalg.svd(W, compute_uv=False).max())


def conv_params(seed, B, rho, bias=0.5):
    """Seeded parameters of f(x) = tanh(conv3x3(x) + b) on (bsz,H,W,B): the B -> B kernel scaled to the spectral norm rho."""
    r = np.random.RandomState(seed)
    w = r.randn(B, B, 3, 3)
    w *= rho / conv_spectral_norm(w)
    return w.astype(np.float32), (bias * r.randn(B)).astype(np.float32)


def conv_map(w, b, dtype, device="cpu"):
    """f(x) = tanh(conv3x3(x) + b) for x (bsz,H,W,B) in torch, at the given precision."""
    import torch
    wt = torch.as_tensor(np.asarray(w), dtype=dtype, device=device)
    bt = torch.as_tensor(np.asarray(b), dtype=dtype, device=device)

    def f(x):
        return torch.tanh(torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt, bt, padding=1)).permute(0, 2, 3, 1)
    return f


def as_g(f, shape):
    """g(x) = f(x) - x on the solver's (bsz, N, 1) view, for a torch map f on tensors of `shape`."""
    def g(x):
        z = x.view(shape)
        return (f(z) - z).reshape(shape[0], -1, 1)
    return g


def as_g_numpy(f, shape):
    """The same g for broyden_f64: float64 numpy in and out, f a torch map run in float64 on the host."""
    import torch

    def g(x):
        z = torch.from_numpy(np.ascontiguousarray(x)).view(shape)
        return (f(z) - z).reshape(shape[0], -1, 1).numpy()
    return g


CASES = {      # name: (kind, shape, seed, rho, threshold, eps); d: bias scale 0.2, slow enough to need more than 27 steps (the history wraps)
    "a": ("conv", (2, 16, 16, 8), 1, 0.9, 12, 1e-9),
    "b": ("conv", (2, 16, 16, 8), 2, 0.5, 40, 1e-3),
    "c": ("conv", (1, 12, 20, 5), 3, 0.9, 9, 1e-5),
    "d": ("conv", (1, 12, 12, 4), 4, 1.25, 60, 4e-4),
}


def case_map(golden, name, dtype, device="cpu"):
    """(f, shape, threshold, eps) of a stored case, f at the given precision on the given device."""
    f = conv_map(golden[f"{name}/p0"], golden[f"{name}/p1"], dtype, device)
    return f, tuple(golden[f"{name}/x0"].shape), int(golden[f"{name}/threshold"]), float(golden[f"{name}/eps"])
