#!/usr/bin/env python3
"""The Jacobian diagnostics on the device: what they cost, and what they say about the shipped denoisers on the shipped clips.

    python tools/jacobian_bench.py [--table] [--iters 180 [30 ...]] [--n_iters 100] [--window 20] [--reps 10] [--out profiles/r08_jacobian.json]

cost   for SimpleCNN and FFDNet, at 1 and 8 measurements of 256 x 256 x 8 (traffic measurement 0; the eight scored measurements of the
       three shipped clips), at the reconstruction of a 30-iteration run, with HIP events after warm-up (ms, median):
           setup   EquilibriumProxGradSCI.device_jacobian: z1, the mask-building forward, the weight packs
           jv      one product J_f v            jtv   one product J_f^T v
           step    one power step (csrc/jacobian.hip, J2) with w and v_prev the SAME buffer (valid; the launch then reads one array
                   where the loop reads two, so this is a lower bound of the loop's step, not its 16 B/element traffic)
           report  one whole power_report, all three quantities, n_iters = 30 (150 products, 240 power steps, the copy of the table)
       and, once, J1 alone (deqsci_ffdnet_head_masked_f32) at 64 images of 256 x 256 with its store bandwidth.
--table  Lip(f), rho(f), Lip(D) of SimpleCNN, RealSN_SimpleCNN and FFDNet on the three shipped clips at the reconstruction of a run of
       --iters DEQ iterations (harness.evaluate(batch="all", jacobian=dict(n_iters=, window=, seed=0))): the mean over a clip's scored
       measurements, every measurement's values in the JSON, and how far the last power step still moved the Lipschitz estimates.

Every GPU step is a child process of its own under `timeout`; the first one that fails ends the run (nothing more is started on the
GPU) with its exit status.  The results are merged into --out under "cost" and "table" (its other keys are kept) and printed as a table.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "data", "test_gray")
WEIGHTS = {"SimpleCNN": "cnn", "RealSN_SimpleCNN": "rsn_cnn", "ffdnet": "ffdnet_gray"}
STEP_SECONDS = {"cost": 240, "table": 600}             # per child; a table step: one reconstruction of 8 measurements + 5 n_iters products
REPORT_ITERS = 30


def time_ms(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def batch(n, dev):
    """(y (n,H,W), Phi (n,H,W,B)): traffic measurement 0, or the first n scored measurements of the shipped clips, each with its mask."""
    import torch
    from deqsci_amd import harness
    clips = [harness.as_clip(c) for c in harness.SCITestDataset(DATA)]
    picks = [(c, m) for c in clips for m in harness.scored_measurements(c['file'], c['meas'].shape[-1])]
    picks = [p for p in picks if "traffic" in p[0]['file']][:1] if n == 1 else picks[:n]
    y = torch.stack([c['meas'][..., m] for c, m in picks]).contiguous().to(dev)
    Phi = torch.stack([c['mask'] for c, _ in picks]).contiguous().to(dev)
    return y, Phi


def step_cost(kind, a):
    import torch
    from deqsci_amd import _hip, checkpoint, jacobian, operators
    from deqsci_amd.cli import build_pipeline
    dev = torch.device("cuda:0")
    solver, deq = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), 30, device=dev)
    out = {"denoiser": kind, "point": "the reconstruction of a 30-iteration run", "report_n_iters": REPORT_ITERS, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "unit": "ms, median of reps, HIP events after warm-up", "rows": []}
    for bsz in (1, 8):
        y, Phi = batch(bsz, dev)
        Ps = operators.phi_sum(Phi)
        with torch.no_grad():
            rec = deq.forward(y, Phi, Ps, initial_point=operators.initial_point(y, Phi, Ps, None), train_flag=False).detach()
            op = deq.jacobian_at(y, Phi, Ps, rec)
            sigma = getattr(op.denoiser, "sigma", None)
            v = jacobian.start_vector(rec[0].numel()).to(dev).view(1, *rec.shape[1:]).expand_as(rec).contiguous()
            flat, row = v.clone().view(bsz, -1), torch.zeros(bsz, 2, dtype=torch.float64, device=dev)
            ws = _hip.power_workspace(bsz, flat.shape[1], dev)
            t = {"setup_ms": time_ms(lambda: solver.device_jacobian(rec, y, Phi, Ps, sigma=sigma), a.reps),
                 "jv_ms": time_ms(lambda: op.jv(v), a.reps),
                 "jtv_ms": time_ms(lambda: op.jtv(v), a.reps),
                 "step_ms": time_ms(lambda: _hip.power_step(v.view(bsz, -1), v.view(bsz, -1), flat, row, ws), a.reps),
                 "report_ms": time_ms(lambda: jacobian.power_report(op, tuple(rec.shape), n_iters=REPORT_ITERS, window=10), a.reps, warmup=1)}
        out["rows"].append({"bsz": bsz, **{k: round(x, 4) for k, x in t.items()}})
    if kind == "ffdnet":                                                  # J1 alone, too large for the Infinity Cache to hold its output
        n, H2 = 64, 256
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, 1, H2, H2, generator=g).to(dev)
        w = _hip.pack_head_masked_weights((torch.randn(64, 4, 3, 3, generator=g) * 0.2).to(dev))
        mask = _hip.relu_mask_pack(torch.randn(n, 64, H2 // 2, H2 // 2, generator=g).to(dev).contiguous(memory_format=torch.channels_last))
        h = _hip.ffdnet_head_masked(x, w, mask)
        ms = time_ms(lambda: _hip.ffdnet_head_masked(x, w, mask, out=h), a.reps)
        stored = h.numel() * 4
        out["j1"] = {"images": n, "H": H2, "W": H2, "ms": round(ms, 4), "stored_bytes": stored, "store_GB_per_s": round(stored / ms / 1e6, 1)}
    return out


def step_table(kind, iters, a):
    import numpy as np
    import torch
    from deqsci_amd import checkpoint, harness
    from deqsci_amd.cli import build_pipeline
    dev = torch.device("cuda:0")
    _, deq = build_pipeline(kind, checkpoint.shipped(WEIGHTS[kind]), iters, device=dev)
    clips = list(harness.SCITestDataset(DATA))
    avg, results = harness.evaluate(deq, clips, device=dev, batch="all", jacobian=dict(n_iters=a.n_iters, window=a.window, seed=0))
    out = {"denoiser": kind, "iters": iters, "n_iters": a.n_iters, "window": a.window, "seed": 0, "psnr_avg": round(float(avg), 4), "clips": {}}
    for r in results:
        j, h = r.jacobian, r.jacobian["histories"]
        last = lambda name: [float(row[-1] / row[-2] - 1) for row in np.asarray(h[name])]
        out["clips"][r.name.split("_")[0]] = {
            "psnr": round(float(r.mean_psnr), 4), "measurements": list(r.info["measurements"]),
            **{k: [float(x) for x in j[k]] for k in harness.JACOBIAN_KEYS},
            "mean": {k: float(np.mean(j[k])) for k in harness.JACOBIAN_KEYS},
            "lipschitz_f_last_step_rel": last("lipschitz_f_history"), "lipschitz_denoiser_last_step_rel": last("lipschitz_denoiser_history"),
            "rho_f_rayleigh_window": [[float(np.min(row[-a.window:])), float(np.max(row[-a.window:]))] for row in np.asarray(h["rho_f_rayleigh"])],
            "rho_f_growth_window": [[float(np.min(row[-a.window:])), float(np.max(row[-a.window:]))] for row in np.asarray(h["rho_f_growth"])]}
    return out


def run_step(name, a):
    """One GPU step as a child process under its own time limit -> its JSON (the last line it prints)."""
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS[name.split(":")[0]]), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps),
           "--n_iters", str(a.n_iters), "--window", str(a.window)]
    print("+", name, file=sys.stderr, flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(f"step {name} ended with status {p.returncode}: nothing more is started", file=sys.stderr)
        sys.exit(p.returncode if p.returncode > 0 else 1)
    return json.loads(p.stdout.strip().splitlines()[-1])


def show(doc):
    for c in doc.get("cost", []):
        for r in c["rows"]:
            print(f"cost  {c['denoiser']:16s} bsz {r['bsz']}: setup {r['setup_ms']:8.3f}  J v {r['jv_ms']:8.3f}  J^T v {r['jtv_ms']:8.3f}  "
                  f"power step {r['step_ms']:7.3f}  report({c['report_n_iters']}) {r['report_ms']:9.2f}  ms")
        if "j1" in c:
            print(f"cost  J1 alone, {c['j1']['images']} images of {c['j1']['H']}x{c['j1']['W']}: {c['j1']['ms']:.3f} ms, {c['j1']['store_GB_per_s']:.0f} GB/s stored")
    for t in doc.get("table", []):
        for name, c in t["clips"].items():
            m = c["mean"]
            print(f"table {t['denoiser']:16s} @{t['iters']:<4d} {name:8s} PSNR {c['psnr']:6.2f}  Lip(f) {m['lipschitz_f']:.4f}  rho(f) {m['rho_f']:.4f}  "
                  f"Lip(D) {m['lipschitz_denoiser']:.4f}  (rho per measurement {min(c['rho_f']):.4f} .. {max(c['rho_f']):.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--iters", type=int, nargs="+", default=[180], help="DEQ iterations of the runs whose reconstructions --table linearises at")
    ap.add_argument("--n_iters", type=int, default=100, help="power steps of --table")
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_jacobian.json"))
    ap.add_argument("--step", help=argparse.SUPPRESS)                     # (a child: cost:<denoiser> or table:<denoiser>:<iters>)
    a = ap.parse_args()
    if a.step:
        what, *rest = a.step.split(":")
        print(json.dumps(step_cost(rest[0], a) if what == "cost" else step_table(rest[0], int(rest[1]), a)))
        return
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc["cost"] = [run_step(f"cost:{k}", a) for k in ("SimpleCNN", "ffdnet")]
    if a.table:
        doc["table"] = [run_step(f"table:{k}:{i}", a) for k in WEIGHTS for i in a.iters]
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    show(doc)


if __name__ == "__main__":
    main()
