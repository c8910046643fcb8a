#!/usr/bin/env python3
"""Time the device-resident Levenberg-Marquardt fit (fitting.fit_profiles_lm) against the host route it replaces.

    python tools/bench_lm_fit.py [--reps N] [--out profiles/bench_lm_fit.jsonl] [--quick] [--step-timeout S]

Shape: 4096 ionograms x 64 frequencies (0.3, 0.4, ... 6.6 MHz of config 3's sweep; NaN where the truth does not reflect),
T = 4 Gaussian directions per column, O mode, 200 points, on config 3's Chapman columns; a fixed 10 evaluations on both
routes (ftol = xtol = 0 on the device: no ionogram ends early; a frozen one would ride along in the same launches anyway).
Host route: per evaluation the trial columns are made on the GPU with torch, ONE library.vertical_jvp call on the
resident tensors gives vh and dvh, both are copied to the host, the step - masked normal equations, damping, a batched
Cholesky solve, accept or reject - is NumPy, vectorised over the ionograms, and the new coefficients go back up.
Method, also written into the line: the measurement runs in a child process under a time limit (the parent never opens
the GPU); everything is resident before the clock starts; each route is warmed up once, then the two alternate `reps`
times; a call's time is the host clock around it, ending in a synchronisation; medians.  The device route's launches are
also read from the context's events (recent_kernel_ms: per evaluation trial columns, operator, JVP, step): their sums
over the call's time are the shares reported.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

METHOD = ("child process under a time limit; resident arrays; 1 warm-up per route, then the routes alternate reps times; "
          "host clock around each call, ending in a synchronisation; medians; device launches from the context's events")
N_EVAL = 10


def host_step(c, c_eval, cost, lam, A, g, vh, dvh, obs, k):
    """One evaluation's step for every ionogram at once (the rule of prhf_lm_step.h, NumPy's own summation order)."""
    kept = np.isfinite(obs)
    m = np.abs(vh)
    ok = kept & np.isfinite(m)
    n = ok.sum(axis=1)
    mean = np.where(n > 0, np.where(ok, m, 0.0).sum(axis=1) / np.maximum(n, 1), np.nan)
    fill = np.maximum(mean, 100.0)
    r = np.where(kept, obs - np.where(np.isnan(vh), fill[:, None], vh), 0.0)
    d = np.where(kept[:, :, None], dvh, 0.0)
    cost_eval = (r * r).sum(axis=1)
    accept = np.ones(len(c), dtype=bool) if k == 0 else cost_eval < cost
    if k > 0:
        lam = np.clip(np.where(accept, lam / 10.0, lam * 10.0), 1e-12, 1e12)
    A_eval = np.einsum("ift,ifs->its", d, d)
    g_eval = np.einsum("ift,if->it", d, r)
    c = np.where(accept[:, None], c_eval, c)
    cost = np.where(accept, cost_eval, cost)
    A = np.where(accept[:, None, None], A_eval, A)
    g = np.where(accept[:, None], g_eval, g)
    diag = np.maximum(np.einsum("itt->it", A), 1e-30)
    M = A + lam[:, None, None] * (np.eye(A.shape[1])[None] * diag[:, :, None])
    lost = ~np.isfinite(M).all(axis=(1, 2)) | (n == 0)           # nothing to fit, or no finite cost: a zero step
    M[lost] = np.eye(A.shape[1])
    g = np.where(lost[:, None], 0.0, g)
    L = np.linalg.cholesky(M)
    delta = np.linalg.solve(np.swapaxes(L, 1, 2), np.linalg.solve(L, g[:, :, None]))[:, :, 0]
    dmax = np.max(np.abs(delta), axis=1)
    delta = delta * np.minimum(1.0, 1.0 / np.maximum(dmax, 1e-300))[:, None]
    return c, c + delta, cost, lam, A, g


def measure(reps, quick):
    import torch
    from pyrayhf_amd import _native, fitting, library, synth
    n_iono, n_freq, n_tan = (256 if quick else 4096), 64, 4
    dev = torch.device("cuda", 0)
    alt, den0, bmag, bpsi = synth.chapman_profiles_torch(n_iono, 3, dev)
    freq_np = synth.sounder_frequencies(3)[2:2 + n_freq]
    freq = torch.as_tensor(freq_np, device=dev)
    peak = torch.argmax(den0, dim=1)
    z = (alt[None, :] - alt[0]) / (alt[peak] - alt[0])[:, None]
    centres = torch.linspace(0.2, 0.9, n_tan, dtype=torch.float64, device=dev)
    basis = torch.exp(-0.5 * ((z[:, None, :] - centres[None, :, None]) / 0.2) ** 2).contiguous()
    c_true = torch.as_tensor(np.random.default_rng(4).uniform(-0.08, 0.08, (n_iono, n_tan)), device=dev)
    truth = den0 * torch.exp(torch.einsum("it,itk->ik", c_true, basis))
    obs = library.vertical_forward_operator(freq, truth, bmag, bpsi, alt, "O", 200)
    obs_np = obs.cpu().numpy()
    ctx = _native.context(0)

    def device_route():
        t0 = time.perf_counter()
        r = fitting.fit_profiles_lm(freq, obs, den0, bmag, bpsi, alt, basis, "O", 200, max_iter=N_EVAL, ftol=0.0, xtol=0.0)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, r

    def host_route():
        t0 = time.perf_counter()
        c = np.zeros((n_iono, n_tan))
        c_eval, cost, lam = c.copy(), np.full(n_iono, np.nan), np.full(n_iono, 1e-3)
        A, g = np.zeros((n_iono, n_tan, n_tan)), np.zeros((n_iono, n_tan))
        for k in range(N_EVAL):
            den = den0 * torch.exp(torch.einsum("it,itk->ik", torch.as_tensor(c_eval, device=dev), basis))
            vh, dvh = library.vertical_jvp(freq, den, bmag, bpsi, alt, den[:, None, :] * basis, "O", 200)
            c, c_eval, cost, lam, A, g = host_step(c, c_eval, cost, lam, A, g, vh.cpu().numpy(), dvh.cpu().numpy(), obs_np, k)
        return time.perf_counter() - t0, (c, cost)

    device_route()
    host_route()
    dev_s, host_s, shares = [], [], []
    for _ in range(reps):
        t, r = device_route()
        ms = ctx.recent_kernel_ms(4 * N_EVAL + 1)
        assert ctx.lm_fit_counters()[:2] == (N_EVAL, 4 * N_EVAL + 1) and len(ms) == 4 * N_EVAL + 1
        per = np.asarray(ms[:4 * N_EVAL]).reshape(N_EVAL, 4).sum(axis=0)
        dev_s.append(t)
        shares.append(per / (t * 1e3))
        t, h = host_route()
        host_s.append(t)
    shares = np.median(np.asarray(shares), axis=0)
    both = np.isfinite(h[1]) & np.isfinite(r.cost.cpu().numpy())
    rec = {"n_iono": n_iono, "n_freq": n_freq, "n_tan": n_tan, "n_alt": int(den0.shape[1]), "mode": "O", "n_points": 200,
           "evaluations": N_EVAL, "reps": reps,
           "device_ms": float(np.median(dev_s) * 1e3), "device_ms_min_max": [float(min(dev_s) * 1e3), float(max(dev_s) * 1e3)],
           "host_route_ms": float(np.median(host_s) * 1e3),
           "host_route_ms_min_max": [float(min(host_s) * 1e3), float(max(host_s) * 1e3)],
           "host_over_device": float(np.median(host_s) / np.median(dev_s)),
           "share_trial_columns": float(shares[0]), "share_operator": float(shares[1]), "share_jvp": float(shares[2]),
           "share_step": float(shares[3]), "host_waits_per_call": int(ctx.lm_fit_counters()[2]),
           "median_cost_device": float(np.median(r.cost.cpu().numpy()[both])), "median_cost_host_route": float(np.median(h[1][both])),
           "method": METHOD}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed calls per route: 30 x 21 ms is 0.6 s on the device route")
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="a small batch, to rehearse the script")
    ap.add_argument("--step-timeout", type=float, default=400.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process and print the line")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.reps, args.quick)), flush=True)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)] + (["--quick"] if args.quick else [])
    try:
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"no result within {args.step_timeout:.0f} s")
    if run.returncode != 0:
        raise SystemExit(f"the measurement failed with status {run.returncode}:\n" + run.stderr[-3000:])
    line = run.stdout.strip().splitlines()[-1]
    json.loads(line)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
