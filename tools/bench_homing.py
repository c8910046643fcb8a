#!/usr/bin/env python3
"""Point-to-point homing (prhf_snell_home_f64) against the best route through the calls that existed before it, on the
same build: 64 Chapman profiles x 128 frequencies x 4 ranges on the default scan grid, both geometries.

    python tools/bench_homing.py [--reps N] [--out profiles/bench_homing.jsonl] [--once]

The host route: (1) one trace_fan_*_snells call on the scan grid, (2) the bracket rule in NumPy, (3) the kernel's own
stepping rule (Illinois, a bisection whenever a step did not halve the bracket) vectorised over all open brackets, ONE
batched trace_rays_*_snells call per step, to the same tolerance and the same max_iter - fewer calls than plain
bisection needs.  Both routes are timed end to end on NumPy arrays (host clock around synchronous calls, the median of
--reps interleaved repetitions after a warm-up); the new call's device time is the context's event pair around its five
kernels.  One JSON line per geometry; --once makes one homing call per geometry and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import _native, synth, tracers  # noqa: E402

P, F = 64, 128
TARGETS = np.array([300.0, 800.0, 1500.0, 2500.0])
TOL, MAX_ITER, MAX_ROOTS = 1e-6, 64, 4


def host_route(spherical, f, alt, den, bmag, bpsi, mode, scan):
    fan_fn = tracers.trace_fan_spherical_snells if spherical else tracers.trace_fan_cartesian_snells
    ray_fn = tracers.trace_rays_spherical_snells if spherical else tracers.trace_rays_cartesian_snells
    d = fan_fn(f, scan, alt, den, bmag, bpsi, mode)["ground_range_km"]              # (P, F, E)
    calls = 1
    f_lo = d[:, :, None, :-1] - TARGETS[None, None, :, None]                         # (P, F, T, E - 1)
    f_hi = d[:, :, None, 1:] - TARGETS[None, None, :, None]
    with np.errstate(invalid="ignore"):
        is_b = np.isfinite(f_lo) & np.isfinite(f_hi) & ((f_lo * f_hi < 0) | (f_lo == 0))
    n_brackets = is_b.sum(axis=-1)
    rank = np.cumsum(is_b, axis=-1) - 1
    pi, fi, ti, ii = np.nonzero(is_b & (rank < MAX_ROOTS))
    lo, hi, f_lo, f_hi = scan[ii], scan[ii + 1], f_lo[pi, fi, ti, ii], f_hi[pi, fi, ti, ii]
    t = TARGETS[ti]
    best_e = np.where(np.abs(f_hi) < np.abs(f_lo), hi, lo)
    best = np.minimum(np.abs(f_lo), np.abs(f_hi))
    status = np.where(best <= TOL, 0, 1)
    g_lo, g_hi = f_lo.copy(), f_hi.copy()
    last = np.zeros(lo.size, dtype=np.int64)
    bisect = np.zeros(lo.size, dtype=bool)
    is_open = status == 1
    for _ in range(MAX_ITER):
        mid = lo + 0.5 * (hi - lo)
        is_open &= (mid > lo) & (mid < hi)
        k = np.nonzero(is_open)[0]
        if k.size == 0:
            break
        with np.errstate(all="ignore"):
            xs = lo[k] - g_lo[k] * ((hi[k] - lo[k]) / (g_hi[k] - g_lo[k]))
        x = np.where(~bisect[k] & (xs > lo[k]) & (xs < hi[k]), xs, mid[k])
        dx = ray_fn(f[fi[k]], x, alt, den, bmag, bpsi, mode, profile_index=pi[k])["ground_range_km"]
        calls += 1
        fx = dx - t[k]
        escaped = ~np.isfinite(dx)
        status[k[escaped]] = 2
        miss = np.where(escaped, np.inf, np.abs(fx))
        better = miss < best[k]
        best[k[better]], best_e[k[better]] = miss[better], x[better]
        done = miss <= TOL
        status[k[done]] = 0
        is_open[k[escaped | done]] = False
        width = hi[k] - lo[k]
        low = (fx < 0) == (f_lo[k] < 0)
        kl, kh = k[low], k[~low]
        g_hi[kl] = np.where(last[kl] == -1, 0.5 * g_hi[kl], g_hi[kl])
        lo[kl], f_lo[kl], g_lo[kl], last[kl] = x[low], fx[low], fx[low], -1
        g_lo[kh] = np.where(last[kh] == 1, 0.5 * g_lo[kh], g_lo[kh])
        hi[kh], g_hi[kh], last[kh] = x[~low], fx[~low], 1
        bisect[k] = (hi[k] - lo[k]) > 0.5 * width
    return {"n_brackets": n_brackets, "link": (pi, fi, ti), "rank": rank[pi, fi, ti, ii], "elevation_deg": best_e,
            "status": status, "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    alt, den, bmag, bpsi = synth.chapman_profiles(P, 7)
    f = np.linspace(2e6, 14e6, F)
    scan = tracers.default_scan_elevations()
    ctx = _native.context(0)
    lines = []
    for spherical, name in ((False, "cartesian"), (True, "spherical")):
        home_fn = tracers.home_rays_spherical_snells if spherical else tracers.home_rays_cartesian_snells

        def new():
            return home_fn(f, TARGETS, alt, den, bmag, bpsi, "O", max_roots=MAX_ROOTS, range_tol_km=TOL, max_iter=MAX_ITER)
        if args.once:
            new()
            continue
        got, want = new(), host_route(spherical, f, alt, den, bmag, bpsi, "O", scan)         # warm-up of every shape
        t_new, t_old, dev_ms = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); got = new(); t_new.append(time.perf_counter() - t0)
            dev_ms.append(ctx.last_kernel_ms())
            t0 = time.perf_counter(); want = host_route(spherical, f, alt, den, bmag, bpsi, "O", scan)
            t_old.append(time.perf_counter() - t0)
        pi, fi, ti = want["link"]
        same = bool(np.array_equal(got["n_brackets"], want["n_brackets"]))
        e_new = got["elevation_deg"][pi, fi, ti, want["rank"]]
        both = (got["status"][pi, fi, ti, want["rank"]] == 0) & (want["status"] == 0)
        lines.append({"geometry": name, "profiles": P, "frequencies": F, "ranges": int(TARGETS.size), "scan_nodes": int(scan.size),
                      "links": int(got["n_brackets"].size), "brackets": int(got["n_brackets"].sum()),
                      "rows_refined": int((got["status"] >= 0).sum()),
                      "status_counts": {str(s): int((got["status"] == s).sum()) for s in (0, 1, 2)},
                      "home_call_s": float(np.median(t_new)), "home_call_s_all": [round(v, 6) for v in t_new],
                      "home_device_ms": float(np.median(dev_ms)),
                      "host_route_s": float(np.median(t_old)), "host_route_s_all": [round(v, 6) for v in t_old],
                      "host_route_native_calls": int(want["calls"]),
                      "host_route_over_home": float(np.median(t_old) / np.median(t_new)),
                      "same_n_brackets": same, "same_status": bool(np.array_equal(got["status"][pi, fi, ti, want["rank"]], want["status"])),
                      "max_elevation_difference_deg_converged": float(np.max(np.abs(e_new - want["elevation_deg"])[both])) if both.any() else None})
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
