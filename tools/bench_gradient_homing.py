#!/usr/bin/env python3
"""Point-to-point homing for the gradient tracers (prhf_gradient_home_f64) against the best route through the calls that
existed before it, on the same build: 64 fields (frequencies of G18's tilted ionosphere, 121 x 201 nodes) x 4 targets
from (-400, 0) on a 33-node scan, both geometries.

    python tools/bench_gradient_homing.py [--reps N] [--warmup N] [--out profiles/bench_gradient_homing.jsonl]

The host route: (1) one trace_fan_*_gradient call on the scan grid, (2) the bracket rule in NumPy, (3) the kernel's own
stepping rule (Illinois, a bisection whenever a step did not halve the bracket, a bracket closed as soon as its status
is decided) vectorised over all open brackets, ONE batched trace_rays_*_gradient call per step, (4) one batched call
for the result rays.  Both routes are timed end to end on NumPy arrays: wall time around the synchronous calls, best and
median of --reps interleaved repetitions after --warmup; the new call's device time is the context's event pair around
its four kernels.  The two routes must return the same elevations and statuses bit for bit (asserted).  One JSON line per
geometry, with the refinement's lane utilisation from the kernels' counters.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import _native, gradient, synth  # noqa: E402

F = 64
TARGETS = np.array([300.0, 100.0, 700.0, -100.0])
X0, Z0 = -400.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TOL, MAX_ITER, MAX_ROOTS = 0.05, 64, 4


def controls(spherical, r_e):
    if spherical:
        return dict(s_max_km=4000.0, max_step_km=2.0, r_max_km=r_e + 600.0, phi_min=-1000.0 / r_e, phi_max=1000.0 / r_e)
    return dict(s_max_km=4000.0, max_step_km=2.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0)


def host_route(spherical, field, ctl):
    fan_fn = gradient.trace_fan_spherical_gradient if spherical else gradient.trace_fan_cartesian_gradient
    ray_fn = gradient.trace_rays_spherical_gradient if spherical else gradient.trace_rays_cartesian_gradient
    d = fan_fn(field, SCAN, X0, Z0, **ctl)["ground_range_km"]                        # (F, E)
    calls = 1
    f_lo = d[:, None, :-1] - TARGETS[None, :, None]                                  # (F, T, E - 1)
    f_hi = d[:, None, 1:] - TARGETS[None, :, None]
    with np.errstate(invalid="ignore"):
        is_b = np.isfinite(f_lo) & np.isfinite(f_hi) & ((f_lo * f_hi < 0) | (f_lo == 0))
    n_brackets = is_b.sum(axis=-1)
    rank = np.cumsum(is_b, axis=-1) - 1
    fi, ti, ii = np.nonzero(is_b & (rank < MAX_ROOTS))
    lo, hi, f_lo, f_hi = SCAN[ii], SCAN[ii + 1], f_lo[fi, ti, ii], f_hi[fi, ti, ii]
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
        dx = ray_fn(field, X0, Z0, x, fi[k], **ctl)["ground_range_km"]
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
        go = ~(escaped | done)
        width = hi[k] - lo[k]
        low = ((fx < 0) == (f_lo[k] < 0)) & go
        high = ~low & go
        kl, kh = k[low], k[high]
        g_hi[kl] = np.where(last[kl] == -1, 0.5 * g_hi[kl], g_hi[kl])
        lo[kl], f_lo[kl], g_lo[kl], last[kl] = x[low], fx[low], fx[low], -1
        g_lo[kh] = np.where(last[kh] == 1, 0.5 * g_lo[kh], g_lo[kh])
        hi[kh], g_hi[kh], last[kh] = x[high], fx[high], 1
        bisect[k] = (hi[k] - lo[k]) > 0.5 * width
    rows = ray_fn(field, X0, Z0, best_e, fi, **ctl)
    calls += 1
    return {"n_brackets": n_brackets, "link": (fi, ti), "rank": rank[fi, ti, ii], "elevation_deg": best_e, "status": status,
            "group_path_km": rows["group_path_km"], "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.3, 18)
    freqs = np.linspace(4e6, 8e6, F)
    r_e = gradient.constants()[2]
    lines = []
    for spherical, name in ((False, "cartesian"), (True, "spherical")):
        field = gradient.refractive_field(freqs, den, bmag, bpsi, z, x, "O", geometry=name)
        ctl = controls(spherical, r_e)
        home_fn = gradient.home_rays_spherical_gradient if spherical else gradient.home_rays_cartesian_gradient
        ctx = field._ctx()

        def new():
            return home_fn(field, TARGETS, X0, Z0, scan_elevation_deg=SCAN, max_roots=MAX_ROOTS, range_tol_km=TOL,
                           max_iter=MAX_ITER, **ctl)
        for _ in range(max(args.warmup, 1)):
            got, want = new(), host_route(spherical, field, ctl)
        t_new, t_old, dev_ms = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); got = new(); t_new.append(time.perf_counter() - t0)
            dev_ms.append(ctx.last_kernel_ms())
            counters = ctx.gradient_home_counters()
            t0 = time.perf_counter(); want = host_route(spherical, field, ctl)
            t_old.append(time.perf_counter() - t0)
        fi, ti = want["link"]
        assert np.array_equal(got["n_brackets"], want["n_brackets"])
        assert np.array_equal(got["status"][fi, ti, want["rank"]], want["status"])
        assert np.array_equal(got["elevation_deg"][fi, ti, want["rank"]], want["elevation_deg"])
        assert np.array_equal(got["group_path_km"][fi, ti, want["rank"]], want["group_path_km"])
        records, rays, slots, waves = counters
        lines.append({"geometry": name, "fields": F, "targets": int(TARGETS.size), "scan_nodes": int(SCAN.size),
                      "grid": [121, 201], "links": int(got["n_brackets"].size), "brackets": int(got["n_brackets"].sum()),
                      "rows_refined": int(records),
                      "status_counts": {str(s): int((got["status"] == s).sum()) for s in (0, 1, 2)},
                      "home_call_s_best": float(np.min(t_new)), "home_call_s_median": float(np.median(t_new)),
                      "home_call_s_all": [round(v, 6) for v in t_new],
                      "home_device_ms_best": float(np.min(dev_ms)), "home_device_ms_median": float(np.median(dev_ms)),
                      "host_route_s_best": float(np.min(t_old)), "host_route_s_median": float(np.median(t_old)),
                      "host_route_s_all": [round(v, 6) for v in t_old], "host_route_native_calls": int(want["calls"]),
                      "host_route_over_home": float(np.median(t_old) / np.median(t_new)),
                      "refine_rays": int(rays), "refine_ray_slots": int(slots), "refine_wavefronts": int(waves),
                      "refine_lane_utilisation": float(rays / slots) if slots else None,
                      "same_elevations_and_statuses": True})
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
