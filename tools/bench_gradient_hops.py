#!/usr/bin/env python3
"""Multi-hop gradient ray tracing and multi-hop homing (prhf_trace_gradient_hops_f64, prhf_gradient_hop_home_f64) against
the route through the one-hop calls with the hops chained on the host, on the same build, both geometries.

    python tools/bench_gradient_hops.py [--reps N] [--warmup N] [--out profiles/bench_gradient_hops.jsonl]

Field: G24's tilted ionosphere (121 x 401 nodes, x within +-2000 km), 64 frequencies of the O mode, launch point
(-1800, 0), max_step_km=5.
  tracing  16 384 chains (64 fields x 256 elevations, 10 .. 50 degrees) of 3 hops: one trace_hops_* call, against three trace_rays_*
           calls with return_paths (the landing direction is the last path node), the reflected elevation computed in
           NumPy and the landed rays launched again.
  homing   64 links (16 fields x 4 targets) on hop 1, 33 scan nodes: one home_hops_* call, against the bracket rule in
           NumPy and the kernel's stepping rule vectorised over the open brackets, D(e) being two chained trace_rays_*
           calls per step.
Both routes are timed end to end on NumPy arrays: wall time around the synchronous calls, best and median of --reps
interleaved repetitions after --warmup.  Bits: the host computes the reflected elevation with np.arctan2, the kernel with
the device's atan2; every hop row whose launch columns agree to the bit must agree in every key (asserted), the rows
whose launch elevations differ (the arctangents' last bits, and what follows from them on later hops) are counted.  Of
the homing routes the brackets, elevations and statuses are compared and counted.  One JSON line per geometry and
workload, the homing lines with the refinement's lane utilisation from the kernels' counters.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import gradient, synth  # noqa: E402

X0, Z0 = -1800.0, 0.0
TRACE_F, TRACE_E, TRACE_H = 64, 256, 3
HOME_F, HOME_H = 16, 2
TARGETS = np.array([-500.0, 0.0, -1100.0, -800.0])
SCAN = np.linspace(10.0, 70.0, 33)
TOL, MAX_ITER, MAX_ROOTS = 0.05, 64, 4
KEYS = gradient._KEYS


def controls(spherical, r_e):
    if spherical:
        return dict(s_max_km=4000.0, max_step_km=5.0, r_max_km=r_e + 600.0, phi_min=-2000.0 / r_e, phi_max=2000.0 / r_e)
    return dict(s_max_km=4000.0, max_step_km=5.0, z_max_km=600.0, x_min_km=-2000.0, x_max_km=2000.0)


def reflect(spherical, r):
    """The launch of the next hop from a one-hop result with paths: (x, elevation) per ray (NaN unless it landed)."""
    last = np.maximum(r["n_nodes"] - 1, 0)[:, None]
    v_h = np.take_along_axis(r["v_phi" if spherical else "vx"], last, axis=1)[:, 0]
    v_v = np.take_along_axis(r["v_r" if spherical else "vz"], last, axis=1)[:, 0]
    landed = r["status"] == 0
    return landed, np.where(landed, r["ground_range_km"], np.nan), np.where(landed, np.degrees(np.arctan2(-v_v, v_h)), np.nan)


def host_chains(spherical, field, ctl, e, fi, n_hops):
    """Rows (R, n_hops, 3 + 11) by the one-hop tracer, chained on the host; the number of native calls."""
    ray_fn = gradient.trace_rays_spherical_gradient if spherical else gradient.trace_rays_cartesian_gradient
    rows = np.full((e.size, n_hops, 3 + len(KEYS)), np.nan)
    rows[:, :, 3 + KEYS.index("status")] = -1
    rows[:, :, 4 + KEYS.index("status"):] = 0
    live = np.arange(e.size)
    x, z, el = np.full(e.size, X0), np.full(e.size, Z0), e
    calls = 0
    for h in range(n_hops):
        if live.size == 0:
            break
        last_hop = h == n_hops - 1
        r = ray_fn(field, x, z, el, fi[live], return_paths=not last_hop, **ctl)
        calls += 1 if last_hop else 2                                       # (return_paths traces twice)
        rows[live, h, 0], rows[live, h, 1], rows[live, h, 2] = x, z, el
        for i, k in enumerate(KEYS):
            rows[live, h, 3 + i] = r[k]
        if last_hop:
            break
        landed, x, el = reflect(spherical, r)
        live, x, el = live[landed], x[landed], el[landed]
        z = np.zeros(live.size)
    return rows, calls


def compare_rows(got, want):
    """got: the one-call dict (R, H); want: host rows.  Asserts equal bits wherever the launch columns agree."""
    cols = gradient._HOP_LAUNCH_KEYS + KEYS
    g = np.stack([got[k].astype(np.float64) for k in cols], axis=-1)
    same = lambda a, b: (a == b) | (np.isnan(a) & np.isnan(b))              # noqa: E731
    launch_same = np.all(same(g[..., :3], want[..., :3]), axis=-1)
    used = np.isfinite(g[..., 2]) & np.isfinite(want[..., 2])
    assert np.all(same(g[launch_same], want[launch_same])), "rows with equal launch columns differ"
    de = np.abs(g[..., 2] - want[..., 2])[used & ~launch_same]
    return {"hop_rows": int(used.sum()), "hop_rows_equal_bits": int((used & launch_same).sum()),
            "hops_in_one_route_only": int((np.isfinite(g[..., 2]) != np.isfinite(want[..., 2])).sum()),
            "max_launch_elevation_difference_deg": float(de.max()) if de.size else 0.0}


def host_home(spherical, field, ctl):
    def chain_d(x, fi):
        rows, calls = host_chains(spherical, field, ctl, x, fi, HOME_H)
        ok = np.all(rows[:, :, 3 + KEYS.index("status")] == 0, axis=1)
        return np.where(ok, rows[:, -1, 3 + KEYS.index("ground_range_km")], np.nan), calls
    nf = field.n_fields
    d, calls = chain_d(np.tile(SCAN, nf), np.repeat(np.arange(nf), SCAN.size))
    d = d.reshape(nf, SCAN.size)
    f_lo = d[:, None, :-1] - TARGETS[None, :, None]
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
        dx, c = chain_d(x, fi[k])
        calls += c
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
    rows, c = host_chains(spherical, field, ctl, best_e, fi, HOME_H)
    return {"n_brackets": n_brackets, "link": (fi, ti), "rank": rank[fi, ti, ii], "elevation_deg": best_e, "status": status,
            "rows": rows, "calls": calls + c}


def timed(new, old, reps, warmup):
    for _ in range(max(warmup, 1)):
        got, want = new(), old()
    t_new, t_old = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); got = new(); t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); want = old(); t_old.append(time.perf_counter() - t0)
    times = {"one_call_s_best": float(np.min(t_new)), "one_call_s_median": float(np.median(t_new)),
             "host_route_s_best": float(np.min(t_old)), "host_route_s_median": float(np.median(t_old)),
             "host_route_over_one_call": float(np.median(t_old) / np.median(t_new))}
    return got, want, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000.0)
    r_e = gradient.constants()[2]
    lines = []
    for spherical, name in ((False, "cartesian"), (True, "spherical")):
        ctl = controls(spherical, r_e)
        field = gradient.refractive_field(np.linspace(5e6, 7e6, TRACE_F), den, bmag, bpsi, z, x, "O", geometry=name)
        hops_fn = gradient.trace_hops_spherical_gradient if spherical else gradient.trace_hops_cartesian_gradient
        e = np.tile(np.linspace(10.0, 50.0, TRACE_E), TRACE_F)
        fi = np.repeat(np.arange(TRACE_F), TRACE_E)
        got, (want, calls), times = timed(lambda: hops_fn(field, X0, Z0, e, TRACE_H, fi, **ctl),
                                          lambda: host_chains(spherical, field, ctl, e, fi, TRACE_H), args.reps, args.warmup)
        lines.append({"workload": "tracing", "geometry": name, "chains": int(e.size), "hops": TRACE_H, "grid": [121, 401],
                      "landed_hops": [int(v) for v in (got["status"] == 0).sum(axis=0)], "host_route_native_calls": int(calls),
                      **times, **compare_rows(got, want)})
        print(json.dumps(lines[-1]), flush=True)

        home_field = gradient.RefractiveField(field.axis0, field.axis1, field.mu[::TRACE_F // HOME_F], field.mup[::TRACE_F // HOME_F],
                                              geometry=name)
        home_fn = gradient.home_hops_spherical_gradient if spherical else gradient.home_hops_cartesian_gradient
        ctx = home_field._ctx()
        got, want, times = timed(lambda: home_fn(home_field, TARGETS, HOME_H, X0, Z0, scan_elevation_deg=SCAN,
                                                 max_roots=MAX_ROOTS, range_tol_km=TOL, max_iter=MAX_ITER, **ctl),
                                 lambda: host_home(spherical, home_field, ctl), args.reps, args.warmup)
        records, rays, slots, waves = ctx.gradient_home_counters()
        f_i, t_i = want["link"]
        same_st = got["status"][f_i, t_i, want["rank"]] == want["status"]
        same_e = got["elevation_deg"][f_i, t_i, want["rank"]] == want["elevation_deg"]
        rows = compare_rows({k: v[f_i, t_i, want["rank"]][same_e] for k, v in
                             ((k, got["ray_status" if k == "status" else k]) for k in gradient._HOP_LAUNCH_KEYS + KEYS)},
                            want["rows"][same_e])
        lines.append({"workload": "homing", "geometry": name, "links": int(got["n_brackets"].size), "hops": HOME_H,
                      "scan_nodes": int(SCAN.size), "brackets": int(got["n_brackets"].sum()), "rows_refined": int(records),
                      "status_counts": {str(s): int((got["status"] == s).sum()) for s in (0, 1, 2)},
                      "host_route_native_calls": int(want["calls"]), **times,
                      "same_brackets": bool(np.array_equal(got["n_brackets"], want["n_brackets"])), "rows_same_status": int(same_st.sum()),
                      "rows_same_elevation_bits": int(same_e.sum()), "rows": int(same_e.size), **rows,
                      "refine_rays": int(rays), "refine_ray_slots": int(slots), "refine_wavefronts": int(waves),
                      "refine_lane_utilisation": float(rays / slots) if slots else None})
        print(json.dumps(lines[-1]), flush=True)
    if args.out and lines:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
