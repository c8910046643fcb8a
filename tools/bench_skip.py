#!/usr/bin/env python3
"""Skip distance (prhf_snell_skip_f64) and MUF (prhf_snell_muf_f64) against the best route through the calls that
existed before them, on the same build: 64 Chapman profiles x 128 frequencies (skip) and 64 profiles x 4 ranges (MUF)
on the default scan grid, both geometries.

    python tools/bench_skip.py [--reps N] [--out profiles/bench_skip.jsonl] [--once]

The host route of the skip distance: (1) one native fan call on the scan grid, (2) the node rule in NumPy (argmin over
the finite D_i, the edge class), (3) the golden-section rule of DESIGN.md section 4.10 vectorised over all open groups,
ONE native fan call per step with one ray per open group.  The host route of the MUF: the bisection of section 4.10 in
NumPy over all links at once with that skip route as S(f).  Both routes are timed end to end on NumPy arrays (host clock
around synchronous calls, the median of --reps interleaved repetitions after a warm-up); the new calls' device time is
the context's event pair around their kernels.  The two routes must agree bit for bit (recorded, and asserted).  One
JSON line per call and geometry; --once makes one call of each per geometry and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import _native, library, synth, tracers  # noqa: E402

P, F = 64, 128
TARGETS = np.array([300.0, 800.0, 1500.0, 2500.0])
F_LO, F_HI, N_BISECT = 2e6, 30e6, 24
TOL, MAX_ITER = 1e-6, 64
GOLD = 0.3819660112501051


class HostRoute:
    """Ground ranges of (group, elevation) rays through prhf_snell_fan_f64, and the rule of section 4.10 on top."""

    def __init__(self, spherical, alt, den, bmag, bpsi, mode, scan):
        self.geometry = 1 if spherical else 0
        self.alt, self.den, self.bmag, self.bpsi = (np.ascontiguousarray(v) for v in (alt, den, bmag, bpsi))
        self.mode = _native.MODE_O if mode == "O" else _native.MODE_X
        self.scan = scan
        self.r_e = library.constants()[2]                             # (the tracers' default R_E)
        self.ctx = _native.host_context(None)
        self.calls = 0

    def rays(self, group_f, group_p, ray_group, ray_e):
        out = np.empty((ray_e.size, 8))
        n_prof, n_alt = self.den.shape
        rc = self.ctx.snell_fan(self.geometry, group_f.ctypes.data, group_p.ctypes.data, group_f.size, ray_group.ctypes.data,
                                ray_e.ctypes.data, ray_e.size, self.den.ctypes.data, self.bmag.ctypes.data,
                                self.bpsi.ctypes.data, self.alt.ctypes.data, n_prof, n_alt, 0, self.mode, self.r_e, 1.0, 200.0,
                                400, out.ctypes.data, None, None, 2 * n_alt + 1, 0)
        _native.raise_for(rc)
        self.calls += 1
        return out[:, 4]

    def skip(self, group_f, group_p):
        """-> status, scan_index, elevation_deg, skip_km, n_evals per group"""
        n, scan = group_f.size, self.scan
        group_f, group_p = np.ascontiguousarray(group_f), np.ascontiguousarray(group_p)
        d = self.rays(group_f, group_p, np.repeat(np.arange(n), scan.size), np.tile(scan, n)).reshape(n, scan.size)
        ok = np.isfinite(d)
        i = np.argmin(np.where(ok, d, np.inf), axis=1)
        none = ~ok.any(axis=1)
        lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, scan.size - 1)
        rows = np.arange(n)
        edge = (i == 0) | (i == scan.size - 1) | ~ok[rows, lo] | ~ok[rows, hi]
        status = np.where(none, -1, np.where(edge, 1, 3))
        a, b, c, db = scan[lo].copy(), scan[i].copy(), scan[hi].copy(), d[rows, i].copy()
        n_evals = np.zeros(n, dtype=np.int64)
        is_open = status == 3
        for _ in range(MAX_ITER + 1):
            k = np.nonzero(is_open)[0]
            if k.size == 0:
                break
            narrow = c[k] - a[k] <= TOL
            right = (c[k] - b[k]) >= (b[k] - a[k])
            x = np.where(right, b[k] + GOLD * (c[k] - b[k]), b[k] - GOLD * (b[k] - a[k]))
            spent = ~((x > a[k]) & (x < c[k])) | (x == b[k])
            status[k[narrow | spent]] = 0
            late = ~(narrow | spent) & (n_evals[k] >= MAX_ITER)
            go = ~(narrow | spent | late)
            is_open[k[~go]] = False
            k, x, right = k[go], x[go], right[go]
            if k.size == 0:
                break
            dx = self.rays(np.ascontiguousarray(group_f[k]), np.ascontiguousarray(group_p[k]), np.arange(k.size),
                           np.ascontiguousarray(x))                  # (only the open groups get tables)
            n_evals[k] += 1
            escaped = ~np.isfinite(dx)
            status[k[escaped]] = 2
            is_open[k[escaped]] = False
            with np.errstate(invalid="ignore"):
                better = ~escaped & (dx < db[k])
            worse = ~escaped & ~better
            kb, kr = k[better], right[better]
            a[kb] = np.where(kr, b[kb], a[kb])
            c[kb] = np.where(kr, c[kb], b[kb])
            b[kb], db[kb] = x[better], dx[better]
            kw, wr = k[worse], right[worse]
            c[kw] = np.where(wr, x[worse], c[kw])
            a[kw] = np.where(wr, a[kw], x[worse])
        return {"status": status, "scan_index": np.where(none, -1, i), "elevation_deg": np.where(none, np.nan, b),
                "skip_km": np.where(none, np.nan, db), "n_evals": n_evals}

    def muf(self, link_p, link_t):
        def s_of(f):
            r = self.skip(f, link_p)
            return np.where(r["status"] == -1, np.inf, r["skip_km"])
        n = link_t.size
        s_lo, s_hi = s_of(np.full(n, F_LO)), s_of(np.full(n, F_HI))
        with np.errstate(invalid="ignore"):
            status = np.where(np.isnan(link_t), -1, np.where(s_lo > link_t, 2, np.where(s_hi <= link_t, 1, 0)))
        lo, hi = np.full(n, F_LO), np.full(n, F_HI)
        for _ in range(N_BISECT):
            m = lo + 0.5 * (hi - lo)
            on = (status == 0) & (m > lo) & (m < hi)
            sm = s_of(np.where(on, m, F_LO))
            lo = np.where(on & (sm <= link_t), m, lo)
            hi = np.where(on & ~(sm <= link_t), m, hi)
        none = (status == -1) | (status == 2)
        return {"status": status, "muf_hz": np.where(none, np.nan, np.where(status == 1, F_HI, lo)),
                "f_above_hz": np.where(none | (status == 1), np.nan, hi)}


def same(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def timed(new, old, reps):
    new(), old()                                                                          # warm-up of every shape
    t_new, t_old, dev_ms = [], [], []
    ctx = _native.host_context(None)
    for _ in range(reps):
        t0 = time.perf_counter(); got = new(); t_new.append(time.perf_counter() - t0)
        dev_ms.append(ctx.last_kernel_ms())
        t0 = time.perf_counter(); want = old(); t_old.append(time.perf_counter() - t0)
    return got, want, {"call_s": float(np.median(t_new)), "call_s_all": [round(v, 6) for v in t_new],
                       "device_ms": float(np.median(dev_ms)), "host_route_s": float(np.median(t_old)),
                       "host_route_s_all": [round(v, 6) for v in t_old],
                       "host_route_over_call": float(np.median(t_old) / np.median(t_new))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    alt, den, bmag, bpsi = synth.chapman_profiles(P, 7)
    f = np.linspace(2e6, 14e6, F)
    scan = tracers.default_scan_elevations()
    lines = []
    for spherical, name in ((False, "cartesian"), (True, "spherical")):
        skip_fn = tracers.skip_distance_spherical_snells if spherical else tracers.skip_distance_cartesian_snells
        muf_fn = tracers.muf_spherical_snells if spherical else tracers.muf_cartesian_snells
        route = HostRoute(spherical, alt, den, bmag, bpsi, "O", scan)
        group_f, group_p = np.tile(f, P), np.repeat(np.arange(P, dtype=np.int64), F)
        link_p, link_t = np.repeat(np.arange(P, dtype=np.int64), TARGETS.size), np.tile(TARGETS, P)

        def new_skip():
            return skip_fn(f, alt, den, bmag, bpsi, "O", elev_tol_deg=TOL, max_iter=MAX_ITER)

        def new_muf():
            return muf_fn(TARGETS, F_LO, F_HI, alt, den, bmag, bpsi, "O", n_bisect=N_BISECT, elev_tol_deg=TOL, max_iter=MAX_ITER)
        if args.once:
            new_skip(), new_muf()
            continue
        route.calls = 0
        got, want, t = timed(new_skip, lambda: route.skip(group_f, group_p), args.reps)
        agree = {k: same(got[k].reshape(-1).astype(float), want[k].astype(float))
                 for k in ("status", "scan_index", "elevation_deg", "skip_km", "n_evals")}
        lines.append({"call": "skip", "geometry": name, "profiles": P, "frequencies": F, "scan_nodes": int(scan.size),
                      "groups": int(got["status"].size),
                      "status_counts": {str(s): int((got["status"] == s).sum()) for s in (-1, 0, 1, 2, 3)},
                      "rays_of_the_searches": int(got["n_evals"].sum()), "longest_search": int(got["n_evals"].max()),
                      "host_route_native_calls": route.calls // (args.reps + 1), "same_bits": agree, **t})
        print(json.dumps(lines[-1]), flush=True)
        assert all(agree.values()), agree
        route.calls = 0
        got, want, t = timed(new_muf, lambda: route.muf(link_p, link_t), args.reps)
        agree = {k: same(got[k].reshape(-1).astype(float), want[k].astype(float)) for k in ("status", "muf_hz", "f_above_hz")}
        lines.append({"call": "muf", "geometry": name, "profiles": P, "ranges": int(TARGETS.size), "scan_nodes": int(scan.size),
                      "links": int(got["status"].size), "n_bisect": N_BISECT, "f_lo_hz": F_LO, "f_hi_hz": F_HI,
                      "status_counts": {str(s): int((got["status"] == s).sum()) for s in (-1, 0, 1, 2)},
                      "host_route_native_calls": route.calls // (args.reps + 1), "same_bits": agree, **t})
        print(json.dumps(lines[-1]), flush=True)
        assert all(agree.values()), agree
    if args.out and lines:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
