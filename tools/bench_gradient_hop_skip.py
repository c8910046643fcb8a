#!/usr/bin/env python3
"""Multi-hop skip distance (prhf_gradient_hop_skip_f64) and MUF (prhf_gradient_hop_muf_f64) of the gradient tracers
against the best route through the calls that existed before them, on the same build: 64 fields x 1 transmitter with
H = 2 and H = 3 (skip) and 64 links with H = 2 and n_bisect = 12 (MUF) through G24's tilted ionosphere on 121 x 401 nodes
from (-1800, 0), the scan np.linspace(5, 85, 33), both geometries - section 4.11's shape.

    python tools/bench_gradient_hop_skip.py [--reps N] [--out profiles/bench_gradient_hop_skip.jsonl] [--once]

The host route of the skip distance: (1) one trace_hop_fan_* call on the scan grid, (2) the node rule in NumPy (argmin
over the finite D_i, the edge class), (3) the golden-section rule of DESIGN.md section 4.10 vectorised over all open
groups, ONE batched trace_hops_*_gradient call per step with one chain per open group.  The host route of the MUF: the
bisection in NumPy over all links at once; per trip the fields of the links' frequencies come from
refractive_field_device and that skip route is S(f).  Both routes are timed end to end on NumPy arrays (host clock
around synchronous calls, the median of --reps interleaved repetitions after a warm-up); the new calls' device time is
the context's event pair around their kernels.  The two routes must agree bit for bit (recorded, and asserted).  One
JSON line per call, hop count and geometry, with the lane utilisation of the refinement and the hop rays per ray slot;
--once makes one call of each per geometry and nothing else (for a kernel trace).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import _native, gradient, synth  # noqa: E402

N = 64
SKIP_FREQS = np.linspace(11.0e6, 16.0e6, N)
F_LO, F_HI, N_BISECT = 12.0e6, 15.0e6, 12
X0, Z0 = -1800.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TOL, MAX_ITER = 1e-3, 64
GOLD = 0.3819660112501051
R_E = gradient.constants()[2]
CTL = (dict(s_max_km=4000.0, max_step_km=2.0, z_max_km=600.0, x_min_km=-2000.0, x_max_km=2000.0),
       dict(s_max_km=4000.0, max_step_km=2.0, r_max_km=R_E + 600.0, phi_min=-2000.0 / R_E, phi_max=2000.0 / R_E))
SKIP = (gradient.skip_distance_hops_cartesian_gradient, gradient.skip_distance_hops_spherical_gradient)
MUF = (gradient.muf_hops_cartesian_gradient, gradient.muf_hops_spherical_gradient)
FAN = (gradient.trace_hop_fan_cartesian_gradient, gradient.trace_hop_fan_spherical_gradient)
HOPS = (gradient.trace_hops_cartesian_gradient, gradient.trace_hops_spherical_gradient)
SKIP_HOPS, MUF_HOPS = (2, 3), 2


class HostRoute:
    """The rule of section 4.10 on the multi-hop tracers' public calls."""

    def __init__(self, geo, iono):
        self.geo, self.iono = geo, iono
        self.calls = 0

    def skip(self, field, n_hops):
        """-> status, scan_index, elevation_deg, skip_km, n_evals per field of `field` (transmitter (X0, Z0))"""
        n, geo = field.n_fields, self.geo
        d = FAN[geo](field, SCAN, n_hops, X0, Z0, **CTL[geo])["total_ground_range_km"]
        self.calls += 1
        ok = np.isfinite(d)
        i = np.argmin(np.where(ok, d, np.inf), axis=1)
        none = ~ok.any(axis=1)
        lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, SCAN.size - 1)
        rows = np.arange(n)
        edge = (i == 0) | (i == SCAN.size - 1) | ~ok[rows, lo] | ~ok[rows, hi]
        status = np.where(none, -1, np.where(edge, 1, 3))
        a, b, c, db = SCAN[lo].copy(), SCAN[i].copy(), SCAN[hi].copy(), d[rows, i].copy()
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
            dx = HOPS[geo](field, X0, Z0, x, n_hops, k, **CTL[geo])["total_ground_range_km"]     # one chain per open group
            self.calls += 1
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

    def field(self, freqs):
        """The fields of `freqs`, built on the device."""
        z, x, den, bmag, bpsi = self.iono
        self.calls += 1
        return gradient.refractive_field_device(freqs, den, bmag, bpsi, z, x, "O", geometry="spherical" if self.geo else "cartesian")

    def muf(self, link_t):
        def s_of(f):
            r = self.skip(self.field(f), MUF_HOPS)
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
    t_new, t_old, dev_ms, counters = [], [], [], None
    ctx = _native.host_context(None)
    for _ in range(reps):
        t0 = time.perf_counter(); got = new(); t_new.append(time.perf_counter() - t0)
        dev_ms.append(ctx.last_kernel_ms())
        counters = ctx.gradient_hop_skip_counters()
        t0 = time.perf_counter(); want = old(); t_old.append(time.perf_counter() - t0)
    groups, rays, slots, waves, hop_rays = counters
    return got, want, {"call_s": float(np.median(t_new)), "call_s_all": [round(v, 6) for v in t_new],
                       "device_ms": float(np.median(dev_ms)), "host_route_s": float(np.median(t_old)),
                       "host_route_s_all": [round(v, 6) for v in t_old],
                       "host_route_over_call": float(np.median(t_old) / np.median(t_new)),
                       "groups_refined": groups, "refine_rays": rays, "refine_ray_slots": slots, "refine_waves": waves,
                       "refine_hop_rays": hop_rays, "lane_utilisation": float(rays / slots) if slots else None,
                       "hop_rays_per_slot": float(hop_rays / slots) if slots else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    iono = synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000)
    z, x, den, bmag, bpsi = iono
    lines = []
    for geo, name in ((0, "cartesian"), (1, "spherical")):
        route = HostRoute(geo, iono)
        field = gradient.refractive_field_device(SKIP_FREQS, den, bmag, bpsi, z, x, "O", geometry=name)

        def new_skip(n_hops):
            return SKIP[geo](field, n_hops, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
        s_lo = float(SKIP[geo](gradient.refractive_field_device([F_LO], den, bmag, bpsi, z, x, "O", geometry=name), MUF_HOPS,
                               X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])["skip_km"][0, 0])
        targets = np.linspace(s_lo + 5.0, s_lo + 215.0, N)

        def new_muf():
            return MUF[geo](targets, MUF_HOPS, den, bmag, bpsi, z, x, "O", F_LO, F_HI, X0, Z0, n_bisect=N_BISECT,
                            scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
        if args.once:
            new_skip(SKIP_HOPS[0]), new_muf()
            continue
        for n_hops in SKIP_HOPS:
            route.calls = 0
            got, want, t = timed(lambda: new_skip(n_hops), lambda: route.skip(field, n_hops), args.reps)
            agree = {k: same(got[k].reshape(-1).astype(float), want[k].astype(float))
                     for k in ("status", "scan_index", "elevation_deg", "skip_km", "n_evals")}
            lines.append({"call": "hop_skip", "geometry": name, "n_hops": n_hops, "fields": N, "transmitters": 1,
                          "scan_nodes": int(SCAN.size),
                          "status_counts": {str(s): int((got["status"] == s).sum()) for s in (-1, 0, 1, 2, 3)},
                          "chains_of_the_searches": int(got["n_evals"].sum()), "longest_search": int(got["n_evals"].max()),
                          "host_route_native_calls": route.calls // (args.reps + 1), "same_bits": agree, **t})
            print(json.dumps(lines[-1]), flush=True)
            assert all(agree.values()), agree
        route.calls = 0
        got, want, t = timed(new_muf, lambda: route.muf(targets), args.reps)
        agree = {k: same(got[k].reshape(-1).astype(float), want[k].astype(float)) for k in ("status", "muf_hz", "f_above_hz")}
        lines.append({"call": "hop_muf", "geometry": name, "n_hops": MUF_HOPS, "links": N, "scan_nodes": int(SCAN.size),
                      "n_bisect": N_BISECT, "f_lo_hz": F_LO, "f_hi_hz": F_HI,
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
