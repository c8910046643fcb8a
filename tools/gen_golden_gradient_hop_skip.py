"""Development-time generator of the multi-hop skip-distance fixture tests/golden/g25_gradient_hop_skip.npz.

    python tools/gen_golden_gradient_hop_skip.py [--jobs N]

Runs the reference's trace_ray_cartesian_gradient (imported through oracle.gen_golden.load_reference_library) on the CPU
and writes arrays only.  The reference has no multi-hop call, no skip distance and no MUF: a chain is DESIGN.md section
4.12 driven from here, as in tools/gen_golden_gradient_hops.py - hop h + 1 launches at (ground_range_km of hop h, 0) with
np.degrees(np.arctan2(-vz, vx)) of hop h's last node, while hop h ends with status "ground" -, D(e) of section 4.13 is the
landing x of hop H - 1 (NaN unless all H hops land), and the rule is the plain-Python restatement in tests/skip_rule.py,
imported, which drives those chains.

Inputs: g24's ionosphere synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000) and launch point (-1800, 0),
s_max_km=4000, z_max_km=600, x within +-2000 km, 12 MHz O and 15 MHz X, H = 2 and H = 3 (case = 2 field + H - 2), the scan
np.linspace(5, 85, 33), elev_tol_deg=1e-3, max_iter=64.  The fields are built with array frequencies
(find_X(Ne, np.array([f]))), whose square is the product f f.  Three runs (RUNS): g23's default, check and truth.  A
chain of three hops holds the chain of two: one scan per field and run serves both hop counts.

Stored per case and run: the scan's D and the rule's result.  e_ref_km = the largest |skip_km(default) - skip_km(truth)|
over the cases; convergence = max |check - truth| / max |default - truth| on skip_km.

MUF: one link, O mode, H = 2, target MUF_TARGET_KM, [12, 15] MHz (an end is moved by 1 MHz while S_ref(f_lo) <= t <
S_ref(f_hi) does not hold), n_bisect = 10 with the reference at the default controls: every trip's (m, S_ref(m), lo, hi)
and muf_safe_trips, the number of leading trips with |S_ref(m) - t| >= 10 e_ref_km.

`check` holds the assertions on the inputs (tests/test_gradient_hop_skip_host.py repeats them on the stored arrays).
"""

from __future__ import annotations

import argparse
import os
import sys
import threading

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import load_reference_library  # noqa: E402
from pyrayhf_amd import synth  # noqa: E402
import skip_rule as rule  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

SEED, NZ, NX, TILT, X_HALF_KM = 24, 121, 401, 0.3, 2000.0
FIELDS = (("O", 12.0e6), ("X", 15.0e6))
HOPS = (2, 3)
X0_KM, Z0_KM, Z_GROUND_KM = -1800.0, 0.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
ELEV_TOL_DEG, MAX_ITER = 1e-3, 64
S_MAX_KM, Z_MAX_KM, X_LIM_KM = 4000.0, 600.0, 2000.0
RUNS = {"default": (1e-7, 1e-9, 2.0), "check": (1e-9, 1e-11, 0.5), "truth": (1e-10, 1e-12, 0.25)}
STATUS = ("ground", "domain", "length", "failure")
N_CASES = len(FIELDS) * len(HOPS)
MUF_TARGET_KM, MUF_MODE, MUF_HOPS, MUF_F_LO, MUF_F_HI, MUF_N_BISECT, MUF_MOVE_HZ = 0.0, "O", 2, 12.0e6, 15.0e6, 10, 1.0e6
SAFE_FACTOR, SAFE_TRIPS_MIN, MAX_CONVERGENCE = 10.0, 4, 0.1

_worker = {}


def _chain(mode, f, run, elev, n_hops):
    """Landing x per hop (n_hops,) of the chain of reference rays through the `mode` field at `f` Hz launched at `elev`
    under the controls of `run`; NaN from the first hop that does not land."""
    if "ref" not in _worker:
        _worker["ref"] = (load_reference_library(), {})
    ref, fields = _worker["ref"]
    if (mode, f) not in fields:
        if len(fields) > 4:
            fields.clear()
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(NZ, NX, TILT, SEED, x_half_km=X_HALF_KM)
        fa = np.array([f])
        mu, mup = ref.find_mu_mup(ref.find_X(den, fa), ref.find_Y(fa, bmag), bpsi, mode)
        fields[(mode, f)] = (ref.build_refractive_index_interpolator_cartesian(z, x, mu), ref.build_mup_function(mup, x, z))
    n_and_grad, mup_func = fields[(mode, f)]
    rtol, atol, step = RUNS[run]
    land = np.full(n_hops, np.nan)
    x0, z0, e = X0_KM, Z0_KM, float(elev)
    for h in range(n_hops):
        with np.errstate(all="ignore"):
            r = ref.trace_ray_cartesian_gradient(n_and_grad, mup_func, x0, z0, e, S_MAX_KM, rtol=rtol, atol=atol,
                                                 max_step_km=step, z_ground_km=Z_GROUND_KM, z_max_km=Z_MAX_KM,
                                                 x_min_km=-X_LIM_KM, x_max_km=X_LIM_KM)
        if STATUS.index(r["status"]) != 0:
            break
        land[h] = x0 = float(r["ground_range_km"])
        z0 = Z_GROUND_KM
        e = float(np.degrees(np.arctan2(-r["vz"][-1], r["vx"][-1])))
    return land


def _d(mode, f, run, elev, n_hops):
    return float(_chain(mode, f, run, elev, n_hops)[n_hops - 1])


def _scan_chain(task):
    mode, f, run, i, n_hops = task
    return task, _chain(mode, f, run, SCAN[i], n_hops)


def _search(task):
    mode, f, run, n_hops, d = task
    r = rule.skip_search(SCAN, d, lambda e: _d(mode, f, run, e, n_hops), ELEV_TOL_DEG, MAX_ITER)
    return task[:4], r


def convergence(g):
    return float(np.abs(g["check_skip_km"] - g["truth_skip_km"]).max() / np.abs(g["default_skip_km"] - g["truth_skip_km"]).max())


def safe_trips(g):
    t, n, safe = float(g["muf_target_km"]), int(g["muf_n_trips"]), 0
    while safe < n and abs(g["muf_trip_s_km"][safe] - t) >= SAFE_FACTOR * float(g["e_ref_km"]):
        safe += 1
    return safe


def check(g):
    """The assertions on the inputs, from the arrays the fixture stores."""
    for c in range(N_CASES):
        d = g["scan_ground_range_km"][c]
        i, edge = rule.scan_node(d)
        assert i == g["default_scan_index"][c] and not edge, f"case {c}: no interior minimum"
        assert 0 < i < d.size - 1 and np.isfinite(d[i - 1]) and np.isfinite(d[i + 1])
        assert g["default_status"][c] == 0
        assert g["default_bracket_deg"][c] <= ELEV_TOL_DEG
        assert SCAN[i - 1] < g["default_elevation_deg"][c] < SCAN[i + 1]
    e_ref = np.abs(g["default_skip_km"] - g["truth_skip_km"]).max()
    assert e_ref == g["e_ref_km"], e_ref
    assert convergence(g) <= MAX_CONVERGENCE, convergence(g)
    t = float(g["muf_target_km"])
    assert g["muf_s_lo_km"] <= t < g["muf_s_hi_km"]
    assert int(g["muf_n_trips"]) == MUF_N_BISECT
    assert safe_trips(g) == g["muf_safe_trips"] and g["muf_safe_trips"] >= SAFE_TRIPS_MIN, safe_trips(g)


def generate(jobs):
    import multiprocessing as mp
    out = {"scan_elevation_deg": SCAN, "freq_hz": np.array([f for _, f in FIELDS]),
           "mode_is_x": np.array([m == "X" for m, _ in FIELDS]), "n_hops": np.array(HOPS, dtype=np.int64),
           "launch_km": np.array([X0_KM, Z0_KM]), "elev_tol_deg": np.float64(ELEV_TOL_DEG), "max_iter": np.int64(MAX_ITER),
           "controls": np.array([S_MAX_KM, Z_MAX_KM, X_LIM_KM]), "muf_target_km": np.float64(MUF_TARGET_KM),
           "muf_n_bisect": np.int64(MUF_N_BISECT), "muf_hops": np.int64(MUF_HOPS)}
    with mp.Pool(jobs) as pool:
        lock = threading.Lock()

        def scan_of(mode, f, run, n_hops):
            """(E, n_hops) landing x per hop of the scan's chains."""
            land = np.full((SCAN.size, n_hops), np.nan)
            tasks = [(mode, f, run, i, n_hops) for i in range(SCAN.size)]
            for (_, _, _, i, _), row in pool.imap_unordered(_scan_chain, tasks):
                land[i] = row
            return land

        # ---- skip distance: per field and run one scan of max(HOPS) hops, then a search per hop count ------------------
        results = {}

        def one(fi, run):
            mode, f = FIELDS[fi]
            land = scan_of(mode, f, run, max(HOPS))
            for hi, n_hops in enumerate(HOPS):
                d = land[:, n_hops - 1].copy()
                r = pool.apply(_search, ((mode, f, run, n_hops, d),))[1]
                with lock:
                    results[(2 * fi + hi, run)] = (d, r)
                    print(f"field {fi} H {n_hops} {run}:", {k: v for k, v in r.items() if k != "triple"}, "\n D:",
                          np.array2string(d, precision=1, max_line_width=200), flush=True)

        # ---- MUF: one link, beside the skip searches ------------------------------------------------------------------
        muf = {}

        def link():
            def s(f):
                d = scan_of(MUF_MODE, float(f), "default", MUF_HOPS)[:, MUF_HOPS - 1].copy()
                r = pool.apply(_search, ((MUF_MODE, float(f), "default", MUF_HOPS, d),))[1]
                v = rule.INF if r["status"] == -1 else r["skip_km"]
                with lock:
                    print(f"S({f!r}) = {v!r} (status {r['status']}, node {r['scan_index']}, {r['n_evals']} chains)", flush=True)
                return v
            f_lo, f_hi = MUF_F_LO, MUF_F_HI
            s_lo, s_hi = s(f_lo), s(f_hi)
            while s_lo > MUF_TARGET_KM:
                f_lo -= MUF_MOVE_HZ
                s_lo = s(f_lo)
            while s_hi <= MUF_TARGET_KM:
                f_hi += MUF_MOVE_HZ
                s_hi = s(f_hi)
            known = {f_lo: s_lo, f_hi: s_hi}
            r = rule.muf_search(lambda f: known[f] if f in known else s(f), MUF_TARGET_KM, f_lo, f_hi, MUF_N_BISECT)
            with lock:
                muf[0] = (f_lo, f_hi, s_lo, s_hi, r)

        threads = [threading.Thread(target=link)]
        threads += [threading.Thread(target=one, args=(fi, run)) for run in ("truth", "check", "default")
                    for fi in range(len(FIELDS))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert len(results) == N_CASES * len(RUNS) and len(muf) == 1, "a worker thread failed"
    for run in RUNS:
        pre = "scan" if run == "default" else run + "_scan"
        out[pre + "_ground_range_km"] = np.array([results[(c, run)][0] for c in range(N_CASES)])
        for k, dt in (("status", np.int64), ("scan_index", np.int64), ("elevation_deg", np.float64),
                      ("skip_km", np.float64), ("bracket_deg", np.float64), ("n_evals", np.int64)):
            out[f"{run}_{k}"] = np.array([results[(c, run)][1][k] for c in range(N_CASES)], dtype=dt)
    out["e_ref_km"] = np.float64(np.abs(out["default_skip_km"] - out["truth_skip_km"]).max())
    print("skip_km default / check / truth:\n", out["default_skip_km"], "\n", out["check_skip_km"], "\n",
          out["truth_skip_km"], "\nE_ref", out["e_ref_km"], "convergence", convergence(out), flush=True)
    f_lo, f_hi, s_lo, s_hi, r = muf[0]
    out["muf_f_lo_hz"], out["muf_f_hi_hz"] = np.float64(f_lo), np.float64(f_hi)
    out["muf_s_lo_km"], out["muf_s_hi_km"] = np.float64(s_lo), np.float64(s_hi)
    out["muf_status"] = np.int64(r["status"])
    out["muf_hz"], out["muf_f_above_hz"] = np.float64(r["muf_hz"]), np.float64(r["f_above_hz"])
    out["muf_n_trips"] = np.int64(len(r["trips"]))
    for j, name in enumerate(("muf_trip_m_hz", "muf_trip_s_km", "muf_trip_lo_hz", "muf_trip_hi_hz")):
        a = np.full(MUF_N_BISECT, np.nan)
        for k, trip in enumerate(r["trips"]):
            a[k] = trip[j]
        out[name] = a
    out["muf_safe_trips"] = np.int64(safe_trips(out))
    print("muf:", out["muf_hz"], out["muf_f_above_hz"], "safe trips", out["muf_safe_trips"], "\n S(m) - t:\n",
          out["muf_trip_s_km"] - MUF_TARGET_KM)
    path = os.path.join(GOLDEN, "g25_gradient_hop_skip.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    check(out)          # (a file that fails here is not a fixture: move the frequency or the target, then run again)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    generate(ap.parse_args().jobs)


if __name__ == "__main__":
    main()
