"""Development-time generator of the gradient skip-distance fixture tests/golden/g23_gradient_skip.npz.

    python tools/gen_golden_gradient_skip.py [--jobs N]

Runs the reference's trace_ray_cartesian_gradient and trace_ray_spherical_gradient (imported through
oracle.gen_golden.load_reference_library; the spherical one with the four event helpers of tools/gen_golden_spherical.py)
on the CPU and writes arrays only.  The reference has neither a skip distance nor a MUF: the rule of DESIGN.md sections
4.10 / 4.11 is the plain-Python restatement in tests/skip_rule.py, which drives the reference's tracers here.

Inputs: g18's tilted (0.3) two-layer ionosphere on the uniform 121 x 201 grid, 12 MHz O and 15 MHz X - both above the
layer's critical frequency, so that D(e) has an interior minimum - both geometries (case = 2 geometry + field), g21's
launch point (-400, 0) and bounded control set (CONTROLS), the scan np.linspace(5, 85, 33), elev_tol_deg=1e-3,
max_iter=64.  The fields are built with array frequencies (find_X(Ne, np.array([f]))), whose square is the product f f.

Stored per case and run (default; check: rtol 1e-9 / atol 1e-11 / max_step_km=0.5; truth: 1e-10 / 1e-12 / 0.25): the scan
(D and status) and the rule's result.  e_ref_km = the largest |skip_km(default) - skip_km(check or truth)| over the cases.

MUF: one link per geometry, target 300 km, O mode, [12, 15] MHz (an end is moved by 1 MHz while S_ref(f_lo) <= t <
S_ref(f_hi) does not hold), n_bisect = 10 with the reference at the default controls: every trip's (m, S_ref(m), lo, hi)
and muf_safe_trips, the number of leading trips with |S_ref(m) - t| >= 10 e_ref_km.

`check` holds the assertions on the inputs (tests/test_gradient_skip_host.py repeats them on the stored arrays).
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
from tools.gen_golden_spherical import Stalled, load_patched_reference  # noqa: E402
import skip_rule as rule  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

SEED, NZ, NX, TILT = 18, 121, 201, 0.3
FIELDS = (("O", 12.0e6), ("X", 15.0e6))
X0_KM, Z0_KM = -400.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
ELEV_TOL_DEG, MAX_ITER = 1e-3, 64
S_MAX_KM, Z_MAX_KM, X_LIM_KM = 4000.0, 600.0, 1000.0
RUNS = {"default": (1e-7, 1e-9, 2.0), "check": (1e-9, 1e-11, 0.5), "truth": (1e-10, 1e-12, 0.25)}
STATUS = ("ground", "domain", "length", "failure")
N_CASES = 4
MUF_TARGET_KM, MUF_MODE, MUF_F_LO, MUF_F_HI, MUF_N_BISECT, MUF_MOVE_HZ = 300.0, "O", 12.0e6, 15.0e6, 10, 1.0e6
SAFE_FACTOR, SAFE_TRIPS_MIN = 10.0, 4

_worker = {}


def _trace(geo, mode, f, run, elev):
    """(D, status) of the reference's ray through the `mode` field at `f` Hz at `elev` under the controls of `run`."""
    if geo not in _worker:
        _worker[geo] = (load_patched_reference() if geo else load_reference_library(), {})
    ref, fields = _worker[geo]
    if (mode, f) not in fields:
        if len(fields) > 4:
            fields.clear()
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(NZ, NX, TILT, SEED)
        fa = np.array([f])
        mu, mup = ref.find_mu_mup(ref.find_X(den, fa), ref.find_Y(fa, bmag), bpsi, mode)
        if geo:
            fields[(mode, f)] = (ref.build_refractive_index_interpolator_spherical(z, x, mu),
                                 ref.build_mup_function(mup, x, z, geometry="spherical"))
        else:
            fields[(mode, f)] = (ref.build_refractive_index_interpolator_cartesian(z, x, mu),
                                 ref.build_mup_function(mup, x, z))
    n_and_grad, mup_func = fields[(mode, f)]
    rtol, atol, step = RUNS[run]
    with np.errstate(all="ignore"):
        if geo:
            r_e = ref.constants()[2]
            try:
                r = ref.trace_ray_spherical_gradient(n_and_grad, mup_func, X0_KM, Z0_KM, float(elev), S_MAX_KM, rtol=rtol,
                                                     atol=atol, max_step_km=step, r_max_km=r_e + Z_MAX_KM,
                                                     phi_min=-X_LIM_KM / r_e, phi_max=X_LIM_KM / r_e)
            except Stalled:
                return np.nan, -1
        else:
            r = ref.trace_ray_cartesian_gradient(n_and_grad, mup_func, X0_KM, Z0_KM, float(elev), S_MAX_KM, rtol=rtol,
                                                 atol=atol, max_step_km=step, z_max_km=Z_MAX_KM, x_min_km=-X_LIM_KM,
                                                 x_max_km=X_LIM_KM)
    st = STATUS.index(r["status"])
    return (float(r["ground_range_km"]) if st == 0 else np.nan), st


def _scan_ray(task):
    geo, mode, f, run, i = task
    d, st = _trace(geo, mode, f, run, SCAN[i])
    return task, d, st


def _search(task):
    geo, mode, f, run, d = task
    r = rule.skip_search(SCAN, d, lambda e: _trace(geo, mode, f, run, e)[0], ELEV_TOL_DEG, MAX_ITER)
    return task[:4], r


def check(g):
    """The assertions on the inputs, from the arrays the fixture stores."""
    for c in range(N_CASES):
        d = g["scan_ground_range_km"][c]
        i, edge = rule.scan_node(d)
        assert i == g["default_scan_index"][c] and not edge, f"case {c}: no interior minimum"
        assert 0 < i < d.size - 1 and np.isfinite(d[i - 1]) and np.isfinite(d[i + 1])
        assert g["default_status"][c] == 0
    e_ref = max(np.abs(g["default_skip_km"] - g["check_skip_km"]).max(), np.abs(g["default_skip_km"] - g["truth_skip_km"]).max())
    assert e_ref == g["e_ref_km"] and e_ref < 0.05, e_ref
    t = float(g["muf_target_km"])
    for geo in range(2):
        assert g["muf_s_lo_km"][geo] <= t < g["muf_s_hi_km"][geo]
        n = int(g["muf_n_trips"][geo])
        assert n == MUF_N_BISECT
        safe = 0
        while safe < n and abs(g["muf_trip_s_km"][geo, safe] - t) >= SAFE_FACTOR * e_ref:
            safe += 1
        assert safe == g["muf_safe_trips"][geo] and safe >= SAFE_TRIPS_MIN, (geo, safe)


def generate(jobs):
    import multiprocessing as mp
    out = {"scan_elevation_deg": SCAN, "freq_hz": np.array([f for _, f in FIELDS]),
           "mode_is_x": np.array([m == "X" for m, _ in FIELDS]), "launch_km": np.array([X0_KM, Z0_KM]),
           "elev_tol_deg": np.float64(ELEV_TOL_DEG), "max_iter": np.int64(MAX_ITER),
           "controls": np.array([S_MAX_KM, Z_MAX_KM, X_LIM_KM]), "muf_target_km": np.float64(MUF_TARGET_KM),
           "muf_n_bisect": np.int64(MUF_N_BISECT)}
    with mp.Pool(jobs) as pool:
        lock = threading.Lock()

        def skip_of(geo, mode, f, run):
            """(scan D, scan status, the rule's result) of one (geometry, field, controls)."""
            d, st = np.full(SCAN.size, np.nan), np.full(SCAN.size, -1, dtype=np.int64)
            for (_, _, _, _, i), di, si in pool.imap_unordered(_scan_ray, [(geo, mode, f, run, i) for i in range(SCAN.size)]):
                d[i], st[i] = di, si
            return d, st, pool.apply(_search, ((geo, mode, f, run, d),))[1]

        # ---- skip distance: 4 cases x 3 runs, every one a thread of this process that feeds the pool ----------------
        results = {}

        def one(c, run):
            geo, fi = divmod(c, 2)
            r = skip_of(geo, FIELDS[fi][0], FIELDS[fi][1], run)
            with lock:
                results[(c, run)] = r
                print(f"case {c} {run}: status {''.join(str(s) if s >= 0 else '-' for s in r[1])}",
                      {k: v for k, v in r[2].items() if k != "triple"}, flush=True)
        threads = [threading.Thread(target=one, args=(c, run)) for c in range(N_CASES) for run in RUNS]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert len(results) == N_CASES * len(RUNS), "a worker thread failed"
        for run in RUNS:
            pre = "scan" if run == "default" else run + "_scan"
            out[pre + "_ground_range_km"] = np.array([results[(c, run)][0] for c in range(N_CASES)])
            out[pre + "_status"] = np.array([results[(c, run)][1] for c in range(N_CASES)])
            for k, dt in (("status", np.int64), ("scan_index", np.int64), ("elevation_deg", np.float64),
                          ("skip_km", np.float64), ("bracket_deg", np.float64), ("n_evals", np.int64)):
                out[f"{run}_{k}"] = np.array([results[(c, run)][2][k] for c in range(N_CASES)], dtype=dt)
        e_ref = max(np.abs(out["default_skip_km"] - out["check_skip_km"]).max(),
                    np.abs(out["default_skip_km"] - out["truth_skip_km"]).max())
        out["e_ref_km"] = np.float64(e_ref)
        print("skip_km default / check / truth:\n", out["default_skip_km"], "\n", out["check_skip_km"], "\n",
              out["truth_skip_km"], "\nE_ref", e_ref, flush=True)

        # ---- MUF: one link per geometry, the two searches side by side ------------------------------------------------
        muf = {}

        def link(geo):
            def s(f):
                r = skip_of(geo, MUF_MODE, float(f), "default")[2]
                v = rule.INF if r["status"] == -1 else r["skip_km"]
                with lock:
                    print(f"geometry {geo}: S({f!r}) = {v!r} (status {r['status']}, {r['n_evals']} rays)", flush=True)
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
                muf[geo] = (f_lo, f_hi, s_lo, s_hi, r)
        threads = [threading.Thread(target=link, args=(geo,)) for geo in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert len(muf) == 2, "a worker thread failed"
    out["muf_f_lo_hz"] = np.array([muf[g][0] for g in range(2)])
    out["muf_f_hi_hz"] = np.array([muf[g][1] for g in range(2)])
    out["muf_s_lo_km"] = np.array([muf[g][2] for g in range(2)])
    out["muf_s_hi_km"] = np.array([muf[g][3] for g in range(2)])
    out["muf_status"] = np.array([muf[g][4]["status"] for g in range(2)], dtype=np.int64)
    out["muf_hz"] = np.array([muf[g][4]["muf_hz"] for g in range(2)])
    out["muf_f_above_hz"] = np.array([muf[g][4]["f_above_hz"] for g in range(2)])
    out["muf_n_trips"] = np.array([len(muf[g][4]["trips"]) for g in range(2)], dtype=np.int64)
    for j, name in enumerate(("muf_trip_m_hz", "muf_trip_s_km", "muf_trip_lo_hz", "muf_trip_hi_hz")):
        a = np.full((2, MUF_N_BISECT), np.nan)
        for g in range(2):
            for k, trip in enumerate(muf[g][4]["trips"]):
                a[g, k] = trip[j]
        out[name] = a
    safe = np.zeros(2, dtype=np.int64)
    for g in range(2):
        while safe[g] < out["muf_n_trips"][g] and abs(out["muf_trip_s_km"][g, safe[g]] - MUF_TARGET_KM) >= SAFE_FACTOR * e_ref:
            safe[g] += 1
    out["muf_safe_trips"] = safe
    print("muf:", out["muf_hz"], out["muf_f_above_hz"], "safe trips", safe, "\n S(m) - t:\n", out["muf_trip_s_km"] - MUF_TARGET_KM)
    path = os.path.join(GOLDEN, "g23_gradient_skip.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    check(out)          # (a file that fails here is not a fixture: move the target or the bracket, then run again)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    generate(ap.parse_args().jobs)


if __name__ == "__main__":
    main()
