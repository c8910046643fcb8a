"""Development-time generator of the gradient-homing fixture tests/golden/g21_gradient_homing.npz.

    python tools/gen_golden_gradient_homing.py [--jobs N]

Runs the reference's trace_ray_cartesian_gradient and trace_ray_spherical_gradient (imported through
oracle.gen_golden.load_reference_library; the spherical one with the four event helpers of tools/gen_golden_spherical.py)
on the CPU and writes arrays only.  The reference has no homing function: the bracket and refine rules of DESIGN.md
section 4.9 are the plain-Python restatement in tests/gradient_homing_rule.py, which drives the reference's tracer here.

Inputs: g18's tilted (0.3) two-layer ionosphere on the uniform 121 x 201 grid, 6 MHz O and 9 MHz X, both geometries
(case = 2 geometry + field), launch point (-400, 0), the bounded control set with max_step_km=2 (CONTROLS), the scan
np.linspace(5, 85, 33), range_tol_km=0.05, max_iter=64, the targets 300, 100, 700, 1500 (out of reach) and NaN.

Stored per case: the default-controls scan (D and status) and a check scan at rtol 1e-9 / atol 1e-11 / max_step_km=0.5;
per link the brackets; per bracket the refine rule's status, elevation and miss with the reference's tracer at the
default controls; per status-0 bracket e_truth (brentq inside the bracket at g18's truth controls), the truth run's
ground range, group path and delay there, their central-difference slopes over +-0.01 degrees, and the default-controls
run at e_truth, whose deviations from the truth run are the reference's own errors.

`check` holds the assertions on the inputs (tests/test_gradient_homing_host.py repeats them on the stored arrays).
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import load_reference_library  # noqa: E402
from pyrayhf_amd import synth  # noqa: E402
from tools.gen_golden_spherical import Stalled, load_patched_reference  # noqa: E402
import gradient_homing_rule as rule  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

SEED, NZ, NX, TILT = 18, 121, 201, 0.3
FIELDS = (("O", 6.0e6), ("X", 9.0e6))
X0_KM, Z0_KM = -400.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TARGETS = np.array([300.0, 100.0, 700.0, 1500.0, np.nan])
RANGE_TOL_KM, MAX_ITER = 0.05, 64
S_MAX_KM, Z_MAX_KM, X_LIM_KM = 4000.0, 600.0, 1000.0
RUNS = {"default": (1e-7, 1e-9, 2.0), "check": (1e-9, 1e-11, 0.5), "truth": (1e-10, 1e-12, 0.25)}
SLOPE_DEG = 0.01
NODE_GAP_KM, JUMP_FACTOR = 1.0, 100.0
STATUS = ("ground", "domain", "length", "failure")
N_CASES = 4

_worker = {}


def _trace(case, run, elev):
    """(D, P, T, status) of the reference's ray of `case` at `elev` under the controls of `run`."""
    geo, fi = divmod(case, 2)
    if geo not in _worker:
        _worker[geo] = (load_patched_reference() if geo else load_reference_library(), {})
    ref, fields = _worker[geo]
    if fi not in fields:
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(NZ, NX, TILT, SEED)
        mode, f = FIELDS[fi]
        mu, mup = ref.find_mu_mup(ref.find_X(den, f), ref.find_Y(f, bmag), bpsi, mode)
        if geo:
            fields[fi] = (ref.build_refractive_index_interpolator_spherical(z, x, mu),
                          ref.build_mup_function(mup, x, z, geometry="spherical"))
        else:
            fields[fi] = (ref.build_refractive_index_interpolator_cartesian(z, x, mu), ref.build_mup_function(mup, x, z))
    n_and_grad, mup_func = fields[fi]
    rtol, atol, step = RUNS[run]
    with np.errstate(all="ignore"):
        if geo:
            r_e = ref.constants()[2]
            try:
                r = ref.trace_ray_spherical_gradient(n_and_grad, mup_func, X0_KM, Z0_KM, float(elev), S_MAX_KM, rtol=rtol,
                                                     atol=atol, max_step_km=step, r_max_km=r_e + Z_MAX_KM,
                                                     phi_min=-X_LIM_KM / r_e, phi_max=X_LIM_KM / r_e)
            except Stalled:
                return np.nan, np.nan, np.nan, -1
        else:
            r = ref.trace_ray_cartesian_gradient(n_and_grad, mup_func, X0_KM, Z0_KM, float(elev), S_MAX_KM, rtol=rtol,
                                                 atol=atol, max_step_km=step, z_max_km=Z_MAX_KM, x_min_km=-X_LIM_KM,
                                                 x_max_km=X_LIM_KM)
    st = STATUS.index(r["status"])
    d = float(r["ground_range_km"]) if st == 0 else np.nan
    return d, float(r["group_path_km"]), float(r["group_delay_sec"]), st


def _scan_ray(task):
    case, run, i = task
    d, _, _, st = _trace(case, run, SCAN[i])
    return task, d, st


def _refine(task):
    case, ti, i, d = task
    r = rule.refine(lambda e: _trace(case, "default", e)[0], SCAN, d, i, TARGETS[ti], RANGE_TOL_KM, MAX_ITER)
    return task[:3], r


def _truth(task):
    from scipy.optimize import brentq
    case, ti, i = task
    t = TARGETS[ti]

    def miss(e):
        d = _trace(case, "truth", e)[0]
        if not np.isfinite(d):
            raise ValueError(f"case {case} target {t}: the truth ray at {e!r} does not land")
        return d - t
    e = brentq(miss, SCAN[i], SCAN[i + 1], xtol=1e-11, rtol=1e-15)
    at = np.array(_trace(case, "truth", e)[:3])
    up = np.array(_trace(case, "truth", e + SLOPE_DEG)[:3])
    dn = np.array(_trace(case, "truth", e - SLOPE_DEG)[:3])
    df = np.array(_trace(case, "default", e)[:3])
    return task, e, at, (up - dn) / (2 * SLOPE_DEG), df


def check(g):
    """The assertions on the inputs, from the arrays the fixture stores."""
    assert np.array_equal(g["scan_status"], g["check_status"]), "default and check scans differ in status"
    gap = np.abs(g["scan_ground_range_km"][:, None, :] - g["target_km"][None, :, None])
    assert np.nanmin(gap) >= NODE_GAP_KM, f"a scan node lands {np.nanmin(gap):.3e} km from a target"
    st, miss = g["bracket_status"], g["bracket_miss_km"]
    ok = ((st == 0) & (miss <= RANGE_TOL_KM)) | (st == 2) | ((st == 1) & (miss >= JUMP_FACTOR * RANGE_TOL_KM))
    assert ok.all(), list(zip(st[~ok].tolist(), miss[~ok].tolist()))
    assert g["n_brackets"].max() >= 3 and (st != 0).any()
    assert g["n_brackets"].sum() == st.size


def generate(jobs):
    import multiprocessing as mp
    out = {"scan_elevation_deg": SCAN, "target_km": TARGETS, "freq_hz": np.array([f for _, f in FIELDS]),
           "mode_is_x": np.array([m == "X" for m, _ in FIELDS]), "launch_km": np.array([X0_KM, Z0_KM]),
           "range_tol_km": np.float64(RANGE_TOL_KM), "max_iter": np.int64(MAX_ITER),
           "controls": np.array([S_MAX_KM, Z_MAX_KM, X_LIM_KM]), "slope_step_deg": np.float64(SLOPE_DEG)}
    with mp.Pool(jobs) as pool:
        scans = {run: (np.full((N_CASES, SCAN.size), np.nan), np.full((N_CASES, SCAN.size), -1, dtype=np.int64))
                 for run in ("default", "check")}
        tasks = [(c, run, i) for run in scans for c in range(N_CASES) for i in range(SCAN.size)]
        for (c, run, i), d, st in pool.imap_unordered(_scan_ray, tasks, chunksize=2):
            scans[run][0][c, i], scans[run][1][c, i] = d, st
        out["scan_ground_range_km"], out["scan_status"] = scans["default"]
        out["check_ground_range_km"], out["check_status"] = scans["check"]
        for c in range(N_CASES):
            print(f"case {c}: status {''.join(str(s) if s >= 0 else '-' for s in out['scan_status'][c])}")
            print("   D:", np.array2string(out["scan_ground_range_km"][c], precision=1, max_line_width=200))
            print("   check - default:", np.nanmax(np.abs(out["check_ground_range_km"][c] - out["scan_ground_range_km"][c])),
                  "status equal:", np.array_equal(out["scan_status"][c], out["check_status"][c]), flush=True)
        nb = np.zeros((N_CASES, TARGETS.size), dtype=np.int64)
        todo = []
        for c in range(N_CASES):
            for ti, t in enumerate(TARGETS):
                idx = rule.brackets(out["scan_ground_range_km"][c], float(t))
                nb[c, ti] = len(idx)
                todo += [(c, ti, i, out["scan_ground_range_km"][c]) for i in idx]
        out["n_brackets"] = nb
        print("n_brackets:\n", nb, flush=True)
        refined = dict(pool.imap_unordered(_refine, todo))
        keys = [t[:3] for t in todo]
        out["bracket_case"], out["bracket_target"], out["bracket_scan_index"] = (np.array(v, dtype=np.int64)
                                                                                   for v in zip(*keys))
        out["bracket_status"] = np.array([refined[k]["status"] for k in keys], dtype=np.int64)
        out["bracket_elevation_deg"] = np.array([refined[k]["elevation_deg"] for k in keys])
        out["bracket_miss_km"] = np.array([refined[k]["miss_km"] for k in keys])
        out["bracket_rays"] = np.array([len(refined[k]["tried"]) for k in keys], dtype=np.int64)
        for k in keys:
            print(k, {n: v for n, v in refined[k].items() if n != "tried"}, len(refined[k]["tried"]), flush=True)
        n = len(keys)
        for name in ("e_truth", "truth_ground_range_km", "truth_group_path_km", "truth_group_delay_sec", "dD_de", "dP_de",
                     "dT_de", "default_ground_range_km", "default_group_path_km", "default_group_delay_sec"):
            out[name] = np.full(n, np.nan)
        conv = [k for k in keys if refined[k]["status"] == 0]
        for k, e, at, slope, df in pool.imap_unordered(_truth, conv):
            b = keys.index(k)
            out["e_truth"][b] = e
            for j, s in enumerate(("ground_range_km", "group_path_km", "group_delay_sec")):
                out["truth_" + s][b], out["default_" + s][b] = at[j], df[j]
            out["dD_de"][b], out["dP_de"][b], out["dT_de"][b] = slope
            print(k, "e_truth", e, "truth", at, "slopes", slope, "default - truth", df - at, flush=True)
    path = os.path.join(GOLDEN, "g21_gradient_homing.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    check(out)          # (a file that fails here is not a fixture: move the target or the scan node, then run again)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    generate(ap.parse_args().jobs)


if __name__ == "__main__":
    main()
