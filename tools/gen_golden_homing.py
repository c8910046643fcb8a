"""Development-time generator of the homing fixture tests/golden/g20_homing.npz.

    python tools/gen_golden_homing.py [--jobs N]

The reference has no homing function, so the fixture is made from its tracers alone: trace_ray_cartesian_snells and
trace_ray_spherical_snells (imported through oracle.gen_golden.load_reference_library, run on the CPU) on the `day`
and `gauss` columns of fixture G8 - read from G8, not copied - and only arrays are written.

Links: both geometries x CASES (day 6 MHz O, day 12 MHz X, gauss 4 MHz O, gauss 5 MHz X) x TARGETS (300, 800, 1500 km)
on the default scan grid np.linspace(2, 88, 345).  Per link the brackets of DESIGN.md section 4.8 are taken from the
reference's own scan - interval i is a bracket when D_i and D_i+1 are finite and (D_i - t), (D_i+1 - t) have opposite
signs or D_i == t; D at the last node == t is a bracket of no width - and every bracket is bisected with the reference's
tracer until it is WIDTH_DEG wide.  Stored per bracket, in (geometry, case, target, elevation) order: the link,
scan_index, the root elevation (the end of the last bracket that lands nearer the target), its miss |D - t|, ground
range, group path and group delay, the class (converged: miss <= 1e-7 km; jump: miss >= 1 km) and - for converged roots
- the local slopes dD/de [km/deg], dP'/dD and dtau/dD [s/km] from two reference rays at root +- SLOPE_DEG.  Stored per
link: n_brackets; per (geometry, case): the reference's ground range at every scan node.

The generator asserts (tests/test_homing_host.py repeats it on the stored arrays): every bracket has a miss of at most
1e-7 km or of at least 1 km; some link has at least 3 brackets, some link has a jump, some link has none; every scan
node of every link has |D_i - t| >= 1e-6 km, so that bracket membership cannot hinge on the last bits; no bisection
meets a ray that does not turn.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.gen_golden import load_reference_library  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

CASES = (("day", 6.0e6, "O"), ("day", 12.0e6, "X"), ("gauss", 4.0e6, "O"), ("gauss", 5.0e6, "X"))
TARGETS = np.array([300.0, 800.0, 1500.0])
SCAN = np.linspace(2.0, 88.0, 345)
WIDTH_DEG, SLOPE_DEG = 1e-12, 1e-6
CONVERGED_KM, JUMP_KM, NODE_KM = 1e-7, 1.0, 1e-6
MAX_BISECTIONS = 200

_worker = {}


def _trace(geometry, case, elevation):
    """(ground_range_km, group_path_km, group_delay_sec) of one reference ray; NaN for a ray that does not turn"""
    if "ref" not in _worker:
        _worker["ref"] = load_reference_library()
        _worker["g8"] = dict(np.load(os.path.join(GOLDEN, "g8_snell.npz")))
    ref, g8 = _worker["ref"], _worker["g8"]
    name, f, mode = CASES[case]
    cols = [g8[f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]
    fn = ref.trace_ray_spherical_snells if geometry else ref.trace_ray_cartesian_snells
    with np.errstate(all="ignore"):
        r = fn(f, float(elevation), *cols, mode)
    return tuple(float(np.asarray(r[k], dtype=float)) for k in ("ground_range_km", "group_path_km", "group_delay_sec"))


def _scan_ray(task):
    geometry, case, i = task
    return task, _trace(geometry, case, SCAN[i])[0]


def brackets_of(d, t):
    """Scan indices of the brackets of target t on the scan's ground ranges d, ascending."""
    f = d - t
    ok = np.isfinite(d[:-1]) & np.isfinite(d[1:])
    with np.errstate(invalid="ignore"):
        is_b = ok & (((f[:-1] < 0) & (f[1:] > 0)) | ((f[:-1] > 0) & (f[1:] < 0)) | (d[:-1] == t))
    idx = list(np.nonzero(is_b)[0])
    if d[-1] == t:
        idx.append(d.size - 1)
    return np.array(idx, dtype=np.int64)


def _refine(task):
    geometry, case, ti, i, d_lo, d_hi = task
    t = TARGETS[ti]
    lo, hi, f_lo, f_hi = SCAN[i], SCAN[min(i + 1, SCAN.size - 1)], d_lo - t, d_hi - t
    for _ in range(MAX_BISECTIONS):
        if hi - lo <= WIDTH_DEG or f_lo == 0.0:
            break
        mid = lo + 0.5 * (hi - lo)
        if not lo < mid < hi:
            break
        f = _trace(geometry, case, mid)[0] - t
        assert np.isfinite(f), ("a ray inside a bracket does not turn", task, mid)
        if (f < 0) == (f_lo < 0) and f != 0.0:
            lo, f_lo = mid, f
        else:
            hi, f_hi = mid, f
    root = lo if abs(f_lo) <= abs(f_hi) else hi
    d, path, delay = _trace(geometry, case, root)
    miss = abs(d - t)
    slopes = (np.nan, np.nan, np.nan)
    if miss <= CONVERGED_KM:
        dm, pm, tm = _trace(geometry, case, root - SLOPE_DEG)
        dp, pp, tp = _trace(geometry, case, root + SLOPE_DEG)
        slopes = ((dp - dm) / (2.0 * SLOPE_DEG), (pp - pm) / (dp - dm), (tp - tm) / (dp - dm))
    return task, (root, miss, d, path, delay) + slopes


def check(out):
    """The generator's assertions on the stored arrays."""
    miss, conv = out["miss_km"], out["converged"]
    assert np.all((miss <= CONVERGED_KM) | (miss >= JUMP_KM)), miss[(miss > CONVERGED_KM) & (miss < JUMP_KM)]
    assert np.array_equal(conv, miss <= CONVERGED_KM)
    nb = out["n_brackets"]
    assert nb.max() >= 3 and nb.min() == 0 and (~conv).any(), (nb.max(), nb.min(), int((~conv).sum()))
    assert nb.sum() == miss.size
    d = out["scan_ground_range_km"]                                 # (geometry, case, scan node)
    gap = np.abs(d[:, :, None, :] - out["target_km"][None, None, :, None])
    assert np.nanmin(gap) >= NODE_KM, np.nanmin(gap)
    assert np.all(np.isfinite(out["dD_de"][conv]) & (out["dD_de"][conv] != 0.0))
    assert np.all(np.isfinite(out["dP_dD"][conv]) & np.isfinite(out["dtau_dD"][conv]))


def generate(jobs):
    import multiprocessing as mp
    n_geo, n_case, n_t = 2, len(CASES), TARGETS.size
    scan_d = np.full((n_geo, n_case, SCAN.size), np.nan)
    with mp.Pool(jobs) as pool:
        tasks = [(g, c, i) for g in range(n_geo) for c in range(n_case) for i in range(SCAN.size)]
        for (g, c, i), d in pool.imap_unordered(_scan_ray, tasks, chunksize=8):
            scan_d[g, c, i] = d
        print(f"scan: {len(tasks)} reference rays, {int(np.isfinite(scan_d).sum())} of them land", flush=True)
        n_br = np.zeros((n_geo, n_case, n_t), dtype=np.int64)
        tasks = []
        for g in range(n_geo):
            for c in range(n_case):
                for ti in range(n_t):
                    idx = brackets_of(scan_d[g, c], TARGETS[ti])
                    n_br[g, c, ti] = idx.size
                    tasks += [(g, c, ti, int(i), scan_d[g, c, i], scan_d[g, c, min(i + 1, SCAN.size - 1)]) for i in idx]
        rows = dict(pool.imap_unordered(_refine, tasks, chunksize=1))
    cols = np.array([rows[t] for t in tasks]).reshape(len(tasks), 8)
    out = {"scan_elevation_deg": SCAN, "target_km": TARGETS, "freq_hz": np.array([f for _, f, _ in CASES]),
           "mode_is_x": np.array([m == "X" for _, _, m in CASES]), "column_is_day": np.array([n == "day" for n, _, _ in CASES]),
           "scan_ground_range_km": scan_d, "n_brackets": n_br,
           "geometry": np.array([t[0] for t in tasks], dtype=np.int64), "case": np.array([t[1] for t in tasks], dtype=np.int64),
           "target": np.array([t[2] for t in tasks], dtype=np.int64), "scan_index": np.array([t[3] for t in tasks], dtype=np.int64),
           "root_elevation_deg": cols[:, 0], "miss_km": cols[:, 1], "ground_range_km": cols[:, 2], "group_path_km": cols[:, 3],
           "group_delay_sec": cols[:, 4], "converged": cols[:, 1] <= CONVERGED_KM, "dD_de": cols[:, 5], "dP_dD": cols[:, 6],
           "dtau_dD": cols[:, 7]}
    print("brackets per link (geometry, case, target):", n_br.tolist())
    print(f"{len(tasks)} brackets: {int(out['converged'].sum())} converged (largest miss "
          f"{out['miss_km'][out['converged']].max():.3e} km), {int((~out['converged']).sum())} jumps (smallest miss "
          f"{out['miss_km'][~out['converged']].min():.1f} km)")
    check(out)
    path = os.path.join(GOLDEN, "g20_homing.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    generate(args.jobs)


if __name__ == "__main__":
    main()
