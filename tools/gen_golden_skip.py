"""Development-time generator of the skip-distance / MUF fixture tests/golden/g22_skip.npz.

    python tools/gen_golden_skip.py [--jobs N]

The reference has neither function, so the fixture is made from its two Snell tracers alone (trace_ray_cartesian_snells
and trace_ray_spherical_snells, imported through oracle.gen_golden.load_reference_library, run on the CPU) with the rule
of DESIGN.md section 4.10 as restated in tests/skip_rule.py, on the `gauss` and `day` columns of fixture G8 - read from
G8, not copied.  Only arrays are written.

Skip cases: both geometries x CASES (O mode) on the default scan np.linspace(2, 88, 345) with the default controls
(elev_tol_deg 1e-6, max_iter 64).  Stored per (geometry, case): the scan's ground ranges, i*, status, the refined
elevation, skip_km, bracket_deg, n_evals and - for a node inside the scan - a dense fan of DENSE nodes across
[e_(i*-1), e_(i*+1)] with its number of slope sign changes.  UNIMODAL names the cases whose dense fan has exactly one:
the generator refuses to write one that has not.

MUF cases: the gauss column, t = 500 km, O mode, f in [9, 15] MHz, n_bisect = 24, flat and spherical.  Every S(f) of
the bisection is the rule on the reference's rays; its margin is the bound of the skip test against the reference,
2 L (w + w_ref) + 1e-9 S, with L the largest |dD/de| between neighbouring nodes of a dense fan of DENSE nodes across that
evaluation's scan bracket and w = w_ref = the evaluation's final bracket (at least elev_tol_deg); 1e-9 S for an
evaluation that ends at a scan node.  Stored: muf_ref, f_above_ref, the trips, muf_margin_km (the largest margin of any evaluation),
muf_window_hz and muf_min_gap_km, the smallest |S(m) - t| over the trips whose bracket was still wider than the window.
The window is the smallest of 100 Hz, 1 kHz, 10 kHz, 100 kHz at whose two ends muf_ref -+ window the reference's S
clears t by ten margins and for which muf_min_gap_km is at least ten margins too: below that the bisection path of
another implementation of the same tracers could part from this one before the bracket is as narrow as the window.
The generator refuses a MUF case for which no window of the four does.
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
import skip_rule  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

CASES = (("gauss", 9e6), ("gauss", 10e6), ("gauss", 12e6), ("gauss", 15e6), ("day", 10e6), ("day", 9e6), ("day", 12e6),
         ("gauss", 4e6), ("gauss", 40e6), ("day", 15e6), ("gauss", 400e6))
# (geometry, case) whose dense fan must be unimodal: gauss flat 9, 10; gauss spherical 9, 12, 15; day 10 both
UNIMODAL = ((0, 0), (0, 1), (1, 0), (1, 2), (1, 3), (0, 4), (1, 4))
SCAN = np.linspace(2.0, 88.0, 345)
DENSE = 801
ELEV_TOL, MAX_ITER = 1e-6, 64
MUF_COLUMN, MUF_T, MUF_LO, MUF_HI, MUF_BISECT = "gauss", 500.0, 9e6, 15e6, 24
WINDOWS = (100.0, 1e3, 1e4, 1e5)

_worker = {}


def _trace(task):
    """ground_range_km of one reference ray (geometry, column, f, elevation); NaN for a ray that does not turn"""
    geometry, name, f, elevation = task
    if "ref" not in _worker:
        _worker["ref"] = load_reference_library()
        _worker["g8"] = dict(np.load(os.path.join(GOLDEN, "g8_snell.npz")))
    ref, g8 = _worker["ref"], _worker["g8"]
    cols = [g8[f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]
    fn = ref.trace_ray_spherical_snells if geometry else ref.trace_ray_cartesian_snells
    with np.errstate(all="ignore"):
        r = fn(float(f), float(elevation), *cols, "O")
    return float(np.asarray(r["ground_range_km"], dtype=float))


def skip_of(pool, geometry, name, f):
    """The rule on the reference's rays: (result dict of skip_rule.skip_search, scan D, the rays the search traced)"""
    d = np.array(pool.map(_trace, [(geometry, name, f, e) for e in SCAN], chunksize=8))
    traced = []

    def ray(e):
        v = _trace((geometry, name, f, e))
        traced.append((e, v))
        return v
    return skip_rule.skip_search(SCAN, d, ray, ELEV_TOL, MAX_ITER), d, traced


def margin_of(pool, geometry, name, f, res):
    """The skip test's bound against the reference for this evaluation: L from its own dense fan (module docstring)."""
    s = res["skip_km"]
    if res["status"] in (1, -1):
        return 1e-9 * s if res["status"] == 1 else 0.0
    i = res["scan_index"]
    e = np.linspace(SCAN[i - 1], SCAN[i + 1], DENSE)
    dd = np.array(pool.map(_trace, [(geometry, name, f, x) for x in e], chunksize=8))
    ok = np.isfinite(dd)
    assert ok.all(), ("a ray of the dense fan does not turn", geometry, name, f)
    w = max(res["bracket_deg"], ELEV_TOL)
    return 2.0 * skip_rule.largest_slope(e, dd) * (2.0 * w) + 1e-9 * s


def generate(jobs):
    import multiprocessing as mp
    n_case = len(CASES)
    out = {"scan_elevation_deg": SCAN, "freq_hz": np.array([f for _, f in CASES]),
           "column_is_day": np.array([n == "day" for n, _ in CASES]),
           "scan_ground_range_km": np.full((2, n_case, SCAN.size), np.nan),
           "scan_index": np.full((2, n_case), -1, dtype=np.int64), "status": np.full((2, n_case), -9, dtype=np.int64),
           "elevation_deg": np.full((2, n_case), np.nan), "skip_km": np.full((2, n_case), np.nan),
           "bracket_deg": np.full((2, n_case), np.nan), "n_evals": np.zeros((2, n_case), dtype=np.int64),
           "dense_elevation_deg": np.full((2, n_case, DENSE), np.nan), "dense_ground_range_km": np.full((2, n_case, DENSE), np.nan),
           "dense_sign_changes": np.full((2, n_case), -1, dtype=np.int64), "unimodal_set": np.zeros((2, n_case), dtype=bool)}
    for g, c in UNIMODAL:
        out["unimodal_set"][g, c] = True
    with mp.Pool(jobs) as pool:
        for g in range(2):
            for c, (name, f) in enumerate(CASES):
                res, d, _ = skip_of(pool, g, name, f)
                out["scan_ground_range_km"][g, c] = d
                for k in ("scan_index", "status", "elevation_deg", "skip_km", "bracket_deg", "n_evals"):
                    out[k][g, c] = res[k]
                i = res["scan_index"]
                line = f"geometry {g} {name} {f / 1e6:g} MHz: i* {i}, status {res['status']}, skip {res['skip_km']:.6f} km"
                if res["status"] not in (1, -1):
                    e = np.linspace(SCAN[i - 1], SCAN[i + 1], DENSE)
                    dd = np.array(pool.map(_trace, [(g, name, f, x) for x in e], chunksize=8))
                    out["dense_elevation_deg"][g, c], out["dense_ground_range_km"][g, c] = e, dd
                    assert np.isfinite(dd).all(), ("a ray of the dense fan does not turn", g, c)
                    n = skip_rule.slope_sign_changes(dd)
                    out["dense_sign_changes"][g, c] = n
                    line += f", dense fan: {n} sign changes, min {dd.min():.6f} km, L {skip_rule.largest_slope(e, dd):.1f} km/deg"
                    if out["unimodal_set"][g, c]:
                        assert n == 1, ("a case of the unimodal set is not unimodal", g, c, n)
                else:
                    assert not out["unimodal_set"][g, c], (g, c)
                print(line, flush=True)
        muf = {k: np.full(2, np.nan) for k in ("muf_ref", "f_above_ref", "muf_window_hz", "muf_min_gap_km", "muf_margin_km")}
        muf["muf_trip_hz"] = np.full((2, MUF_BISECT), np.nan)
        muf["muf_trip_skip_km"] = np.full((2, MUF_BISECT), np.nan)
        for g in range(2):
            margins = []

            def s_of(f):
                res, d, traced = skip_of(pool, g, MUF_COLUMN, f)
                margins.append(margin_of(pool, g, MUF_COLUMN, f, res))
                return np.inf if res["status"] == -1 else res["skip_km"]
            r = skip_rule.muf_search(s_of, MUF_T, MUF_LO, MUF_HI, MUF_BISECT)
            assert r["status"] == 0 and len(r["trips"]) == MUF_BISECT, r
            muf["muf_ref"][g], muf["f_above_ref"][g] = r["muf_hz"], r["f_above_hz"]
            muf["muf_trip_hz"][g] = [t[0] for t in r["trips"]]
            muf["muf_trip_skip_km"][g] = [t[1] for t in r["trips"]]
            for w in WINDOWS:
                below, above = s_of(r["muf_hz"] - w), s_of(r["muf_hz"] + w)
                margin = max(margins)
                gaps = [abs(sm - MUF_T) for m, sm, lo, hi in r["trips"] if hi - lo > w]
                if below <= MUF_T - 10.0 * margin and above >= MUF_T + 10.0 * margin and min(gaps) >= 10.0 * margin:
                    muf["muf_window_hz"][g], muf["muf_margin_km"][g], muf["muf_min_gap_km"][g] = w, margin, min(gaps)
                    break
            assert np.isfinite(muf["muf_window_hz"][g]), ("no window clears the target by ten margins at its ends and on "
                                                          "the trips wider than it", g, max(margins))
            print(f"MUF geometry {g}: {r['muf_hz']:.3f} Hz, window {muf['muf_window_hz'][g]:g} Hz, margin "
                  f"{muf['muf_margin_km'][g]:.3e} km, smallest gap of the wide trips {muf['muf_min_gap_km'][g]:.3e} km", flush=True)
    out.update(muf)
    out.update(muf_target_km=np.array(MUF_T), muf_f_lo_hz=np.array(MUF_LO), muf_f_hi_hz=np.array(MUF_HI),
               muf_n_bisect=np.array(MUF_BISECT))
    path = os.path.join(GOLDEN, "g22_skip.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) <= 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    generate(args.jobs)


if __name__ == "__main__":
    main()
