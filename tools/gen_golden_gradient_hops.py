"""Development-time generator of the multi-hop fixture tests/golden/g24_gradient_hops.npz.

    python tools/gen_golden_gradient_hops.py [--jobs N]

Runs the reference's trace_ray_cartesian_gradient (imported through oracle.gen_golden.load_reference_library) on the CPU
and writes arrays only.  The reference has no multi-hop call: a chain is DESIGN.md section 4.12 driven from here - hop
h + 1 launches at (ground_range_km of hop h, 0) with np.degrees(np.arctan2(-vz, vx)) of hop h's last node, while hop h
ends with status "ground".  The homing part follows tools/gen_golden_gradient_homing.py: the reference's chain driven
through tests/gradient_homing_rule.py, and truth roots from the truth run.

Inputs: synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000), 6 MHz O and 9 MHz X, launch point (-1800, 0), the
elevations np.linspace(10, 70, 13), 3 hops, s_max_km=4000, z_max_km=600, x within +-2000 km.  Three runs per chain
(RUNS): default, truth, check.  max_step_km=1 in the default run is deliberate: the cap then fixes the step sequence,
and a launch elevation perturbed by 1e-9 degrees reproduces the reference's error against truth on every hop; with 2
and more the reference's own error is no longer reproducible within a factor of 2.

Stored per run (R = default / truth / check), shape (2 fields, 13 elevations, 3 hops): R_status (-1: unused hop),
R_launch_x_km, R_launch_elevation_deg, R_group_path_km, R_group_delay_sec, R_ground_range_km, R_z_apex_km,
R_next_elevation_deg (the reflected elevation at the landing of that hop; NaN unless it landed) and R_z_apex_node_km.

The apex.  The reference's z_apex_km is the highest NODE of a ray (R_z_apex_node_km, all three runs).  A node lies up to
half a step from the ray's highest point, so that number is below it by up to curvature x step^2 / 8: 2.7 m at the
default run's 1 km cap, 0.65 m at 0.5 km, and still 0.16 m at 0.25 km.  Between the three caps this alone fixes
max |check - truth| / max |default - truth| near (0.5^2 - 0.25^2) / (1^2 - 0.25^2) = 0.2 (0.242 on these rays): the
truth run's node is no converged value of the apex.  The value the node maximum converges to is the highest point of
the ray itself, so truth_z_apex_km and check_z_apex_km are that point of their own runs: the maximum of the cubic
Hermite interpolant through the two nodes (s, z, dz/ds = vz) between which vz changes sign next to the highest node
(`apex`; error of fourth order in the step, the node itself where vz does not change sign).  default_z_apex_km stays
the reference's own number, the one a tracer at these controls returns and the GPU tests compare.

Homing part (field O, 2 hops, the elevations as scan grid, D(e) = landing x of hop 1): per target the brackets of the
default run's scan; per bracket the refine rule's status, elevation and miss on the reference's chain; per status-0
bracket e_truth (brentq inside the bracket on the truth run's chain), the truth chain's total range, path and delay
there, their central-difference slopes over +-0.01 degrees and the default run's chain at e_truth.

`check` holds the assertions on the inputs (tests/test_gradient_hops_host.py repeats them on the stored arrays).
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
import gradient_homing_rule as rule  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

SEED, NZ, NX, TILT, X_HALF_KM = 24, 121, 401, 0.3, 2000.0
FIELDS = (("O", 6.0e6), ("X", 9.0e6))
X0_KM, Z0_KM, Z_GROUND_KM = -1800.0, 0.0, 0.0
ELEVATIONS = np.linspace(10.0, 70.0, 13)
N_HOPS = 3
S_MAX_KM, Z_MAX_KM, X_LIM_KM = 4000.0, 600.0, 2000.0
RUNS = {"default": (1e-7, 1e-9, 1.0), "truth": (1e-10, 1e-12, 0.25), "check": (1e-9, 1e-11, 0.5)}
KEYS = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km", "next_elevation_deg")
STATUS = ("ground", "domain", "length", "failure")
MIN_STATUS_AGREEMENT, MAX_CONVERGENCE = 0.9, 0.1

HOME_FIELD, HOME_HOPS = 0, 2
TARGETS = np.array([-500.0, 0.0, -1100.0, 1900.0, np.nan])
RANGE_TOL_KM, MAX_ITER = 0.05, 64
SLOPE_DEG = 0.01

_worker = {}


def apex(t, z, vz):
    """The highest point of a ray from its nodes: the maximum of the cubic Hermite interpolant of z(s), dz/ds = vz, on
    the interval next to the highest node on which vz goes from > 0 to <= 0; the highest node where there is none."""
    t, z, vz = (np.asarray(v, dtype=np.float64) for v in (t, z, vz))
    k = int(np.nanargmax(z))
    best = float(z[k])
    for i in (k - 1, k):
        if i < 0 or i + 1 >= z.size or not (vz[i] > 0.0 >= vz[i + 1]):
            continue
        h = t[i + 1] - t[i]
        m0, m1, dz = h * vz[i], h * vz[i + 1], z[i + 1] - z[i]
        # p(u) = z_i + m0 u + (3 dz - 2 m0 - m1) u^2 + (m0 + m1 - 2 dz) u^3 on [0, 1]; p'(u) = 0
        b, c = 3.0 * dz - 2.0 * m0 - m1, m0 + m1 - 2.0 * dz
        roots = np.roots([3.0 * c, 2.0 * b, m0]) if c != 0.0 else np.array([-m0 / (2.0 * b)])
        for u in roots:
            if abs(u.imag) == 0.0 and 0.0 <= u.real <= 1.0:
                u = float(u.real)
                best = max(best, float(z[i] + m0 * u + b * u * u + c * u ** 3))
    return best


def _chain(fi, run, elev, n_hops):
    """The chain of `n_hops` reference rays of field `fi` from the launch point at `elev` under the controls of `run`:
    rows (n_hops, 9) of status, launch x, launch elevation, KEYS and the reference's own z_apex_km; unused hops have
    status -1 and NaN."""
    if "ref" not in _worker:
        _worker["ref"] = load_reference_library()
    ref = _worker["ref"]
    if fi not in _worker:
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(NZ, NX, TILT, SEED, x_half_km=X_HALF_KM)
        mode, f = FIELDS[fi]
        mu, mup = ref.find_mu_mup(ref.find_X(den, f), ref.find_Y(f, bmag), bpsi, mode)
        _worker[fi] = (ref.build_refractive_index_interpolator_cartesian(z, x, mu), ref.build_mup_function(mup, x, z))
    n_and_grad, mup_func = _worker[fi]
    rtol, atol, step = RUNS[run]
    rows = np.full((n_hops, 9), np.nan)
    rows[:, 0] = -1
    x0, z0, e = X0_KM, Z0_KM, float(elev)
    for h in range(n_hops):
        with np.errstate(all="ignore"):
            r = ref.trace_ray_cartesian_gradient(n_and_grad, mup_func, x0, z0, e, S_MAX_KM, rtol=rtol, atol=atol,
                                                 max_step_km=step, z_ground_km=Z_GROUND_KM, z_max_km=Z_MAX_KM,
                                                 x_min_km=-X_LIM_KM, x_max_km=X_LIM_KM)
        st = STATUS.index(r["status"])
        rows[h, :3] = st, x0, e
        rows[h, 3:7] = [float(r[k]) for k in KEYS[:4]]
        rows[h, 8] = float(r["z_apex_km"])
        if run != "default":
            rows[h, 6] = apex(r["t"], r["z"], r["vz"])
        if st != 0:
            break
        x0, z0 = float(r["ground_range_km"]), Z_GROUND_KM
        e = float(np.degrees(np.arctan2(-r["vz"][-1], r["vx"][-1])))
        rows[h, 7] = e
    return rows


def totals(rows):
    """(D, P, T) of a chain: landing x of the last hop (NaN unless every hop landed), path and delay summed in hop order."""
    landed = np.all(rows[:, 0] == 0)
    used = rows[:, 0] >= 0
    return (rows[-1, 5] if landed else np.nan, float(np.sum(rows[used, 3])), float(np.sum(rows[used, 4])))


def _chain_task(task):
    fi, run, i = task
    return task, _chain(fi, run, ELEVATIONS[i], N_HOPS)


def _home_d(run, e):
    return totals(_chain(HOME_FIELD, run, e, HOME_HOPS))


def _refine(task):
    ti, i, d = task
    r = rule.refine(lambda e: _home_d("default", e)[0], ELEVATIONS, d, i, TARGETS[ti], RANGE_TOL_KM, MAX_ITER)
    return task[:2], r


def _truth(task):
    from scipy.optimize import brentq
    ti, i = task
    t = TARGETS[ti]

    def miss(e):
        d = _home_d("truth", e)[0]
        if not np.isfinite(d):
            raise ValueError(f"target {t}: the truth chain at {e!r} does not land")
        return d - t
    e = brentq(miss, ELEVATIONS[i], ELEVATIONS[i + 1], xtol=1e-11, rtol=1e-15)
    at = np.array(_home_d("truth", e))
    up = np.array(_home_d("truth", e + SLOPE_DEG))
    dn = np.array(_home_d("truth", e - SLOPE_DEG))
    df = np.array(_home_d("default", e))
    return task, e, at, (up - dn) / (2 * SLOPE_DEG), df


def agreement(g):
    """Hop rows on which the three runs agree in status, and their share of all rows."""
    same = (g["default_status"] == g["truth_status"]) & (g["default_status"] == g["check_status"])
    return same, float(same.mean())


def convergence(g):
    """Per key: max |check - truth| / max |default - truth| over the landed hop rows on which the runs agree."""
    same, _ = agreement(g)
    ok = same & (g["truth_status"] == 0)
    return {k: float(np.abs(g["check_" + k][ok] - g["truth_" + k][ok]).max() /
                     np.abs(g["default_" + k][ok] - g["truth_" + k][ok]).max()) for k in KEYS}


def check(g):
    """The assertions on the inputs, from the arrays the fixture stores."""
    _, share = agreement(g)
    assert share >= MIN_STATUS_AGREEMENT, f"the runs agree in status on {share:.3f} of the hop rows"
    conv = convergence(g)
    assert max(conv.values()) <= MAX_CONVERGENCE, conv
    st = g["default_status"]
    assert (st[..., 0] != 0).any() and ((st[..., 0] == 0) & (st[..., 1] > 0)).any(), "no chain ends early"
    assert np.all(st[..., 1:][st[..., :-1] != 0] == -1)
    assert g["n_brackets"].max() >= 3 and g["n_brackets"].sum() == g["bracket_status"].size


def generate(jobs):
    import multiprocessing as mp
    out = {"elevation_deg": ELEVATIONS, "n_hops": np.int64(N_HOPS), "freq_hz": np.array([f for _, f in FIELDS]),
           "mode_is_x": np.array([m == "X" for m, _ in FIELDS]), "launch_km": np.array([X0_KM, Z0_KM]),
           "controls": np.array([S_MAX_KM, Z_MAX_KM, X_LIM_KM]), "target_km": TARGETS, "home_hops": np.int64(HOME_HOPS),
           "range_tol_km": np.float64(RANGE_TOL_KM), "max_iter": np.int64(MAX_ITER), "slope_step_deg": np.float64(SLOPE_DEG)}
    shape = (len(FIELDS), ELEVATIONS.size, N_HOPS)
    names = ("status", "launch_x_km", "launch_elevation_deg") + KEYS + ("z_apex_node_km",)
    with mp.Pool(jobs) as pool:
        rows = {run: np.full(shape + (9,), np.nan) for run in RUNS}
        tasks = [(fi, run, i) for run in ("truth", "check", "default") for fi in range(len(FIELDS))
                 for i in range(ELEVATIONS.size)]
        for (fi, run, i), r in pool.imap_unordered(_chain_task, tasks):
            rows[run][fi, i] = r
        for run in RUNS:
            for j, k in enumerate(names):
                v = rows[run][..., j]
                out[f"{run}_{k}"] = v.astype(np.int64) if k == "status" else v.copy()
        for fi in range(len(FIELDS)):
            for run in RUNS:
                print(f"field {fi} {run}:", " ".join("".join(str(s) if s >= 0 else "-" for s in c)
                                                     for c in out[run + "_status"][fi]), flush=True)
        print("status agreement:", agreement(out)[1], "convergence:", convergence(out), flush=True)
        # homing on hop 1 of field HOME_FIELD: the scan is the chains above
        def scan_of(run):
            st = out[run + "_status"][HOME_FIELD, :, :HOME_HOPS]
            return np.where(np.all(st == 0, axis=1), out[run + "_ground_range_km"][HOME_FIELD, :, HOME_HOPS - 1], np.nan)
        d = scan_of("default")
        out["scan_ground_range_km"], out["check_scan_ground_range_km"] = d, scan_of("check")
        print("D:", np.array2string(d, precision=1, max_line_width=200), flush=True)
        todo = []
        nb = np.zeros(TARGETS.size, dtype=np.int64)
        for ti, t in enumerate(TARGETS):
            idx = rule.brackets(d, float(t))
            nb[ti] = len(idx)
            todo += [(ti, i, d) for i in idx]
        out["n_brackets"] = nb
        print("n_brackets:", nb, flush=True)
        refined = dict(pool.imap_unordered(_refine, todo))
        keys = [t[:2] for t in todo]
        out["bracket_target"], out["bracket_scan_index"] = (np.array(v, dtype=np.int64) for v in zip(*keys))
        out["bracket_status"] = np.array([refined[k]["status"] for k in keys], dtype=np.int64)
        out["bracket_elevation_deg"] = np.array([refined[k]["elevation_deg"] for k in keys])
        out["bracket_miss_km"] = np.array([refined[k]["miss_km"] for k in keys])
        out["bracket_rays"] = np.array([len(refined[k]["tried"]) for k in keys], dtype=np.int64)
        for k in keys:
            print(k, {n: v for n, v in refined[k].items() if n != "tried"}, len(refined[k]["tried"]), flush=True)
        n = len(keys)
        for name in ("e_truth", "truth_total_ground_range_km", "truth_total_group_path_km", "truth_total_group_delay_sec",
                     "dD_de", "dP_de", "dT_de", "default_total_ground_range_km", "default_total_group_path_km",
                     "default_total_group_delay_sec"):
            out[name] = np.full(n, np.nan)
        conv = [k for k in keys if refined[k]["status"] == 0]
        for k, e, at, slope, df in pool.imap_unordered(_truth, conv):
            b = keys.index(k)
            out["e_truth"][b] = e
            for j, s in enumerate(("ground_range_km", "group_path_km", "group_delay_sec")):
                out["truth_total_" + s][b], out["default_total_" + s][b] = at[j], df[j]
            out["dD_de"][b], out["dP_de"][b], out["dT_de"][b] = slope
            print(k, "e_truth", e, "truth", at, "slopes", slope, "default - truth", df - at, flush=True)
    path = os.path.join(GOLDEN, "g24_gradient_hops.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    check(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    generate(ap.parse_args().jobs)


if __name__ == "__main__":
    main()
