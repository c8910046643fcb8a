"""Development-time generator of the spherical gradient-tracer fixture tests/golden/g19_spherical_rays.npz.

    python tools/gen_golden_spherical.py [--jobs N]

Runs the reference's trace_ray_spherical_gradient (imported through oracle.gen_golden.load_reference_library) on the
CPU and writes arrays only.  The reference wires the Cartesian event helpers to the spherical state [r, phi, v_r, v_phi]
(its library.py:2239-2243 with :1009-1031), so that no stop condition can fire; the four helpers are replaced ON THE
IMPORTED MODULE by the ones DESIGN.md section 4.7 defines (EVENTS below: the component indices are the only change) and
everything else - rhs_spherical, solve_ivp, the path, delay, midpoint and apex formulas - is the reference's own code.

Inputs as for g18 (tools/gen_golden_gradient.py): the tilted (0.3) two-layer ionosphere and its zero-tilt twin on a
uniform 121 x 201 grid, 6 MHz O and 9 MHz X, 16 elevations from 5 to 85 degrees from (0, 0), two control sets (a bounded
domain with max_step_km=5; the reference's defaults), three reference runs per ray (see RUNS).  For the zero-tilt twin
every run also stores the drift of the Bouguer invariant mu r v_phi over the path nodes, mu from the reference's own
interpolator.  The generator asserts that the three runs' statuses agree for >= 90 % of the rays, that the truth run
has converged - per control set and key, max|check - truth| <= 0.1 max|default - truth| - and that at least 8 rays of
every control set end on the ground.

A run the reference does not finish.  r = R_E + z resolves 9.1e-13 km, which is more than the smallest step solve_ivp
takes (10 ulp of s: 2.8e-13 km at s = 236 km).  A ray that runs into the underside of the mu = NaN cap at a grid line
(9 MHz X, tilt 0.3, 74.3 degrees: r = 6591 km) comes to rest one ulp below the line: every step that would move r is
rejected on the NaN beyond it, every smaller one is accepted and leaves r where it was, and s advances by 1e-12 km per
step towards s_max_km.  STALL_CALLS right-hand-side calls over which s advances by less than STALL_KM abandon such a
run; its status is stored as -1 (NO_RESULT), its scalars as NaN, and `agree` is false for the ray.
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.gen_golden import load_reference_library  # noqa: E402
from pyrayhf_amd import synth  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")

SEED, NZ, NX = 18, 121, 201
TILTS = (0.3, 0.0)
CASES = (("O", 6.0e6), ("X", 9.0e6))
ELEVATIONS = np.linspace(5.0, 85.0, 16)
RUNS = (("default", 1e-7, 1e-9, None), ("truth", 1e-10, 1e-12, 0.25), ("check", 1e-9, 1e-11, 0.5))
SCALARS = ("group_path_km", "group_delay_sec", "ground_range_km", "x_apex_km", "z_apex_km", "x_midpoint", "z_midpoint")
CONVERGED = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km")
STATUS = ("ground", "domain", "length", "failure")
NO_RESULT = -1
STALL_CALLS, STALL_KM = 20000, 1e-6


class Stalled(Exception):
    pass

# The terminal events on y = [r, phi, v_r, v_phi], direction + -> - (the keyword names are the reference's: it binds
# them with functools.partial)
EVENTS = {
    "event_ground": lambda s, y, z_ground_km: y[0] - z_ground_km - 1e-3,
    "event_z_top": lambda s, y, z_max_km: z_max_km - y[0],
    "event_x_left": lambda s, y, x_min_km: y[1] - x_min_km,
    "event_x_right": lambda s, y, x_max_km: x_max_km - y[1],
}


def control_sets(r_e):
    """The bounded set and the reference's defaults (library.py:2135-2145)."""
    return (dict(s_max_km=4000.0, max_step_km=5.0, r_max_km=r_e + 600.0, phi_min=-1000.0 / r_e, phi_max=1000.0 / r_e),
            dict(max_step_km=2.0))


def load_patched_reference():
    ref = load_reference_library()
    for name, fn in EVENTS.items():
        setattr(ref, name, fn)
    rhs = ref.rhs_spherical
    watch = {"n": 0, "s": 0.0}

    def watched_rhs(s, y, n_and_grad_rphi, renormalize_every, eval_counter):
        """rhs_spherical itself; counts the calls since the ray began (eval_counter is the reference's, new per ray)"""
        if eval_counter["n"] == 0:
            watch["n"], watch["s"] = 0, 0.0
        watch["n"] += 1
        if watch["n"] % STALL_CALLS == 0:
            if s - watch["s"] < STALL_KM:
                raise Stalled()
            watch["s"] = s
        return rhs(s, y, n_and_grad_rphi, renormalize_every, eval_counter)

    ref.rhs_spherical = watched_rhs
    return ref


_worker = {}


def _ray(task):
    ti, ci, si, ei, ri = task
    if "ref" not in _worker:
        _worker["ref"] = load_patched_reference()
        _worker["fields"] = {}
    ref = _worker["ref"]
    r_e = ref.constants()[2]
    if (ti, ci) not in _worker["fields"]:
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(NZ, NX, TILTS[ti], SEED)
        mode, f = CASES[ci]
        mu, mup = ref.find_mu_mup(ref.find_X(den, f), ref.find_Y(f, bmag), bpsi, mode)
        _worker["fields"][(ti, ci)] = (ref.build_refractive_index_interpolator_spherical(z, x, mu),
                                       ref.build_mup_function(mup, x, z, geometry="spherical"))
    n_and_grad, mup_func = _worker["fields"][(ti, ci)]
    _, rtol, atol, step = RUNS[ri]
    kw = dict(control_sets(r_e)[si])
    if step is not None:
        kw["max_step_km"] = step
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        try:
            r = ref.trace_ray_spherical_gradient(n_and_grad, mup_func, 0.0, 0.0, float(ELEVATIONS[ei]), rtol=rtol,
                                                 atol=atol, **kw)
        except Stalled:
            return task, [np.nan] * len(SCALARS), NO_RESULT, time.perf_counter() - t0, 0, np.nan
        dt = time.perf_counter() - t0
        drift = np.nan
        if TILTS[ti] == 0.0:
            mu = np.asarray(n_and_grad(r["phi"], r["r"])[0], dtype=float)
            inv = mu * r["r"] * r["v_phi"]
            d = np.abs(inv / inv[0] - 1.0)
            if np.isfinite(d).any():
                drift = float(np.nanmax(d))
    return task, [float(r[k]) for k in SCALARS], STATUS.index(r["status"]), dt, len(r["t"]), drift


def check(agree, status, vals):
    """The generator's assertions on the stored arrays (tests/test_gpu_spherical_gradient.py repeats them)."""
    assert agree.mean() >= 0.9, f"the three runs' statuses agree for {agree.mean():.3f} of the rays only"
    for si in range(agree.shape[2]):
        m = agree[:, :, si]
        n_ground = int((status[0][:, :, si][m] == 0).sum())
        print(f"  set {si}: {n_ground} rays end on the ground")
        assert n_ground >= 8, (si, n_ground)
        for key in CONVERGED:
            ki = SCALARS.index(key)
            d = np.abs(vals[0][:, :, si, :, ki] - vals[1][:, :, si, :, ki])[m]
            c = np.abs(vals[2][:, :, si, :, ki] - vals[1][:, :, si, :, ki])[m]
            ok = np.isfinite(d) & np.isfinite(c)
            assert ok.sum() >= 8, (key, si, int(ok.sum()))
            print(f"  set {si} {key}: max|default - truth| = {d[ok].max():.3e}, max|check - truth| = {c[ok].max():.3e}, "
                  f"ratio {c[ok].max() / d[ok].max():.3f}")
            assert c[ok].max() <= 0.1 * d[ok].max(), (key, si)


def generate(jobs):
    import multiprocessing as mp
    shape = (len(TILTS), len(CASES), 2, len(ELEVATIONS))
    tasks = [(ti, ci, si, ei, ri) for ri in (1, 2, 0) for ti in range(shape[0]) for ci in range(shape[1])
             for si in range(shape[2]) for ei in range(shape[3])]
    vals = np.full((len(RUNS),) + shape + (len(SCALARS),), np.nan)
    status = np.full((len(RUNS),) + shape, -1, dtype=np.int64)
    secs = np.zeros((len(RUNS),) + shape)
    nodes = np.zeros((len(RUNS),) + shape, dtype=np.int64)
    drift = np.full((len(RUNS),) + shape, np.nan)
    with mp.Pool(jobs) as pool:
        for k, (task, v, st, dt, n, dr) in enumerate(pool.imap_unordered(_ray, tasks, chunksize=2)):
            ti, ci, si, ei, ri = task
            at = (ri, ti, ci, si, ei)
            vals[at], status[at], secs[at], nodes[at], drift[at] = v, st, dt, n, dr
            if k % 32 == 0:
                print(f"  {k}/{len(tasks)} rays", flush=True)
    agree = (status[0] == status[1]) & (status[0] == status[2]) & (status[0] != NO_RESULT)
    print("statuses (default run):", {STATUS[s]: int((status[0] == s).sum()) for s in range(4)},
          "runs without a result:", [int((status[ri] == NO_RESULT).sum()) for ri in range(len(RUNS))], "agree:", agree.mean())
    check(agree, status, vals)
    flat = TILTS.index(0.0)
    out = {"elevation_deg": ELEVATIONS, "tilts": np.array(TILTS), "freq_hz": np.array([f for _, f in CASES]),
           "mode_is_x": np.array([m == "X" for m, _ in CASES]), "agree": agree, "seconds_per_ray": secs, "n_nodes": nodes}
    for ri, (name, *_rest) in enumerate(RUNS):
        out[name + "_status"] = status[ri]
        out[name + "_bouguer_drift"] = np.ascontiguousarray(drift[ri][flat])          # (case, set, elevation)
        for ki, key in enumerate(SCALARS):
            out[f"{name}_{key}"] = np.ascontiguousarray(vals[ri][..., ki])
    path = os.path.join(GOLDEN, "g19_spherical_rays.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; reference seconds per ray (default run): "
          f"median {np.median(secs[0]):.3f}, max {secs[0].max():.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    generate(args.jobs)


if __name__ == "__main__":
    main()
