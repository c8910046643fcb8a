"""Development-time generator of the gradient-tracer fixtures tests/golden/g17_fields.npz and g18_gradient_rays.npz.

    python tools/gen_golden_gradient.py [g17] [g18] [--jobs N]

Runs the reference (imported through oracle.gen_golden.load_reference_library), NumPy and SciPy on the CPU and writes
arrays only.  The 2-D inputs come from pyrayhf_amd.synth.tilted_ionosphere, so the tests rebuild them; g17 also carries
its mu and mu' planes, because np.gradient is pinned bit for bit and must see the very values the reference produced.

g17: fields and sampler.  A non-uniform and a uniform 41 x 33 grid, O mode at 6 MHz and X mode at 9 MHz (both with a
NaN cap above reflection); np.gradient at both edge orders in both geometries; RegularGridInterpolator values (through
the reference's builders) at ~2000 points per grid and mode: grid nodes, grid lines next to NaN nodes, hull edges and
corners, points outside, NaN coordinates, random interior points.

g18: rays.  A tilted (0.3) two-layer ionosphere and its zero-tilt twin on a uniform 121 x 201 grid, 6 MHz O and 9 MHz X,
16 elevations from 5 to 85 degrees from the centre of the domain, two control sets (the reference's own test's:
max_step_km=5 in a bounded domain; the defaults: max_step_km=None), three reference runs per ray (see RUNS).  The
generator asserts that the three runs' statuses agree for >= 90 % of the rays and that the truth run has converged:
per key, max|check - truth| <= 0.1 max|default - truth|.
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

# ---- g17 ----------------------------------------------------------------------------------------------------------
G17_SEED, G17_TILT, G17_NZ, G17_NX = 17, 0.3, 41, 33
G17_GRIDS = (("nonuniform", False), ("uniform", True))
G17_MODES = (("O", 6.0e6), ("X", 9.0e6))


def g17_points(rng, z, x, mu):
    """~2000 (z, x) sample points of every kind the sampler must get right."""
    nz, nx = mu.shape
    pts = []
    i = rng.integers(0, nz, 400)
    j = rng.integers(0, nx, 400)
    pts.append(np.column_stack([z[i], x[j]]))                                  # grid nodes
    nan = np.isnan(mu)
    edge = nan & ~(np.roll(nan, 1, 0) & np.roll(nan, -1, 0) & np.roll(nan, 1, 1) & np.roll(nan, -1, 1))
    near = np.argwhere(edge | np.roll(edge, 1, 0) | np.roll(edge, -1, 0) | np.roll(edge, 1, 1) | np.roll(edge, -1, 1))
    near = near[(near[:, 0] < nz - 1) & (near[:, 1] < nx - 1)]
    pick = near[rng.integers(0, len(near), 500)]
    fz, fx = rng.uniform(0, 1, 500), rng.uniform(0, 1, 500)
    zi, xi = z[pick[:, 0]], x[pick[:, 1]]
    dz, dx = z[pick[:, 0] + 1] - zi, x[pick[:, 1] + 1] - xi
    pts.append(np.column_stack([zi, xi + fx * dx])[:200])                      # on a z line next to NaN nodes
    pts.append(np.column_stack([zi + fz * dz, xi])[200:400])                   # on an x line next to NaN nodes
    pts.append(np.column_stack([zi + fz * dz, xi + fx * dx])[400:])            # inside cells next to NaN nodes
    u = rng.uniform(0, 1, 60)
    zr, xr = z[0] + u * (z[-1] - z[0]), x[0] + u[::-1] * (x[-1] - x[0])
    pts.append(np.column_stack([np.full(60, z[0]), xr]))                       # hull edges
    pts.append(np.column_stack([np.full(60, z[-1]), xr]))
    pts.append(np.column_stack([zr, np.full(60, x[0])]))
    pts.append(np.column_stack([zr, np.full(60, x[-1])]))
    pts.append(np.array([[z[0], x[0]], [z[0], x[-1]], [z[-1], x[0]], [z[-1], x[-1]]]))
    eps = 1e-9
    pts.append(np.column_stack([np.full(30, z[0] - eps), xr[:30]]))            # just outside, far outside
    pts.append(np.column_stack([np.full(30, np.nextafter(z[-1], np.inf)), xr[:30]]))
    pts.append(np.column_stack([zr[:30], np.full(30, np.nextafter(x[0], -np.inf))]))
    pts.append(np.column_stack([zr[:30], np.full(30, x[-1] + 1e4)]))
    pts.append(np.array([[-np.inf, 0.0], [np.inf, 0.0], [z[3], np.inf], [z[3], -np.inf]]))
    pts.append(np.array([[np.nan, x[3]], [z[3], np.nan], [np.nan, np.nan], [np.nan, 1e9], [-1e9, np.nan]]))
    n_more = 2000 - sum(len(p) for p in pts)
    pts.append(np.column_stack([rng.uniform(z[0], z[-1], n_more), rng.uniform(x[0], x[-1], n_more)]))
    return np.ascontiguousarray(np.vstack(pts))


def gen_g17(ref):
    out = {}
    r_e = ref.constants()[2]
    rng = np.random.default_rng(G17_SEED)
    for gname, uniform in G17_GRIDS:
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(G17_NZ, G17_NX, G17_TILT, G17_SEED, uniform=uniform)
        for mode, f in G17_MODES:
            mu, mup = ref.find_mu_mup(ref.find_X(den, f), ref.find_Y(f, bmag), bpsi, mode)
            mu, mup = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(mup, dtype=np.float64)
            assert np.isnan(mu).any() and np.isfinite(mu).any(), "the field needs a NaN cap"
            key = f"{gname}_{mode}"
            out[key + "_mu"], out[key + "_mup"] = mu, mup
            for geo, (a0, a1) in (("cartesian", (z, x)), ("spherical", (r_e + z, x / r_e))):
                for order in (1, 2):
                    with np.errstate(all="ignore"):
                        d0, d1 = np.gradient(mu, a0, a1, edge_order=order)
                    out[f"{key}_{geo}_e{order}_d0"], out[f"{key}_{geo}_e{order}_d1"] = d0, d1
            pts = g17_points(rng, z, x, mu)
            n_and_grad = ref.build_refractive_index_interpolator_cartesian(z, x, mu)
            mup_func = ref.build_mup_function(mup, x, z)
            with np.errstate(all="ignore"):
                n, dndx, dndz = n_and_grad(pts[:, 1], pts[:, 0])
                m = mup_func(pts[:, 1], pts[:, 0])
            out[key + "_points"] = pts
            out[key + "_rgi"] = np.ascontiguousarray(np.stack([n, dndx, dndz, m]))
            # the spherical builder on the same field: (phi, r) -> (mu, dmu/dr, dmu/dphi)
            sph = ref.build_refractive_index_interpolator_spherical(z, x, mu)
            with np.errstate(all="ignore"):
                out[key + "_rgi_spherical"] = np.ascontiguousarray(np.stack(sph(pts[:, 1] / r_e, r_e + pts[:, 0])))
    path = os.path.join(GOLDEN, "g17_fields.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


# ---- g18 ----------------------------------------------------------------------------------------------------------
G18_SEED, G18_NZ, G18_NX = 18, 121, 201
G18_TILTS = (0.3, 0.0)
G18_CASES = (("O", 6.0e6), ("X", 9.0e6))
G18_ELEVATIONS = np.linspace(5.0, 85.0, 16)
G18_SETS = (dict(s_max_km=4000.0, max_step_km=5.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0),   # test_core.py:818-828
            dict(max_step_km=None))                                                                     # the defaults
RUNS = (("default", 1e-7, 1e-9, None), ("truth", 1e-10, 1e-12, 0.25), ("check", 1e-9, 1e-11, 0.5))
SCALARS = ("group_path_km", "group_delay_sec", "ground_range_km", "x_apex_km", "z_apex_km")
STATUS = ("ground", "domain", "length", "failure")

_worker = {}


def _g18_ray(task):
    ti, ci, si, ei, ri = task
    if "ref" not in _worker:
        _worker["ref"] = load_reference_library()
        _worker["fields"] = {}
    ref = _worker["ref"]
    if (ti, ci) not in _worker["fields"]:
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(G18_NZ, G18_NX, G18_TILTS[ti], G18_SEED)
        mode, f = G18_CASES[ci]
        mu, mup = ref.find_mu_mup(ref.find_X(den, f), ref.find_Y(f, bmag), bpsi, mode)
        _worker["fields"][(ti, ci)] = (ref.build_refractive_index_interpolator_cartesian(z, x, mu),
                                       ref.build_mup_function(mup, x, z))
    n_and_grad, mup_func = _worker["fields"][(ti, ci)]
    _, rtol, atol, step = RUNS[ri]
    kw = dict(G18_SETS[si])
    if step is not None:
        kw["max_step_km"] = step
    if kw["max_step_km"] is None:
        # The reference hands None straight to solve_ivp(max_step=...), which the installed SciPy refuses
        # ("'<=' not supported between 'NoneType' and 'int'"): the default set is run with what None stands for in
        # solve_ivp's documentation, no limit.
        kw["max_step_km"] = np.inf
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        r = ref.trace_ray_cartesian_gradient(n_and_grad, mup_func, 0.0, 0.0, float(G18_ELEVATIONS[ei]), rtol=rtol, atol=atol,
                                             **kw)
    dt = time.perf_counter() - t0
    return task, [float(r[k]) for k in SCALARS], STATUS.index(r["status"]), dt, len(r["t"])


def gen_g18(jobs):
    import multiprocessing as mp
    shape = (len(G18_TILTS), len(G18_CASES), len(G18_SETS), len(G18_ELEVATIONS))
    tasks = [(ti, ci, si, ei, ri) for ri in (1, 2, 0) for ti in range(shape[0]) for ci in range(shape[1])
             for si in range(shape[2]) for ei in range(shape[3])]
    vals = np.full((len(RUNS),) + shape + (len(SCALARS),), np.nan)
    status = np.full((len(RUNS),) + shape, -1, dtype=np.int64)
    secs = np.zeros((len(RUNS),) + shape)
    nodes = np.zeros((len(RUNS),) + shape, dtype=np.int64)
    with mp.Pool(jobs) as pool:
        for k, (task, v, st, dt, n) in enumerate(pool.imap_unordered(_g18_ray, tasks, chunksize=2)):
            ti, ci, si, ei, ri = task
            vals[(ri, ti, ci, si, ei)] = v
            status[(ri, ti, ci, si, ei)] = st
            secs[(ri, ti, ci, si, ei)] = dt
            nodes[(ri, ti, ci, si, ei)] = n
            if k % 32 == 0:
                print(f"  {k}/{len(tasks)} rays", flush=True)
    agree = (status[0] == status[1]) & (status[0] == status[2])
    print("statuses (default run):", {STATUS[s]: int((status[0] == s).sum()) for s in range(4)}, "agree:", agree.mean())
    assert agree.mean() >= 0.9, f"the three runs' statuses agree for {agree.mean():.3f} of the rays only"
    for ki, key in enumerate(SCALARS):
        for si in range(shape[2]):
            m = agree[:, :, si]
            d = np.abs(vals[0][:, :, si, :, ki] - vals[1][:, :, si, :, ki])[m]
            c = np.abs(vals[2][:, :, si, :, ki] - vals[1][:, :, si, :, ki])[m]
            ok = np.isfinite(d) & np.isfinite(c)
            ratio = c[ok].max() / d[ok].max() if ok.any() and d[ok].max() > 0 else 0.0
            print(f"  set {si} {key}: max|default - truth| = {d[ok].max() if ok.any() else 0:.3e}, "
                  f"max|check - truth| = {c[ok].max() if ok.any() else 0:.3e}, ratio {ratio:.3f}")
            if key != "x_apex_km":          # (the x of whichever node is highest moves with the step sequence)
                assert ratio <= 0.1, (key, si, ratio)
    out = {"elevation_deg": G18_ELEVATIONS, "tilts": np.array(G18_TILTS), "freq_hz": np.array([f for _, f in G18_CASES]),
           "mode_is_x": np.array([m == "X" for m, _ in G18_CASES]), "agree": agree, "seconds_per_ray": secs,
           "n_nodes": nodes}
    for ri, (name, *_rest) in enumerate(RUNS):
        out[name + "_status"] = status[ri]
        for ki, key in enumerate(SCALARS):
            out[f"{name}_{key}"] = np.ascontiguousarray(vals[ri][..., ki])
    path = os.path.join(GOLDEN, "g18_gradient_rays.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; reference seconds per ray (default run): "
          f"median {np.median(secs[0]):.3f}, max {secs[0].max():.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="*", default=["g17", "g18"])
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    if "g17" in args.which:
        gen_g17(load_reference_library())
    if "g18" in args.which:
        gen_g18(args.jobs)


if __name__ == "__main__":
    main()
