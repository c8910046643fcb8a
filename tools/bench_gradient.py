"""Measure a gradient tracer: a fan of 64 fields x 256 elevations in one launch.

    python tools/bench_gradient.py [--geometry cartesian|spherical] [--repeats N] [--accuracy]

Prints one JSON line and appends it to profiles/bench_gradient.jsonl: rays/s and right-hand-side evaluations/s from
the launch's device time (HIP events, library.last_kernel_ms), the lane utilisation
sum(n_rhs) / (64 * sum over waves of max n_rhs) from the kernel's own counters, and - for scale only - the reference's
seconds per ray as recorded in tests/golden/g18_gradient_rays.npz (spherical: g19_spherical_rays.npz), a CPU figure
from another host.  With --accuracy also writes profiles/gradient_accuracy.md (profiles/spherical_gradient_accuracy.md):
per control set and key, max|GPU - truth| against max|reference - truth| over the rays of the fixture.  Recorded
figures; nothing here passes or fails.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from pyrayhf_amd import gradient, library, synth  # noqa: E402

R_E = library.constants()[2]
SETS = {"cartesian": (dict(s_max_km=4000.0, max_step_km=5.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0),
                      dict(max_step_km=None)),
        "spherical": (dict(s_max_km=4000.0, max_step_km=5.0, r_max_km=R_E + 600.0, phi_min=-1000.0 / R_E,
                           phi_max=1000.0 / R_E), dict())}
FAN = {"cartesian": gradient.trace_fan_cartesian_gradient, "spherical": gradient.trace_fan_spherical_gradient}
FIXTURE = {"cartesian": "g18_gradient_rays.npz", "spherical": "g19_spherical_rays.npz"}
KEYS = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km")


def bench(repeats, geometry):
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.3, 18)
    field = gradient.refractive_field(np.linspace(4.0e6, 10.0e6, 64), den, bmag, bpsi, z, x, "O", geometry=geometry)
    elev = np.linspace(5.0, 85.0, 256)
    sets, fan = SETS[geometry], FAN[geometry]
    fan(field, elev, **sets[0])                                                    # warm-up
    ms = []
    for _ in range(repeats):
        r = fan(field, elev, **sets[0])
        ms.append(library.last_kernel_ms(0))
    n_rhs = r["n_rhs"].reshape(-1).astype(np.float64)                              # (field, elevation) order = launch order
    waves = n_rhs.reshape(-1, 64)
    g = np.load(os.path.join(REPO, "tests", "golden", FIXTURE[geometry]))
    best = min(ms)
    name = "gradient fan" if geometry == "cartesian" else "spherical gradient fan"
    return {"workload": f"{name}, 64 fields x 256 elevations, 121 x 201 grid, max_step_km=5", "rays": int(n_rhs.size),
            "kernel_ms_min": best, "kernel_ms_median": float(np.median(ms)), "repeats": repeats,
            "rays_per_s": n_rhs.size / (best * 1e-3), "rhs_evaluations": int(n_rhs.sum()),
            "rhs_per_s": float(n_rhs.sum()) / (best * 1e-3),
            "rhs_note": "counted calls of the ray itself; the midpoint replay repeats about half of them on top",
            "nodes": int(r["n_nodes"].sum()), "rejected_steps": int(r["n_rejected"].sum()),
            "lane_utilisation": float(n_rhs.sum() / (64.0 * waves.max(axis=1).sum())),
            "status_counts": {gradient.STATUS_NAMES[s]: int((r["status"] == s).sum()) for s in range(4)},
            "reference_cpu_seconds_per_ray_median": float(np.median(g["seconds_per_ray"][0])),
            "reference_note": f"CPU figure from another host ({FIXTURE[geometry][:3]} default run), for scale only"}


def accuracy(geometry):
    g = np.load(os.path.join(REPO, "tests", "golden", FIXTURE[geometry]))
    sets, fan = SETS[geometry], FAN[geometry]
    title = "Gradient tracer" if geometry == "cartesian" else "Spherical gradient tracer"
    lines = [f"# {title}: error against the reference's converged run (fixture {FIXTURE[geometry][:3]})", "",
             "Per control set and key: max over the rays whose three reference runs agree in status of |value - truth|,",
             "truth = reference at rtol 1e-10, atol 1e-12, max_step 0.25 km; GPU and reference both at rtol 1e-7, atol 1e-9.",
             "", "| control set | key | GPU | reference | GPU / reference | rays |", "|---|---|---|---|---|---|"]
    got = {}
    for ti, tilt in enumerate((0.3, 0.0)):
        z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, tilt, 18)
        parts = [gradient.refractive_field([f], den, bmag, bpsi, z, x, m, geometry=geometry)
                 for m, f in (("O", 6.0e6), ("X", 9.0e6))]
        field = gradient.RefractiveField(parts[0].axis0, parts[0].axis1, np.concatenate([p.mu for p in parts]),
                                         np.concatenate([p.mup for p in parts]), geometry=geometry)
        for si in range(2):
            got[ti, si] = fan(field, g["elevation_deg"], **sets[si])
    for si, name in enumerate(("max_step_km=5, bounded domain", "defaults")):
        agree = g["agree"][:, :, si]
        status = np.stack([got[ti, si]["status"] for ti in range(2)])
        same = int((status[agree] == g["default_status"][:, :, si][agree]).sum())
        for key in KEYS:
            truth, ref = g["truth_" + key][:, :, si], g["default_" + key][:, :, si]
            gpu = np.stack([got[ti, si][key] for ti in range(2)])
            m = agree & np.isfinite(truth) & np.isfinite(ref) & np.isfinite(gpu)
            e_gpu, e_ref = np.abs(gpu[m] - truth[m]).max(), np.abs(ref[m] - truth[m]).max()
            lines.append(f"| {name} | {key} | {e_gpu:.3e} | {e_ref:.3e} | {e_gpu / e_ref:.3f} | {int(m.sum())} |")
        lines.append(f"| {name} | status | {same} of {int(agree.sum())} equal | | | {int(agree.sum())} |")
    path = os.path.join(REPO, "profiles", ("" if geometry == "cartesian" else "spherical_") + "gradient_accuracy.md")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--geometry", choices=("cartesian", "spherical"), default="cartesian")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bench_gradient.jsonl"))
    args = ap.parse_args()
    row = bench(args.repeats, args.geometry)
    print(json.dumps(row))
    with open(args.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")
    if args.accuracy:
        accuracy(args.geometry)


if __name__ == "__main__":
    main()
