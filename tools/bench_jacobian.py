#!/usr/bin/env python3
"""Time the vector-Jacobian product of the forward operator (library.vertical_vjp) against the forward launch itself.

    python tools/bench_jacobian.py [--reps N] [--out profiles/bench_jacobian.jsonl] [--parent-tree PATH] [--quick]

Shapes (one JSON line each):
  config3        10 000 profiles x 174 frequencies, O mode, 200 points
  config4_shard  12 500 profiles x 256 frequencies, X mode, 20 000 points (config 4's per-GPU shard)
Method, also written into every line: all arrays are resident on the GPU before the clock starts (Chapman profiles built
there, the upstream gradient drawn there); each launch is timed by the context's own start / stop events
(library.last_kernel_ms: device time of the launch, tables included); one warm-up launch and `reps` timed launches of
the forward operator, then the same of the VJP; medians.  `forward_parent_ms`: the same forward timing in a
fresh process that imports the package from --parent-tree (a checkout of the parent commit with its library built) - it
must equal `forward_ms` within the +-3 % by which the boxes differ.  `fd_route_ms` is the finite-difference route to the same
gradient, K + 1 forward launches with K the highest density peak of the batch: computed as (K + 1) x forward_ms, not run.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"config3": (10_000, 3, "O", 200, 3), "config4_shard": (12_500, 4, "X", 20_000, 4)}
QUICK = {"config3": (500, 3, "O", 200, 3), "config4_shard": (200, 4, "X", 2_000, 4)}
METHOD = ("resident arrays; device time of each launch from the context's events (last_kernel_ms); 1 warm-up + reps forward "
          "launches, then 1 warm-up + reps VJP launches; medians; forward_parent_ms: the forward leg in a fresh process on the "
          "parent commit's tree; fd_route_ms = (K + 1) x forward_ms, computed")


def inputs(name, quick):
    import torch
    from pyrayhf_amd import synth
    n_prof, config, mode, n_points, seed = (QUICK if quick else SHAPES)[name]
    dev = torch.device("cuda", 0)
    alt, den, bmag, bpsi = synth.chapman_profiles_torch(n_prof, seed, dev)
    freq = torch.as_tensor(synth.sounder_frequencies(config), device=dev)
    return freq, den, bmag, bpsi, alt, mode, n_points


def time_shape(name, reps, quick, forward_only):
    import torch
    from pyrayhf_amd import library
    freq, den, bmag, bpsi, alt, mode, n_points = inputs(name, quick)
    gen = torch.Generator(device=den.device).manual_seed(11)
    g = torch.rand((den.shape[0], freq.numel()), dtype=torch.float64, device=den.device, generator=gen) - 0.5
    out = torch.empty((den.shape[0], freq.numel()), dtype=torch.float64, device=den.device)

    def forward():
        library.vertical_forward_operator(freq, den, bmag, bpsi, alt, mode, n_points, out=out)
        return library.last_kernel_ms(0)

    def vjp():
        library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, n_points)
        return library.last_kernel_ms(0)

    # the forward launches first, by themselves - exactly what the parent-tree leg does - then the VJP launches: a
    # second-long VJP in front of a forward launch changes the clocks that launch runs at
    forward()
    t_f = [forward() for _ in range(reps)]
    t_v = []
    if not forward_only:
        vjp()
        t_v = [vjp() for _ in range(reps)]
    rec = {"shape": name, "n_prof": int(den.shape[0]), "n_freq": int(freq.numel()), "n_alt": int(den.shape[1]), "mode": mode,
           "n_points": n_points, "reps": reps, "forward_ms": float(np.median(t_f)),
           "forward_ms_min_max": [float(min(t_f)), float(max(t_f))]}
    if not forward_only:
        peak = int(torch.argmax(den, dim=1).max())
        rec.update(vjp_ms=float(np.median(t_v)), vjp_ms_min_max=[float(min(t_v)), float(max(t_v))],
                   vjp_over_forward=float(np.median(t_v) / np.median(t_f)), highest_peak_level=peak,
                   fd_route_ms=float((peak + 1) * np.median(t_f)),
                   fd_route_over_vjp=float((peak + 1) * np.median(t_f) / np.median(t_v)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its libprhf.so built")
    ap.add_argument("--tree", default=HERE, help="(used for the --parent-tree leg) the tree to import pyrayhf_amd from")
    ap.add_argument("--quick", action="store_true", help="small shapes, to rehearse the script")
    ap.add_argument("--forward-only", action="store_true", help="(used for the --parent-tree leg) print forward timings only")
    ap.add_argument("--shapes", default="config3,config4_shard")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    lines = []
    for name in args.shapes.split(","):
        rec = time_shape(name, args.reps, args.quick, args.forward_only)
        if args.parent_tree and not args.forward_only:
            cmd = [sys.executable, os.path.abspath(__file__), "--forward-only", "--reps", str(args.reps), "--shapes", name,
                   "--tree", args.parent_tree]
            run = subprocess.run(cmd + (["--quick"] if args.quick else []), capture_output=True, text=True, timeout=1200)
            if run.returncode != 0:
                raise SystemExit("the parent-tree leg failed:\n" + run.stderr[-3000:])
            parent = json.loads(run.stdout.strip().splitlines()[-1])
            rec["forward_parent_ms"] = parent["forward_ms"]
            rec["forward_over_parent"] = rec["forward_ms"] / parent["forward_ms"]
        if not args.forward_only:
            rec["method"] = METHOD
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out and not args.forward_only:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
