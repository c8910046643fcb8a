#!/usr/bin/env python3
"""Time the Jacobian-vector product of the forward operator (library.vertical_jvp) against the forward launch and the
vector-Jacobian product (library.vertical_vjp) in one sitting.

    python tools/bench_jvp.py [--reps N] [--out profiles/bench_jvp.jsonl] [--quick] [--step-timeout S]

Shapes (one JSON line each):
  config3        10 000 profiles x 174 frequencies, O mode, 200 points
  config4_shard  12 500 profiles x 256 frequencies, X mode, 20 000 points (config 4's per-GPU shard)
Method, also written into every line: each shape runs in a child process of its own under a time limit (the parent never
opens the GPU; a child that fails or runs out of time ends the run); all arrays are resident on the GPU before the clock
starts (Chapman profiles built there, upstream gradient and tangents drawn there, tangents scaled by the density); each
call is timed by the context's own start / stop events (library.last_kernel_ms: device time of the call's launches - for
the JVP all of its chunk launches, without the operator's own launch that fills vh); one warm-up and `reps` timed calls of
the forward operator, then of the VJP, then of the JVP with T = 1, then with T = 8; medians.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

SHAPES = {"config3": (10_000, 3, "O", 200, 3), "config4_shard": (12_500, 4, "X", 20_000, 4)}
QUICK = {"config3": (500, 3, "O", 200, 3), "config4_shard": (200, 4, "X", 2_000, 4)}
METHOD = ("one child process per shape under a time limit; resident arrays; device time of each call from the context's events "
          "(last_kernel_ms; JVP: its chunk launches, not the operator's launch for vh); 1 warm-up + reps calls each of forward, "
          "VJP, JVP T=1, JVP T=8, in that order; medians")


def time_shape(name, reps, quick):
    import torch
    from pyrayhf_amd import library, synth
    n_prof, config, mode, n_points, seed = (QUICK if quick else SHAPES)[name]
    dev = torch.device("cuda", 0)
    alt, den, bmag, bpsi = synth.chapman_profiles_torch(n_prof, seed, dev)
    freq = torch.as_tensor(synth.sounder_frequencies(config), device=dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    g = torch.rand((n_prof, freq.numel()), dtype=torch.float64, device=dev, generator=gen) - 0.5
    tan = (2.0 * torch.rand((n_prof, 8, den.shape[1]), dtype=torch.float64, device=dev, generator=gen) - 1.0) * den[:, None, :]
    tan1 = tan[:, 0].contiguous()
    out = torch.empty((n_prof, freq.numel()), dtype=torch.float64, device=dev)

    def forward():
        library.vertical_forward_operator(freq, den, bmag, bpsi, alt, mode, n_points, out=out)

    def vjp():
        library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, n_points)

    def jvp1():
        library.vertical_jvp(freq, den, bmag, bpsi, alt, tan1, mode, n_points)

    def jvp8():
        library.vertical_jvp(freq, den, bmag, bpsi, alt, tan, mode, n_points)

    rec = {"shape": name, "n_prof": n_prof, "n_freq": int(freq.numel()), "n_alt": int(den.shape[1]), "mode": mode,
           "n_points": n_points, "reps": reps, "highest_peak_level": int(torch.argmax(den, dim=1).max())}
    for key, call in (("forward", forward), ("vjp", vjp), ("jvp1", jvp1), ("jvp8", jvp8)):
        call()
        times = []
        for _ in range(reps):
            call()
            times.append(library.last_kernel_ms(0))
        rec[key + "_ms"] = float(np.median(times))
        rec[key + "_ms_min_max"] = [float(min(times)), float(max(times))]
    rec.update(jvp1_over_forward=rec["jvp1_ms"] / rec["forward_ms"], jvp1_over_vjp=rec["jvp1_ms"] / rec["vjp_ms"],
               jvp8_over_forward=rec["jvp8_ms"] / rec["forward_ms"], jvp8_over_vjp=rec["jvp8_ms"] / rec["vjp_ms"],
               jvp8_over_jvp1=rec["jvp8_ms"] / rec["jvp1_ms"], method=METHOD)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes, to rehearse the script")
    ap.add_argument("--shapes", default="config3,config4_shard")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a shape's child process may take")
    ap.add_argument("--child", default=None, help="(internal) time this shape in this process and print its line")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(time_shape(args.child, args.reps, args.quick)), flush=True)
        return
    lines = []
    for name in args.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps)] + (["--quick"] if args.quick else [])
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{name}: no result within {args.step_timeout:.0f} s; nothing further is started")
        if run.returncode != 0:
            raise SystemExit(f"{name} failed with status {run.returncode}; nothing further is started:\n" + run.stderr[-3000:])
        lines.append(run.stdout.strip().splitlines()[-1])
        json.loads(lines[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
