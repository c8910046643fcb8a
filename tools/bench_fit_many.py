#!/usr/bin/env python3
"""Many ionograms fitted in one launch (fitting.residual_VH_many) against the loop of single-trace calls that existed
before it, on the same build: one fitting.residual_VH_batch call per ionogram on its kept frequencies, its cost row
copied to the host and a host argmin.

    python tools/bench_fit_many.py [--reps N] [--loop-reps N] [--out profiles/bench_fit_many.jsonl] [--quick]

Two layouts, one JSON line each:
  own     256 ionograms x 1681 candidates of their own (a 41 x 41 grid) x 80 grid frequencies, O mode, 200 points;
  shared  4096 ionograms against one library of 16384 candidates, 80 grid frequencies, O mode, 200 points.
Every ionogram observes the trace of one of its candidates plus noise and misses a random fifth of the grid.  All
arrays live on the GPU before the clock starts (Chapman candidates built there; the loop's per-ionogram frequency and
observation tensors too), so both routes are timed on launches, kernels and the copies of their RESULTS: the loop brings
every cost row to the host, the one-launch call brings best and best_cost.  Host clock around work that ends in a
synchronising copy; medians of interleaved repetitions after a warm-up of both routes.  The two routes must name the
same winners (asserted) - the costs themselves are compared and recorded.  --quick: small shapes, to rehearse the script.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from pyrayhf_amd import fitting, library, synth  # noqa: E402

MODE, N_POINTS, F = "O", 200, 80


def _median(xs):
    return float(np.median(np.asarray(xs)))


def _observations(freq, den, bmag, bpsi, alt, truth_rows, seed):
    """(I, F) observations on the device: the trace of one candidate per ionogram + 0.5 km noise, a fifth missing."""
    import torch
    rng = np.random.default_rng(seed)
    traces = library.vertical_forward_operator(torch.as_tensor(freq, device=den.device), den[truth_rows], bmag, bpsi, alt,
                                               MODE, N_POINTS).cpu().numpy()
    obs = traces + rng.normal(0.0, 0.5, traces.shape)
    obs[rng.random(obs.shape) < 0.2] = np.nan
    obs[:, 0] = np.where(np.isnan(obs).all(axis=1), 250.0, obs[:, 0])      # (never an ionogram without an echo)
    return obs


def _loop_inputs(freq, obs, dev):
    import torch
    out = []
    for row in obs:
        keep = np.isfinite(row)
        out.append((torch.as_tensor(freq[keep], device=dev), torch.as_tensor(row[keep], device=dev)))
    return out


def _loop(per_ionogram, candidates_of, bmag, bpsi, alt):
    """Today's route: one call per ionogram, the cost row to the host, argmin there."""
    best = np.empty(len(per_ionogram), dtype=np.int64)
    best_cost = np.empty(len(per_ionogram))
    for i, (f, o) in enumerate(per_ionogram):
        _, cost = fitting.residual_VH_batch(f, o, candidates_of(i), bmag, bpsi, alt, MODE, N_POINTS)
        cost = cost.cpu().numpy()
        finite = np.isfinite(cost)
        k = int(np.argmin(np.where(finite, cost, np.inf))) if finite.any() else -1
        best[i], best_cost[i] = k, (cost[k] if k >= 0 else np.nan)
    return best, best_cost


def _time_routes(many, loop, reps, loop_reps):
    many(), loop()                                         # warm-up: code objects, scratch buffers, cached grids
    t_many, t_loop = [], []
    for r in range(max(reps, loop_reps)):
        if r < reps:
            t0 = time.perf_counter()
            many()
            t_many.append(time.perf_counter() - t0)
        if r < loop_reps:
            t0 = time.perf_counter()
            loop()
            t_loop.append(time.perf_counter() - t0)
    return t_many, t_loop


def _record(layout, shape, t_many, t_loop, kernel_ms, got, want):
    (best, best_cost), (best_l, best_cost_l) = got, want
    assert np.array_equal(best, best_l), f"{layout}: the two routes name different winners"
    ok = np.isfinite(best_cost_l)
    rel = np.abs(best_cost - best_cost_l)[ok] / np.abs(best_cost_l[ok])
    rec = dict(layout=layout, mode=MODE, n_points=N_POINTS, n_freq=F, **shape,
               one_launch_ms=1e3 * _median(t_many), one_launch_ms_min=1e3 * min(t_many), one_launch_reps=len(t_many),
               one_launch_device_ms=kernel_ms, loop_ms=1e3 * _median(t_loop), loop_ms_min=1e3 * min(t_loop),
               loop_reps=len(t_loop), loop_over_one_launch=_median(t_loop) / _median(t_many),
               winners_equal=True, ionograms_with_a_winner=int(ok.sum()),
               best_cost_bit_equal=bool(np.array_equal(best_cost[ok], best_cost_l[ok])),
               best_cost_max_rel_diff=float(rel.max()) if rel.size else 0.0)
    print(json.dumps(rec), flush=True)
    return rec


def bench_own(dev, n_iono, per, reps, loop_reps):
    import torch
    alt, den, bmag, bpsi = synth.chapman_profiles_torch(n_iono * per, 11, dev)
    bmag, bpsi = bmag[0].clone(), bpsi[0].clone()           # one site: the candidates of a fit share the field
    freq = np.linspace(1.5, 12.0, F)
    ion = torch.arange(n_iono, device=dev, dtype=torch.int32).repeat_interleave(per)
    truth = np.arange(n_iono) * per + np.random.default_rng(3).integers(0, per, n_iono)
    obs = _observations(freq, den, bmag, bpsi, alt, torch.as_tensor(truth, device=dev), 5)
    t_freq, t_obs = torch.as_tensor(freq, device=dev), torch.as_tensor(obs, device=dev)
    per_ionogram = _loop_inputs(freq, obs, dev)
    result = {}

    def many():
        _, best, best_cost = fitting.residual_VH_many(t_freq, t_obs, den, bmag, bpsi, alt, MODE, N_POINTS, ionogram_of_row=ion)
        result["many"] = (best.cpu().numpy(), best_cost.cpu().numpy())

    def loop():
        best, best_cost = _loop(per_ionogram, lambda i: den[i * per:(i + 1) * per], bmag, bpsi, alt)
        result["loop"] = (best + np.arange(n_iono) * per, best_cost)

    t_many, t_loop = _time_routes(many, loop, reps, loop_reps)
    many()
    kernel_ms = library.last_kernel_ms(dev.index or 0)
    return _record("own", dict(n_ionograms=n_iono, candidates_per_ionogram=per, n_alt=int(alt.numel())), t_many, t_loop,
                   kernel_ms, result["many"], result["loop"])


def bench_shared(dev, n_iono, n_cand, reps, loop_reps):
    import torch
    alt, den, bmag, bpsi = synth.chapman_profiles_torch(n_cand, 13, dev)
    bmag, bpsi = bmag[0].clone(), bpsi[0].clone()
    freq = np.linspace(1.5, 12.0, F)
    truth = np.random.default_rng(4).integers(0, n_cand, n_iono)
    obs = _observations(freq, den, bmag, bpsi, alt, torch.as_tensor(truth, device=dev), 6)
    t_freq, t_obs = torch.as_tensor(freq, device=dev), torch.as_tensor(obs, device=dev)
    per_ionogram = _loop_inputs(freq, obs, dev)
    result = {}

    def many():
        _, best, best_cost = fitting.residual_VH_many(t_freq, t_obs, den, bmag, bpsi, alt, MODE, N_POINTS, shared=True)
        result["many"] = (best.cpu().numpy(), best_cost.cpu().numpy())

    def loop():
        result["loop"] = _loop(per_ionogram, lambda i: den, bmag, bpsi, alt)

    t_many, t_loop = _time_routes(many, loop, reps, loop_reps)
    many()
    kernel_ms = library.last_kernel_ms(dev.index or 0)
    return _record("shared", dict(n_ionograms=n_iono, n_candidates=n_cand, n_alt=int(alt.numel())), t_many, t_loop,
                   kernel_ms, result["many"], result["loop"])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of the one-launch call")
    ap.add_argument("--loop-reps", type=int, default=3, help="timed repetitions of the loop of single-trace calls")
    ap.add_argument("--out", default=os.path.join("profiles", "bench_fit_many.jsonl"))
    ap.add_argument("--quick", action="store_true", help="small shapes (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_many.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    own = (8, 25) if args.quick else (256, 1681)
    shared = (16, 64) if args.quick else (4096, 16384)
    records = [bench_own(dev, *own, args.reps, args.loop_reps)]
    torch.cuda.empty_cache()
    records.append(bench_shared(dev, *shared, args.reps, args.loop_reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in records:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
