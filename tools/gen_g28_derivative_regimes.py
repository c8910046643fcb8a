#!/usr/bin/env python
"""Write tests/golden/g28_derivative_regimes.npz: the shapes and data the derivative kernels take
other paths on than on fixture g26 - tall columns (fewer frequency waves / smaller tangent chunks by height, the peak
pre-pass), long grids (2000 and 20 000 points) and bad data (NaN psi, |B|, density) - with the 50-digit Jacobians of
tests/mp_vfo.py.  Layout and key names of g26; a batch case has a leading profile axis on den, bmag, bpsi, alt, vh_mp
and jac_mp.  jac_mp holds the columns below the highest peak only (the rest is zero).  Data only; needs mpmath and g++ (the
planning tools), not the reference tree; about a minute and a half on eight cores.

Per case also ``<name>_regime`` = [VJP waves, VJP lds_levels, Jacobian waves, Jacobian lds_levels, JVP chunk of the unit
tangents the GPU test runs (24 on a tall case, every level below the peak elsewhere), JVP lds_levels, JVP chunk of its
three dense tangents] as the host planning tools give it (waves / chunk 0: refused), ``kinds`` (tall, long or bad,
parallel to ``cases``) and, for a batch, ``<name>_regime_alone``: the same for each of its profiles called alone.  The frequencies of a batch
are the recipes of its profiles merged, so that every profile has reflecting pairs.

Asserted per pair as in tools/gen_g26_jacobian.py: the 50-digit value within 1e-12 (X) / 1e-6 (O) of the oracle with
the oracle's NaN mask, no kink of the operator within 1e-9; per case: the float64 restatement
tests/vfo_jacobian_numpy.py within g26's e_ref[mode] of the truth - a case that is not gets ``<name>_e_ref`` and is
listed in ``own_e_ref``.  ``e_ref28_O`` / ``e_ref28_X``: the restatement's largest row error on the bad-data cases.
``limits``: the largest level counts the VJP, Jacobian and JVP launches stage, from the tools' refusal messages.

The Chapman rows of the tall cases are chosen among the first eight so that the oracle can pin every value: a
first-interval O-mode pair of row 0 at 1400 levels sits 1.3e-5 from the 50-digit value (the oracle's own noise there,
as on g26's two-point grid), one X-mode pair of row 1 at peak 300 / 1400 levels 2.0e-12 and one O-mode pair of row 2
there 1.6e-6; rows 5, 2 and 1 take their places.  ``python gen_g28_derivative_regimes.py t5 psi`` is a dry run of the
cases whose names start so.
"""

from __future__ import annotations

import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import derivative_regimes as dr                          # noqa: E402
import mp_vfo                                            # noqa: E402
import vfo_jacobian_numpy as vj                          # noqa: E402
from gen_g26_jacobian import KINK, bracket, frequencies, grid_kink   # noqa: E402
from oracle import vfo_numpy as orc                      # noqa: E402
from pyrayhf_amd import synth                            # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g28_derivative_regimes.npz")
G26 = os.path.join(REPO, "tests", "golden", "g26_jacobian.npz")

# (name, [(Chapman row, peak level), ...], levels, mode, n_points): one profile, or a batch staged together
TALL = [("t1a", [(3, 700)], 1000, "O", 64), ("t1b", [(3, 700)], 1000, "X", 65),
        ("t2a", [(6, 900)], 1200, "X", 64), ("t2b", [(6, 900)], 1200, "O", 65),
        ("t3a", [(4, 1240)], 1300, "O", 65), ("t3b", [(4, 1240)], 1300, "X", 64),
        ("t4a", [(5, 1000)], 1400, "X", 200), ("t4b", [(5, 1000)], 1400, "O", 64),
        ("t5a", [(2, 300), (3, 1200)], 1400, "X", 65), ("t5b", [(1, 300), (3, 1200)], 1400, "O", 64)]


def _row(task):
    f, den, bmag, bpsi, alt, mode, n_points, unmag = task
    return mp_vfo.jacobian_row(f, den, bmag, bpsi, alt, mode, orc.stretch_multiplier(n_points), unmag)


def build_cases():
    """[(name, kind, freq, den (P, n_alt), bmag, bpsi, alt, mode, n_points)]; alt (n_alt,) or one row per profile"""
    alt620, den620, bmag620, bpsi620 = synth.chapman_profiles(40, 26)
    thin = slice(None, None, 8)
    cases = []
    for name, parts, levels, mode, n_points in TALL:
        cols = [dr.resample(alt620, den620[r], bmag620[r], bpsi620[r], levels, peak) for r, peak in parts]
        # (a batch: the recipe of every profile, merged - each profile has pairs that reflect in it)
        freq = np.unique(np.concatenate([frequencies(c[1], c[2], c[0], mode) for c in cols]))
        cases.append((name, "tall", freq, *[np.stack([c[i] for c in cols]) for i in (1, 2, 3, 0)], mode, n_points))
    # long grids: g26's case h (78 levels) and case o (620 levels)
    h = (den620[3, thin].copy(), bmag620[3, thin].copy(), bpsi620[3, thin].copy(), alt620[thin].copy())
    o = (den620[5].copy(), bmag620[5].copy(), bpsi620[5].copy(), alt620.copy())

    def three(col):
        fo = (orc.plasma_frequency(col[0][:int(np.argmax(col[0]))]) * 1e-6).max()
        return np.array([0.55 * fo, 0.97 * fo, 1.4 * fo + 1.0])
    cases.append(("lx20k", "long", three(h), h[0][None], h[1][None], h[2][None], h[3], "X", 20000))
    for name, mode in (("lx2k", "X"), ("lo2k", "O")):
        cases.append((name, "long", frequencies(h[0], h[1], h[3], mode), h[0][None], h[1][None], h[2][None], h[3], mode, 2000))
    cases.append(("lo2k620", "long", three(o), o[0][None], o[1][None], o[2][None], o[3], "O", 2000))
    # bad data on the 78-level column
    for kind in dr.BAD_COLUMNS:
        den, bmag, bpsi, alt = dr.bad_column(kind, *h)
        for mode in "OX":
            clean_b = h[1] * (1e-12 if kind == "btiny" else 1.0)
            freq = frequencies(den, clean_b, alt, mode, first_interval=False)
            if freq.size < 5:
                fo = (orc.plasma_frequency(den[:int(np.argmax(den))]) * 1e-6).max()
                freq = np.array(sorted([0.3 * fo, *freq]))
            assert freq.size == 5, (kind, mode, freq)
            for n_points in (64, 200):
                cases.append((f"{kind}_{mode}{n_points}", "bad", freq, den[None], bmag[None], bpsi[None], alt, mode, n_points))
    return cases


def main():
    if not mp_vfo.available():
        raise SystemExit("mpmath is needed")
    t0 = time.time()
    with np.load(G26) as z:
        e26 = {"O": float(z["e_ref_O"]), "X": float(z["e_ref_X"])}
    cases = build_cases()
    only = sys.argv[1:]                                  # name prefixes: a dry run of those cases, nothing is written
    if only:
        cases = [c for c in cases if c[0].startswith(tuple(only))]
    tasks, where = [], []
    for ci, (name, kind, freq, den, bmag, bpsi, alt, mode, n_points) in enumerate(cases):
        for p in range(den.shape[0]):
            unmag = mp_vfo.unmagnetised(freq, den[p], bmag[p])
            for i, f in enumerate(freq):
                tasks.append((float(f), den[p], bmag[p], bpsi[p], alt[p] if alt.ndim == 2 else alt, mode, n_points, unmag))
                where.append((ci, p, i))
    order = sorted(range(len(tasks)), key=lambda t: -tasks[t][6] * tasks[t][1].size)        # the long ones first
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        done = pool.map(_row, [tasks[t] for t in order], chunksize=1)
    results = {where[t]: r for t, r in zip(order, done)}
    print(f"{len(tasks)} rows in {time.time() - t0:.0f} s")

    out = {"cases": np.array([c[0] for c in cases]), "kinds": np.array([c[1] for c in cases])}
    e28 = {"O": 0.0, "X": 0.0}
    own, seen = [], {"valley_tall": 0, "escape": 0, "skipped_terms": 0, "nan_trace": 0, "unmag_by_nanmax": 0}
    with tempfile.TemporaryDirectory() as tmp:
        exes = dr.build_tools(tmp)
        limits = np.array(dr.limits(exes), dtype=np.int64)     # largest staged levels: VJP, Jacobian, JVP
        for ci, (name, kind, freq, den, bmag, bpsi, alt, mode, n_points) in enumerate(cases):
            P, n_alt = den.shape
            peak = dr.highest_peak(den)
            vh_mp = np.empty((P, freq.size))
            J_mp = np.zeros((P, freq.size, n_alt))
            worst = 0.0
            for p in range(P):
                K = int(np.argmax(den[p]))
                alt_p = alt[p] if alt.ndim == 2 else alt
                finite = den[p][~np.isnan(den[p])]
                top2 = np.sort(finite)[-2:]
                assert np.isnan(den[p]).any() or (top2[1] - top2[0]) / top2[1] > KINK, (name, "argmax tie")
                for i in range(freq.size):
                    vh_mp[p, i], J_mp[p, i] = results[(ci, p, i)]
                with np.errstate(all="ignore"):
                    vh_orc = orc.virtual_heights(freq, den[p], bmag[p], bpsi[p], alt_p, mode, n_points)
                    vh_np, J_np = vj.jacobian(freq, den[p], bmag[p], bpsi[p], alt_p, mode, orc.stretch_multiplier(n_points))
                assert np.array_equal(np.isnan(vh_mp[p]), np.isnan(vh_orc)), (name, vh_mp[p], vh_orc)
                assert np.array_equal(np.isnan(vh_np), np.isnan(vh_orc)), (name, vh_np, vh_orc)
                ok = np.isfinite(vh_orc)
                if ok.any():
                    pin = np.abs(vh_mp[p][ok] - vh_orc[ok]) / np.abs(vh_orc[ok])
                    assert pin.max() <= (1e-12 if mode == "X" else 1e-6), (name, "mp value against the oracle", pin)
                for i, f in enumerate(freq):
                    with np.errstate(all="ignore"):
                        reflects, j, jm, dist = bracket(f, den[p], bmag[p], alt_p, mode)
                        gk = grid_kink(f, den[p], bmag[p], bpsi[p], alt_p, mode, n_points)
                    if np.isnan(dist):                  # a NaN |B| in the X-mode cutoff: no bracket, no value
                        assert np.isnan(vh_orc[i]), (name, f)
                        seen["nan_trace"] += 1
                    else:
                        assert dist > KINK, (name, f, "bracket kink", dist)
                        assert gk > KINK, (name, f, "grid point on a level")
                    seen["escape"] += int(not reflects)
                    seen["valley_tall"] += int(kind == "tall" and bool(reflects) and 0 <= jm < j)
                    scale = np.abs(J_mp[p, i]).max()
                    assert np.isfinite(J_mp[p, i]).all() and np.isfinite(J_np[i]).all() and not J_mp[p, i, K:].any(), name
                    if scale > 0.0:
                        assert np.isfinite(vh_orc[i]), name
                        worst = max(worst, float(np.abs(J_np[i] - J_mp[p, i]).max() / scale))
                    else:
                        assert np.isnan(vh_orc[i]) and not J_np[i].any(), (name, i)
                if kind == "bad" and ok.any():
                    # a pair with a value although some of its terms are NaN and skipped
                    with np.errstate(all="ignore"):
                        cols = orc.stretched_columns(freq * 1e6, den[p], bmag[p], bpsi[p], alt_p, mode, n_points)
                    holes = np.isnan(cols["bmag"]) | np.isnan(cols["bpsi"])
                    seen["skipped_terms"] += int((holes.any(axis=1) & ok).sum())
                if name.startswith("btiny_O"):
                    assert mp_vfo.unmagnetised(freq, den[p], bmag[p])
                    seen["unmag_by_nanmax"] += 1
            if kind == "bad":
                e28[mode] = max(e28[mode], worst)
            if worst > e26[mode]:
                own.append(name)
                out[f"{name}_e_ref"] = np.array(worst)
                print("   OWN e_ref:", name, worst, "g26", e26[mode])
            reg = dr.regime(exes, P, freq.size, n_alt, peak, dr.n_unit(kind, peak))
            if P > 1:                                   # ... and of each profile of a batch called alone
                out[f"{name}_regime_alone"] = np.stack([dr.regime(exes, 1, freq.size, n_alt, int(np.argmax(d)), dr.N_UNIT)
                                                        for d in den])
                assert all(np.isfinite(vh_mp[p]).sum() >= 2 and J_mp[p].any(axis=1).sum() >= 2 for p in range(P)), name
            single = P == 1
            out.update({f"{name}_freq": freq, f"{name}_den": den[0] if single else den,
                        f"{name}_bmag": bmag[0] if single else bmag, f"{name}_bpsi": bpsi[0] if single else bpsi,
                        f"{name}_alt": alt[0] if single and alt.ndim == 2 else alt, f"{name}_mode": np.array(mode), f"{name}_n_points": np.array(n_points),
                        f"{name}_vh_mp": vh_mp[0] if single else vh_mp,
                        f"{name}_jac_mp": J_mp[0, :, :peak] if single else J_mp[:, :, :peak],
                        f"{name}_regime": reg})
            print(f"{name:12s} {mode} n={n_points:<6d} levels {n_alt:<5d} peak {peak:<5d} F {freq.size} regime {reg.tolist()} "
                  f"restatement err {worst:.2e} ({worst / e26[mode]:.2f} x g26 e_ref)")
    if only:
        return
    assert seen["valley_tall"] and seen["escape"] and seen["skipped_terms"] and seen["nan_trace"] and seen["unmag_by_nanmax"], seen
    out["own_e_ref"] = np.array(own, dtype="U16")
    out["limits"] = limits
    out["e_ref28_O"] = np.array(e28["O"])
    out["e_ref28_X"] = np.array(e28["X"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", seen, "e_ref28", e28, "own e_ref:", own, f"{time.time() - t0:.0f} s")
    assert os.path.getsize(OUT) < 400_000


if __name__ == "__main__":
    main()
