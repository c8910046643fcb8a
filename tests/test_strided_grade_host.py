"""The zones of the strided sum (option strided_grade) restated in NumPy on the oracle's own terms, with
the kernel's cuts written out (strided_zones in prhf_kernels.hip): no GPU.

The stretch [a, E) of a top segment that tests/test_strided_sum_host.py sums at stride 8 is cut at z2 <= z1, multiples
of 64: [a, z2] at stride 32, [z2, z1] at stride 16, [z1, b] at stride 8, b = E - 8.  z1 is the largest multiple of 64 that
is at most E - 64, at least 512 indices below the index i_sing where the segment's continuation reaches X + Y = 1, and
below which 1 - X - Y >= 1e-5; z2 the largest that is at most z1, at least 1024 below i_sing and below which
1 - X - Y >= 1.6e-4 (the end corrections' coefficients grow like s^4: 13, 164, 2431); then z2 - a is rounded down to a
multiple of 2048 and z1 - z2 to one of 1024, whole wave-iterations of 64 coarse points.  A segment with i_sing below it is not cut; where X + Y is constant the coarse
zones need |1 - X - Y| >= 1e-5 and 1.6e-4.  With EM the four-term Euler-Maclaurin rule of that module,

    sum_{i=a..b} g(i) = sum_k EM(p_k, p_k+1, s_k) - sum over the interior junctions of g(p_k).

Bound: 2e-12 of the virtual height, the bound of the stride-8 rule's own host test.  Measured here (worst per group):
G14 rows 0-3 8.2e-14, plateau rows at 8192 and 20 000 points 1.2e-13, the flat-layer pairs 1.9e-13 / 2.4e-13 / 1.5e-13
(row 8421 without the bound 8.3e-12, G14 row 0 without the junction terms 5.5e-07, lane slots 48.0 % of the plain rule's).
The same rule without the conditioning bound on the coarse strides must miss row 8421 by more than 1e-12, and without
the derivative terms at the junctions G14 row 0 by more than 1e-8: the terms under test are what makes it pass.  The
lane slots of the top three segments (every zone's 14 stencil points counted) must be fewer than half the plain
rule's on G14, so that a rule that never grades fails."""

import numpy as np

from conftest import load_golden
from oracle import vfo_numpy as orc
from test_strided_sum_host import (D1, D3, TAU, index_of, plateau_inputs, strided_bounds, top_runs, width, worst)

TAU_COARSE = 1e-5      # no point of stride 16 where 1 - X - Y is below this ...
TAU_32 = 16.0          # ... nor one of stride 32 where it is below this many times that (the end corrections grow like s^4)
NEAR = {16: 512, 32: 1024}


def zones(a, e, lo, q, begin, n_points, m_sing, dm_coarse, flat_gap, tau_coarse=TAU_COARSE):
    """[(p, p', stride)] of the stretch [a, E), coarsest first, as strided_zones cuts it."""
    z1 = z2 = a
    cap = e - 64
    graded = True
    if m_sing is not None:
        i_sing = index_of(m_sing, n_points)
        a0 = begin if begin >= lo + 3 else begin + 64
        if not 2.0 * i_sing >= a0 + q:
            graded = False
        else:
            lim1 = i_sing - NEAR[16]
            if tau_coarse > 0.0:
                lim1 = min(lim1, index_of(m_sing - dm_coarse, n_points))
            lim2 = i_sing - NEAR[32]
            if tau_coarse > 0.0:
                lim2 = min(lim2, index_of(m_sing - TAU_32 * dm_coarse, n_points))
            z1 = min(cap, int(np.floor(lim1)) & ~63)
            z2 = min(z1, int(np.floor(lim2)) & ~63)
    elif tau_coarse > 0.0 and not abs(flat_gap) >= tau_coarse:
        graded = False
    else:
        z1 = cap
        z2 = cap if abs(flat_gap) >= TAU_32 * tau_coarse else a
    if graded:
        # whole wave-iterations only: 64 points of stride 32, then 64 of stride 16
        z2 = a + (max(z2 - a, 0) & ~2047)
        z1 = z2 + (max(z1 - z2, 0) & ~1023)
    else:
        z1 = z2 = a
    out = [(p, p2, s) for p, p2, s in ((a, z2, 32), (z2, z1, 16), (z1, e - 8, 8)) if p2 > p]
    for p, p2, s in out:
        assert p % 64 == 0 and (p2 - p) % s == 0
        if s > 8 and m_sing is not None:
            assert p2 <= index_of(m_sing, n_points) - 32 * s
    return out


def em(g, p, p2, s, derivatives_at=(True, True)):
    """Euler-Maclaurin sum of g[p .. p2] from every s-th point; derivatives_at: the derivative terms at p and at p2."""
    rule = s * g[p:p2 + 1:s].sum() - (s - 1) / 2 * (g[p] + g[p2])
    for end, sign, on in ((p, 1.0, derivatives_at[0]), (p2, -1.0, derivatives_at[1])):
        if on:
            rule += sign * ((s * s - 1) / 12 * (D1 @ g[end - 3:end + 4]) - (s ** 4 - 1) / 720 * (D3 @ g[end - 3:end + 4]))
    return rule


def graded_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points, tau_coarse=TAU_COARSE, junction_terms=True,
                           stats=None):
    """X-mode virtual heights of one profile with the top segments summed zone by zone; everything else is the oracle's
    own sum."""
    with np.errstate(all="ignore"):
        cap = orc.stage_capture(freq_mhz, den, bmag, bpsi, alt, "X", n_points)
        den_b, bmag_b, _, alt_b = orc.bottomside(den, bmag, bpsi, alt)
        mult = orc.stretch_multiplier(n_points)
        w = width(mult, n_points)
        out = np.full(cap["vh"].shape, np.nan)
        for f in range(cap["vh"].size):
            if not np.isfinite(cap["vh"][f]):
                continue
            f_hz = cap["freq"][f, 0]
            span = cap["crit_height"][f, 0] - alt_b[0]
            terms = cap["mup"][f] * cap["dist"][f]
            g = cap["mup"][f] * (w * span)
            total = np.nansum(terms)
            cond = orc.ratio_X(den_b, f_hz) + orc.ratio_Y(f_hz, bmag_b)
            for j, lo, q, begin, _ in top_runs(cap["alt"][f], alt_b, n_points):
                slope = (cond[j + 1] - cond[j]) / (alt_b[j + 1] - alt_b[j]) * span
                m_sing = dm = dm_coarse = None
                if abs(slope) > 1e-300:
                    m_sing = (alt_b[j] - alt_b[0]) / span + (1.0 - cond[j]) / slope
                    dm = TAU / abs(slope)
                    dm_coarse = tau_coarse / abs(slope)
                elif not abs(1.0 - cond[j]) >= TAU:
                    continue
                ae = strided_bounds(lo, q, begin, n_points, m_sing, dm)
                if ae is None:
                    continue
                a, e = ae
                b = e - 8
                zs = zones(a, e, lo, q, begin, n_points, m_sing, dm_coarse, 1.0 - cond[j], tau_coarse)
                assert zs[0][0] == a and zs[-1][1] == b and zs[-1][2] == 8
                rule = 0.0
                for k, (p, p2, s) in enumerate(zs):
                    rule += em(g, p, p2, s, (junction_terms or k == 0, junction_terms or k == len(zs) - 1))
                    if k:
                        rule -= g[p]
                total += rule - terms[a:b + 1].sum()
                if stats is not None:
                    stats["plain"] = stats.get("plain", 0) + (b - a) // 8 + 1 + 14
                    stats["graded"] = stats.get("graded", 0) + sum((p2 - p) // s + 1 + 14 for p, p2, s in zs)
                    stats["coarse"] = stats.get("coarse", 0) + (len(zs) > 1)
                    stats["both"] = stats.get("both", 0) + (len(zs) == 3)
            out[f] = total + np.min(alt)
        return out, cap["vh"]


def test_zones_on_config4_rows():
    g = load_golden("g14_config4_rows.npz")
    freq = g["freq"][::4]
    stats = {}
    for r in range(4):
        got, want = graded_virtual_heights(freq, g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"], 20000, stats=stats)
        err = worst(got, want)
        print(f"G14 row {r}: {err:.2e}")
        assert err <= 2e-12
    share = stats["graded"] / stats["plain"]
    print(f"lane slots of the top three segments: {stats['graded']} against {stats['plain']} ({share:.3f}); "
          f"{stats['coarse']} stretches with a coarse zone")
    assert share < 0.49                                    # (0.480 measured; the issue asks for less than half)
    assert stats["both"] > 0                               # (the 32 | 16 junction is among what was summed)
    got, want = graded_virtual_heights(freq, g["den"][0], g["bmag"][0], g["bpsi"][0], g["alt"], 20000, junction_terms=False)
    miss = worst(got, want)
    print(f"G14 row 0 without the junctions' derivative terms: {miss:.2e}")
    assert miss > 1e-8


def test_zones_on_plateau_vacuum_and_no_field_rows():
    freq, alt, den, bmag, bpsi = plateau_inputs()
    for n_points in (8192, 20000):
        for r in (0, 5, 7, 9, 12, 25):
            got, want = graded_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points)
            err = worst(got, want)
            print(f"plateau row {r} at {n_points} points: {err:.2e}")
            assert err <= 2e-12


def test_conditioning_bound_on_nearly_flat_layers():
    """The pairs of test_strided_sum_host's conditioning test: with weights of 16 and 32 the bound on 1 - X - Y has to be
    ten times wider than the stride-8 rule's at stride 16 and 160 times wider at stride 32
    (TAU_COARSE, TAU_32: the end corrections' coefficients grow like s^4)."""
    from pyrayhf_amd import synth
    freq = np.linspace(0.5, 16.0, 256)
    for row, f in ((8421, 14), (107, 2), (10344, 14)):
        alt, den, bmag, bpsi = synth.chapman_profiles(100000, 20260004, rows=slice(row, row + 1))
        got, want = graded_virtual_heights(freq[f:f + 1], den[0], bmag[0], bpsi[0], alt, 20000)
        err = worst(got, want)
        print(f"row {row} at {freq[f]:.2f} MHz, {want[0]:.1f} km: {err:.2e}")
        assert err <= 2e-12
    alt, den, bmag, bpsi = synth.chapman_profiles(100000, 20260004, rows=slice(8421, 8422))
    got, want = graded_virtual_heights(freq[14:15], den[0], bmag[0], bpsi[0], alt, 20000, tau_coarse=0.0)
    miss = worst(got, want)
    print(f"row 8421 without the bound on the coarse strides: {miss:.2e}")
    assert miss > 1e-12


def test_the_kernels_coefficient_table_is_the_formulas():
    """kGradeCoef, the per-lane coefficients of a stretch with coarse zones (strided_run): lanes 0-6 around a, 7-17 around
    b and the ordinary points behind it, 18-24 around z1, 25-31 around z2; rows for the strides 32-16-8, 32-8 and 16-8.
    Every entry must be the formula's value to the last digit."""
    import os
    import re
    from fractions import Fraction as F
    src = open(os.path.join(os.path.dirname(__file__), "..", "pyrayhf_amd", "csrc", "prhf_kernels.hip")).read()
    body = re.search(r"kGradeCoef\[3 \* 32\] = \{(.*?)\};", src, re.S).group(1)
    got = [float(x) for x in body.replace("\n", " ").split(",") if x.strip()]
    assert len(got) == 96
    d1, d3 = (F(3, 4), F(-3, 20), F(1, 60)), (F(-13, 8), F(1), F(-1, 8))

    def mag(s, q):
        k = abs(q) - 1
        return (1 if q > 0 else -1) * (F(s * s - 1, 12) * d1[k] - F(s ** 4 - 1, 720) * d3[k])

    def at_a(s):
        return [F(1 - s, 2) if q == 0 else mag(s, q) for q in range(-3, 4)]

    def at_b():
        return [(F(-7, 2) if q == 0 else (-mag(8, q) if abs(q) <= 3 else F(0))) + (1 if q >= 1 else 0) for q in range(-3, 8)]

    def junction(left, right):
        return [F(left - right, 2) if q == 0 else mag(right, q) - mag(left, q) for q in range(-3, 4)]

    none = [F(0)] * 7
    want = (at_a(32) + at_b() + junction(16, 8) + junction(32, 16) + at_a(32) + at_b() + junction(32, 8) + none +
            at_a(16) + at_b() + junction(16, 8) + none)
    assert got == [float(x) for x in want]
    # the rule these coefficients implement, on a smooth summand: zones of 32, 16 and 8 against the plain sum
    i = np.arange(0, 8192, dtype=np.float64)
    g = np.exp(-i / 1500.0) * (1.0 + 0.1 * np.sin(i / 700.0))
    a, z2, z1, b = 64, 64 + 2048, 64 + 2048 + 1024, 64 + 2048 + 1024 + 504
    lanes = np.concatenate([np.arange(a - 3, a + 4), np.arange(b - 3, b + 8), np.arange(z1 - 3, z1 + 4), np.arange(z2 - 3, z2 + 4)])
    rule = (32 * g[a:z2:32].sum() + 16 * g[z2:z1:16].sum() + 8 * g[z1:b + 1:8].sum() + np.dot(got[:32], g[lanes]))
    exact = g[a:b + 8].sum()
    assert abs(rule - exact) <= 1e-12 * exact
