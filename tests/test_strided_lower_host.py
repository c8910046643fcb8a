"""The strided sum of the segments below the top three (option strided_lower) restated in NumPy on
the oracle's own terms, with the kernel's choice of the region R, its boundaries and its guard written out
(lean_loop_body): no GPU.  The top three segments are test_strided_sum_host's rule, unchanged.

R is the run of consecutive segments directly below the top three that hold at least MIN_SEGMENT points each, cut
to [S_R, E_R), multiples of 64.  Segment j begins at the real-valued index x_j of the stretch's closed form; around
the boundary x of two segments b = 8 floor((x - 4.5) / 8) is the last strided point of the lower one and
a = 8 ceil((x + 4.5) / 8) the first of the upper one.  `rule_coefficients` below is the definition of the rule: per
segment the Euler-Maclaurin sum over [a, b], one by one between a b and the next a and from E_R - 7 on.
`two_pass_coefficients` is the kernel's form of the same thing - every multiple of 8 weighted by 8, then per
boundary a 32-point vector of coefficients - and must give every grid point the same coefficient.

Bounds: 2e-12 of the virtual height, test_strided_sum_host's bound (8.2e-14 measured on the G14 rows, 1.1e-13 on the
plateau rows); the share of point slots that are still evaluated must stay below 0.33 on the G14 rows (0.300 with
the rule as stated, 0.459 with the top three segments alone; a boundary counts as 32 lane slots).  Without the
guard's fallback, plateau row 7 at 8192 points must miss by more than 1e-10 and row 5 at 20 000 by more than 1e-8:
the guard is what makes them pass."""

from unittest import mock

import numpy as np
import pytest

from conftest import load_golden
from oracle import vfo_numpy as orc
from test_strided_sum_host import index_of, plateau_inputs, strided_virtual_heights, top_runs, width, worst

S = 8
GUARD = 256
TAU = 1e-6
MARGIN = 4.5
MIN_SEGMENT = 64                # PRHF_STRIDED_MIN_SEGMENT
MIN_REGION = 256                # E_R - S_R at least
D1 = np.array([-1 / 60, 3 / 20, -3 / 4, 0.0, 3 / 4, -3 / 20, 1 / 60])
D3 = np.array([1 / 8, -1.0, 13 / 8, 0.0, -13 / 8, 1.0, -1 / 8])
MAG = {0: 0.0, 1: 13.1796875, 2: -6.475, 3: 0.7984375}     # (s^2-1)/12 D1[3+q] - (s^4-1)/720 D3[3+q], q = 1, 2, 3


def grid_bits(m):
    """The header word of grid_strided_kernel: bit 0, a width deviates from the stretch's by more than 1e-14; bit 1,
    the stretch's origin (m_0 = 0, m_N-1 = 1) does not hold."""
    n = m.size
    bad = not np.all(np.abs(np.diff(m) - width(m[:-1], n)) <= 1e-14)
    origin = abs(m[0]) <= 1e-14 and abs(m[-1] - 1.0) <= 1e-14
    return int(bad) | (0 if origin else 2)


def lower_region(x, lo2, min_segment=MIN_SEGMENT):
    """x[l], l = 0, 1, ..: where segment j_b0 - l begins (closed form; x[0] belongs to the lowest of the top three
    segments, whose first point in the table is lo2).  Returns S_R, E_R, the boundaries inside R (top first) and
    R's segments as (a, b), top first - or None."""
    n_0 = 0
    while n_0 + 1 < len(x) and n_0 < 62 and x[n_0] - x[n_0 + 1] >= min_segment:
        n_0 += 1
    a_gen = [8 * int(np.ceil((x[l + 1] + MARGIN) / 8)) for l in range(n_0)]
    b_gen = [8 * int(np.floor((x[l] - MARGIN) / 8)) for l in range(n_0)]
    s_l = [64 * int(np.ceil((x[l + 1] + MARGIN) / 64)) for l in range(n_0)]
    e_l = [((lo2 + 4) & ~63) if l == 0 else 64 * int(np.floor((x[l] + 3.5) / 64)) for l in range(n_0)]
    tops = [l for l in range(n_0) if a_gen[l] + 16 <= e_l[l]]
    if not tops:
        return None
    l_top = tops[0]
    bots = [l for l in range(l_top, n_0) if s_l[l] + 8 <= b_gen[l]]
    if not bots:
        return None
    l_bot = bots[-1]
    s_r, e_r = s_l[l_bot], e_l[l_top]
    if e_r - s_r < MIN_REGION or abs(x[0] - lo2) >= 1.5:
        return None
    segs = [(s_r if l == l_bot else a_gen[l], e_r - 8 if l == l_top else b_gen[l]) for l in range(l_top, l_bot + 1)]
    return s_r, e_r, [x[l] for l in range(l_top + 1, l_bot + 1)], segs, l_top


def segment_clear(a, b, n_points, m_sing, dm, const_gap):
    """Guards (1) and (2) of one segment of R: no strided or stencil point (a-3 .. b+3) within GUARD indices of the
    point where the segment's continuation reaches X + Y = 1, none where 1 - X - Y < TAU."""
    if m_sing is None:
        return abs(const_gap) >= TAU
    i_sing = index_of(m_sing, n_points)
    below = np.floor(min(i_sing - (GUARD + 1), index_of(m_sing - dm, n_points)))
    above = np.ceil(max(i_sing + (GUARD + 1), index_of(m_sing + dm, n_points)))
    return b + 3 <= below or a - 3 >= above


def rule_coefficients(s_r, e_r, segs):
    """The definition: coefficient of every grid point of [s_r - 3, e_r), as an array indexed from s_r - 3."""
    c = np.zeros(e_r - (s_r - 3))
    at = lambda i: i - (s_r - 3)                            # noqa: E731
    c[at(s_r):] = 1.0                                       # one by one ...
    for a, b in segs:                                       # ... except [a, b] of every segment
        c[at(a):at(b) + 1] = 0.0
        c[at(a):at(b) + 1:S] += S
        c[at(a)] -= (S - 1) / 2
        c[at(b)] -= (S - 1) / 2
        c[at(b) - 3:at(b) + 4] -= (S * S - 1) / 12 * D1
        c[at(a) - 3:at(a) + 4] += (S * S - 1) / 12 * D1
        c[at(b) - 3:at(b) + 4] += (S ** 4 - 1) / 720 * D3
        c[at(a) - 3:at(a) + 4] -= (S ** 4 - 1) / 720 * D3
    return c                                                # (s_r - 3 .. s_r - 1: the correction only - the ordinary
                                                            #  steps below R add their own 1)


def around(p, pa):
    """The kernel's coefficient of point b - 3 + p around a boundary whose a sits at p == pa."""
    if p < 3:
        return MAG[3 - p]
    if p == 3:
        return -3.5
    if p <= 6:
        return 1.0 - MAG[p - 3]
    if p < pa - 3:
        return -7.0 if (p & 7) == 3 else 1.0
    if p < pa:
        return 1.0 - MAG[pa - p]
    if p == pa:
        return -3.5
    return MAG.get(p - pa, 0.0)


def two_pass_coefficients(s_r, e_r, boundaries):
    """The kernel's form: pass 1 weighs every multiple of 8 in [s_r, e_r) by 8, pass 2 adds a 32-point vector per
    boundary and one for the two ends of R."""
    c = np.zeros(e_r - (s_r - 3))
    at = lambda i: i - (s_r - 3)                            # noqa: E731
    c[at(s_r)::S] += S
    for x in boundaries:
        b, a = 8 * int(np.floor((x - MARGIN) / 8)), 8 * int(np.ceil((x + MARGIN) / 8))
        assert a - b in (16, 24)
        for p in range(32):
            c[at(b - 3 + p)] += around(p, a - b + 3)
    for p in range(18):
        if p < 7:
            c[at(s_r - 3 + p)] += -MAG[3 - p] if p < 3 else (-3.5 if p == 3 else MAG[p - 3])
        else:
            c[at(e_r - 18 + p)] += around(p - 7, 64)
    return c


def lower_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points, guard=True, min_segment=MIN_SEGMENT, stats=None,
                          checks=None):
    """X-mode virtual heights of one profile: the top three segments by test_strided_sum_host's rule, R by the rule
    above, everything else the oracle's own sum."""
    top_stats = {}
    with np.errstate(all="ignore"):
        cap = orc.stage_capture(freq_mhz, den, bmag, bpsi, alt, "X", n_points)
        # (the stages are the slow part: test_strided_sum_host's rule reads the ones captured here)
        with mock.patch.object(orc, "stage_capture", lambda *a, **k: cap):
            got, want = strided_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points, stats=top_stats)
        den_b, bmag_b, _, alt_b = orc.bottomside(den, bmag, bpsi, alt)
        mult = orc.stretch_multiplier(n_points)
        if n_points < 8192 or grid_bits(mult) != 0 or np.unique(np.round(np.diff(alt_b), 9)).size > 1:
            return got, want
        w = width(mult, n_points)
        skipped = 0
        for f in range(want.size):
            if not np.isfinite(want[f]):
                continue
            f_hz = cap["freq"][f, 0]
            span = cap["crit_height"][f, 0] - alt_b[0]
            terms = cap["mup"][f] * cap["dist"][f]
            g = cap["mup"][f] * (w * span)
            runs = top_runs(cap["alt"][f], alt_b, n_points)
            if len(runs) != 3:
                continue
            j_b0, lo2 = runs[2][0], runs[2][1]
            x = [index_of((alt_b[j] - alt_b[0]) / span, n_points) for j in range(j_b0, -1, -1)]
            region = lower_region(x, lo2, min_segment)
            if region is None:
                continue
            s_r, e_r, boundaries, segs, l_top = region
            cond = orc.ratio_X(den_b, f_hz) + orc.ratio_Y(f_hz, bmag_b)
            clear = True
            if checks is not None:
                seg = np.searchsorted(alt_b, cap["alt"][f], side="right") - 1      # non-decreasing
            for k, (a, b) in enumerate(segs):
                j = j_b0 - 1 - l_top - k
                slope = (cond[j + 1] - cond[j]) / (alt_b[j + 1] - alt_b[j]) * span
                m_sing = dm = None
                if abs(slope) > 1e-300:
                    m_sing = (alt_b[j] - alt_b[0]) / span + (1.0 - cond[j]) / slope
                    dm = TAU / abs(slope)
                clear = clear and segment_clear(a, b, n_points, m_sing, dm, 1.0 - cond[j])
                if checks is not None:
                    first, last = int(np.searchsorted(seg, j)), int(np.searchsorted(seg, j + 1)) - 1
                    assert a - 3 >= first and b + 3 <= last, (f, j, a, b, first, last)
                    assert abs(x[l_top + k + 1] - first) < 1.0 and abs(x[l_top + k] - (last + 1)) < 1.0
                    checks["segments"] = checks.get("segments", 0) + 1
            if checks is not None:
                c_rule, c_kernel = rule_coefficients(s_r, e_r, segs), two_pass_coefficients(s_r, e_r, boundaries)
                assert np.max(np.abs(c_rule - c_kernel)) <= 1e-14
            if stats is not None:
                stats["pairs"] = stats.get("pairs", 0) + 1
            if guard and not clear:
                if stats is not None:
                    stats["fell_back"] = stats.get("fell_back", 0) + 1
                continue
            c = rule_coefficients(s_r, e_r, segs)
            got[f] += c @ g[s_r - 3:e_r] - terms[s_r:e_r].sum()
            skipped += (e_r - s_r) - ((e_r - s_r) // S + 32 * len(segs))
        if stats is not None:
            stats["skipped"] = stats.get("skipped", 0) + top_stats.get("skipped", 0) + skipped
            stats["points"] = stats.get("points", 0) + top_stats.get("points", 0)
        return got, want


def test_rule_on_config4_rows():
    g = load_golden("g14_config4_rows.npz")
    freq = g["freq"][::4]
    stats, checks = {}, {}
    for r in range(4):
        got, want = lower_virtual_heights(freq, g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"], 20000, stats=stats,
                                          checks=checks)
        err = worst(got, want)
        print(f"G14 row {r}: {err:.2e}")
        assert err <= 2e-12
    share = 1.0 - stats["skipped"] / stats["points"]
    print(f"share of point slots evaluated: {share:.3f}; {stats['pairs']} pairs with a region, "
          f"{stats.get('fell_back', 0)} fell back, {checks['segments']} segments checked")
    assert share < 0.33
    assert stats["pairs"] > 50 and checks["segments"] > 500


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_rule_on_plateau_vacuum_and_no_field_rows(n_points):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    stats, checks = {}, {}
    for r in (0, 5, 7, 9, 12, 25):
        got, want = lower_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points, stats=stats, checks=checks)
        err = worst(got, want)
        print(f"plateau row {r} at {n_points}: {err:.2e}")
        assert err <= 2e-12
    print(f"{stats.get('fell_back', 0)} of {stats['pairs']} pairs kept the sum of before")
    assert 0 < stats.get("fell_back", 0) < stats["pairs"] // 4


@pytest.mark.parametrize("row, n_points, miss", [(7, 8192, 1e-10), (5, 20000, 1e-8)])
def test_guard_is_what_makes_the_plateau_rows_pass(row, n_points, miss):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    got, want = lower_virtual_heights(freq, den[row], bmag[row], bpsi[row], alt, n_points, guard=False)
    err = worst(got, want)
    print(f"row {row} at {n_points} without the guard's fallback: {err:.2e}")
    assert err > miss


def test_boundary_coefficients_are_the_rule():
    """Both spacings a - b, every residue of the boundary: the two-pass form gives each point the rule's coefficient."""
    for x0 in np.arange(1000.0, 1008.0, 0.25):
        x = [3000.2, 2400.0 + 0.3, x0 + 700.0, x0, 800.6, 600.1]
        region = lower_region(x, 3001)
        assert region is not None
        s_r, e_r, boundaries, segs, _ = region
        assert s_r % 64 == 0 and e_r % 64 == 0 and len(boundaries) == len(segs) - 1
        assert np.max(np.abs(rule_coefficients(s_r, e_r, segs) - two_pass_coefficients(s_r, e_r, boundaries))) <= 1e-14
        # a constant summand: the rule is exact, so the coefficients of [s_r, e_r) and the three corrections sum to its length
        assert abs(rule_coefficients(s_r, e_r, segs).sum() - (e_r - s_r)) <= 1e-10
    assert {8 * int(np.ceil((v + MARGIN) / 8)) - 8 * int(np.floor((v - MARGIN) / 8)) for v in np.arange(0, 8, 0.125)} == {16, 24}


def test_grid_check():
    for n in (8192, 20000):
        m = orc.stretch_multiplier(n)
        assert grid_bits(m) == 0
        assert grid_bits(m + 1e-6) & 2                      # a stretch shifted by m_0 = 1e-6: its origin is not the closed form's
        assert grid_bits(orc.stretch_multiplier(n, sharpness=5.0)) != 0
        assert grid_bits(np.linspace(0.0, 1.0, n)) != 0
