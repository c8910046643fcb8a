"""The region of the panel sum under option panel_upper restated in NumPy on the model of
test_panel_cut_host, which is imported and not edited: no GPU.  This model is the specification of what the option adds
to the panel block of lean_loop_body.

1. The upper end.  With the option on, the region of a pair with three top segments may end at
   E_up = (first point of the top segment + 4) & ~63 instead of test_panel_sum_host.region_of's end below the third
   segment from the top.  First points are the panel sum's own: the first i with (int)(m_i kj) >= j.  The cuts do not
   change: the new runs are the whole of segments j_top - 2 and j_top - 1 and, where E_up lies above it, the top
   segment's first one to four points.
2. The decision, per pair, before any of them is summed: the runs of [first point of segment j_top - 3, E_up) - those
   whose extent is the upper region's, segment j_top - 3 reaching to its end and not to today's region end - are put to
   the tests every run passes - 1 - X - Y >= 1e-6 at both levels and |i_sing - centre| >= max(32, 4 n) for every base
   piece of more than eight points, at most 128 entries at the run's level s.  Where all pass, the region ends at E_up
   and only the top segment keeps its strided sum; where one fails, the pair keeps the lower region and the strided sums
   of all three top segments ("kept the lower region").  It does not fall back as a whole on that account, so the pairs
   that fall back as a whole are those of the present cuts.
3. Everything else - base pieces, levels, parts, nodes, lists - is test_panel_cut_host.cut_virtual_heights, which also
   asserts for every part of more than four points, those of the upper runs included, the far test for its own centre
   and length.

Bounds: 2e-12 of the virtual height against the oracle (the sibling host tests' bound); per row at most twice the
present cuts' error; on G14 rows 0-3 at every 4th frequency fewer than 700 lane slots and 11.5 evaluation iterations
per pair, list passes within 0.05 of the present cuts', no more pairs falling back than under the present cuts, at most
4 of 111 pairs keeping the lower region; on the plateau rows some pair, not all, keeps the lower region.  Each test
prints its figures."""

import numpy as np
import pytest
from unittest import mock

from conftest import load_golden
from oracle import vfo_numpy as orc
import test_panel_cut_host as cut
import test_strided_sum_host as tss
from test_panel_cut_host import LIST_ENTRIES, base_pieces, cut_virtual_heights, report, runs_of
from test_panel_nodes_host import D_FAR, LOG2E
from test_panel_sum_host import TAU
from test_strided_sum_host import C0, index_of, plateau_inputs, worst


def upper_end(seg):
    """E_up and the first point of the segment three below the top one, by the panel sum's own membership."""
    j_top = int(seg[-1])
    return (int(np.argmax(seg >= j_top)) + 4) & ~63, int(np.argmax(seg >= j_top - 3))


def upper_runs_pass(seg, s_p, cond, alt_b, span, n_points):
    """The decision of one pair: every run of [first point of segment j_top - 3, E_up) - the runs whose extent is the
    upper region's: segment j_top - 3 no longer ends at today's end - passes the runs' tests."""
    step = alt_b[1] - alt_b[0]
    e_up, lo3 = upper_end(seg)
    for p, n, j in runs_of(seg, max(lo3, s_p), e_up):
        jj = min(j + 1, alt_b.size - 1)
        slope = (cond[jj] - cond[j]) / step * span
        g_lo, g_hi = 1.0 - cond[j], 1.0 - cond[jj]
        levels_ok = g_lo >= TAU and g_hi >= TAU
        gap = g_lo + slope * (alt_b[j] - alt_b[0]) / span
        i_sing = index_of(gap / slope, n_points) if abs(slope) > 1e-300 else None
        k, L, pieces = base_pieces(p, n)
        for p_b, n_b in pieces:
            if n_b > 8:
                if not levels_ok:
                    return False
                if i_sing is not None and abs(i_sing - (p_b + 0.5 * (n_b - 1))) < max(32.0, 4.0 * n_b):
                    return False
        s = 0
        while True:
            n_s = -(-L >> s)
            centre = (p + n - 1) - 0.5 * (n_s - 1) if slope >= 0 else p + 0.5 * ((L >> s) - 1)
            i_far = centre + np.copysign(D_FAR * n_s + 2, slope)
            e_far = float(np.exp2(np.float32(-i_far * (10.0 / (n_points - 1) * LOG2E))))
            if n_s <= 4 or (levels_ok and (1.0 + C0) * slope - gap <= slope * ((1.0 + C0) * e_far)):
                break
            s += 1
        if k << s > LIST_ENTRIES:
            return False
    return True


def decision_of(cap, den_b, bmag_b, alt_b, mult, n_points):
    """One frequency: None where the pair has no panel region, else whether its region reaches the top segment."""
    if not np.isfinite(cap["vh"][0]):
        return None
    f_hz = cap["freq"][0, 0]
    span = cap["crit_height"][0, 0] - alt_b[0]
    kj = span / (alt_b[1] - alt_b[0])
    top = tss.top_runs(cap["alt"][0], alt_b, n_points)
    if len(top) != 3:
        return None
    seg = (mult * kj).astype(int)
    region = cut.region_of(mult, seg, kj, top[2][1], n_points, cut.B, cut.MIN_SEGMENT)
    if region is None:
        return None
    cond = orc.ratio_X(den_b, f_hz) + orc.ratio_Y(f_hz, bmag_b)
    return upper_runs_pass(seg, region[0], cond, alt_b, span, n_points)


def upper_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points, stats=None):
    """X-mode virtual heights of one profile under option panel_upper, and the oracle's: (got, want).  One frequency at
    a time, so that the pair's decision is handed to the patched pieces of the model as it is."""
    stats = {} if stats is None else stats
    freq_mhz = np.asarray(freq_mhz, dtype=float)
    got, want = np.full(freq_mhz.size, np.nan), np.full(freq_mhz.size, np.nan)
    real_region_of, real_top_runs, real_strided = cut.region_of, tss.top_runs, cut.strided_virtual_heights
    with np.errstate(all="ignore"):
        den_b, bmag_b, _, alt_b = orc.bottomside(den, bmag, bpsi, alt)
        mult = orc.stretch_multiplier(n_points)
    eligible_grid = (n_points >= 8192 and cut.grid_bits(mult) == 0
                     and np.unique(np.round(np.diff(alt_b), 9)).size == 1)
    for f in range(freq_mhz.size):
        one = freq_mhz[f:f + 1]
        with np.errstate(all="ignore"):
            cap = orc.stage_capture(one, den, bmag, bpsi, alt, "X", n_points)
            up = decision_of(cap, den_b, bmag_b, alt_b, mult, n_points) if eligible_grid else None

        def region_of(mult_, seg, kj, lo2, n, block, min_segment, up=up):
            region = real_region_of(mult_, seg, kj, lo2, n, block, min_segment)
            return region if region is None or not up else (region[0], upper_end(seg)[0])

        def top_runs(z, alt_b_, n, up=up):
            runs = real_top_runs(z, alt_b_, n)
            return runs[:1] if up else runs

        def strided_virtual_heights(*a, **k):                    # (the whole-pair fall-back keeps its three segments)
            with mock.patch.object(tss, "top_runs", top_runs):
                return real_strided(*a, **k)

        took = stats.get("took", 0)
        with mock.patch.object(orc, "stage_capture", lambda *a, cap=cap, **k: cap), \
                mock.patch.object(cut, "region_of", region_of), \
                mock.patch.object(cut, "strided_virtual_heights", strided_virtual_heights):
            g, w = cut_virtual_heights(one, den, bmag, bpsi, alt, n_points, stats=stats)
        got[f], want[f] = g[0], w[0]
        if up is not None:
            stats["eligible"] = stats.get("eligible", 0) + 1
            stats["kept_lower"] = stats.get("kept_lower", 0) + (0 if up else 1)
            if stats.get("took", 0) > took:                      # (what prhf_panel_upper_counters' second word counts)
                stats["kept_lower_took"] = stats.get("kept_lower_took", 0) + (0 if up else 1)
    return got, want


def summary(stats):
    return f"{report(stats)}; {stats.get('kept_lower', 0)} of {stats.get('eligible', 0)} kept the lower region"


@pytest.fixture(scope="module")
def g14():
    """Per G14 row 0-3 at every 4th frequency and 20 000 points: (error with the upper region, of the present cuts),
    and the counts of both."""
    g = load_golden("g14_config4_rows.npz")
    freq = g["freq"][::4]
    s_up, s_now, rows = {}, {}, []
    for r in range(4):
        args = (freq, g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"], 20000)
        got, want = upper_virtual_heights(*args, stats=s_up)
        now, want_now = cut_virtual_heights(*args, stats=s_now)
        rows.append((worst(got, want), worst(now, want_now)))
    return rows, s_up, s_now


def test_upper_region_on_config4_rows(g14):
    rows, s_up, s_now = g14
    for r, (err, err_now) in enumerate(rows):
        print(f"G14 row {r}: upper region {err:.2e}, present cuts {err_now:.2e}")
        assert err <= 2e-12
        assert err <= 2.0 * err_now
    print("upper region:", summary(s_up))
    print("present cuts:", report(s_now))
    assert s_up["pairs"] == s_now["pairs"] == s_up["eligible"] == 111
    assert s_up["slots"] / s_up["took"] < 700
    assert s_up["iters"] / s_up["took"] < 11.5
    assert abs(s_up["passes"] / s_up["took"] - s_now["passes"] / s_now["took"]) <= 0.05
    assert s_up.get("fell_back", 0) <= s_now.get("fell_back", 0)
    assert s_up["kept_lower"] <= 4


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_upper_region_on_plateau_vacuum_and_no_field_rows(n_points):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    s_up, s_now = {}, {}
    for r in (0, 5, 7, 9, 12, 25):
        got, want = upper_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points, stats=s_up)
        now, want_now = cut_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points, stats=s_now)
        err, err_now = worst(got, want), worst(now, want_now)
        print(f"plateau row {r} at {n_points}: upper region {err:.2e}, present cuts {err_now:.2e}")
        assert err <= 2e-12
        assert err <= 2.0 * err_now
    print("upper region:", summary(s_up))
    print("present cuts:", report(s_now))
    assert s_up.get("fell_back", 0) == s_now.get("fell_back", 0)
    assert 0 < s_up["kept_lower"] < s_up["eligible"]


# pairs of plateau rows 5-9 that take the panel sum and keep the lower region: what tests/test_gpu_panel_upper.py expects of
# prhf_panel_upper_counters' second word
GPU_ROWS_KEPT = {8192: 2, 20000: 2}


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_rows_of_the_gpu_test_keep_the_lower_region_somewhere(n_points):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    stats = {}
    for r in range(5, 10):
        upper_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points, stats=stats)
    print(f"plateau rows 5-9 at {n_points}: {stats['kept_lower']} of {stats['eligible']} eligible pairs keep the lower "
          f"region, {stats.get('kept_lower_took', 0)} of the {stats['took']} that take the panel sum")
    assert stats.get("kept_lower_took", 0) == GPU_ROWS_KEPT[n_points]
