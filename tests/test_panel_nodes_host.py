"""The two classes of piece of the panel sum (option panel_nodes = 4) restated in NumPy on the model of
test_panel_sum_host, whose region, pieces and pair-level guard are unchanged: no GPU.

A piece [p, p + n) inside segment j takes FOUR lanes where it holds at most four points (its own points) or where the
kernel's logarithm-free test places the index at which the segment's continuation reaches X + Y = 1 at least
D n + 2 indices from the piece's centre c = p + (n - 1) / 2.  On the continuation 1 - X - Y = gap - sl m, and the
stretch has 1 - m_i + c0 = (1 + c0) exp(-10 i / (N - 1)), so with one single-precision exp2 per piece the test is

    1 - X - Y >= 1e-6 at both levels of the segment,
    (1 + c0) sl - gap <= sl (1 + c0) exp(-10 (c +- (D n + 2)) / (N - 1)),      + where sl >= 0, - where sl < 0

(X + Y = 1 lies above the segment where sl > 0, below it where sl < 0: multiplied by sl, both inequalities read the
same; the two spare indices cover the single-precision exponential, worth 0.002 of an index).  Such a piece of more
than four points is summed from the four nodes of the Gauss rule of the counting measure on its n points
(pyrayhf_amd/csrc/prhf_panel4_table.inc, tools/gen_panel4_table.py): exact for the discrete sum of every polynomial of
degree 7, like the eight-node rule.  Every other piece takes EIGHT lanes as before: its own points up to eight, the
eight Gauss-Legendre nodes above that.  Pieces of 5 .. 8 points that pass the test take the four nodes too (chosen on
this model: the errors below do not move).  D = 16.

Bounds: 2e-12 of the virtual height against the oracle, the bound of the strided host tests; and per row at most twice
the eight-node model's error, because the class test is there so that accuracy does not move.  Lane slots of the region
per pair on the G14 rows: at most 800 (the eight-node rule has 1 292).  Each test prints its figures."""

import os

import numpy as np
import pytest
from unittest import mock

from conftest import load_golden
from oracle import vfo_numpy as orc
from test_panel_sum_host import B, MIN_SEGMENT, OFF, TAU, W, pieces_of, region_of
from test_strided_lower_host import grid_bits, lower_virtual_heights
from test_strided_sum_host import C0, index_of, plateau_inputs, strided_virtual_heights, top_runs, worst

LOG2E = 1.4426950408889634
D_FAR = 16                      # the class test's distance, in piece lengths
TABLE4 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyrayhf_amd", "csrc",
                      "prhf_panel4_table.inc")


def load_table4():
    """(node offsets OFF4[n][4], weights W4[n][4] for n = 0 .. 128) as the kernel includes them."""
    rows = []
    with open(TABLE4) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(("0x", "-0x")):
                rows.append([float.fromhex(v) for v in line.rstrip(",").split(", ")])
    pairs = np.array(rows)
    assert pairs.shape == (129, 8)
    return pairs[:, 0::2], pairs[:, 1::2]


OFF4, W4 = load_table4()


def two_class_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points, d_far=D_FAR, stats=None):
    """X-mode virtual heights of one profile by the two-class rule and by the eight-node rule, and the oracle's:
    (got4, got8, want).  The pair-level guard and its fallback are test_panel_sum_host's."""
    stats = {} if stats is None else stats
    with np.errstate(all="ignore"):
        cap = orc.stage_capture(freq_mhz, den, bmag, bpsi, alt, "X", n_points)
        with mock.patch.object(orc, "stage_capture", lambda *a, **k: cap):
            got, want = strided_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points)
            fallback, _ = lower_virtual_heights(freq_mhz, den, bmag, bpsi, alt, n_points)
        den_b, bmag_b, bpsi_b, alt_b = orc.bottomside(den, bmag, bpsi, alt)
        mult = orc.stretch_multiplier(n_points)
        if n_points < 8192 or grid_bits(mult) != 0 or np.unique(np.round(np.diff(alt_b), 9)).size > 1:
            return fallback, fallback.copy(), want
        got4, got8 = got, got.copy()
        c1 = -np.expm1(-10.0 / (n_points - 1))
        step = alt_b[1] - alt_b[0]
        for f in range(want.size):
            if not np.isfinite(want[f]):
                continue
            f_hz = cap["freq"][f, 0]
            span = cap["crit_height"][f, 0] - alt_b[0]
            kj = span / step
            runs = top_runs(cap["alt"][f], alt_b, n_points)
            region = None
            if len(runs) == 3:
                seg = (mult * kj).astype(int)
                region = region_of(mult, seg, kj, runs[2][1], n_points, B, MIN_SEGMENT)
            if region is None:
                got4[f] = got8[f] = fallback[f]
                continue
            s_p, e_p = region
            stats["pairs"] = stats.get("pairs", 0) + 1
            pieces = pieces_of(seg, s_p, e_p, B)
            cond = orc.ratio_X(den_b, f_hz) + orc.ratio_Y(f_hz, bmag_b)
            clear = True
            nodes = {4: ([], [], []), 8: ([], [], [])}           # m, w, j of the two rules
            slots = big = big4 = 0

            def m_lo(j):
                return (alt_b[j] - alt_b[0]) / span

            def own_points(p, n, j, into):
                idx = np.arange(p, p + n)
                into[0].append(mult[idx])
                into[1].append(c1 * ((1.0 - mult[idx]) + C0))
                into[2].append(np.full(n, j))

            def from_table(p, n, j, off, wgt, into):
                x_k = p + off[n]
                assert p < x_k[0] and x_k[-1] < p + n - 1
                i0 = np.rint(x_k).astype(int)
                e_k = ((1.0 - mult[i0]) + C0) * np.exp(-10.0 * (x_k - i0) / (n_points - 1))
                into[0].append((1.0 + C0) - e_k)
                into[1].append(wgt[n] * (c1 * e_k))
                into[2].append(np.full(x_k.size, j))

            for p, n, j in pieces:
                jj = min(j + 1, alt_b.size - 1)
                slope = (cond[jj] - cond[j]) / step * span
                g_lo, g_hi = 1.0 - cond[j], 1.0 - cond[jj]
                levels_ok = g_lo >= TAU and g_hi >= TAU
                centre = p + 0.5 * (n - 1)
                # 1 - m + c0 at the index D n + 2 from the centre, on the side where the continuation heads for X + Y = 1,
                # by the stretch's closed form and a single-precision exp2
                i_far = centre + np.copysign(d_far * n + 2, slope)
                e_far = float(np.exp2(np.float32(-i_far * (10.0 / (n_points - 1) * LOG2E))))
                far = levels_ok and (1.0 + C0) * slope - (g_lo + slope * m_lo(j)) <= slope * ((1.0 + C0) * e_far)
                # the eight-node rule, as test_panel_sum_host has it
                if n <= 8:
                    own_points(p, n, j, nodes[8])
                else:
                    from_table(p, n, j, OFF, W, nodes[8])
                    ok = levels_ok
                    if abs(slope) > 1e-300:
                        m_sing = (alt_b[j] - alt_b[0]) / span + g_lo / slope
                        i_sing = index_of(m_sing, n_points)
                        ok = ok and abs(i_sing - (p + 0.5 * (n - 1))) >= max(32.0, 4.0 * n)
                        if far:                                  # what the test claims holds
                            assert abs(i_sing - (p + 0.5 * (n - 1))) >= d_far * n
                    clear = clear and ok
                    big += 1
                # the two classes
                if n <= 4:
                    own_points(p, n, j, nodes[4])
                    slots += 4
                elif far:
                    from_table(p, n, j, OFF4, W4, nodes[4])
                    slots += 4
                    big4 += n > 8
                else:
                    if n <= 8:
                        own_points(p, n, j, nodes[4])
                    else:
                        from_table(p, n, j, OFF, W, nodes[4])
                    slots += 8
            if not clear:
                stats["fell_back"] = stats.get("fell_back", 0) + 1
                got4[f] = got8[f] = fallback[f]
                continue
            terms = cap["mup"][f] * cap["dist"][f]
            base = got[f] - terms[s_p:e_p].sum()
            for k, out in ((4, got4), (8, got8)):
                m_k, w_k, j_k = (np.concatenate(v) for v in nodes[k])
                # every node lies inside its own segment, by the kernel's own membership
                assert np.array_equal((m_k * kj).astype(int), j_k), (f, k)
                z = m_k * span + alt_b[0]
                X = orc.ratio_X(np.interp(z, alt_b, den_b), f_hz)
                Y = orc.ratio_Y(f_hz, np.interp(z, alt_b, bmag_b))
                _, mup = orc.phase_group_index(X, Y, np.interp(z, alt_b, bpsi_b), "X")
                out[f] = base + np.sum(mup * w_k) * span
            stats["took"] = stats.get("took", 0) + 1
            stats["slots"] = stats.get("slots", 0) + slots
            stats["slots8"] = stats.get("slots8", 0) + 8 * len(pieces)
            stats["big"] = stats.get("big", 0) + big
            stats["big4"] = stats.get("big4", 0) + big4
        return got4, got8, want


def test_table():
    """What tools/gen_panel4_table.py asserts, on the doubles the kernel reads."""
    for n in range(5, 129):
        x, w = OFF4[n], W4[n]
        assert abs(w.sum() - n) <= 1e-13 * n
        assert (w > 0).all() and (x > 0).all() and (x < n - 1).all() and (np.diff(x) > 0).all()
        half = 0.5 * (n - 1)
        tau = (np.arange(n) - half) / max(half, 1.0)
        for d in range(8):
            assert abs(w @ ((x - half) / max(half, 1.0)) ** d - np.sum(tau ** d)) <= 1e-13 * n, (n, d)
        # the closed form: roots of t^4 - (3 n^2 - 13) / 14 t^2 + 3 (n^2 - 1) (n^2 - 9) / 560
        t = x - half
        poly = t ** 4 - (3 * n * n - 13) / 14 * t ** 2 + 3 * (n * n - 1) * (n * n - 9) / 560
        assert np.max(np.abs(poly)) <= 1e-12 * half ** 4
    for n in range(5):
        assert np.array_equal(W4[n], (np.arange(4) < n).astype(float))
        assert np.array_equal(OFF4[n], np.where(np.arange(4) < n, np.arange(4.0), 0.0))


def test_two_classes_on_config4_rows():
    g = load_golden("g14_config4_rows.npz")
    freq = g["freq"][::4]
    stats = {}
    for r in range(4):
        got4, got8, want = two_class_virtual_heights(freq, g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"], 20000,
                                                     stats=stats)
        err4, err8 = worst(got4, want), worst(got8, want)
        print(f"G14 row {r}: two classes {err4:.2e}, eight nodes {err8:.2e}")
        assert err4 <= 2e-12
        assert err4 <= 2.0 * err8
    slots, slots8 = stats["slots"] / stats["took"], stats["slots8"] / stats["took"]
    print(f"{stats['pairs']} pairs with a region, {stats.get('fell_back', 0)} fell back; lane slots of the region per "
          f"pair {slots:.0f} (eight nodes: {slots8:.0f}); {stats['big4']} of {stats['big']} pieces of more than 8 points "
          f"take four nodes ({stats['big4'] / stats['big']:.1%})")
    assert (stats["pairs"], stats.get("fell_back", 0)) == (111, 1)          # the eight-node model's counts
    assert slots <= 800


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_two_classes_on_plateau_vacuum_and_no_field_rows(n_points):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    stats = {}
    for r in (0, 5, 7, 9, 12, 25):
        got4, got8, want = two_class_virtual_heights(freq, den[r], bmag[r], bpsi[r], alt, n_points, stats=stats)
        err4, err8 = worst(got4, want), worst(got8, want)
        print(f"plateau row {r} at {n_points}: two classes {err4:.2e}, eight nodes {err8:.2e}")
        assert err4 <= 2e-12
        assert err4 <= 2.0 * err8
    print(f"{stats.get('fell_back', 0)} of {stats['pairs']} pairs kept the sum of before; "
          f"{stats['big4']} of {stats['big']} pieces of more than 8 points take four nodes")
    assert (stats["pairs"], stats.get("fell_back", 0)) == {8192: (522, 96), 20000: (524, 105)}[n_points]
