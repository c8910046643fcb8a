"""The quick bound of the panel sum's lists (option panel_quick) stated in NumPy, and the lists of the
panel block of lean_loop_body under option panel_upper as the kernel makes them: no GPU.  The exact rules of a run -
levels, guard, level s, at most 128 entries - are those of test_panel_cut_host and test_panel_upper_host, imported and
put to one run at a time; nothing of them is restated here.

The bound of one run [p, p + n) of segment j, with g_j and g_{j+1} = 1 - X - Y at the segment's two levels, sl =
(g_j - g_{j+1}) kj, L the points of the run's base pieces and D = 16 L + 10 (0 where L <= 4):

    g_j >= 1e-3, g_{j+1} >= 1e-3, and
    sl >= 0:  (n1 / 10) g_{j+1} >= D sl ((1 - m_hi) + c0)            X + Y = 1 lies D indices behind the segment's end
    sl <  0:  (n1 / 10) g_j     >= D (|sl| ((1 - m_lo) + c0) + g_j)   ... D indices in front of its first point

since the index of the stretch grows by at least (n1 / 10) / (1 - m + c0) per unit of m.  The exact tests ask for
max(32, 4 n) indices from a piece's centre and 16 L + 2 from the centre of the run's last (first) part; the eight
indices more cover their single-precision exponential and logarithm.

The proof obligation, asserted for every live run of every list on every input below, with no exception: a run that
passes the bound has both levels at 1e-6 or more, no piece that fails the guard, level 0 and at most 128 entries - what
the kernel's quick path assumes.  With D cut to a quarter the implication fails on these inputs (the plateau rows): they
exercise it.

A list of the kernel: lane l holds the run of segment j_0 + l, the lanes being the runs left, at most 64, the last of
64 only finding the first point that ends lane 62's run.  The list takes the quick path where every live lane passes
(a lane without points passes).  QUICK_PASSES records what this model finds on the launches of
tests/test_gpu_panel_quick.py, which holds prhf_panel_quick_counters to it."""

import numpy as np
import pytest
from unittest import mock

from conftest import load_golden
from oracle import vfo_numpy as orc
import test_panel_cut_host as cut
import test_panel_upper_host as upper
import test_strided_sum_host as tss
from test_panel_cut_host import LIST_ENTRIES, base_pieces
from test_panel_upper_host import upper_end
from test_panel_sum_host import TAU
from test_strided_sum_host import C0, plateau_inputs

LEVEL_MIN = 1e-3
LANES = 64


def quick_bound(g_j, g_n, kj, j, n1, L, d_scale=1.0):
    """panel_run_quick of prhf_kernels.hip."""
    rkj = 1.0 / kj
    m_lo, m_hi = j * rkj, (j + 1) * rkj
    sl = (g_j - g_n) * kj
    D = 0.0 if L <= 4 else d_scale * (16 * L + 10)
    if sl >= 0.0:
        lhs, rhs = (n1 * 0.1) * g_n, D * (sl * ((1.0 - m_hi) + C0))
    else:
        lhs, rhs = (n1 * 0.1) * g_j, D * (g_j - sl * ((1.0 - m_lo) + C0))
    return bool(g_j >= LEVEL_MIN and g_n >= LEVEL_MIN and lhs >= rhs)


class ExactRules:
    """test_panel_upper_host.upper_runs_pass put to one run: (no piece fails the guard and at most 128 entries at the
    run's level, level 0).  The second comes from the same function with the cap on a run's entries set to the run's
    base pieces: it then passes only at level 0."""

    def __enter__(self):
        self.run = None
        self.patches = [mock.patch.object(upper, "runs_of", lambda *a: [self.run]),
                        mock.patch.object(upper, "upper_end", lambda seg: (0, 0))]
        for p in self.patches:
            p.start()
        return self

    def __exit__(self, *exc):
        for p in self.patches:
            p.stop()

    def __call__(self, run, cond, alt_b, span, n_points):
        self.run = run
        good = upper.upper_runs_pass(None, 0, cond, alt_b, span, n_points)
        k = base_pieces(run[0], run[1])[0]
        with mock.patch.object(upper, "LIST_ENTRIES", k):
            flat = upper.upper_runs_pass(None, 0, cond, alt_b, span, n_points)
        return good, good and flat


def pair_setup(freq_mhz, den, bmag, bpsi, alt, n_points):
    """What the panel block knows of one pair, or None where the pair does not come to it (decision_of's gates)."""
    with np.errstate(all="ignore"):
        cap = orc.stage_capture(np.asarray([freq_mhz], dtype=float), den, bmag, bpsi, alt, "X", n_points)
        den_b, bmag_b, _, alt_b = orc.bottomside(den, bmag, bpsi, alt)
        mult = orc.stretch_multiplier(n_points)
    if not np.isfinite(cap["vh"][0]) or alt_b.size < 2:
        return None
    if n_points < 8192 or n_points >= 65536 or cut.grid_bits(mult) != 0 or np.unique(np.round(np.diff(alt_b), 9)).size > 1:
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
    with np.errstate(all="ignore"):
        cond = orc.ratio_X(den_b, f_hz) + orc.ratio_Y(f_hz, bmag_b)
    return dict(seg=seg, s_p=region[0], e_lo=region[1], cond=cond, alt_b=alt_b, span=span, kj=kj, n_points=n_points)


def lists_of(pair, rules, d_scale=1.0, stats=None):
    """The list passes of one pair as the kernel makes them under option panel_upper: [(quick, live runs)].  Every live
    run that passes the bound is put to the exact rules, and what they find is added to stats["broken"] where it is not
    what the quick path assumes."""
    stats = {} if stats is None else stats
    seg, s_p, e_lo, cond, alt_b = (pair[k] for k in ("seg", "s_p", "e_lo", "cond", "alt_b"))
    span, kj, n_points = pair["span"], pair["kj"], pair["n_points"]
    n1 = float(n_points - 1)
    j_top = int(seg[-1])
    e_up = upper_end(seg)[0]
    j_s, j_e = int(seg[s_p]), int(seg[e_lo - 1])
    up = int(seg[e_up - 1]) - (j_top - 1)
    in_upper = up in (0, 1)
    left, e_p = (j_top + up - j_s, e_up) if in_upper else (j_e - j_s + 1, e_lo)
    j_0 = j_s
    first_point = lambda j: int(np.argmax(seg >= j))          # noqa: E731
    passes, fell_back = [], False
    while left > 0:
        lanes = min(left, LANES)
        p = [max(first_point(j_0 + l), s_p) for l in range(lanes)] + [e_p]
        runs, quick, bad, counts = [], True, [], []
        for l in range(lanes):
            j = j_0 + l
            n = max(min(p[l + 1], e_p) - p[l], 0) if l < LANES - 1 else 0
            if n == 0:
                bad.append(False)
                counts.append(0)
                continue
            k, L, _ = base_pieces(p[l], n)
            jj = min(j + 1, alt_b.size - 1)
            g_j, g_n = 1.0 - cond[j], 1.0 - cond[jj]
            passed = k <= LIST_ENTRIES and quick_bound(g_j, g_n, kj, j, n1, L, d_scale)
            good, flat = rules((p[l], n, j), cond, alt_b, span, n_points)
            stats["runs"] = stats.get("runs", 0) + 1
            stats["passed"] = stats.get("passed", 0) + int(passed)
            if passed and not (good and flat and g_j >= TAU and g_n >= TAU):
                stats["broken"] = stats.get("broken", 0) + 1
            quick = quick and passed
            bad.append(not good)
            # (a run's entries at its level: one call more of the rules per halving, and only for the rare run above 0)
            s = 0
            if good and not flat:
                s = 1
                while True:
                    with mock.patch.object(upper, "LIST_ENTRIES", k << s):
                        if upper.upper_runs_pass(None, 0, cond, alt_b, span, n_points):
                            break
                    s += 1
            counts.append(k << s)
            runs.append((p[l], n, j))
        passes.append((quick, len(runs)))
        if not quick and any(bad):
            if not in_upper or any(b and j_0 + l < j_top - 3 for l, b in enumerate(bad)):
                fell_back = True
                break
            if left <= LANES - 1:
                in_upper, e_p, left = False, e_lo, j_e - j_0 + 1
                continue
        total = min(LANES - 1, left)
        if left > LANES - 1 and in_upper:
            total = min(total, j_top - 3 - j_0)
        incl = np.cumsum(counts)
        n_take = int(np.sum(incl[:total] <= LIST_ENTRIES))
        assert n_take >= 1
        j_0 += n_take
        left -= n_take
    return passes, fell_back


def sweep(rows, sizes, freqs, d_scale=1.0):
    """Every pair of the rows at every size and frequency: the counts of its lists and runs."""
    stats = {"pairs": 0, "quick": 0, "exact": 0, "pairs_with_quick": 0, "fell_back": 0}
    with ExactRules() as rules:
        for den, bmag, bpsi, alt in rows:
            for n_points in sizes:
                for f in freqs:
                    pair = pair_setup(f, den, bmag, bpsi, alt, n_points)
                    if pair is None:
                        continue
                    passes, fell = lists_of(pair, rules, d_scale, stats)
                    stats["pairs"] += 1
                    stats["fell_back"] += int(fell)
                    stats["quick"] += sum(1 for q, _ in passes if q)
                    stats["exact"] += sum(1 for q, _ in passes if not q)
                    stats["pairs_with_quick"] += int(any(q for q, _ in passes))
    return stats


def g14_rows():
    g = load_golden("g14_config4_rows.npz")
    return [(g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"]) for r in range(4)], g["freq"][::4]


def plateau_rows(rows=(0, 5, 7, 9, 12, 25)):
    freq, alt, den, bmag, bpsi = plateau_inputs()
    return [(den[r], bmag[r], bpsi[r], alt) for r in rows], freq


def chapman_rows():
    from pyrayhf_amd import synth
    alt, den, bmag, bpsi = synth.chapman_profiles(24, 20261020)
    return [(den[r], bmag[r], bpsi[r], alt) for r in range(24)], np.linspace(1.5, 12.5, 5)


def say(label, s):
    print(f"{label}: {s['pairs']} pairs, {s.get('runs', 0)} live runs with points, {s.get('passed', 0)} pass the bound, "
          f"{s.get('broken', 0)} of them against the exact rules; lists: {s['quick']} quick, {s['exact']} exact, "
          f"{s['pairs_with_quick']} pairs with a quick list, {s['fell_back']} fell back")


@pytest.fixture(scope="module")
def g14():
    rows, freq = g14_rows()
    return sweep(rows, (20000,), freq)


def test_bound_implies_the_exact_rules_on_config4_rows(g14):
    say("G14 rows 0-3 at 20000", g14)
    assert g14["pairs"] == 111 and g14.get("passed", 0) > 0
    assert g14.get("broken", 0) == 0


def test_most_pairs_of_config4_rows_have_a_quick_list(g14):
    """Most: more than half of the pairs.  Found: 70 of 111 pairs (0.631) have a list on the quick path, 148 of the 256
    lists are quick.  On the launch of the GPU test (24 Chapman profiles x 48 frequencies at 20 000 points) 535 of 638
    pairs and 1 103 of 1 612 lists."""
    share_pairs = g14["pairs_with_quick"] / g14["pairs"]
    share_lists = g14["quick"] / (g14["quick"] + g14["exact"])
    print(f"G14: {g14['pairs_with_quick']} of {g14['pairs']} pairs ({share_pairs:.3f}) have a quick list; {g14['quick']} of "
          f"{g14['quick'] + g14['exact']} lists ({share_lists:.3f}) are quick")
    assert share_pairs > 0.5


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_bound_implies_the_exact_rules_on_plateau_vacuum_and_no_field_rows(n_points):
    rows, freq = plateau_rows()
    s = sweep(rows, (n_points,), freq)
    say(f"plateau rows at {n_points}", s)
    assert s["pairs"] > 0 and s.get("passed", 0) > 0 and s["fell_back"] > 0
    assert s.get("broken", 0) == 0


@pytest.mark.parametrize("n_points", [8192, 8200, 20000, 65535])
def test_bound_implies_the_exact_rules_on_chapman_profiles(n_points):
    rows, freq = chapman_rows()
    s = sweep(rows, (n_points,), freq)
    say(f"24 Chapman profiles at {n_points}", s)
    assert s["pairs"] > 0 and s.get("passed", 0) > 0
    assert s.get("broken", 0) == 0


def test_a_quarter_of_the_distance_breaks_the_implication():
    """The inputs exercise the bound: with D / 4 a run passes that the exact rules halve or refuse."""
    rows, freq = plateau_rows()
    broken = 0
    for n_points in (8192, 20000):
        s = sweep(rows, (n_points,), freq, d_scale=0.25)
        say(f"plateau rows at {n_points}, D / 4", s)
        broken += s.get("broken", 0)
    assert broken > 0


# list passes (quick, exact) of the launches of tests/test_gpu_panel_quick.py by this model: what
# prhf_panel_quick_counters must report there
QUICK_PASSES = {"b20000_p4": (1103, 509), "plateau20000": (213, 377)}


def gpu_case_passes(name):
    """(quick, exact) of one launch of tests/panel_bits_cases.py."""
    import panel_bits_cases as cases
    _, (freq, den, bmag, bpsi, alt, n_points), _ = cases.inputs()[name]
    rows = [(den[r], bmag[r], bpsi[r], alt) for r in range(np.atleast_2d(den).shape[0])]
    s = sweep(rows, (n_points,), freq)
    say(name, s)
    return s["quick"], s["exact"]


def test_list_passes_of_the_gpu_launch():
    for name, want in QUICK_PASSES.items():
        got = gpu_case_passes(name)
        print(f"{name}: {got[0]} quick and {got[1]} exact list passes")
        assert got[0] > 0
        assert got == want
