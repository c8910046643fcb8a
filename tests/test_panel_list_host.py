"""The general list of the panel sum (the panel block of lean_loop_body) restated in NumPy: no GPU.

When some run of a list has a count other than 1, entry slot e of the list finds its run from the inclusive running sum
of the lanes' counts and cuts its part from the run's (p, n), L and level s.

The rule: at(e) = the number of lanes 0 .. 62 whose running sum is at most e, found by bisection
(six steps of 32, 16, .. 1, each a look-up of the running sum at lane at + step - 1); the run is lane at.
The kernel has this rule.  A second construction with a shorter chain was built and measured, gained nothing by the
ten-spreads rule and was taken out again (profiles/ab_panel_pipeline.txt); it is kept here beside the rule for whoever
tries the next one: the running sum never falls, so the steps of 32 and 16 are three compares with the sums of lanes
15, 31 and 47 - at = 16 x (how many of them are at most e) - and the steps of 8, 4, 2 and 1 follow as before.  Both are
stated below lane by lane, as a kernel computes them, checked against the plain count, and must give the same list words

  w(e) = (p + i L + a) | (b - a) << 16,  i = q >> s, t = q & (2^s - 1), q = e - (entries before the run),
         n_b = max(min(L, n - i L), 0), a = t n_b >> s, b = (t + 1) n_b >> s;  0 for e >= total

for every count vector of the NumPy model's G14 pairs (test_panel_upper_host's rows, every 4th frequency, 20 000
points; the model's lists are cut from them as the kernel cuts them: at most 63 runs and 128 entries) and for 10 000
random vectors of 63 counts in 0 .. 32, zeros among them, capped at 128 entries."""

import numpy as np
import pytest
from unittest import mock

from conftest import load_golden
import test_panel_cut_host as cut
from test_panel_cut_host import LIST_ENTRIES, LIST_RUNS
from test_panel_upper_host import upper_virtual_heights


def running_sum(cnt):
    """(inclusive running sum over 64 lanes, runs taken, entries of the list): lane 63 never holds a run."""
    c = np.zeros(64, dtype=np.int64)
    c[:len(cnt)] = cnt
    incl = np.cumsum(c)
    n_take = int(np.count_nonzero((np.arange(64) < min(len(cnt), LIST_RUNS)) & (incl <= LIST_ENTRIES)))
    return c, incl, n_take, (int(incl[n_take - 1]) if n_take else 0)


def at_by_bisection(incl, e):
    at = np.zeros_like(e)
    for step in (32, 16, 8, 4, 2, 1):
        at = at + np.where(incl[at + step - 1] <= e, step, 0)
    return at


def at_by_pivots(incl, e):
    at = ((incl[15] <= e).astype(np.int64) + (incl[31] <= e) + (incl[47] <= e)) << 4
    for step in (8, 4, 2, 1):
        at = at + np.where(incl[at + step - 1] <= e, step, 0)
    return at


def list_words(cnt, p, n, L, s, at_of):
    c, incl, n_take, total = running_sum(cnt)
    words = []
    for half in range(2 if total > 64 else 1):
        e = 64 * half + np.arange(64)
        at = at_of(incl, e)
        r_p, r_n, r_L, r_s = p[at], n[at], L[at], s[at]
        q = e - (incl[at] - c[at])
        i, t = q >> r_s, q & ((1 << r_s) - 1)
        n_b = np.maximum(np.minimum(r_L, r_n - i * r_L), 0)
        a, b = (t * n_b) >> r_s, ((t + 1) * n_b) >> r_s
        words.append(np.where(e < total, (r_p + i * r_L + a) | ((b - a) << 16), 0))
    return np.concatenate(words), total


def runs_with_counts(cnt, rng):
    """Runs (p, n, L, s) per lane whose entries number cnt: k << s with k = ceil(n / 128) base pieces."""
    cnt = np.asarray(cnt, dtype=np.int64)
    p, n, L, s = (np.zeros(64, dtype=np.int64) for _ in range(4))
    for lane, c in enumerate(cnt):
        if c > 0:
            s[lane] = int(rng.integers(0, int(np.log2(c & -c)) + 1))        # c = k << s
            k = c >> s[lane]
            n[lane] = int(rng.integers(128 * (k - 1) + 1, 128 * k + 1))
            L[lane] = -(-n[lane] // k)
        p[lane] = 100 + 7 * lane                             # (distinct; a word has 16 bits for the point)
    return p, n, L, s


def same_words(cnt, rng):
    p, n, L, s = runs_with_counts(cnt, rng)
    old, total = list_words(cnt, p, n, L, s, at_by_bisection)
    new, _ = list_words(cnt, p, n, L, s, at_by_pivots)
    assert np.array_equal(old, new), cnt
    # every entry slot below the total holds a part of the run the plain count names, and the parts tile the runs
    c, incl, n_take, _ = running_sum(cnt)
    assert np.array_equal(at_by_pivots(incl, np.arange(total)), np.searchsorted(incl[:63], np.arange(total), side="right"))
    assert int((new >> 16).sum()) == int(n[:n_take].sum())
    return total


def kernel_lists(counts):
    """The count vectors of one pair's lists, cut as the kernel cuts them (test_panel_cut_host's loop)."""
    at = 0
    while at < len(counts):
        take, entries = 0, 0
        while at + take < len(counts) and take < LIST_RUNS and entries + counts[at + take] <= LIST_ENTRIES:
            entries += counts[at + take]
            take += 1
        yield counts[at:at + LIST_RUNS], take                # (the lanes behind the list's end hold runs too)
        at += take


@pytest.fixture(scope="module")
def g14_counts():
    """Every pair's count vector, caught where the model tests it against the list's capacity."""
    caught = []

    def catching_max(*args, **kwargs):
        if len(args) == 1 and isinstance(args[0], list):
            caught.append(list(args[0]))
        return max(*args, **kwargs)

    g = load_golden("g14_config4_rows.npz")
    with mock.patch.object(cut, "max", catching_max, create=True):
        for r in range(4):
            upper_virtual_heights(g["freq"][::4], g["den"][r], g["bmag"][r], g["bpsi"][r], g["alt"], 20000)
    return caught


def test_g14_count_vectors(g14_counts):
    rng = np.random.default_rng(27)
    lists = general = longest = 0
    assert len(g14_counts) >= 100
    for counts in g14_counts:
        if max(counts) > LIST_ENTRIES:
            continue
        for cnt, take in kernel_lists(counts):
            total = same_words(cnt, rng)
            assert total == sum(cnt[:take])
            lists += 1
            general += any(c != 1 for c in cnt[:take])
            longest = max(longest, total)
    print(f"{len(g14_counts)} pairs, {lists} lists, {general} of them general, longest {longest} entries")
    assert general > 0


def test_random_count_vectors():
    rng = np.random.default_rng(20261019)
    longest = over = 0
    for _ in range(10000):
        cnt = rng.integers(0, 33, size=63)
        cnt[rng.random(63) < 0.2] = 0
        if rng.random() < 0.5:
            cnt = np.where(rng.random(63) < 0.8, 1, cnt)     # mostly single entries, as the kernel's lists are
        if cnt[0] == 0:
            cnt[0] = 1                                       # (lane 0 is a live run)
        total = same_words(cnt, rng)
        assert 1 <= total <= LIST_ENTRIES
        longest = max(longest, total)
        over += total > 64
    print(f"10 000 vectors: longest list {longest} entries, {over} of more than 64")
    assert longest == LIST_ENTRIES and over > 1000
