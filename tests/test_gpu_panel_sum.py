"""The panel sum of the segments below the top three (option panel_lower) against the same binary with
the option off, in one process: whole pairs of at least 8192 points in X mode on a uniform altitude grid and the
reference's stretch sum the region below the top three segments from eight nodes per piece where the pair's guard
allows it; everything else must not notice.

Bound: 1e-11 of the virtual height against panel_lower = 0, the bound of test_gpu_strided_lower; the rule's own error,
measured on the CPU against the oracle (tests/test_panel_sum_host.py), is below 1.5e-13 from 8192 points up.  The
rule's integers are computed by the pair's wave from the pair alone, so whether the pair ran from a plan, how many plan
records fit and what else the launch holds must not change a bit (same_bits).

The counters (prhf_panel_counters: pairs that took the rule, eligible pairs that fell back) show which path ran.

Contexts of the test's own with target_waves = 64, as in test_gpu_strided_lower.py: 24 x 48 pairs are whole work
items, one profile x 48 frequencies is still chunked.  The launches of the three sizes are made once and shared."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import assert_masks, assert_x_mode, rel_err

pytestmark = pytest.mark.gpu

FREQ = np.linspace(0.5, 13.0, 48)
SIZES = (8192, 8200, 20000)


@pytest.fixture(scope="module")
def ctxs():
    from pyrayhf_amd import _native
    on, off, unplanned, capped = (_native.Context(0) for _ in range(4))
    for c in (on, off, unplanned, capped):
        c.set_option("target_waves", 64)
    off.set_option("panel_lower", 0)
    unplanned.set_option("pair_plan", 0)
    capped.set_option("pair_plan_cap", 4)
    yield on, off, unplanned, capped
    for c in (on, off, unplanned, capped):
        c.close()


@pytest.fixture(scope="module")
def profiles():
    from pyrayhf_amd import synth
    return synth.chapman_profiles(24, 20261019)          # alt, den, bmag, bpsi


def grid(n_points, sharpness=10.0):
    from pyrayhf_amd import library
    return np.ascontiguousarray(library.smooth_nonuniform_grid(0, 1, n_points, sharpness))


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mult=None, mode="X"):
    """(virtual heights, pairs that took the rule in this call, eligible pairs that fell back in this call)"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points) if mult is None else mult
    out = np.full((d.shape[0], f.size), -7.0)
    before = ctx.panel_counters()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    after = ctx.panel_counters()
    return out, after[0] - before[0], after[1] - before[1]


@pytest.fixture(scope="module")
def batches(ctxs, profiles):
    """{n_points: (run with the rule, run with panel_lower = 0)} of the 24 x 48 batch, made once."""
    alt, den, bmag, bpsi = profiles
    on, off = ctxs[:2]
    return {n: (run(on, FREQ, den, bmag, bpsi, alt, n), run(off, FREQ, den, bmag, bpsi, alt, n)) for n in SIZES}


def close(got, want, label):
    assert_masks(got, want)
    err, ok = rel_err(got, want)
    worst = float(err.max(initial=0.0))
    print(f"{label}: {int(ok.sum())} finite pairs, worst {worst:.2e}, {int((got[ok] != want[ok]).sum())} pairs differ")
    assert worst <= 1e-11


@pytest.mark.parametrize("n_points", SIZES)
def test_batch_against_panel_lower_off(batches, n_points):
    (got, took, fell), (want, took_off, fell_off) = batches[n_points]
    assert np.isfinite(want).mean() > 0.3
    close(got, want, f"24 x 48 X/{n_points} against panel_lower = 0")
    assert (took_off, fell_off) == (0, 0)
    assert took > 0 and not same_bits(got, want)           # (the rule was taken)


@pytest.mark.parametrize("n_points", SIZES)
def test_nan_masks(batches, n_points):
    (got, _, _), (want, _, _) = batches[n_points]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert not (got == -7.0).any()


@pytest.mark.parametrize("n_points", SIZES)
def test_same_bits_with_and_without_plans_and_twice(ctxs, profiles, batches, n_points):
    alt, den, bmag, bpsi = profiles
    on, _, unplanned, capped = ctxs
    got, took, fell = batches[n_points][0]
    for label, ctx in (("pair_plan = 0", unplanned), ("pair_plan_cap = 4", capped), ("a second launch", on)):
        again, took2, fell2 = run(ctx, FREQ, den, bmag, bpsi, alt, n_points)
        assert same_bits(got, again), label
        assert (took2, fell2) == (took, fell), label


def test_mixed_work_list_equals_separate_launches(ctxs, profiles, batches):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on = ctxs[0]
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    before = on.panel_counters()
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert on.panel_counters()[0] > before[0]              # the X/20000 slice took the rule
    assert same_bits(out[:10], run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O")[0])
    assert same_bits(out[10:], batches[20000][0][0][10:])  # a pair's value does not depend on what else is launched


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - the pairs where the guard decides."""
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    on, off = ctxs[:2]
    got, took, fell = run(on, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    want, _, _ = run(off, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    close(got, want, f"plateau rows 5-9 X/{n_points} against panel_lower = 0")
    print(f"plateau rows 5-9 X/{n_points}: {took} pairs took the rule, {fell} fell back")
    assert took > 0 and fell > 0


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    got, took, fell = run(ctxs[0], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference: {worst:.2e}; {took} pairs took the rule, {fell} fell back")
    assert took > 0


def test_other_launches_keep_their_path(ctxs, profiles):
    alt, den, bmag, bpsi = profiles
    on, off = ctxs[:2]

    def untouched(label, *args, **kwargs):
        got, took, fell = run(on, *args, **kwargs)
        assert np.isfinite(got).any(), label
        assert same_bits(got, run(off, *args, **kwargs)[0]), label
        assert (took, fell) == (0, 0), label

    g = load_golden("g7_edges.npz")
    nfreq, nden, nbmag, nbpsi, nalt = (g[f"nonuniform_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt"))
    assert np.unique(np.round(np.diff(nalt), 6)).size > 1
    tile = lambda x: np.tile(x, (24, 1))                   # noqa: E731
    untouched("a non-uniform altitude grid", nfreq, tile(nden), tile(nbmag), tile(nbpsi), nalt, 8192)
    untouched("sharpness 5", FREQ, den, bmag, bpsi, alt, 8192, mult=grid(8192, sharpness=5.0))
    untouched("O mode", FREQ, den, bmag, bpsi, alt, 8192, mode="O")
    untouched("one profile, chunked", FREQ, den[3], bmag[3], bpsi[3], alt, 20000)
    untouched("4096 points", FREQ, den, bmag, bpsi, alt, 4096)


def test_most_reflecting_pairs_take_the_rule(batches):
    (got, took, fell), _ = batches[20000]
    reflecting = int(np.isfinite(got).sum())
    print(f"24 x 48 X/20000: {took} of {reflecting} reflecting pairs took the rule ({took / reflecting:.1%}), {fell} fell back")
    assert took > reflecting // 2
    assert took + fell <= reflecting
