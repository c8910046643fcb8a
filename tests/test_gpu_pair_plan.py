"""The planning pass (option pair_plan): the integers that steer a long X-mode pair's strided sum are
computed once per pair by one thread of the workgroup instead of by all 64 lanes of the pair's wave.  The integers are
the same either way, so every comparison here is bit identity (same_bits), not a tolerance: pair_plan = 1 against
pair_plan = 0 of the same binary in one process, and against pair_plan_cap = 4, which leaves room for four plans per
workgroup so that planned and self-planned pairs mix in every profile.

The counters (prhf_pair_plan_counters: pairs that ran from a plan, eligible pairs that planned themselves) show that
the planned path was actually taken - or, for the launches that must keep the path of before, that it was not.

Contexts of the test's own with target_waves = 64, as in test_gpu_strided_lower.py: 24 x 48 pairs are whole work
items, one profile x 48 frequencies is still chunked."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import assert_x_mode

pytestmark = pytest.mark.gpu

FREQ = np.linspace(0.5, 13.0, 48)


@pytest.fixture(scope="module")
def ctxs():
    from pyrayhf_amd import _native
    on, off, capped = _native.Context(0), _native.Context(0), _native.Context(0)
    for c in (on, off, capped):
        c.set_option("target_waves", 64)
    off.set_option("pair_plan", 0)
    capped.set_option("pair_plan_cap", 4)
    yield on, off, capped
    for c in (on, off, capped):
        c.close()


@pytest.fixture(scope="module")
def profiles():
    from pyrayhf_amd import synth
    return synth.chapman_profiles(24, 20261018)          # alt, den, bmag, bpsi


def grid(n_points, sharpness=10.0):
    from pyrayhf_amd import library
    return np.ascontiguousarray(library.smooth_nonuniform_grid(0, 1, n_points, sharpness))


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mult=None, mode="X"):
    """(virtual heights, pairs planned by this call, eligible pairs that planned themselves in this call)"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points) if mult is None else mult
    out = np.full((d.shape[0], f.size), -7.0)
    before = ctx.pair_plan_counters()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    after = ctx.pair_plan_counters()
    return out, after[0] - before[0], after[1] - before[1]


@pytest.mark.parametrize("n_points", [8191, 8192, 8200, 20000])
def test_plain_batch(ctxs, profiles, n_points):
    alt, den, bmag, bpsi = profiles
    on, off, _ = ctxs
    got, planned, own = run(on, FREQ, den, bmag, bpsi, alt, n_points)
    want, planned_off, own_off = run(off, FREQ, den, bmag, bpsi, alt, n_points)
    reflecting = int(np.isfinite(want).sum())
    print(f"24 x 48 X/{n_points}: {reflecting} reflecting pairs, {planned} planned, {own} planned themselves")
    assert reflecting > 0.3 * want.size
    assert same_bits(got, want)
    assert (planned_off, own_off) == (0, 0)
    if n_points < 8192:                                    # below the threshold of the strided sum: nothing is planned
        assert (planned, own) == (0, 0)
    else:
        assert planned > reflecting // 2
        assert planned + own <= reflecting


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_and_no_field_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - the pairs where the guards decide."""
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    on, off, capped = ctxs
    got, planned, own = run(on, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    print(f"plateau rows 5-9 X/{n_points}: {planned} planned, {own} planned themselves")
    assert same_bits(got, run(off, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)[0])
    assert same_bits(got, run(capped, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)[0])


@pytest.mark.parametrize("n_freq", [48, 512])
def test_peak_at_the_top_of_the_column(ctxs, profiles, n_freq):
    """The density peak at the last level but one: no node of the staged arrays is free above the peak."""
    alt, den, bmag, bpsi = profiles
    row = int(np.argmax(np.argmax(den, axis=1)))          # the profile with the highest peak: the most levels
    k = int(np.argmax(den[row]))
    cut = slice(0, k + 2)
    assert int(np.argmax(den[row, cut])) == (k + 2) - 2
    tile = lambda x: np.tile(x[row, cut], (24, 1))         # noqa: E731
    freq = np.linspace(0.5, 13.0, n_freq)
    on, off, _ = ctxs
    got, planned, own = run(on, freq, tile(den), tile(bmag), tile(bpsi), alt[cut], 8192)
    print(f"peak at level {k} of {k + 2}, {n_freq} frequencies: {planned} planned, {own} planned themselves")
    assert np.isfinite(got).any()
    assert same_bits(got, run(off, freq, tile(den), tile(bmag), tile(bpsi), alt[cut], 8192)[0])


def test_unplanned_paths_keep_their_launch(ctxs, profiles):
    alt, den, bmag, bpsi = profiles
    on, off, _ = ctxs

    def unplanned(label, *args, **kwargs):
        got, planned, _ = run(on, *args, **kwargs)
        assert np.isfinite(got).mean() > 0.3, label
        assert same_bits(got, run(off, *args, **kwargs)[0]), label
        assert planned == 0, label

    # 600 frequencies: more than one round of threads, reflection heights are not settled per thread
    unplanned("600 frequencies", np.linspace(0.5, 13.0, 600), den, bmag, bpsi, alt, 8192)
    # a non-uniform altitude grid
    g = load_golden("g7_edges.npz")
    nfreq, nden, nbmag, nbpsi, nalt = (g[f"nonuniform_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt"))
    assert np.unique(np.round(np.diff(nalt), 6)).size > 1
    tile = lambda x: np.tile(x, (24, 1))                   # noqa: E731
    got, planned, _ = run(on, nfreq, tile(nden), tile(nbmag), tile(nbpsi), nalt, 8192)
    assert np.isfinite(got).any() and planned == 0
    assert same_bits(got, run(off, nfreq, tile(nden), tile(nbmag), tile(nbpsi), nalt, 8192)[0])
    # grids the C ABI accepts that are not the reference's stretch
    unplanned("sharpness 5", FREQ, den, bmag, bpsi, alt, 8192, mult=grid(8192, sharpness=5.0))
    unplanned("linear grid", FREQ, den, bmag, bpsi, alt, 8192, mult=np.linspace(0.0, 1.0, 8192))
    unplanned("O mode", FREQ, den, bmag, bpsi, alt, 8192, mode="O")
    # one profile: the pairs are cut into chunks
    unplanned("one profile", FREQ, den[3], bmag[3], bpsi[3], alt, 20000)


def test_mixed_work_list_equals_separate_launches(ctxs, profiles):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on, off, _ = ctxs
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    before = on.pair_plan_counters()
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert on.pair_plan_counters()[0] > before[0]          # the X/20000 slice ran from plans
    assert same_bits(out[:10], run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O")[0])
    sep, planned, _ = run(on, FREQ, den[10:], bmag[10:], bpsi[10:], alt, 20000)
    assert planned > 0
    assert same_bits(out[10:], sep)
    assert same_bits(sep, run(off, FREQ, den[10:], bmag[10:], bpsi[10:], alt, 20000)[0])


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    on, off, _ = ctxs
    got, planned, own = run(on, g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference: {worst:.2e}; {planned} planned, {own} planned themselves")
    assert planned > 0
    assert same_bits(got, run(on, g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)[0])
    assert same_bits(got, run(off, g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)[0])


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_forced_lack_of_room(ctxs, profiles, n_points):
    """Four plans per workgroup: the other pairs of every profile plan themselves.  Same bits as with every plan and
    with none."""
    alt, den, bmag, bpsi = profiles
    on, off, capped = ctxs
    got, planned, own = run(capped, FREQ, den, bmag, bpsi, alt, n_points)
    print(f"at most 4 plans per workgroup, X/{n_points}: {planned} planned, {own} planned themselves")
    assert planned > 0 and own > 0
    assert same_bits(got, run(off, FREQ, den, bmag, bpsi, alt, n_points)[0])
    full, planned_full, _ = run(on, FREQ, den, bmag, bpsi, alt, n_points)
    assert planned_full > planned
    assert same_bits(got, full)
