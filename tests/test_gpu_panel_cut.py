"""The cuts of the panel sum (the rule in NumPy: tests/test_panel_cut_host.py) against the same binary
with panel_lower = 0, in one process.  The region below the top three segments is cut at every segment's first point
into runs, a run into ceil(n / 128) base pieces, and under panel_nodes = 4 (the default) the base pieces of a run too
near to X + Y = 1 into 2^s parts; every entry is summed on four lanes.  One lane stands for a run, a running sum over
the lanes turns runs into entries, and a list holds up to 128 entries of up to 63 runs.

Sizes: 8192 points, where a run below the top three holds two base pieces; 8200 and 20000; 65535, the largest
eligible grid - up to 15 base pieces in a run, and a piece's first point at the edge of its 16 bits.  Plateau rows 5-9
are where pieces are split and pairs fall back.

Bound: 1e-11 of the virtual height against panel_lower = 0, the bound of test_gpu_panel_sum and
test_gpu_panel_nodes; the rule's own error against the oracle, measured on the CPU, is below 1.1e-13.  Runs, pieces
and parts are computed by the pair's wave from the pair alone, so whether the pair ran from a plan, how many plan
records fit and what else the launch holds must not change a bit (same_bits).

Contexts of the test's own with target_waves = 64; the launches of the sizes are made once and shared."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import assert_masks, assert_x_mode, rel_err
from test_gpu_panel_sum import FREQ, SIZES, grid, run

pytestmark = pytest.mark.gpu

LARGEST = 65535
FREQ_LARGEST = FREQ[::6]                                   # 8 frequencies


@pytest.fixture(scope="module")
def ctxs():
    from pyrayhf_amd import _native
    c = {k: _native.Context(0) for k in ("on", "off", "unplanned", "capped")}
    for ctx in c.values():
        ctx.set_option("target_waves", 64)
    c["off"].set_option("panel_lower", 0)
    c["unplanned"].set_option("pair_plan", 0)
    c["capped"].set_option("pair_plan_cap", 4)
    yield c
    for ctx in c.values():
        ctx.close()


@pytest.fixture(scope="module")
def profiles():
    from pyrayhf_amd import synth
    return synth.chapman_profiles(24, 20261019)          # alt, den, bmag, bpsi


@pytest.fixture(scope="module")
def batches(ctxs, profiles):
    """{n_points: {context: (heights, took, fell)}}: 24 x 48 at the three sizes, 24 x 8 at 65535, made once."""
    alt, den, bmag, bpsi = profiles
    out = {n: {k: run(ctxs[k], FREQ, den, bmag, bpsi, alt, n) for k in ("on", "off")} for n in SIZES}
    out[LARGEST] = {k: run(ctxs[k], FREQ_LARGEST, den, bmag, bpsi, alt, LARGEST) for k in ("on", "off")}
    return out


def close(got, want, label):
    assert_masks(got, want)
    err, ok = rel_err(got, want)
    worst = float(err.max(initial=0.0))
    print(f"{label}: {int(ok.sum())} finite pairs, worst {worst:.2e}, {int((got[ok] != want[ok]).sum())} pairs differ")
    assert worst <= 1e-11


@pytest.mark.parametrize("n_points", SIZES + (LARGEST,))
def test_rule_against_panel_lower_off(batches, n_points):
    assert SIZES == (8192, 8200, 20000)
    got, took, fell = batches[n_points]["on"]
    want, took_off, fell_off = batches[n_points]["off"]
    assert np.isfinite(want).mean() > 0.3
    close(got, want, f"24 x {got.shape[1]} X/{n_points} against panel_lower = 0")
    print(f"X/{n_points}: {took} pairs took the rule, {fell} fell back")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not (got == -7.0).any()
    assert (took_off, fell_off) == (0, 0) and took > 0
    assert not same_bits(got, want)                        # (the rule summed something)


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - pieces are split, pairs fall back."""
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    got, took, fell = run(ctxs["on"], freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    want, _, _ = run(ctxs["off"], freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    close(got, want, f"plateau rows 5-9 X/{n_points} against panel_lower = 0")
    print(f"plateau rows 5-9 X/{n_points}: {took} pairs took the rule, {fell} fell back")
    assert took > 0 and fell > 0


@pytest.mark.parametrize("n_points", SIZES)
def test_same_bits_with_and_without_plans_and_twice(ctxs, profiles, batches, n_points):
    alt, den, bmag, bpsi = profiles
    got, took, fell = batches[n_points]["on"]
    for label in ("unplanned", "capped", "on"):
        again, took2, fell2 = run(ctxs[label], FREQ, den, bmag, bpsi, alt, n_points)
        assert same_bits(got, again), label
        assert (took2, fell2) == (took, fell), label


def test_mixed_work_list_equals_separate_launches(ctxs, profiles, batches):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on = ctxs["on"]
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
    assert same_bits(out[10:], batches[20000]["on"][0][10:])


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    got, took, fell = run(ctxs["on"], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference: {worst:.2e}; {took} pairs took the rule, {fell} fell back")
    assert took > 0


def test_other_launches_keep_their_bits(ctxs, profiles):
    alt, den, bmag, bpsi = profiles

    def untouched(label, *args, **kwargs):
        got, took, fell = run(ctxs["on"], *args, **kwargs)
        assert np.isfinite(got).any(), label
        assert (took, fell) == (0, 0), label
        assert same_bits(got, run(ctxs["off"], *args, **kwargs)[0]), label

    g = load_golden("g7_edges.npz")
    nfreq, nden, nbmag, nbpsi, nalt = (g[f"nonuniform_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt"))
    assert np.unique(np.round(np.diff(nalt), 6)).size > 1
    tile = lambda x: np.tile(x, (24, 1))                   # noqa: E731
    untouched("a non-uniform altitude grid", nfreq, tile(nden), tile(nbmag), tile(nbpsi), nalt, 8192)
    untouched("O mode", FREQ, den, bmag, bpsi, alt, 8192, mode="O")
    untouched("one profile, chunked", FREQ, den[3], bmag[3], bpsi[3], alt, 20000)
    untouched("4096 points", FREQ, den, bmag, bpsi, alt, 4096)
    # more than 1400 levels below the highest peak: the profiles are staged in global memory (vfo_tall_kernel)
    tall = np.linspace(alt[0], alt[-1], 12001)
    assert (tall < alt[np.argmax(den[:6], axis=1)].max()).sum() > 1400
    cols = [np.stack([np.interp(tall, alt, r) for r in x[:6]]) for x in (den, bmag, bpsi)]
    untouched("tall profiles", FREQ, *cols, tall, 8192)
