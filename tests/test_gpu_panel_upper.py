"""Option panel_upper (the rule in NumPy: tests/test_panel_upper_host.py) against the same binary with
panel_upper = 0 and with panel_lower = 0, in one process.  With the option on, the region of the panel sum ends at the
top segment's first point where the runs from segment j_top - 3 up pass the runs' tests, which the pair's wave settles
in the first list whose lanes hold every run that is left, before any of those runs is summed; a pair where one fails
keeps the lower region and the strided sums of the two segments below the top one, and does not fall back as a whole
on that account.

Sizes: those of test_gpu_panel_cut - 24 x 48 at 8192, 8200 and 20000 points, 24 x 8 at 65535, the largest eligible grid,
where the segment below the top one holds the most base pieces.  Plateau rows 5-9 are where pairs keep the lower
region and where pairs fall back.  prhf_panel_upper_counters' second word counts the pairs that take the panel sum and
keep the lower region; the host model counts those for the same rows (tests/test_panel_upper_host.py, GPU_ROWS_KEPT: 2
of 294 at 8192 points, 2 of 250 at 20000 - of all eligible pairs, those that fall back as a whole included, 11 and 5
keep it) and the kernel's count must equal the model's.

Bound: 1e-11 of the virtual height, the standing bound of the panel tests; the rule's own error against the oracle,
measured on the CPU, is below 1.1e-13.  The decision and the runs are computed by the pair's wave from the pair alone,
so whether the pair ran from a plan, how many plan records fit and what else the launch holds must not change a bit
(same_bits).

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
    c = {k: _native.Context(0) for k in ("on", "upper_off", "lower_off", "unplanned", "capped", "eight")}
    for ctx in c.values():
        ctx.set_option("target_waves", 64)
    c["upper_off"].set_option("panel_upper", 0)
    c["lower_off"].set_option("panel_lower", 0)
    c["unplanned"].set_option("pair_plan", 0)
    c["capped"].set_option("pair_plan_cap", 4)
    c["eight"].set_option("panel_nodes", 8)
    yield c
    for ctx in c.values():
        ctx.close()


@pytest.fixture(scope="module")
def profiles():
    from pyrayhf_amd import synth
    return synth.chapman_profiles(24, 20261019)          # alt, den, bmag, bpsi


def run_upper(ctx, *args, **kwargs):
    """(virtual heights, (took, fell) of prhf_panel_counters, (reached, kept) of prhf_panel_upper_counters) of one call"""
    before = ctx.panel_upper_counters()
    got, took, fell = run(ctx, *args, **kwargs)
    after = ctx.panel_upper_counters()
    return got, (took, fell), (after[0] - before[0], after[1] - before[1])


@pytest.fixture(scope="module")
def batches(ctxs, profiles):
    """{n_points: {context: (heights, (took, fell), (reached, kept))}}: 24 x 48 at the three sizes, 24 x 8 at 65535."""
    alt, den, bmag, bpsi = profiles
    keys = ("on", "upper_off", "lower_off")
    out = {n: {k: run_upper(ctxs[k], FREQ, den, bmag, bpsi, alt, n) for k in keys} for n in SIZES}
    out[LARGEST] = {k: run_upper(ctxs[k], FREQ_LARGEST, den, bmag, bpsi, alt, LARGEST) for k in keys}
    return out


def close(got, want, label):
    assert_masks(got, want)
    err, ok = rel_err(got, want)
    worst = float(err.max(initial=0.0))
    print(f"{label}: {int(ok.sum())} finite pairs, worst {worst:.2e}, {int((got[ok] != want[ok]).sum())} pairs differ")
    assert worst <= 1e-11


@pytest.mark.parametrize("n_points", SIZES + (LARGEST,))
def test_default_against_both_options_off(batches, n_points):
    assert SIZES == (8192, 8200, 20000)
    got, panel, upper = batches[n_points]["on"]
    no_upper, panel_0, upper_0 = batches[n_points]["upper_off"]
    no_panel, _, upper_l = batches[n_points]["lower_off"]
    assert np.isfinite(no_panel).mean() > 0.3
    close(got, no_upper, f"24 x {got.shape[1]} X/{n_points} against panel_upper = 0")
    close(got, no_panel, f"24 x {got.shape[1]} X/{n_points} against panel_lower = 0")
    assert np.array_equal(np.isnan(got), np.isnan(no_upper)) and np.array_equal(np.isnan(got), np.isnan(no_panel))
    assert not (got == -7.0).any()
    print(f"X/{n_points}: {panel[0]} pairs took the rule, {panel[1]} fell back; {upper[0]} reached the top segment, "
          f"{upper[1]} kept the lower region")
    assert upper[0] > 0
    assert upper[0] + upper[1] == panel[0]
    assert upper_0 == (0, 0) and upper_l == (0, 0)
    assert panel == panel_0
    assert not same_bits(got, no_upper)                    # (the upper runs summed something)


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - pairs keep the lower region, as many as in
    the host model, and pairs fall back."""
    from test_panel_upper_host import GPU_ROWS_KEPT
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    rows = (freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)
    got, panel, upper = run_upper(ctxs["on"], *rows)
    no_upper, panel_0, upper_0 = run_upper(ctxs["upper_off"], *rows)
    no_panel, _, _ = run_upper(ctxs["lower_off"], *rows)
    close(got, no_upper, f"plateau rows 5-9 X/{n_points} against panel_upper = 0")
    close(got, no_panel, f"plateau rows 5-9 X/{n_points} against panel_lower = 0")
    print(f"plateau rows 5-9 X/{n_points}: {panel[0]} pairs took the rule, {panel[1]} fell back; {upper[0]} reached the "
          f"top segment, {upper[1]} kept the lower region")
    assert panel == panel_0 and panel[0] > 0 and panel[1] > 0
    assert upper[0] > 0 and upper[1] == GPU_ROWS_KEPT[n_points] and upper_0 == (0, 0)


@pytest.mark.parametrize("n_points", SIZES)
def test_same_bits_with_and_without_plans_and_twice(ctxs, profiles, batches, n_points):
    alt, den, bmag, bpsi = profiles
    got, panel, upper = batches[n_points]["on"]
    for label in ("unplanned", "capped", "on"):
        again, panel2, upper2 = run_upper(ctxs[label], FREQ, den, bmag, bpsi, alt, n_points)
        assert same_bits(got, again), label
        assert (panel2, upper2) == (panel, upper), label


def test_mixed_work_list_equals_separate_launches(ctxs, profiles, batches):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on = ctxs["on"]
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    before = on.panel_upper_counters()
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert on.panel_upper_counters()[0] > before[0]        # the X/20000 slice reached the top segment
    assert same_bits(out[:10], run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O")[0])
    assert same_bits(out[10:], batches[20000]["on"][0][10:])


@pytest.mark.parametrize("n_points", SIZES)
def test_eight_nodes_with_the_upper_region(ctxs, profiles, batches, n_points):
    alt, den, bmag, bpsi = profiles
    got, panel, upper = run_upper(ctxs["eight"], FREQ, den, bmag, bpsi, alt, n_points)
    close(got, batches[n_points]["lower_off"][0], f"panel_nodes = 8, X/{n_points} against panel_lower = 0")
    print(f"panel_nodes = 8, X/{n_points}: {upper[0]} reached the top segment, {upper[1]} kept the lower region")
    assert upper[0] > 0 and panel == batches[n_points]["on"][1]


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    got, panel, upper = run_upper(ctxs["on"], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference: {worst:.2e}; {panel[0]} pairs took the rule, {panel[1]} fell back; {upper[0]} "
          f"reached the top segment, {upper[1]} kept the lower region")
    assert upper[0] > 0


def test_other_launches_keep_their_bits(ctxs, profiles):
    alt, den, bmag, bpsi = profiles

    def untouched(label, *args, **kwargs):
        got, _, upper = run_upper(ctxs["on"], *args, **kwargs)
        assert np.isfinite(got).any(), label
        assert upper == (0, 0), label
        assert same_bits(got, run(ctxs["upper_off"], *args, **kwargs)[0]), label

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
