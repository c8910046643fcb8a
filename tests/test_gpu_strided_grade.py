"""The zones of the strided sum (option strided_grade) against the same binary with strided_grade = 0 and
with strided_top = 0, in one process.  With strided_grade = 1 the strided stretch of each of the top three segments takes
every 32nd and every 16th point away from X + Y = 1 and every eighth next to it; everything outside those stretches
must not notice.

Bound: 1e-11 of the virtual height, the suite's X-mode bound against strided_top = 0 (test_gpu_strided_sum); the
rule's own error, measured on the CPU against the oracle (tests/test_strided_grade_host.py), is below 2.5e-13.
Measured here: at most 2.0e-13 against strided_top = 0 and 4.5e-14 against strided_grade = 0.  The
zones are a function of the pair alone - the plan's thread and the pair's wave go through one function - so whether
the pair ran from a plan, how many plan records fit and what else the launch holds must not change a bit (same_bits).

Contexts of the test's own with target_waves = 64, as in test_gpu_panel_sum.py; the launches of the three sizes are
made once and shared."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import assert_masks, assert_x_mode, rel_err
from test_gpu_panel_sum import FREQ, SIZES, grid, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    from pyrayhf_amd import _native
    names = ("graded", "plain", "full", "unplanned", "capped", "untouched")
    c = {k: _native.Context(0) for k in names}
    for ctx in c.values():
        ctx.set_option("target_waves", 64)
    for k in ("graded", "unplanned", "capped"):
        c[k].set_option("strided_grade", 1)
    c["plain"].set_option("strided_grade", 0)
    c["full"].set_option("strided_top", 0)
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
    """{n_points: {context: heights}} of the 24 x 48 batch, made once."""
    alt, den, bmag, bpsi = profiles
    return {n: {k: run(ctxs[k], FREQ, den, bmag, bpsi, alt, n)[0] for k in ("graded", "plain", "full")} for n in SIZES}


def close(got, want, label):
    assert_masks(got, want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not (got == -7.0).any()
    err, ok = rel_err(got, want)
    worst = float(err.max(initial=0.0))
    print(f"{label}: {int(ok.sum())} finite pairs, worst {worst:.2e}, {int((got[ok] != want[ok]).sum())} pairs differ")
    assert worst <= 1e-11


@pytest.mark.parametrize("n_points", SIZES)
def test_zones_against_stride_8_and_against_the_full_sum(batches, n_points):
    got, plain, full = (batches[n_points][k] for k in ("graded", "plain", "full"))
    assert np.isfinite(full).mean() > 0.3
    close(got, plain, f"24 x 48 X/{n_points}, strided_grade = 1 against 0")
    close(got, full, f"24 x 48 X/{n_points}, strided_grade = 1 against strided_top = 0")
    close(plain, full, f"24 x 48 X/{n_points}, strided_grade = 0 against strided_top = 0")
    assert not same_bits(got, plain)                       # (coarse zones were summed)


@pytest.mark.parametrize("n_points", SIZES)
def test_same_bits_with_and_without_plans_and_twice(ctxs, profiles, batches, n_points):
    alt, den, bmag, bpsi = profiles
    for label in ("unplanned", "capped", "graded"):
        before = ctxs[label].pair_plan_counters()
        again = run(ctxs[label], FREQ, den, bmag, bpsi, alt, n_points)[0]
        after = ctxs[label].pair_plan_counters()
        assert same_bits(batches[n_points]["graded"], again), label
        planned, own = after[0] - before[0], after[1] - before[1]
        if label == "unplanned":
            assert planned == 0
        elif label == "capped":
            assert planned > 0 and own > 0
        else:
            assert planned > 0


def test_grade_off_repeats_and_an_untouched_context_takes_the_default(ctxs, profiles, batches):
    """strided_grade = 0 gives the same bits twice (that they are the bits of the build before the option is shown by
    profiles/ab_strided_grade.txt, section 2: two builds do not fit one process).  The default is 1 (prhf_plan.h): an
    untouched context gives strided_grade = 1's bits, and 2 is no value."""
    alt, den, bmag, bpsi = profiles
    for n_points in (8192, 20000):
        assert same_bits(run(ctxs["plain"], FREQ, den, bmag, bpsi, alt, n_points)[0], batches[n_points]["plain"])
    assert same_bits(run(ctxs["untouched"], FREQ, den, bmag, bpsi, alt, 8192)[0], batches[8192]["graded"])
    with pytest.raises(Exception):
        ctxs["untouched"].set_option("strided_grade", 2)


def test_mixed_work_list_equals_separate_launches(ctxs, profiles, batches):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on = ctxs["graded"]
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert same_bits(out[:10], run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O")[0])
    assert same_bits(out[10:], batches[20000]["graded"][10:])
    # ... and across two launches: the first ten profiles alone
    assert same_bits(run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 20000)[0], batches[20000]["graded"][:10])


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - X + Y constant in a segment, and segments
    whose continuation reaches X + Y = 1 right behind their end."""
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    got, plain, full = (run(ctxs[k], freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points)[0]
                        for k in ("graded", "plain", "full"))
    close(got, full, f"plateau rows 5-9 X/{n_points}, strided_grade = 1 against strided_top = 0")
    close(got, plain, f"plateau rows 5-9 X/{n_points}, strided_grade = 1 against 0")


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    got = run(ctxs["graded"], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)[0]
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference, strided_grade = 1: {worst:.2e}")
    assert not same_bits(got, run(ctxs["plain"], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)[0])


def test_other_launches_keep_their_bits(ctxs, profiles):
    alt, den, bmag, bpsi = profiles

    def untouched(label, *args, **kwargs):
        got = run(ctxs["graded"], *args, **kwargs)[0]
        assert np.isfinite(got).any(), label
        assert same_bits(got, run(ctxs["plain"], *args, **kwargs)[0]), label

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
