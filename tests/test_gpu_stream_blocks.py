"""The streaming form of the persistent launch (option stream_blocks): one 16-wave workgroup per CU with two
staged profiles, the next one staged by a single wave while the others sum the current one, no barrier per profile.  A
value never depended on which wave computed it, nor on how many threads staged its profile, so every comparison here
is bit identity (same_bits): stream_blocks = 2 against stream_blocks = 0 of the same binary in one process - virtual
heights, the three pairs of counters (prhf_pair_plan_counters, prhf_panel_counters, prhf_panel_upper_counters) and the
call's status - and, for the launches of tests/panel_bits_cases.py, against tests/golden/g27_panel_bits.npz.

stream_blocks = 2 takes the form for launches of fewer blocks than the device keeps resident; stream_grid = 1 lets ONE
workgroup draw every block (24 profiles x 48 whole pairs are 72 blocks: each of its two slots is recycled 36 times),
stream_grid = 2 two.  prhf_stream_launches tells that a launch took the form - or, for the launches that must keep the
general kernel (O mode, a mixed list, a tall column, chunked pairs, few profiles), that it did not.

Contexts of the test's own with target_waves = 64, as in test_gpu_pair_plan.py: 24 x 48 pairs are whole work items."""

import numpy as np
import pytest

import panel_bits_cases as cases
from conftest import load_golden, same_bits
from test_gpu_panel_sum import FREQ, grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    made = {"off": cases.make_context(stream_blocks=0),
            "one": cases.make_context(stream_blocks=2, stream_grid=1),
            "two": cases.make_context(stream_blocks=2, stream_grid=2),
            "all": cases.make_context(stream_blocks=2),
            "default": cases.make_context(),
            "nodes8 off": cases.make_context(stream_blocks=0, panel_nodes=8),
            "nodes8 one": cases.make_context(stream_blocks=2, stream_grid=1, panel_nodes=8),
            "no plans off": cases.make_context(stream_blocks=0, pair_plan=0),
            "no plans one": cases.make_context(stream_blocks=2, stream_grid=1, pair_plan=0),
            "cap off": cases.make_context(stream_blocks=0, pair_plan_cap=4),
            "cap one": cases.make_context(stream_blocks=2, stream_grid=1, pair_plan_cap=4),
            # the quartered tail at this size: tail_rounds x 512 slots = the last six of 24 one-block profiles
            "tail off": cases.make_context(stream_blocks=0, split_few_profiles=0, tail_bpp=4, tail_rounds=6.0 / 512),
            "tail one": cases.make_context(stream_blocks=2, stream_grid=1, split_few_profiles=0, tail_bpp=4, tail_rounds=6.0 / 512),
            "tail two": cases.make_context(stream_blocks=2, stream_grid=2, split_few_profiles=0, tail_bpp=4, tail_rounds=6.0 / 512)}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mode="X", check=True):
    """(virtual heights, the six counters' increase, return code, launches that took the streaming form) of one call"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points)
    out = np.full((d.shape[0], f.size), -7.0)
    counters = lambda: ctx.pair_plan_counters() + ctx.panel_counters() + ctx.panel_upper_counters()     # noqa: E731
    before, streamed = counters(), ctx.stream_launches()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    if check:
        _native.raise_for(rc)
    after = counters()
    return out, np.array([x - y for x, y in zip(after, before)], dtype=np.int64), rc, ctx.stream_launches() - streamed


def same_launch(ctxs, on, off, *args, streamed=1, label="", **kwargs):
    """The call on context `on` against context `off`: bits, counters, status; `streamed`: launches that took the form."""
    want, counted_off, rc_off, s_off = run(ctxs[off], *args, check=False, **kwargs)
    got, counted, rc, s_on = run(ctxs[on], *args, check=False, **kwargs)
    finite = int(np.isfinite(want).sum())
    print(f"{label or on}: {want.shape[0]} x {want.shape[1]}, {finite} finite, counters {counted.tolist()} (off: {counted_off.tolist()}), "
          f"status {rc} (off: {rc_off}), streamed {s_on}")
    assert s_off == 0
    assert s_on == streamed, label
    assert rc == rc_off, label
    assert same_bits(got, want), label
    assert np.array_equal(counted, counted_off), label
    return got, counted, rc


# ---- the base case: 24 x 48 at the smallest grids of the strided and panel sums ----------------------------------------

@pytest.mark.parametrize("n_points", [8192, 8200, 20000])
@pytest.mark.parametrize("on", ["one", "two", "all"])
def test_base_case_against_the_general_kernel_and_the_recorded_bits(ctxs, inputs, on, n_points):
    _, args, kwargs = inputs[f"b{n_points}_p4"]
    got, counted, rc = same_launch(ctxs, on, "off", *args, **kwargs)
    assert rc == 0 and np.isfinite(got).mean() > 0.3 and counted[0] > 0 and counted[2] > 0
    recorded = load_golden("g27_panel_bits.npz")
    if str(recorded["hipcc"]) == cases.hipcc_version_line():
        assert same_bits(got, recorded[f"b{n_points}_p4_vh"])
    else:
        print("the fixture was written under another compiler: its bits are not this build's")
    assert np.array_equal(counted[2:], recorded[f"b{n_points}_p4_counters"])


@pytest.mark.parametrize("name", ["b8192_p8", "b8200_p8", "long65535", "plateau8192", "plateau20000"])
def test_recorded_launches(ctxs, inputs, name):
    """The other launches of g27 that are eligible: eight-lane pieces, 65535 points, the plateau rows (pairs that fall back)."""
    nodes, args, kwargs = inputs[name]
    on, off = ("nodes8 one", "nodes8 off") if nodes == 8 else ("one", "off")
    got, counted, _ = same_launch(ctxs, on, off, *args, label=name, **kwargs)
    recorded = load_golden("g27_panel_bits.npz")
    if str(recorded["hipcc"]) == cases.hipcc_version_line():
        assert same_bits(got, recorded[f"{name}_vh"])
    assert np.array_equal(counted[2:], recorded[f"{name}_counters"])


# ---- frequency counts: the stager's rounds of 64 --------------------------------------------------------------------------

@pytest.mark.parametrize("n_freq", [256, 100, 512, 64, 65])
def test_frequency_rounds(ctxs, inputs, n_freq):
    """256: four rounds; 100: a ragged last round; 512: the limit; 64 and 65: one round exactly, one frequency more."""
    _, (_, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    freq = np.linspace(0.5, 13.0, n_freq)
    rows = slice(0, 6)
    got, counted, _ = same_launch(ctxs, "one", "off", freq, den[rows], bmag[rows], bpsi[rows], alt, 8192, label=f"{n_freq} frequencies")
    assert np.isfinite(got).mean() > 0.3 and counted[0] > 0


# ---- block counts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("on", ["one", "two", "all"])
@pytest.mark.parametrize("rows,n_freq", [(1, 80), (2, 100), (3, 48)])
def test_block_counts(ctxs, inputs, on, rows, n_freq):
    """One profile (80 whole pairs: eight blocks), two profiles, three profiles x 48 (nine blocks: an odd number - the
    last visit of one slot finds the queue empty)."""
    _, (_, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    freq = np.linspace(0.5, 13.0, n_freq)
    got, _, _ = same_launch(ctxs, on, "off", freq, den[:rows], bmag[:rows], bpsi[:rows], alt, 8192, label=f"{rows} profiles, {on}")
    assert np.isfinite(got).any()


# ---- unusual profiles -----------------------------------------------------------------------------------------------------

def unusual(inputs, kind):
    _, (_, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    den, bmag, bpsi = den.copy(), bmag.copy(), bpsi.copy()
    alt2 = np.tile(alt, (den.shape[0], 1))
    freq = FREQ
    k = int(np.argmax(den[5]))
    if kind == "no reflecting frequency":
        den[5] *= 1e-4                         # every plasma frequency far below the lowest sounding frequency: an empty slot
    elif kind == "NaN row":
        bmag[5, k // 2] = np.nan               # NaN in |B| below the peak: the whole X-mode row is NaN, no error
    elif kind == "NaN altitude":
        alt2[5, 3] = np.nan                    # NaN in the altitude column: a NaN row
    elif kind == "negative density":
        den[5, k // 3] = -1.0                  # the call's error status, the other rows as ever
    elif kind == "ragged altitudes":
        alt2[5, 1:k] += 0.37 * np.sin(np.arange(1, k))     # still increasing (the levels are kilometres apart): the hint table
    elif kind == "peak at level 1":
        den[5, 1] = 10.0 * den[5].max()        # K = 1: one level below the peak
    elif kind == "peak at level 0":
        den[5, 0] = 10.0 * den[5].max()        # K = 0: the call's error status
    return freq, den, bmag, bpsi, alt2


@pytest.mark.parametrize("kind", ["no reflecting frequency", "NaN row", "NaN altitude", "negative density", "ragged altitudes",
                                  "peak at level 1", "peak at level 0"])
def test_unusual_profiles(ctxs, inputs, kind):
    freq, den, bmag, bpsi, alt2 = unusual(inputs, kind)
    if kind == "ragged altitudes":
        assert (np.diff(alt2[5]) > 0).all() and np.unique(np.round(np.diff(alt2[5, :40]), 6)).size > 1
    got, _, rc = same_launch(ctxs, "one", "off", freq, den, bmag, bpsi, alt2, 8192, label=kind)
    assert (rc != 0) == (kind in ("negative density", "peak at level 0")), rc
    if kind in ("no reflecting frequency", "NaN row", "NaN altitude"):
        assert np.isnan(got[5]).all()
    assert np.isfinite(np.delete(got, 5, axis=0)).mean() > 0.3
    # ... and the profiles beside the unusual one are what they are in the plain batch
    _, (_, d0, b0, p0, a0, _), _ = inputs["b8192_p4"]
    plain = run(ctxs["off"], FREQ, d0, b0, p0, a0, 8192)[0]
    assert same_bits(np.delete(got, 5, axis=0), np.delete(plain, 5, axis=0))


# ---- the tail, the plans, a second run -----------------------------------------------------------------------------------

@pytest.mark.parametrize("on", ["tail one", "tail two"])
def test_quartered_tail(ctxs, inputs, on):
    """tail_bpp = 4 over the last six of 24 one-block profiles (24 >= 4 x 6; 48 frequencies >= 4 x 8): 18 + 24 blocks in
    the general kernel, 18 + 12 in the streaming form, which cuts its tail half as fine."""
    _, args, kwargs = inputs["b8192_p4"]
    got, _, _ = same_launch(ctxs, on, "tail off", *args, label=on, **kwargs)
    assert same_bits(got, run(ctxs["off"], *args, **kwargs)[0])


@pytest.mark.parametrize("plans", ["no plans", "cap"])
@pytest.mark.parametrize("n_points", [8192, 20000])
def test_without_plans_and_with_four_per_block(ctxs, inputs, plans, n_points):
    _, args, kwargs = inputs[f"b{n_points}_p4"]
    got, counted, _ = same_launch(ctxs, f"{plans} one", f"{plans} off", *args, label=plans, **kwargs)
    assert (counted[0] == 0) if plans == "no plans" else (counted[0] > 0 and counted[1] > 0)
    assert same_bits(got, run(ctxs["off"], *args, **kwargs)[0])


def test_second_run_of_the_same_call(ctxs, inputs):
    _, args, kwargs = inputs["b8200_p4"]
    first, counted, _ = same_launch(ctxs, "one", "off", *args, **kwargs)
    again, counted2, rc, streamed = run(ctxs["one"], *args, **kwargs)
    assert streamed == 1 and rc == 0
    assert same_bits(first, again) and np.array_equal(counted, counted2)


# ---- launches that keep the general kernel --------------------------------------------------------------------------------

def test_ineligible_launches_keep_the_general_kernel(ctxs, inputs):
    from pyrayhf_amd import _native
    _, (freq, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    on, off = ctxs["all"], ctxs["off"]

    def kept(label, *args, **kwargs):
        got, _, _ = same_launch(ctxs, "all", "off", *args, streamed=0, label=label, **kwargs)
        assert np.isfinite(got).any(), label

    kept("O mode", freq, den, bmag, bpsi, alt, 8192, mode="O")
    kept("4096 points", freq, den, bmag, bpsi, alt, 4096)
    kept("600 frequencies", np.linspace(0.5, 13.0, 600), den[:4], bmag[:4], bpsi[:4], alt, 8192)
    kept("one profile, chunked pairs", freq, den[3], bmag[3], bpsi[3], alt, 20000)
    # g27's non-uniform altitude grid: 42 frequencies on 12 levels - more frequencies than the staged arrays have levels,
    # so reflection heights are not settled per thread
    _, nargs, nkw = inputs["nonuniform"]
    kept("more frequencies than levels", *nargs, **nkw)
    # a tall column: more levels than LDS holds below the peak
    tall_alt = np.linspace(alt[0], alt[-1], 3000)
    interp = lambda x: np.stack([np.interp(tall_alt, alt, r) for r in x[:2]])           # noqa: E731
    tden = interp(den)
    assert int(np.argmax(tden, axis=1).max()) > 1400
    kept("tall column", freq, tden, interp(bmag), interp(bpsi), tall_alt, 8192)
    # few profiles with the default option: fewer blocks than resident slots is not a persistent launch
    got, _, _, streamed = run(ctxs["default"], freq, den, bmag, bpsi, alt, 8192)
    assert streamed == 0 and same_bits(got, run(off, freq, den, bmag, bpsi, alt, 8192)[0])
    # a mixed list
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * freq.size)]
    outs = []
    for ctx in (on, off):
        out = np.full((24, freq.size), -7.0)
        streamed = ctx.stream_launches()
        rc = ctx.vfo_worklist(freq.ctypes.data, freq.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                              24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
        _native.raise_for(rc)
        assert ctx.stream_launches() == streamed
        outs.append(out)
    assert same_bits(outs[0], outs[1])
    # ... whose long slice alone takes the form, with the same bits
    alone = same_launch(ctxs, "all", "off", freq, den[10:], bmag[10:], bpsi[10:], alt, 20000, label="the long slice alone")[0]
    assert same_bits(outs[0][10:], alone)
