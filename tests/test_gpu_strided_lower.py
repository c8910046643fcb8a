"""The strided sum of the segments below the top three (option strided_lower) against the same binary
with the option off and with strided_top off, in one process: whole pairs of at least 8192 points in X mode on a
uniform altitude grid and the reference's stretch take the rule, everything else must not notice.

Bound: 1e-11 of the virtual height, the bound of test_gpu_strided_sum; the rule's own error, measured on the CPU
against the oracle (tests/test_strided_lower_host.py), is below 1.1e-13 from 8192 points up.

Three contexts of the test's own (options are per context).  target_waves = 64 so that 24 x 48 pairs are whole work
items, while one profile x 48 frequencies is still chunked."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from parity import assert_masks, assert_x_mode, rel_err

pytestmark = pytest.mark.gpu

FREQ = np.linspace(0.5, 13.0, 48)


@pytest.fixture(scope="module")
def ctxs():
    from pyrayhf_amd import _native
    on, top_only, full = _native.Context(0), _native.Context(0), _native.Context(0)
    for c in (on, top_only, full):
        c.set_option("target_waves", 64)
    top_only.set_option("strided_lower", 0)
    full.set_option("strided_top", 0)
    yield on, top_only, full
    for c in (on, top_only, full):
        c.close()


@pytest.fixture(scope="module")
def profiles():
    from pyrayhf_amd import synth
    return synth.chapman_profiles(24, 20261017)          # alt, den, bmag, bpsi


def grid(n_points, sharpness=10.0):
    from pyrayhf_amd import library
    return np.ascontiguousarray(library.smooth_nonuniform_grid(0, 1, n_points, sharpness))


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mult=None, mode="X"):
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points) if mult is None else mult
    out = np.full((d.shape[0], f.size), -7.0)
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    return out


def close(got, want, label):
    assert_masks(got, want)
    err, ok = rel_err(got, want)
    worst = float(err.max(initial=0.0))
    print(f"{label}: {int(ok.sum())} finite pairs, worst {worst:.2e}, {int((got[ok] != want[ok]).sum())} pairs differ")
    assert worst <= 1e-11


@pytest.mark.parametrize("n_points", [8191, 8192, 8200, 20000])
def test_synthetic_batch_against_both_other_sums(ctxs, profiles, n_points):
    alt, den, bmag, bpsi = profiles
    got, top_only, full = (run(c, FREQ, den, bmag, bpsi, alt, n_points) for c in ctxs)
    assert np.isfinite(full).mean() > 0.3
    if n_points < 8192:                                    # below the threshold: today's launch
        assert same_bits(got, top_only) and same_bits(got, full)
        return
    close(got, top_only, f"24 x 48 X/{n_points} against strided_lower = 0")
    close(got, full, f"24 x 48 X/{n_points} against strided_top = 0")
    assert not same_bits(got, top_only)                    # (the rule was taken: another order of additions at least)


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_rows(ctxs, n_points):
    """Rows 5-9: a vacuum-to-plasma jump and a plateau under the reflection - the pairs where the guard decides."""
    from test_strided_sum_host import plateau_inputs
    freq, alt, den, bmag, bpsi = plateau_inputs()
    got, top_only = (run(c, freq, den[5:10], bmag[5:10], bpsi[5:10], alt, n_points) for c in ctxs[:2])
    close(got, top_only, f"plateau rows 5-9 X/{n_points} against strided_lower = 0")


def test_config4_rows_against_the_reference_g14(ctxs):
    g = load_golden("g14_config4_rows.npz")
    got = run(ctxs[0], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000)
    worst = assert_x_mode(got, g["X_20000_vh"], tol=1e-10)
    print(f"G14 against the reference: {worst:.2e}")
    assert not same_bits(got, run(ctxs[1], g["freq"], g["den"], g["bmag"], g["bpsi"], g["alt"], 20000))


def test_nonuniform_altitude_grid_keeps_its_launch(ctxs):
    g = load_golden("g7_edges.npz")
    freq, den, bmag, bpsi, alt = (g[f"nonuniform_{k}"] for k in ("freq", "den", "bmag", "bpsi", "alt"))
    assert np.unique(np.round(np.diff(alt), 6)).size > 1
    tile = lambda x: np.tile(x, (24, 1))                   # noqa: E731
    a = run(ctxs[0], freq, tile(den), tile(bmag), tile(bpsi), alt, 8192)
    assert np.isfinite(a).any()
    assert same_bits(a, run(ctxs[1], freq, tile(den), tile(bmag), tile(bpsi), alt, 8192))


def test_other_grids_chunked_launches_and_o_mode_keep_their_launch(ctxs, profiles):
    alt, den, bmag, bpsi = profiles
    on, top_only = ctxs[:2]
    m5 = grid(8192, sharpness=5.0)                         # a grid the C ABI accepts that is not the reference's stretch
    a = run(on, FREQ, den, bmag, bpsi, alt, 8192, mult=m5)
    assert np.isfinite(a).mean() > 0.3
    assert same_bits(a, run(top_only, FREQ, den, bmag, bpsi, alt, 8192, mult=m5))
    lin = np.linspace(0.0, 1.0, 8192)
    assert same_bits(run(on, FREQ, den, bmag, bpsi, alt, 8192, mult=lin), run(top_only, FREQ, den, bmag, bpsi, alt, 8192, mult=lin))
    # one profile: the pairs are cut into chunks
    one = run(on, FREQ, den[3], bmag[3], bpsi[3], alt, 20000)
    assert np.isfinite(one).mean() > 0.3
    assert same_bits(one, run(top_only, FREQ, den[3], bmag[3], bpsi[3], alt, 20000))
    o = run(on, FREQ, den, bmag, bpsi, alt, 8192, mode="O")
    assert np.isfinite(o).mean() > 0.3
    assert same_bits(o, run(top_only, FREQ, den, bmag, bpsi, alt, 8192, mode="O"))


def test_mixed_work_list_equals_separate_launches(ctxs, profiles):
    from pyrayhf_amd import _native
    alt, den, bmag, bpsi = profiles
    on = ctxs[0]
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert same_bits(out[:10], run(on, FREQ, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O"))
    sep = run(on, FREQ, den[10:], bmag[10:], bpsi[10:], alt, 20000)
    assert same_bits(out[10:], sep)
    assert not same_bits(sep, run(ctxs[1], FREQ, den[10:], bmag[10:], bpsi[10:], alt, 20000))


def test_two_launches_are_bit_identical(ctxs, profiles):
    alt, den, bmag, bpsi = profiles
    assert same_bits(run(ctxs[0], FREQ, den, bmag, bpsi, alt, 20000), run(ctxs[0], FREQ, den, bmag, bpsi, alt, 20000))
