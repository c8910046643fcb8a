"""The quick bound of the panel sum's lists (option panel_quick): a list whose runs all pass a bound from
1 - X - Y at their segments' levels skips the runs' exact tests, which would find nothing.  The bound implies what the
tests find (tests/test_panel_quick_host.py), so every comparison here is bit identity (same_bits) and equal counters
(prhf_panel_counters, prhf_panel_upper_counters, prhf_panel_plan_counters, prhf_pair_plan_counters), not a tolerance:
panel_quick = 1 against panel_quick = 0 of the same binary in one process, on the five arms of test_gpu_panel_plan.py -
default, pair_plan = 0, pair_plan_cap = 4, stream_blocks = 0, the streaming form.

prhf_panel_quick_counters is what shows that the quick path runs at all: its first word, the list passes that took it, is
positive with the option on and is the NumPy model's count on the launches test_panel_quick_host.QUICK_PASSES records;
its second word, the passes that took the exact tests, is the model's too, and both words together are the passes of
the launch with the option off.  The first word is zero with the option off, and both are zero on every launch the
panel sum's upper instance does not touch: O mode, a non-uniform altitude grid, 4096 points, and panel_upper,
panel_lower or strided_lower off.

The launches are those of tests/panel_bits_cases.py.  Contexts with target_waves = 64, as in test_gpu_pair_plan.py."""

import numpy as np
import pytest

import panel_bits_cases as cases
from conftest import same_bits
from test_gpu_panel_plan import ARMS
from test_gpu_panel_sum import grid
from test_panel_quick_host import QUICK_PASSES

pytestmark = pytest.mark.gpu

NAMES = ("planned", "own", "took", "fell", "reached", "kept", "region", "quick", "exact")
SAME = ("planned", "own", "took", "fell", "reached", "kept", "region")


@pytest.fixture(scope="module")
def ctxs():
    """{arm: (context with panel_quick = 1, with panel_quick = 0)}"""
    made = {name: (cases.make_context(**options), cases.make_context(panel_quick=0, **options))
            for name, options in ARMS.items()}
    yield made
    for pair in made.values():
        for c in pair:
            c.close()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mode="X", mult=None):
    """(virtual heights, {counter: increase}) of one call"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points) if mult is None else np.ascontiguousarray(mult, dtype=np.float64)
    out = np.full((d.shape[0], f.size), -7.0)
    counters = lambda: (ctx.pair_plan_counters() + ctx.panel_counters() + ctx.panel_upper_counters() +     # noqa: E731
                        ctx.panel_plan_counters() + ctx.panel_quick_counters())
    before = counters()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    return out, dict(zip(NAMES, (x - y for x, y in zip(counters(), before))))


def all_arms(ctxs, label, case, *args, **kwargs):
    """The launch with and without the option on every arm.  Returns the default arm's counters with the option on."""
    first = None
    for name, (on, off) in ctxs.items():
        out_on, c_on = run(on, *args, **kwargs)
        out_off, c_off = run(off, *args, **kwargs)
        print(f"{label}, {name}: {int(np.isfinite(out_on).sum())} finite; on {c_on}; off {c_off}")
        assert same_bits(out_on, out_off), (label, name)
        assert [c_on[k] for k in SAME] == [c_off[k] for k in SAME], (label, name)
        # the lists are the same lists: the option only moves a pass from one word to the other
        assert c_off["quick"] == 0, (label, name)
        assert c_on["quick"] + c_on["exact"] == c_off["exact"], (label, name)
        assert c_on["quick"] > 0, (label, name)
        if first is None:
            first = (out_on, c_on)
        # ... and what the passes are depends on the pair alone, not on who planned it or which kernel summed it
        assert same_bits(out_on, first[0]), (label, name)
        assert (c_on["quick"], c_on["exact"]) == (first[1]["quick"], first[1]["exact"]), (label, name)
    if case in QUICK_PASSES:
        assert (first[1]["quick"], first[1]["exact"]) == QUICK_PASSES[case], label
    return first[1]


@pytest.mark.parametrize("n_points", [8192, 8200, 20000])
def test_plain_batch(ctxs, inputs, n_points):
    case = f"b{n_points}_p4"
    _, args, kwargs = inputs[case]
    c = all_arms(ctxs, f"24 x 48 X/{n_points}", case, *args, **kwargs)
    assert c["took"] > 0


def test_largest_grid(ctxs, inputs):
    _, args, kwargs = inputs["long65535"]
    c = all_arms(ctxs, "24 x 8 X/65535", "long65535", *args, **kwargs)
    assert c["took"] > 0


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_and_no_field_rows(ctxs, inputs, n_points):
    """Pairs that fall back and pairs that keep the lower region: lists made a second time, lists left half-way."""
    case = f"plateau{n_points}"
    _, args, kwargs = inputs[case]
    c = all_arms(ctxs, f"plateau rows 5-9 X/{n_points}", case, *args, **kwargs)
    assert c["fell"] > 0 and c["kept"] > 0


def test_launches_the_quick_path_does_not_touch(ctxs, inputs):
    on, off = ctxs["default"]

    def none(label, *args, **kwargs):
        out, c = run(on, *args, **kwargs)
        print(f"{label}: {c}")
        assert np.isfinite(out).any(), label
        assert (c["quick"], c["exact"]) == (0, 0), label
        assert same_bits(out, run(off, *args, **kwargs)[0]), label

    for name in cases.UNTOUCHED:
        _, args, kwargs = inputs[name]
        none(name, *args, **kwargs)
    _, (freq, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    for option in ("panel_upper", "panel_lower", "strided_lower"):
        ctx, ref = cases.make_context(**{option: 0}), cases.make_context(panel_quick=0, **{option: 0})
        try:
            out, c = run(ctx, freq, den, bmag, bpsi, alt, 8192)
            print(f"{option} = 0: {c}")
            assert np.isfinite(out).any(), option
            assert (c["quick"], c["exact"]) == (0, 0), option
            assert same_bits(out, run(ref, freq, den, bmag, bpsi, alt, 8192)[0]), option
        finally:
            ctx.close()
            ref.close()
