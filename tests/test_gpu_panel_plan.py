"""The panel region from the plan: for a pair whose panel block will pass its entry test the planner's
thread computes the region's set-up - its first point S_P, the segments j_s and j_e of its ends, whether it reaches the
top segment - with the functions the pair's wave uses, and leaves out the zones of the two segments below the top one;
the wave reads the record instead of computing the same integers on 64 lanes.  The integers are the same either way, so
every comparison here is bit identity (same_bits) and equal counters (prhf_panel_counters, prhf_panel_upper_counters),
not a tolerance: four arms of the same binary in one process -

  default             every pair of a block has its record
  pair_plan = 0       no records: every wave computes the region itself
  pair_plan_cap = 4   four records per workgroup: both kinds of pair in every profile
  stream_blocks = 0   the general kernel whatever the launch (the workgroup-wide form of plan_pair)

- and a fifth, stream_blocks = 2 with stream_grid = 1, which takes the streaming form, whose lone stager runs the other
form of plan_pair.  prhf_panel_plan_counters counts the records that carry a region: positive, at most
prhf_pair_plan_counters' first word and at most the pairs that came to the panel block (took + fell back), wherever pairs
are planned; zero without plans and on every launch the panel sum does not touch.

The launches are those of tests/panel_bits_cases.py: 24 x 48 at 8192 points (j_min > 0 for every pair that reflects more
than about 102 levels up, so S_P > 0 and first_point(j_min) decides), 8200 (a region end that is no multiple of the
block) and 20000 (j_min = 0 for nearly every pair); 24 x 8 at 65535, the largest grid the block takes; the plateau rows
5-9, whose pairs fall back or keep the lower region and so compute the zones of segments j_top - 1 and j_top - 2
themselves although their record has none.  Contexts with target_waves = 64, as in test_gpu_pair_plan.py."""

import numpy as np
import pytest

import panel_bits_cases as cases
from conftest import same_bits
from test_gpu_panel_sum import FREQ, grid

pytestmark = pytest.mark.gpu

ARMS = {"default": {}, "no plans": {"pair_plan": 0}, "cap 4": {"pair_plan_cap": 4}, "general": {"stream_blocks": 0},
        "stream": {"stream_blocks": 2, "stream_grid": 1}}


@pytest.fixture(scope="module")
def ctxs():
    made = {name: cases.make_context(**options) for name, options in ARMS.items()}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


def run(ctx, freq, den, bmag, bpsi, alt, n_points, mode="X", mult=None):
    """(virtual heights, {counter: increase}, launches that took the streaming form) of one call"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points) if mult is None else np.ascontiguousarray(mult, dtype=np.float64)
    out = np.full((d.shape[0], f.size), -7.0)
    counters = lambda: (ctx.pair_plan_counters() + ctx.panel_counters() + ctx.panel_upper_counters() +     # noqa: E731
                        ctx.panel_plan_counters())
    before, streamed = counters(), ctx.stream_launches()
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    _native.raise_for(rc)
    diff = [x - y for x, y in zip(counters(), before)]
    names = ("planned", "own", "took", "fell", "reached", "kept", "region")
    return out, dict(zip(names, diff)), ctx.stream_launches() - streamed


def all_arms(ctxs, label, *args, **kwargs):
    """The launch on every arm: equal bits, equal panel counters; what the new counter must be on each.  Returns the
    default arm's heights and the counters per arm."""
    got = {name: run(ctx, *args, **kwargs) for name, ctx in ctxs.items()}
    want, base, _ = got["no plans"]
    for name, (out, c, streamed) in got.items():
        print(f"{label}, {name}: {int(np.isfinite(out).sum())} finite, {c}, streamed {streamed}")
        assert same_bits(out, want), (label, name)
        assert [c[k] for k in ("took", "fell", "reached", "kept")] == [base[k] for k in ("took", "fell", "reached", "kept")], (label, name)
        assert streamed == (1 if name == "stream" else 0), (label, name)
        assert 0 <= c["region"] <= c["planned"], (label, name)
        # a record carries a region if and only if its pair passes the block's entry test: each such pair then takes the
        # rule or falls back, and a pair that took the rule had a region in its record unless it planned itself
        assert c["region"] <= c["took"] + c["fell"], (label, name)
        if name != "no plans":
            assert c["region"] >= c["took"] - c["own"], (label, name)
    assert (base["planned"], base["own"], base["region"]) == (0, 0, 0), label
    # the two forms of plan_pair make the same records
    assert got["stream"][1] == got["general"][1] == got["default"][1], label
    return got["default"][0], {name: c for name, (_, c, _) in got.items()}


@pytest.mark.parametrize("n_points", [8192, 8200, 20000])
def test_plain_batch(ctxs, inputs, n_points):
    _, args, kwargs = inputs[f"b{n_points}_p4"]
    out, c = all_arms(ctxs, f"24 x 48 X/{n_points}", *args, **kwargs)
    assert np.isfinite(out).mean() > 0.3
    for name in ("default", "general", "stream", "cap 4"):
        assert c[name]["took"] > 0 and c[name]["region"] > 0, name
    assert c["cap 4"]["own"] > 0 and c["cap 4"]["region"] < c["default"]["region"]


def test_largest_grid(ctxs, inputs):
    _, args, kwargs = inputs["long65535"]
    out, c = all_arms(ctxs, "24 x 8 X/65535", *args, **kwargs)
    assert np.isfinite(out).mean() > 0.3
    assert c["default"]["took"] > 0 and c["default"]["region"] > 0 and c["cap 4"]["region"] > 0


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_plateau_vacuum_and_no_field_rows(ctxs, inputs, n_points):
    """Pairs that fall back and pairs that keep the lower region: with a record of the second form they compute the
    zones of the two segments below the top one themselves."""
    _, args, kwargs = inputs[f"plateau{n_points}"]
    out, c = all_arms(ctxs, f"plateau rows 5-9 X/{n_points}", *args, **kwargs)
    assert np.isfinite(out).any()
    assert c["default"]["fell"] > 0 and c["default"]["kept"] > 0
    assert c["default"]["region"] > 0


def test_launches_without_a_region_in_the_plan(ctxs, inputs):
    on, off = ctxs["default"], ctxs["no plans"]

    def none(label, *args, **kwargs):
        out, c, _ = run(on, *args, **kwargs)
        print(f"{label}: {c}")
        assert np.isfinite(out).any(), label
        assert c["region"] == 0, label
        assert same_bits(out, run(off, *args, **kwargs)[0]), label

    for name in ("omode", "nonuniform"):
        _, args, kwargs = inputs[name]
        none(name, *args, **kwargs)
    _, (freq, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    from pyrayhf_amd import library
    none("sharpness 5", freq, den, bmag, bpsi, alt, 8192,
         mult=np.ascontiguousarray(library.smooth_nonuniform_grid(0, 1, 8192, 5.0)))
    none("linear grid", freq, den, bmag, bpsi, alt, 8192, mult=np.linspace(0.0, 1.0, 8192))
    # the options the second form needs, one at a time: every record keeps the first form
    for option in ("panel_upper", "panel_lower", "strided_lower"):
        ctx = cases.make_context(**{option: 0})
        try:
            out, c, _ = run(ctx, freq, den, bmag, bpsi, alt, 8192)
            print(f"{option} = 0: {c}")
            assert c["planned"] > 0 and c["region"] == 0, option
            ref = cases.make_context(pair_plan=0, **{option: 0})
            try:
                assert same_bits(out, run(ref, freq, den, bmag, bpsi, alt, 8192)[0]), option
            finally:
                ref.close()
        finally:
            ctx.close()
