"""The diagnostic counters after the workgroups count in LDS and flush once, when they leave the kernel:
the seven words of KArgs::plan_counters and the two sums of the quick slots are what they were when every wave added to
them at the end of every block.  Counts are integers, so every comparison is equality.

Each figure is the increase over one call, read after the call returned: prhf_pair_plan_counters (planned, own),
prhf_panel_counters (took, fell), prhf_panel_upper_counters (reached, kept), prhf_panel_plan_counters (region) and
prhf_panel_quick_counters (quick, exact) - nine figures in the order of NAMES.

The ways out of a kernel, each of which must flush:
  one / two / all   the streaming form with one workgroup (each slot recycled 36 times), two, one per two blocks: every
                    wave leaves through the slot's `finished` word, the workgroup's last barrier, two slots' counts
  off               stream_blocks = 0; 72 blocks are fewer than the device keeps resident, so this is the general
                    kernel with one block per workgroup, as with persistent = 0 (`no queue`)
  queue             stream_blocks = 0 on 528 profiles: more blocks than any device has slots (at least one per
                    profile), the general kernel's persistent loop, left through the empty queue
  tail *            the quartered tail of test_gpu_stream_blocks.py
Independent truths: tests/golden/g27_panel_bits.npz's counters of the 24 x 48 launches, recorded several commits ago,
and the NumPy model's list passes (tests/test_panel_quick_host.py).

Contexts of tests/panel_bits_cases.py: target_waves = 64, so that 24 x 48 pairs are whole work items."""

import numpy as np
import pytest

import panel_bits_cases as cases
from conftest import load_golden, same_bits
from test_gpu_panel_sum import FREQ, grid
from test_gpu_stream_blocks import unusual
from test_panel_quick_host import QUICK_PASSES

pytestmark = pytest.mark.gpu

NAMES = ("planned", "own", "took", "fell", "reached", "kept", "region", "quick", "exact")
TAIL = dict(split_few_profiles=0, tail_bpp=4, tail_rounds=6.0 / 512)
ARMS = {"off": dict(stream_blocks=0),
        "no queue": dict(stream_blocks=0, persistent=0),
        "one": dict(stream_blocks=2, stream_grid=1),
        "two": dict(stream_blocks=2, stream_grid=2),
        "all": dict(stream_blocks=2),
        "tail off": dict(stream_blocks=0, **TAIL),
        "tail one": dict(stream_blocks=2, stream_grid=1, **TAIL),
        "tail two": dict(stream_blocks=2, stream_grid=2, **TAIL)}
STREAMED = ("one", "two", "all", "tail one", "tail two")
TILES = 22                                     # 22 x 24 = 528 profiles: the `queue` launch


@pytest.fixture(scope="module")
def ctxs():
    made = {name: cases.make_context(**options) for name, options in ARMS.items()}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


def read(ctx):
    return np.array(ctx.pair_plan_counters() + ctx.panel_counters() + ctx.panel_upper_counters() + ctx.panel_plan_counters() +
                    ctx.panel_quick_counters(), dtype=np.int64)


def call(ctx, freq, den, bmag, bpsi, alt, n_points, mode="X"):
    """(virtual heights, return code) of one call; reads no counter"""
    from pyrayhf_amd import _native
    f = np.ascontiguousarray(freq, dtype=np.float64)
    d, b, p = (np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64) for x in (den, bmag, bpsi))
    a = np.ascontiguousarray(alt, dtype=np.float64)
    m = grid(n_points)
    out = np.full((d.shape[0], f.size), -7.0)
    rc = ctx.vfo_batch(f.ctypes.data, f.size, d.ctypes.data, b.ctypes.data, p.ctypes.data, a.ctypes.data, d.shape[0],
                       d.shape[1], d.shape[1], d.shape[1] if a.ndim == 2 else 0, m.ctypes.data, int(n_points),
                       _native.MODE_X if mode == "X" else _native.MODE_O, out.ctypes.data, 0)
    return out, rc


def run(ctx, *args, **kwargs):
    """(virtual heights, the nine figures' increase, return code, launches that took the streaming form) of one call"""
    before, streamed = read(ctx), ctx.stream_launches()
    out, rc = call(ctx, *args, **kwargs)
    return out, read(ctx) - before, rc, ctx.stream_launches() - streamed


def every_arm(ctxs, arms, label, *args, forms=True, **kwargs):
    """The call on every arm: equal bits, status and figures (forms: and the streaming arms took the streaming form).
    Returns the first arm's."""
    first = None
    for name in arms:
        out, counted, rc, streamed = run(ctxs[name], *args, **kwargs)
        print(f"{label}, {name}: {dict(zip(NAMES, counted.tolist()))}, status {rc}, streamed {streamed}")
        if forms:
            assert streamed == (1 if name in STREAMED else 0), (label, name)
        if first is None:
            first = (out, counted, rc)
        assert same_bits(out, first[0]), (label, name)
        assert rc == first[2], (label, name)
        assert np.array_equal(counted, first[1]), (label, name)
    return first


# ---- 1. every exit path gives the same totals -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(ctxs, inputs):
    """{n_points: (bits, figures)} of the 24 x 48 launches, every arm held to the first"""
    found = {}
    for n_points in (8192, 20000):
        _, args, kwargs = inputs[f"b{n_points}_p4"]
        out, counted, rc = every_arm(ctxs, ("off", "no queue", "one", "two", "all"), f"24 x 48 X/{n_points}", *args, **kwargs)
        assert rc == 0
        found[n_points] = (out, counted)
    return found


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_every_exit_path_gives_the_recorded_totals(base, n_points):
    _, counted = base[n_points]
    c = dict(zip(NAMES, counted.tolist()))
    recorded = load_golden("g27_panel_bits.npz")
    assert np.array_equal(counted[2:6], recorded[f"b{n_points}_p4_counters"])
    assert c["planned"] > 0 and c["took"] > 0 and c["region"] > 0 and c["quick"] > 0
    # a pair runs from a plan or plans itself; one that took the panel sum under panel_upper reached the top or kept the lower region
    assert c["reached"] + c["kept"] == c["took"] and c["region"] <= c["planned"]
    if n_points == 20000:
        assert (c["quick"], c["exact"]) == QUICK_PASSES["b20000_p4"] == (1103, 509)


@pytest.mark.parametrize("n_points", [8192, 20000])
def test_the_quartered_tail_gives_the_same_totals(ctxs, inputs, base, n_points):
    """The tail cuts six profiles into more blocks: other workgroups count the same pairs."""
    _, args, kwargs = inputs[f"b{n_points}_p4"]
    out, counted, _ = every_arm(ctxs, ("tail off", "tail one", "tail two"), f"tail X/{n_points}", *args, **kwargs)
    assert same_bits(out, base[n_points][0])
    assert np.array_equal(counted, base[n_points][1])


def test_the_persistent_loop_of_the_general_kernel(ctxs, inputs, base):
    """528 profiles (the 24 of the base case, 22 times) are more blocks than workgroup slots: with stream_blocks = 0 the
    general kernel's workgroups each run several blocks and flush behind the loop.  A count belongs to a pair, so the
    figures are 22 times the base case's, as they are with one block per workgroup."""
    _, (freq, den, bmag, bpsi, alt, n), _ = inputs["b8192_p4"]
    tile = lambda x: np.tile(x, (TILES, 1))                # noqa: E731
    args = (freq, tile(den), tile(bmag), tile(bpsi), alt, n)
    out, counted, rc, streamed = run(ctxs["off"], *args)
    out0, counted0, rc0, _ = run(ctxs["no queue"], *args)
    print(f"queue: {counted.tolist()}; no queue: {counted0.tolist()}")
    assert rc == 0 and rc0 == 0 and streamed == 0
    assert same_bits(out, out0) and same_bits(out, np.tile(base[8192][0], (TILES, 1)))
    assert np.array_equal(counted, counted0)
    assert np.array_equal(counted, TILES * base[8192][1])


# ---- 2. accumulation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ["one", "all", "off"])
def test_three_calls_leave_three_times_one_calls_increase(ctxs, inputs, base, arm):
    _, args, kwargs = inputs["b20000_p4"]
    ctx = ctxs[arm]
    before = read(ctx)
    for _ in range(3):
        out, rc = call(ctx, *args, **kwargs)
        assert rc == 0
    counted = read(ctx) - before
    print(f"{arm}: {counted.tolist()}")
    assert same_bits(out, base[20000][0])
    assert np.array_equal(counted, 3 * base[20000][1])


def test_three_calls_on_the_persistent_general_kernel(ctxs, inputs, base):
    _, (freq, den, bmag, bpsi, alt, n), _ = inputs["b8192_p4"]
    tile = lambda x: np.tile(x, (TILES, 1))                # noqa: E731
    ctx = ctxs["off"]
    before = read(ctx)
    for _ in range(3):
        assert call(ctx, freq, tile(den), tile(bmag), tile(bpsi), alt, n)[1] == 0
    assert np.array_equal(read(ctx) - before, 3 * TILES * base[8192][1])


# ---- 3. block counts that end a slot early ------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,n_freq", [(1, 80), (3, 48)])
def test_block_counts(ctxs, inputs, rows, n_freq):
    """One profile x 80 whole pairs: eight blocks; three profiles x 48: nine blocks, the last visit of one slot finds the
    queue empty."""
    _, (_, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    freq = np.linspace(0.5, 13.0, n_freq)
    out, counted, rc = every_arm(ctxs, ("off", "one", "two", "all"), f"{rows} x {n_freq}", freq, den[:rows], bmag[:rows],
                                 bpsi[:rows], alt, 8192)
    assert rc == 0 and np.isfinite(out).any() and counted[0] > 0 and counted[2] > 0


# ---- 4. bad rows ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["negative density", "NaN row", "peak at level 0", "no reflecting frequency"])
def test_bad_rows(ctxs, inputs, base, kind):
    """A block that counts nothing and a call that returns an error flush like any other: the other 23 profiles' counts."""
    freq, den, bmag, bpsi, alt2 = unusual(inputs, kind)
    out, counted, rc = every_arm(ctxs, ("off", "one", "two", "all"), kind, freq, den, bmag, bpsi, alt2, 8192)
    assert (rc != 0) == (kind in ("negative density", "peak at level 0")), rc
    c, whole = dict(zip(NAMES, counted.tolist())), dict(zip(NAMES, base[8192][1].tolist()))
    assert 0 < c["planned"] + c["own"] < whole["planned"] + whole["own"]
    assert 0 < c["took"] < whole["took"]
    # the bad profile alone counts nothing (one profile: whichever kernel the launch takes)
    row = slice(5, 6)
    _, alone, rc5 = every_arm(ctxs, ("off", "one"), kind + ", alone", freq, den[row], bmag[row], bpsi[row], alt2[row], 8192,
                             forms=False)
    assert (rc5 != 0) == (rc != 0)
    assert not alone.any(), alone


# ---- 5. kernels that count little or nothing ---------------------------------------------------------------------------------

def test_kernels_that_count_little_or_nothing(ctxs, inputs):
    """O mode, 4096 points, a non-uniform altitude grid (the launches of panel_bits_cases.UNTOUCHED), a tall column
    (vfo_tall_kernel) and a mixed work list (vfo_kernel<2, 512>), at the shapes of test_gpu_stream_blocks.py: the figures of
    the default arm are those of one block per workgroup, and the panel words are zero where nothing takes the panel sum."""
    from pyrayhf_amd import _native
    _, (freq, den, bmag, bpsi, alt, _), _ = inputs["b8192_p4"]
    arms = ("off", "no queue", "all")
    for name in cases.UNTOUCHED:
        _, args, kwargs = inputs[name]
        out, counted, rc, streamed = run(ctxs["off"], *args, **kwargs)
        for arm in arms[1:]:
            out1, counted1, rc1, streamed1 = run(ctxs[arm], *args, **kwargs)
            assert same_bits(out1, out) and rc1 == rc and np.array_equal(counted1, counted), (name, arm)
            assert streamed1 == 0, (name, arm)
        print(f"{name}: {dict(zip(NAMES, counted.tolist()))}")
        assert rc == 0 and np.isfinite(out).any(), name
        assert not counted[2:6].any() and not counted[6:].any(), name      # no panel sum: took, fell, reached, kept, region, passes
    c = dict(zip(NAMES, run(ctxs["off"], *inputs["omode"][1], **inputs["omode"][2])[1].tolist()))
    assert c["planned"] == 0 and c["own"] == 0         # O mode plans nothing
    # a tall column: more levels than LDS holds below the peak; its kernel plans nothing and takes no panel sum
    tall_alt = np.linspace(alt[0], alt[-1], 3000)
    interp = lambda x: np.stack([np.interp(tall_alt, alt, r) for r in x[:2]])           # noqa: E731
    tden = interp(den)
    assert int(np.argmax(tden, axis=1).max()) > 1400
    results = [run(ctxs[arm], freq, tden, interp(bmag), interp(bpsi), tall_alt, 8192) for arm in arms]
    for arm, (out, counted, rc, streamed) in zip(arms, results):
        print(f"tall column, {arm}: {counted.tolist()}")
        assert rc == 0 and streamed == 0 and np.isfinite(out).any()
        assert same_bits(out, results[0][0])
        assert not counted.any(), arm
    # a mixed list: ten profiles O/200, fourteen X/20000 in one launch; the long slice counts what it counts alone
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * freq.size)]
    mixed = []
    for arm in arms:
        ctx = ctxs[arm]
        out = np.full((24, freq.size), -7.0)
        before, streamed = read(ctx), ctx.stream_launches()
        rc = ctx.vfo_worklist(freq.ctypes.data, freq.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                              24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
        _native.raise_for(rc)
        mixed.append((out, read(ctx) - before))
        print(f"mixed list, {arm}: {mixed[-1][1].tolist()}")
        assert ctx.stream_launches() == streamed
        assert same_bits(out, mixed[0][0]) and np.array_equal(mixed[-1][1], mixed[0][1]), arm
    alone = run(ctxs["no queue"], freq, den[10:], bmag[10:], bpsi[10:], alt, 20000)
    assert same_bits(mixed[0][0][10:], alone[0])
    assert mixed[0][1][0] > 0 and mixed[0][1][2] > 0
    assert np.array_equal(mixed[0][1], alone[1])
