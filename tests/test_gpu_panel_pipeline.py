"""The panel sum's evaluation loop fetches the next entry's look-ups before it evaluates the entry it has (DESIGN.md
4.1): order of issue and integer bookkeeping only, so every output keeps the bits it had before.  The bits
of before are tests/golden/g27_panel_bits.npz, written by tools/gen_golden_panel_bits.py on the commit before the
change; the launches are those of tests/panel_bits_cases.py, the smallest at which each part can go wrong:

  24 x 48 at X/8192, X/8200, X/20000, panel_nodes 4 and 8   several lists per pair, the general list, a region end that
                                                            is no multiple of the block
  24 x 8 at X/65535                                         lists of more than 64 entries: the second list register
                                                            under the look-ahead, runs near the cap of 128 entries
                                                            (the NumPy model, rows 0-2 of this case: 29 of 50 lists
                                                            have more than 64 entries, 9 have 113 to 128, the
                                                            longest 128)
  plateau rows 5-9 at 8192 and 20000                        pairs that fall back, pairs that keep the lower region (a list
                                                            made a second time)
  O mode, a non-uniform altitude grid, 4096 points          not the panel sum's: same bits, nothing counted

Bound: equal bits, and equal counters (prhf_panel_counters, prhf_panel_upper_counters).  The same source gives the same
bits only under the same compiler: where the fixture's `hipcc --version` line is not the running one, the comparison is
at 1e-13 of the virtual height instead - the size of the differences a change of the order of summation makes - and the
test prints that it did.  The line is that of the compiler installed beside the test, not read from the loaded library:
a library built earlier under another compiler is still held to bits (and may fail for that reason alone), and where
no hipcc is found the line is `unknown` and the comparison is the one at 1e-13.  The other tests compare launches of
the running build with each other: bits, always.

Contexts of the test's own with target_waves = 64, as in test_gpu_panel_sum.py."""

import numpy as np
import pytest

import panel_bits_cases as cases
from conftest import load_golden, same_bits
from parity import rel_err
from test_gpu_panel_sum import FREQ, SIZES, grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return load_golden("g27_panel_bits.npz")


@pytest.fixture(scope="module")
def ctxs():
    made = {4: cases.make_context(panel_nodes=4), 8: cases.make_context(panel_nodes=8),
            "pair_plan = 0": cases.make_context(pair_plan=0), "pair_plan_cap = 4": cases.make_context(pair_plan_cap=4)}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    return cases.inputs()


@pytest.fixture(scope="module")
def launched(ctxs, inputs):
    """{case: (virtual heights, counters)} of every case, made once."""
    return {name: cases.launch(ctxs[nodes], *args, **kwargs) for name, (nodes, args, kwargs) in inputs.items()}


@pytest.fixture(scope="module")
def same_compiler(recorded):
    then, now = str(recorded["hipcc"]), cases.hipcc_version_line()
    if then != now:
        print(f"the fixture was written under another compiler: comparing at 1e-13, not bits\n  then: {then}\n  now:  {now}")
    return then == now


CASES = [f"b{n}_p{nodes}" for n in SIZES for nodes in (4, 8)] + ["long65535", "plateau8192", "plateau20000"]


@pytest.mark.parametrize("name", CASES + list(cases.UNTOUCHED))
def test_bits_and_counters_of_before(launched, recorded, same_compiler, name):
    got, counted = launched[name]
    want, counted_then = recorded[f"{name}_vh"], recorded[f"{name}_counters"]
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err, ok = rel_err(got, want)
    differ = int((got[ok] != want[ok]).sum())
    print(f"{name}: {int(ok.sum())} finite pairs, {differ} differ, worst {float(err.max(initial=0.0)):.2e}; counters "
          f"{counted.tolist()} (recorded {counted_then.tolist()})")
    if same_compiler:
        assert same_bits(got, want)
    else:
        assert float(err.max(initial=0.0)) <= 1e-13
    assert np.array_equal(counted, counted_then)
    if name in cases.UNTOUCHED:
        assert not counted.any()
    else:
        assert counted[0] > 0


def test_cases_take_the_paths_they_are_there_for(launched):
    """Some pair falls back and some keeps the lower region on the plateau rows; the long grid keeps it too."""
    for name in ("plateau8192", "plateau20000"):
        took, fell, reached, kept = launched[name][1]
        assert took > 0 and fell > 0 and reached > 0 and kept > 0, name
    assert launched["long65535"][1][3] > 0


@pytest.mark.parametrize("name", [f"b{n}_p4" for n in SIZES] + ["long65535", "plateau20000"])
def test_same_bits_with_and_without_plans_and_twice(ctxs, inputs, launched, name):
    got, counted = launched[name]
    _, args, kwargs = inputs[name]
    for label in ("pair_plan = 0", "pair_plan_cap = 4", 4):
        again, counted2 = cases.launch(ctxs[label], *args, **kwargs)
        assert same_bits(got, again), label
        assert np.array_equal(counted, counted2), label


def test_mixed_work_list_equals_separate_launches(ctxs, inputs, launched):
    from pyrayhf_amd import _native
    _, (freq, den, bmag, bpsi, alt, _), _ = inputs["b20000_p4"]
    on = ctxs[4]
    mult = np.ascontiguousarray(np.concatenate([grid(200), grid(20000)]))       # the long grid at an offset
    S = _native.Segment
    segs = [S(0, 10, _native.MODE_O, 200, 0, 0), S(10, 24, _native.MODE_X, 20000, 200, 10 * FREQ.size)]
    out = np.full((24, FREQ.size), -7.0)
    before = on.panel_counters()
    rc = on.vfo_worklist(FREQ.ctypes.data, FREQ.size, den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, alt.ctypes.data,
                         24, den.shape[1], den.shape[1], 0, mult.ctypes.data, mult.size, segs, out.ctypes.data, 0)
    _native.raise_for(rc)
    assert on.panel_counters()[0] > before[0]              # the X/20000 slice took the rule
    assert same_bits(out[:10], cases.launch(on, freq, den[:10], bmag[:10], bpsi[:10], alt, 200, mode="O")[0])
    assert same_bits(out[10:], launched["b20000_p4"][0][10:])
