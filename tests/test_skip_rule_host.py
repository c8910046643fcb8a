"""Host-side checks of the skip distance and the MUF search: the rule as restated in
tests/skip_rule.py on synthetic ground-range functions and on the CPU oracle's rays, the exports, and the argument
checks that run before any native call."""

import math

import numpy as np
import pytest

import skip_rule
from conftest import load_golden

SCAN = np.linspace(2.0, 88.0, 345)
# (column, MHz): (flat i*, flat D_i* [km], spherical i*, spherical D_i* [km]) of the CPU oracle's scan, O mode
NODES = {("gauss", 9): (327, 92.51, 326, 95.97), ("gauss", 10): (218, 438.38, 213, 452.32),
         ("gauss", 12): (161, 671.90, 152, 704.04), ("gauss", 15): (116, 942.82, 105, 1013.85),
         ("day", 10): (329, 59.65, 329, 58.52), ("day", 9): (344, None, 344, None), ("day", 12): (344, None, 344, None),
         ("gauss", 4): (317, 52.33, 316, 54.36)}


def _search(fn, scan, **kw):
    scan = np.asarray(scan, dtype=np.float64)
    calls = []

    def ray(e):
        calls.append(e)
        return fn(e)
    res = skip_rule.skip_search(scan, np.array([fn(e) for e in scan]), ray, **kw)
    assert res["n_evals"] == len(calls)
    return res, calls


def test_a_kink_and_a_parabola_converge_onto_the_minimum():
    scan = np.linspace(0.0, 10.0, 11)
    for fn, e0 in ((lambda e: abs(e - 4.3) + 7.0, 4.3), (lambda e: (e - 6.6) ** 2 + 1.0, 6.6),
                   (lambda e: abs(e - 5.0) + 2.0, 5.0)):
        res, calls = _search(fn, scan)
        assert res["status"] == 0 and res["scan_index"] == int(round(e0))
        assert res["bracket_deg"] <= 1e-6 and abs(res["elevation_deg"] - e0) <= 1e-6
        a, b, c = res["triple"]
        assert a < b < c and a <= e0 <= c and res["bracket_deg"] == c - a
        assert res["skip_km"] == fn(res["elevation_deg"]) <= fn(scan[res["scan_index"]])
        assert 0 < res["n_evals"] <= 64 and all(scan[res["scan_index"] - 1] < x < scan[res["scan_index"] + 1] for x in calls)


def test_first_index_wins_and_a_tie_keeps_b():
    scan = np.arange(5.0)
    d = np.array([3.0, 1.0, 1.0, 1.0, 3.0])
    assert skip_rule.scan_node(d) == (1, False)
    res = skip_rule.skip_search(scan, d, lambda e: 1.0)               # a plateau: every ray ties with D_b
    assert res["status"] == 0 and res["scan_index"] == 1 and res["elevation_deg"] == 1.0 and res["skip_km"] == 1.0
    assert res["n_evals"] > 0 and res["bracket_deg"] <= 1e-6
    # the first step goes right when the two halves are equally wide: x = b + g (c - b)
    seen = []
    skip_rule.skip_search(scan, d, lambda e: seen.append(e) or 1.0, max_iter=1)
    assert seen == [1.0 + skip_rule.GOLD * (2.0 - 1.0)]


def test_rays_that_do_not_turn():
    scan = np.arange(5.0)
    nan = float("nan")
    res = skip_rule.skip_search(scan, np.array([5.0, 4.0, 1.0, 2.0, 3.0]), lambda e: nan)
    assert res["status"] == 2 and res["n_evals"] == 1 and res["elevation_deg"] == 2.0 and res["skip_km"] == 1.0
    assert res["bracket_deg"] == 2.0 and res["scan_index"] == 2
    for d in ([5.0, nan, 1.0, 2.0, 3.0], [5.0, 4.0, 1.0, nan, 3.0], [5.0, 4.0, 1.0, float("inf"), 3.0]):
        res = skip_rule.skip_search(scan, np.array(d), lambda e: pytest.fail("an edge node is not refined"))
        assert res["status"] == 1 and res["scan_index"] == 2 and res["elevation_deg"] == 2.0 and res["n_evals"] == 0
        assert math.isnan(res["bracket_deg"])
    res = skip_rule.skip_search(scan, np.full(5, nan), lambda e: 0.0)
    assert res["status"] == -1 and res["scan_index"] == -1 and res["n_evals"] == 0 and math.isnan(res["skip_km"])
    # infinity is not a ground range
    assert skip_rule.scan_node(np.array([float("inf"), 3.0, float("-inf")])) == (1, True)


def test_scans_of_one_two_and_three_nodes():
    never = lambda e: pytest.fail("no ray is traced")                 # noqa: E731
    assert skip_rule.skip_search([10.0], [7.0], never)["status"] == 1
    for d in ([7.0, 8.0], [8.0, 7.0]):
        res = skip_rule.skip_search([10.0, 20.0], d, never)
        assert res["status"] == 1 and res["scan_index"] == int(np.argmin(d)) and res["skip_km"] == 7.0
    assert skip_rule.skip_search([10.0, 20.0, 30.0], [7.0, 8.0, 9.0], never)["status"] == 1
    res, _ = _search(lambda e: abs(e - 18.0), [10.0, 20.0, 30.0])
    assert res["status"] == 0 and res["scan_index"] == 1 and abs(res["elevation_deg"] - 18.0) <= 1e-6


def test_no_tolerance_ends_when_the_doubles_are_exhausted():
    res, _ = _search(lambda e: abs(e - 4.3), np.linspace(0.0, 10.0, 11), elev_tol_deg=0.0, max_iter=128)
    assert res["status"] == 0 and res["n_evals"] < 128
    a, b, c = res["triple"]
    assert a < b < c and c - a <= 4 * np.spacing(b) and res["bracket_deg"] == c - a


def test_max_iter_bounds_the_rays():
    for max_iter in (1, 5):
        res, calls = _search(lambda e: abs(e - 4.3), np.linspace(0.0, 10.0, 11), max_iter=max_iter)
        assert res["status"] == 3 and res["n_evals"] == max_iter == len(calls)


@pytest.mark.parametrize("case", sorted(NODES))
@pytest.mark.parametrize("spherical", [False, True])
def test_scan_nodes_of_the_cpu_oracle(spherical, case):
    """i* (and D_i* to the table's two decimals) of the oracle's scan, pinned to the reference: the interior minima,
    the E-layer skip of the day column, the last scan node where no skip zone lies inside the scan, the node beside
    the first penetrating ray."""
    from oracle import snell_numpy
    g = load_golden("g8_snell.npz")
    name, mhz = case
    cols = [g[f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]
    fn = snell_numpy.trace_spherical if spherical else snell_numpy.trace_cartesian
    d = np.array([float(fn(mhz * 1e6, e, *cols, "O")["ground_range_km"]) for e in SCAN])
    i, edge = skip_rule.scan_node(d)
    want_i, want_d = NODES[case][2 * spherical:2 * spherical + 2]
    assert i == want_i
    if want_d is not None:
        assert abs(d[i] - want_d) <= 0.0051
    assert edge == (case in (("day", 9), ("day", 12), ("gauss", 4)))
    if case == ("gauss", 4):
        assert not np.isfinite(d[i + 1]) and np.isfinite(d[i - 1])


def test_muf_bisection_on_a_function_that_is_not_monotone():
    s = lambda f: 300.0 + 60.0 * (f / 1e6 - 9.0) + 80.0 * math.sin(2.5 * f / 1e6)      # noqa: E731
    t = 480.0
    assert s(9e6) <= t < s(15e6)
    grid = np.linspace(9e6, 15e6, 601)
    up = np.array([s(f) for f in grid]) > t
    assert np.count_nonzero(up[1:] != up[:-1]) >= 3                   # several crossings: S is not monotone
    for n in (1, 24, 40, 64):
        r = skip_rule.muf_search(s, t, 9e6, 15e6, n)
        assert r["status"] == 0 and s(r["muf_hz"]) <= t < s(r["f_above_hz"])
        lo, hi = 9e6, 15e6
        for m, sm, l0, h0 in r["trips"]:
            assert (l0, h0) == (lo, hi) and m == lo + 0.5 * (hi - lo)
            lo, hi = (m, hi) if sm <= t else (lo, m)
        assert (lo, hi) == (r["muf_hz"], r["f_above_hz"])
    assert len(skip_rule.muf_search(s, t, 9e6, 15e6, 24)["trips"]) == 24
    # a bracket of neighbouring doubles cannot be split: the trips change nothing
    lo = 9e6
    hi = np.nextafter(lo, np.inf)
    r = skip_rule.muf_search(lambda f: 0.0 if f <= lo else 1e3, t, lo, hi, 5)
    assert r["status"] == 0 and (r["muf_hz"], r["f_above_hz"]) == (lo, hi) and r["trips"] == []


def test_muf_statuses_from_the_end_points():
    s = lambda f: f / 1e4                                             # noqa: E731  900 km at 9 MHz, 1500 km at 15 MHz
    assert skip_rule.muf_search(s, float("nan"), 9e6, 15e6)["status"] == -1
    r = skip_rule.muf_search(s, 10.0, 9e6, 15e6)
    assert r["status"] == 2 and math.isnan(r["muf_hz"])
    r = skip_rule.muf_search(s, 2000.0, 9e6, 15e6)
    assert r["status"] == 1 and r["muf_hz"] == 15e6 and math.isnan(r["f_above_hz"])
    r = skip_rule.muf_search(lambda f: float("inf"), 500.0, 9e6, 15e6)    # no ray lands even at f_lo
    assert r["status"] == 2
    r = skip_rule.muf_search(s, 1200.0, 9e6, 15e6, 40)
    assert r["status"] == 0 and r["muf_hz"] <= 12e6 < r["f_above_hz"] and r["f_above_hz"] - r["muf_hz"] < 1e-5


def test_functions_are_exported():
    import pyrayhf_amd
    from pyrayhf_amd import _native, tracers
    for name in ("skip_distance_cartesian_snells", "skip_distance_spherical_snells", "muf_cartesian_snells",
                 "muf_spherical_snells"):
        assert name in pyrayhf_amd.__all__ and name in tracers.__all__
        assert getattr(pyrayhf_amd, name) is getattr(tracers, name)
    for name in ("prhf_snell_skip_f64", "prhf_snell_muf_f64"):
        assert name in _native.exported_symbols() and hasattr(_native.load(), name)
    assert set(tracers.SKIP_STATUS_NAMES) == {-1, 0, 1, 2, 3} and set(tracers.MUF_STATUS_NAMES) == {-1, 0, 1, 2}


@pytest.mark.parametrize("spherical", [False, True])
def test_arguments_are_validated_before_any_native_call(monkeypatch, spherical):
    from pyrayhf_amd import _native, tracers

    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    g = load_golden("g8_snell.npz")
    cols = [g[f"gauss_{k}"] for k in ("alt", "den", "bmag", "bpsi")]
    skip = tracers.skip_distance_spherical_snells if spherical else tracers.skip_distance_cartesian_snells
    muf = tracers.muf_spherical_snells if spherical else tracers.muf_cartesian_snells
    f, t = np.array([9e6, 10e6]), np.array([500.0, 800.0])
    calls = (lambda *c, **kw: skip(f, *c, **kw), lambda *c, **kw: muf(t, 9e6, 15e6, *c, **kw))
    bad = (dict(scan_elevation_deg=[]), dict(scan_elevation_deg=[10.0, 10.0]), dict(scan_elevation_deg=[20.0, 10.0, 30.0]),
           dict(scan_elevation_deg=[10.0, np.nan, 30.0]), dict(scan_elevation_deg=[np.nan]), dict(scan_elevation_deg=np.ones((2, 3))),
           dict(max_iter=0), dict(max_iter=129), dict(elev_tol_deg=-1e-9), dict(elev_tol_deg=np.nan), dict(elev_tol_deg=np.inf))
    for call in calls:
        with pytest.raises(ValueError, match="Mode must be O or X"):
            call(*cols, "Z")
        for kw in bad:
            with pytest.raises(ValueError):
                call(*cols, "O", **kw)
        with pytest.raises(ValueError):
            call(cols[0], cols[1][:-1], cols[2], cols[3], "O")            # columns of different lengths
        with pytest.raises(ValueError):
            call(cols[0][:-1], cols[1], cols[2], cols[3], "O")            # one altitude per level
        with pytest.raises(ValueError):
            call(np.tile(cols[0], (3, 1)), *(np.tile(c, (2, 1)) for c in cols[1:]), "O")
    with pytest.raises(ValueError):
        skip(f.reshape(1, 2), *cols, "O")                                 # frequencies are 1-D
    with pytest.raises(ValueError):
        skip(np.array([]), *cols, "O")
    with pytest.raises(ValueError):
        muf(t.reshape(2, 1), 9e6, 15e6, *cols, "O")                       # targets are 1-D
    for lo, hi in ((0.0, 15e6), (-1.0, 15e6), (15e6, 15e6), (15e6, 9e6), (np.nan, 15e6), (9e6, np.inf)):
        with pytest.raises(ValueError, match="f_lo_Hz"):
            muf(t, lo, hi, *cols, "O")
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_bisect"):
            muf(t, 9e6, 15e6, *cols, "O", n_bisect=n)


def test_native_calls_validate_without_a_gpu():
    """Both entry points reject a null context before anything else: PRHF_EINVAL with a message, no device touched."""
    from pyrayhf_amd import _native
    lib = _native.load()
    rc = lib.prhf_snell_skip_f64(None, 0, None, None, 0, None, 0, None, None, None, None, 0, 0, 0, 0, 6371.0, 1.0, 200.0,
                                 400, 1e-6, 64, None, 0)
    assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()
    rc = lib.prhf_snell_muf_f64(None, 0, None, None, 0, 9e6, 15e6, 24, None, 0, None, None, None, None, 0, 0, 0, 0, 6371.0,
                                1.0, 200.0, 400, 1e-6, 64, None, 0)
    assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()


def test_fixture_satisfies_the_generators_invariants():
    """G22 (tools/gen_golden_skip.py, reference-run): the stored nodes and statuses are the rule applied to the stored
    scans, the refined rows improve on their nodes, the unimodal set is unimodal, and the MUF cases clear their
    margins."""
    g = load_golden("g22_skip.npz")
    assert np.array_equal(g["scan_elevation_deg"], SCAN)
    d, idx, st = g["scan_ground_range_km"], g["scan_index"], g["status"]
    for geo in range(2):
        for c in range(idx.shape[1]):
            i, edge = skip_rule.scan_node(d[geo, c])
            assert i == idx[geo, c]
            assert st[geo, c] == (-1 if i < 0 else 1 if edge else st[geo, c]) and st[geo, c] in (-1, 0, 1, 2, 3)
            if st[geo, c] in (0, 2, 3):
                assert g["skip_km"][geo, c] <= d[geo, c, i]
                e = g["dense_elevation_deg"][geo, c]
                assert e[0] == SCAN[i - 1] and e[-1] == SCAN[i + 1] and np.isfinite(g["dense_ground_range_km"][geo, c]).all()
                assert g["dense_sign_changes"][geo, c] == skip_rule.slope_sign_changes(g["dense_ground_range_km"][geo, c])
                assert e[0] <= g["elevation_deg"][geo, c] <= e[-1]
            elif st[geo, c] == 1:
                assert g["skip_km"][geo, c] == d[geo, c, i] and g["elevation_deg"][geo, c] == SCAN[i]
    assert g["unimodal_set"].sum() == 7 and np.all(g["dense_sign_changes"][g["unimodal_set"]] == 1)
    assert np.all(st[g["unimodal_set"]] == 0)
    assert np.all(g["muf_min_gap_km"] >= 10.0 * g["muf_margin_km"]) and np.all(np.isin(g["muf_window_hz"], (1e2, 1e3, 1e4, 1e5)))
    assert np.all((g["muf_ref"] > g["muf_f_lo_hz"]) & (g["f_above_ref"] < g["muf_f_hi_hz"]) & (g["muf_ref"] < g["f_above_ref"]))
