"""Skip distance and MUF on the GPU (prhf_snell_skip_f64, prhf_snell_muf_f64) against the
rule restated in NumPy (tests/skip_rule.py) driven by the existing fan kernel, against the reference-run fixture G22
(tools/gen_golden_skip.py) and on the shapes where the kernels take another path."""

import numpy as np
import pytest

import skip_rule
from conftest import load_golden, same_bits

pytestmark = pytest.mark.gpu

KEYS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_turn_km", "z_turn_km",
        "n_path")
ROW = ("skip_km", "elevation_deg", "status", "scan_index", "bracket_deg", "n_evals") + KEYS
SCAN = np.linspace(2.0, 88.0, 345)
# those of G22, in its order (column, Hz); all O mode
CASES = (("gauss", 9e6), ("gauss", 10e6), ("gauss", 12e6), ("gauss", 15e6), ("day", 10e6), ("day", 9e6), ("day", 12e6),
         ("gauss", 4e6), ("gauss", 40e6), ("day", 15e6), ("gauss", 400e6))
_cache = {}


def _column(name):
    g = _cache.setdefault("g8", load_golden("g8_snell.npz"))
    return [g[f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]


def _skip(spherical, *args, **kw):
    from pyrayhf_amd import tracers
    return (tracers.skip_distance_spherical_snells if spherical else tracers.skip_distance_cartesian_snells)(*args, **kw)


def _muf(spherical, *args, **kw):
    from pyrayhf_amd import tracers
    return (tracers.muf_spherical_snells if spherical else tracers.muf_cartesian_snells)(*args, **kw)


def _fan(spherical, *args, **kw):
    from pyrayhf_amd import tracers
    return (tracers.trace_fan_spherical_snells if spherical else tracers.trace_fan_cartesian_snells)(*args, **kw)


def _case_freqs(name):
    return np.array([f for n, f in CASES if n == name])


def _g22_calls(geometry):
    """Per column the skip call on the frequencies of G22's cases with the defaults, and the fan call over the same
    scan: made once per geometry, shared, not modified.  -> {case index: (row dict of scalars, scan D (345,))}"""
    key = ("g22", geometry)
    if key not in _cache:
        out = {}
        for name in ("gauss", "day"):
            f = _case_freqs(name)
            res = _skip(bool(geometry), f, *_column(name), "O")
            fan = _fan(bool(geometry), f, SCAN, *_column(name), "O")["ground_range_km"]
            assert res["skip_km"].shape == (f.size,) and fan.shape == (f.size, SCAN.size)
            for k, fk in enumerate(f):
                out[CASES.index((name, fk))] = ({key_: res[key_][k] for key_ in ROW}, fan[k])
        _cache[key] = out
    return _cache[key]


def _ray_of(spherical, f, prof, mode):
    """D(e) of one group through the existing fan kernel, one elevation a call"""
    return lambda e: float(_fan(spherical, np.array([f]), np.array([e]), *prof, mode)["ground_range_km"][0, 0])


def _dense(geometry, case):
    """An 801-node fan call (the existing kernel) across the scan bracket of a case: (elevations, D)"""
    key = ("dense", geometry, case)
    if key not in _cache:
        row, _ = _g22_calls(geometry)[case]
        i = int(row["scan_index"])
        e = np.linspace(SCAN[i - 1], SCAN[i + 1], 801)
        name, f = CASES[case]
        _cache[key] = (e, _fan(bool(geometry), np.array([f]), e, *_column(name), "O")["ground_range_km"][0])
    return _cache[key]


def check_node(row, d):
    """scan_index and the edge class of a result row against the NumPy rule on the scan's ground ranges d"""
    i, edge = skip_rule.scan_node(d)
    assert row["scan_index"] == i, (row["scan_index"], i)
    if i < 0:
        assert row["status"] == -1 and row["n_path"] == 0 and row["n_evals"] == 0
        assert all(np.isnan(row[k]) for k in ("skip_km", "elevation_deg", "bracket_deg") + KEYS[:-1])
    elif edge:
        assert row["status"] == 1 and row["n_evals"] == 0 and np.isnan(row["bracket_deg"])
        assert same_bits(row["skip_km"], d[i])
    else:
        assert row["status"] in (0, 2, 3) and row["skip_km"] <= d[i] and np.isfinite(row["bracket_deg"])
    return i, edge


@pytest.mark.parametrize("geometry", [0, 1])
def test_scan_node_and_edge_class(geometry):
    """i* and the edge class equal the NumPy rule on a fan call over the same scan, exactly, and equal G22's i* and status
    for every case: interior minima, gauss 4 MHz beside penetration (1), day 9 and 12 MHz at the last node (1), no turning
    ray at all (-1: 400 MHz, and 40 MHz over the spherical Earth).  Every interior case: skip_km <= D_i* exactly."""
    g = load_golden("g22_skip.npz")
    assert np.array_equal(g["freq_hz"], [f for _, f in CASES])
    calls = _g22_calls(geometry)
    seen = set()
    for case in range(len(CASES)):
        row, d = calls[case]
        i, edge = check_node(row, d)
        assert i == g["scan_index"][geometry, case], (case, i)
        assert row["status"] == g["status"][geometry, case], (case, row["status"])
        assert same_bits(row["skip_km"], row["ground_range_km"])
        if i >= 0:
            assert same_bits(row["elevation_deg"] if edge else SCAN[i], SCAN[i])
            assert SCAN[max(i - 1, 0)] <= row["elevation_deg"] <= SCAN[min(i + 1, SCAN.size - 1)]
        seen.add(int(row["status"]))
    assert {-1, 0, 1} <= seen
    assert calls[7][0]["status"] == 1 and calls[5][0]["scan_index"] == 344 and calls[10][0]["status"] == -1


@pytest.mark.parametrize("case", [1, 4])
@pytest.mark.parametrize("geometry", [0, 1])
def test_the_numpy_restatement_gives_the_same_bits(geometry, case):
    """tests/skip_rule.py driven by one-elevation fan calls gives the kernel's elevation_deg, status, n_evals and
    bracket_deg bit for bit (gauss 10 MHz and day 10 MHz, both geometries)."""
    name, f = CASES[case]
    row, d = _g22_calls(geometry)[case]
    want = skip_rule.skip_search(SCAN, d, _ray_of(bool(geometry), f, _column(name), "O"))
    assert want["status"] == row["status"] == 0 and want["n_evals"] == row["n_evals"] > 0
    assert want["scan_index"] == row["scan_index"]
    for k in ("elevation_deg", "bracket_deg", "skip_km"):
        assert same_bits(want[k], row[k]), (k, want[k], row[k])


@pytest.mark.parametrize("spherical", [False, True])
def test_the_row_is_the_tracers_row(spherical):
    """A fan call at the returned elevation gives the eight outputs bit for bit; the per-ray call in the reference's
    operation order gives them to 1e-12 relative."""
    from pyrayhf_amd import _native, tracers
    ray_fn = tracers.trace_rays_spherical_snells if spherical else tracers.trace_rays_cartesian_snells
    calls = _g22_calls(int(spherical))
    n = 0
    for case, (name, f) in enumerate(CASES):
        row, _ = calls[case]
        if row["status"] < 0:
            continue
        fan = _fan(spherical, np.array([f]), np.array([row["elevation_deg"]]), *_column(name), "O")
        ray = ray_fn(np.array([f]), np.array([row["elevation_deg"]]), *_column(name), "O", math=_native.MATH_FAITHFUL)
        for k in KEYS:
            assert same_bits(fan[k][0, 0], row[k]), (case, k)
            if k == "n_path":
                assert ray[k][0] == row[k]
            else:
                assert abs(ray[k][0] - row[k]) <= 1e-12 * abs(row[k]), (case, k, ray[k][0], row[k])
        n += 1
    assert n >= 9


@pytest.mark.parametrize("geometry", [0, 1])
def test_minimality_on_the_unimodal_set(geometry):
    """A status-0 row of the unimodal set against an 801-node dense fan call (the existing kernel) over the scan bracket:
    with h its spacing, L its largest |dD/de| and w the returned bracket_deg, the fan is unimodal (asserted first, so
    that the test cannot pass vacuously) and min(dense) - 2 L h <= skip_km <= min(dense) + 2 L w; the factor 2 because L
    is sampled, not a bound."""
    g = load_golden("g22_skip.npz")
    cases = np.nonzero(g["unimodal_set"][geometry])[0]
    assert cases.size >= 3
    for case in cases:
        row, _ = _g22_calls(geometry)[case]
        assert row["status"] == 0
        e, d = _dense(geometry, case)
        assert np.isfinite(d).all() and skip_rule.slope_sign_changes(d) == 1, (case, skip_rule.slope_sign_changes(d))
        h, big_l, w = e[1] - e[0], skip_rule.largest_slope(e, d), row["bracket_deg"]
        lo, hi = d.min() - 2.0 * big_l * h, d.min() + 2.0 * big_l * w
        print(f"skip vs dense fan, geometry {geometry} case {case}: skip {row['skip_km']:.9f} km, dense min {d.min():.9f} km, "
              f"L {big_l:.1f} km/deg, w {w:.3e} deg, allowed [{lo:.9f}, {hi:.9f}]")
        assert lo <= row["skip_km"] <= hi, (case, lo, row["skip_km"], hi)


@pytest.mark.parametrize("geometry", [0, 1])
def test_against_the_reference_on_the_unimodal_set(geometry):
    """|skip_km - G22's| <= 2 L_ref (w + w_ref) + 1e-9 skip_km: L_ref from G22's dense fan (the reference's rays), w and
    w_ref the two final brackets, the last term the tracers' stated default-tier parity with room.  The worst ratio of
    error to bound is printed (profiles/skip_accuracy.md keeps it)."""
    g = load_golden("g22_skip.npz")
    worst = 0.0
    for case in np.nonzero(g["unimodal_set"][geometry])[0]:
        row, _ = _g22_calls(geometry)[case]
        l_ref = skip_rule.largest_slope(g["dense_elevation_deg"][geometry, case], g["dense_ground_range_km"][geometry, case])
        bound = 2.0 * l_ref * (row["bracket_deg"] + g["bracket_deg"][geometry, case]) + 1e-9 * row["skip_km"]
        err = abs(row["skip_km"] - g["skip_km"][geometry, case])
        worst = max(worst, err / bound)
        print(f"skip vs G22, geometry {geometry} case {case}: error {err:.3e} km, bound {bound:.3e} km, "
              f"elevation {row['elevation_deg']:.9f} vs {g['elevation_deg'][geometry, case]:.9f}")
        assert err <= bound, (case, err, bound)
    print(f"skip vs G22, geometry {geometry}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n_scan", [1, 2, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("spherical", [False, True])
def test_scan_grids_around_the_wavefront_size(spherical, n_scan):
    """The refine kernel reduces 64 nodes a trip: grids of 1, 2, 3, 63, 64, 65 and 129 nodes against the fan call and
    the NumPy rule, the row against the fan call at its elevation."""
    scan = np.linspace(2.0, 88.0, n_scan) if n_scan > 1 else np.array([45.0])
    f = np.array([4e6, 10e6, 12e6, 400e6])
    prof = _column("gauss")
    res = _skip(spherical, f, *prof, "O", scan_elevation_deg=scan)
    fan = _fan(spherical, f, scan, *prof, "O")["ground_range_km"]
    for k in range(f.size):
        row = {key: res[key][k] for key in ROW}
        i, edge = check_node(row, fan[k])
        if i >= 0:
            again = _fan(spherical, f[k:k + 1], np.array([row["elevation_deg"]]), *prof, "O")
            for key in KEYS:
                assert same_bits(again[key][0, 0], row[key]), key
            if not edge:
                assert scan[i - 1] < row["elevation_deg"] < scan[i + 1]
    if n_scan <= 2:
        assert np.isin(res["status"], (1, -1)).all() and np.all(res["n_evals"] == 0)     # no node has two neighbours
    assert res["status"][3] == -1


@pytest.mark.parametrize("spherical", [False, True])
def test_one_group_and_130_groups(spherical):
    """1 group; 130 groups (more than two trips of anything sized 64), each checked against the fan call's scan, and one
    of them equal to the same group searched alone - bit for bit."""
    prof = _column("gauss")
    f = np.linspace(9e6, 15e6, 130)
    res = _skip(spherical, f, *prof, "O")
    fan = _fan(spherical, f, SCAN, *prof, "O")["ground_range_km"]
    assert res["skip_km"].shape == (130,)
    for k in range(f.size):
        check_node({key: res[key][k] for key in ROW}, fan[k])
    assert (res["status"] == 0).sum() > 64
    one = _skip(spherical, f[77:78], *prof, "O")
    for key in ROW:
        assert one[key].shape == (1,) and same_bits(one[key][0], res[key][77]), key


@pytest.mark.parametrize("spherical", [False, True])
def test_a_column_of_three_levels(spherical):
    alt = np.array([60.0, 100.0, 250.0])
    den = np.array([0.0, 2e11, 1.2e12])
    bmag, bpsi = np.full(3, 4.5e-5), np.full(3, 60.0)
    f = np.array([5e6, 12e6, 20e6])
    res = _skip(spherical, f, alt, den, bmag, bpsi, "O")
    fan = _fan(spherical, f, SCAN, alt, den, bmag, bpsi, "O")["ground_range_km"]
    for k in range(f.size):
        check_node({key: res[key][k] for key in ROW}, fan[k])
    assert (res["status"] >= 0).any()


@pytest.mark.parametrize("spherical", [False, True])
def test_the_controls_bound_the_search(spherical):
    """max_iter = 1: status 3 after one ray; elev_tol_deg = 0: the doubles are exhausted (status 0) before 128 rays, and
    both equal the NumPy restatement bit for bit."""
    name, f = CASES[1]
    prof = _column(name)
    row, d = _g22_calls(int(spherical))[1]
    ray = _ray_of(spherical, f, prof, "O")
    for kw in (dict(max_iter=1), dict(elev_tol_deg=0.0, max_iter=128)):
        res = _skip(spherical, np.array([f]), *prof, "O", **kw)
        want = skip_rule.skip_search(SCAN, d, ray, kw.get("elev_tol_deg", 1e-6), kw["max_iter"])
        assert res["status"][0] == want["status"] == (3 if kw["max_iter"] == 1 else 0)
        assert res["n_evals"][0] == want["n_evals"] and res["scan_index"][0] == row["scan_index"]
        for k in ("elevation_deg", "bracket_deg", "skip_km"):
            assert same_bits(res[k][0], want[k]), k
        assert res["skip_km"][0] <= d[int(row["scan_index"])]
    assert res["n_evals"][0] < 128 and res["bracket_deg"][0] <= 4 * np.spacing(res["elevation_deg"][0])


@pytest.mark.parametrize("spherical", [False, True])
def test_x_mode_and_per_profile_altitudes(spherical):
    """X mode on three Chapman profiles, (P, N_alt) columns with an altitude grid per profile: shapes (P, F), every
    group against the fan call's scan, every profile equal to the same profile searched alone, and a second call
    identical to the first - bit for bit."""
    from pyrayhf_amd import synth
    alt, den, bmag, bpsi = synth.chapman_profiles(3, 11)
    alt2 = np.ascontiguousarray(alt[None, :] + np.array([0.0, 1.5, 3.25])[:, None])
    f = np.array([4e6, 7e6, 10e6, 14e6])
    res = _skip(spherical, f, alt2, den, bmag, bpsi, "X")
    fan = _fan(spherical, f, SCAN, alt2, den, bmag, bpsi, "X")["ground_range_km"]
    assert res["skip_km"].shape == (3, 4) and fan.shape == (3, 4, 345)
    for p in range(3):
        for k in range(f.size):
            check_node({key: res[key][p, k] for key in ROW}, fan[p, k])
        alone = _skip(spherical, f, alt2[p], den[p], bmag[p], bpsi[p], "X")
        for key in ROW:
            assert same_bits(alone[key], res[key][p]), (p, key)
    assert (res["status"] == 0).any()
    again = _skip(spherical, f, alt2, den, bmag, bpsi, "X")
    for key in ROW:
        assert same_bits(again[key], res[key]), key


# ---- MUF ----------------------------------------------------------------------------------------------------------
T_KM, F_LO, F_HI, N_BISECT = 500.0, 9e6, 15e6, 24


def _muf_call(spherical):
    key = ("muf", spherical)
    if key not in _cache:
        t = np.array([T_KM, 2000.0, 10.0, np.nan])
        _cache[key] = (t, _muf(spherical, t, F_LO, F_HI, *_column("gauss"), "O", n_bisect=N_BISECT))
    return _cache[key]


@pytest.mark.parametrize("spherical", [False, True])
def test_muf_invariant_through_the_skip_call(spherical):
    """skip_distance_* at muf_hz gives the returned row bit for bit with skip_km <= t; at f_above_hz it gives > t, or
    status -1."""
    t, res = _muf_call(spherical)
    assert res["muf_hz"].shape == (4,) and res["status"][0] == 0
    assert F_LO <= res["muf_hz"][0] < res["f_above_hz"][0] <= F_HI
    at = _skip(spherical, np.array([res["muf_hz"][0], res["f_above_hz"][0]]), *_column("gauss"), "O")
    for key in ROW:
        assert same_bits(at[key][0], res["skip_status" if key == "status" else key][0]), key
    assert at["skip_km"][0] <= T_KM
    assert at["skip_km"][1] > T_KM or at["status"][1] == -1


@pytest.mark.parametrize("spherical", [False, True])
def test_muf_is_the_bisection_of_the_skip_call(spherical):
    """muf_hz and f_above_hz are what tests/skip_rule.py's 24 halvings of (f_hi - f_lo) give when driven by the GPU skip
    call - bit for bit."""
    t, res = _muf_call(spherical)

    def s_of(f):
        r = _skip(spherical, np.array([f]), *_column("gauss"), "O")
        return np.inf if r["status"][0] == -1 else float(r["skip_km"][0])
    want = skip_rule.muf_search(s_of, T_KM, F_LO, F_HI, N_BISECT)
    assert want["status"] == 0 and len(want["trips"]) == N_BISECT
    assert same_bits(want["muf_hz"], res["muf_hz"][0]) and same_bits(want["f_above_hz"], res["f_above_hz"][0])


@pytest.mark.parametrize("spherical", [False, True])
def test_muf_statuses_from_the_end_points(spherical):
    """t = 2000 km: open at f_hi (1), the row is the skip row at f_hi; t = 10 km: unreachable at f_lo (2); t = NaN: -1."""
    t, res = _muf_call(spherical)
    assert np.array_equal(res["status"], [0, 1, 2, -1])
    assert res["muf_hz"][1] == F_HI and np.isnan(res["f_above_hz"][1])
    at = _skip(spherical, np.array([F_HI, F_LO]), *_column("gauss"), "O")
    for key in ROW:
        assert same_bits(at[key][0], res["skip_status" if key == "status" else key][1]), key
    assert at["skip_km"][0] <= 2000.0 and at["skip_km"][1] > 10.0
    for k in (2, 3):
        assert res["skip_status"][k] == -1 and res["scan_index"][k] == -1 and res["n_path"][k] == 0 and res["n_evals"][k] == 0
        for key in ("muf_hz", "f_above_hz", "skip_km", "elevation_deg", "bracket_deg") + KEYS[:-1]:
            assert np.isnan(res[key][k]), (k, key)


@pytest.mark.parametrize("geometry", [0, 1])
def test_muf_against_the_reference(geometry):
    """|muf_hz - G22's muf_ref| <= muf_window_hz: the window inside which the reference's own bisection path is decided
    by more than ten skip margins (tools/gen_golden_skip.py)."""
    g = load_golden("g22_skip.npz")
    assert (g["muf_target_km"], g["muf_f_lo_hz"], g["muf_f_hi_hz"], g["muf_n_bisect"]) == (T_KM, F_LO, F_HI, N_BISECT)
    t, res = _muf_call(bool(geometry))
    err = abs(res["muf_hz"][0] - g["muf_ref"][geometry])
    print(f"MUF vs G22, geometry {geometry}: {res['muf_hz'][0]:.3f} Hz vs {g['muf_ref'][geometry]:.3f} Hz, "
          f"error {err:.3f} Hz, window {g['muf_window_hz'][geometry]:g} Hz")
    assert err <= g["muf_window_hz"][geometry]


@pytest.mark.parametrize("spherical", [False, True])
def test_one_link_and_65_links(spherical):
    """65 links (two workgroups of the per-link kernels); one of them searched alone gives the same bits."""
    prof = _column("gauss")
    t = np.linspace(300.0, 1500.0, 65)
    res = _muf(spherical, t, F_LO, F_HI, *prof, "O", n_bisect=N_BISECT)
    assert res["muf_hz"].shape == (65,) and np.isin(res["status"], (0, 1, 2)).all() and (res["status"] == 0).sum() > 20
    ok = res["status"] == 0
    assert np.all(res["skip_km"][ok] <= t[ok]) and np.all(res["muf_hz"][ok] < res["f_above_hz"][ok])
    one = _muf(spherical, t[20:21], F_LO, F_HI, *prof, "O", n_bisect=N_BISECT)
    assert res["status"][20] == 0
    for key in ("muf_hz", "f_above_hz", "status", "skip_status") + ROW[:2] + ROW[3:]:
        assert one[key].shape == (1,) and same_bits(one[key][0], res[key][20]), key
