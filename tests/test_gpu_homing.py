"""Point-to-point homing on the GPU (prhf_snell_home_f64) against the reference-run fixture
G20, against the existing tracers (every returned ray re-traced; the brackets from a fan call and the bracket rule in
NumPy) and on the shapes where the kernels take another path."""

import numpy as np
import pytest

from conftest import load_golden, same_bits

pytestmark = pytest.mark.gpu

KEYS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_turn_km", "z_turn_km",
        "n_path")
TOL = 1e-6                                        # the default range_tol_km
CASES = (("day", 6.0e6, "O"), ("day", 12.0e6, "X"), ("gauss", 4.0e6, "O"), ("gauss", 5.0e6, "X"))   # those of G20
TARGETS = np.array([300.0, 800.0, 1500.0])
_cache = {}


def _column(name):
    g = _cache.setdefault("g8", load_golden("g8_snell.npz"))
    return [g[f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]


def _home(spherical, *args, **kw):
    from pyrayhf_amd import tracers
    return (tracers.home_rays_spherical_snells if spherical else tracers.home_rays_cartesian_snells)(*args, **kw)


def _fan(spherical, *args, **kw):
    from pyrayhf_amd import tracers
    return (tracers.trace_fan_spherical_snells if spherical else tracers.trace_fan_cartesian_snells)(*args, **kw)


def _g20_result(geometry, case):
    """The homing call of one (geometry, case) of G20 with the defaults: made once, shared, not modified"""
    key = ("g20", geometry, case)
    if key not in _cache:
        name, f, mode = CASES[case]
        _cache[key] = _home(bool(geometry), np.array([f]), TARGETS, *_column(name), mode)
    return _cache[key]


def host_brackets(d, t):
    """The bracket rule of DESIGN.md section 4.8 on the ground ranges d (E,) of a scan: interval indices, ascending"""
    f = d - t
    with np.errstate(invalid="ignore"):
        is_b = np.isfinite(d[:-1]) & np.isfinite(d[1:]) & (((f[:-1] < 0) & (f[1:] > 0)) | ((f[:-1] > 0) & (f[1:] < 0)) |
                                                           (d[:-1] == t))
    idx = list(np.nonzero(is_b)[0])
    if d[-1] == t:
        idx.append(d.size - 1)
    return np.array(idx, dtype=np.int64)


def check_against_host_route(spherical, res, f, t, prof, mode, scan, max_roots=4):
    """n_brackets and scan_index of `res` equal what a fan call on the same scan grid and the bracket rule give; first:
    no node within 1e-9 km of a target (an exact match is then owed)."""
    fan = _fan(spherical, f, scan, *prof, mode)["ground_range_km"]
    lead = fan.shape[:-1]
    fan = fan.reshape(-1, scan.size)
    nb = res["n_brackets"].reshape(fan.shape[0], t.size)
    si = res["scan_index"].reshape(fan.shape[0], t.size, max_roots)
    assert res["n_brackets"].shape == lead + (t.size,)
    for gi in range(fan.shape[0]):
        for ti in range(t.size):
            if np.isfinite(t[ti]):
                assert not (np.abs(fan[gi] - t[ti]) < 1e-9).any()
            want = host_brackets(fan[gi], t[ti])
            assert nb[gi, ti] == want.size, (gi, ti, nb[gi, ti], want)
            k = min(want.size, max_roots)
            assert np.array_equal(si[gi, ti, :k], want[:k]) and np.all(si[gi, ti, k:] == -1), (gi, ti, si[gi, ti], want)


def check_rows(res, t, scan, tol=TOL):
    """What every result owes: used slots first, in ascending elevation inside their brackets; unused slots NaN with
    status -1; status-0 rays within the tolerance."""
    nb, st, e, si = res["n_brackets"], res["status"], res["elevation_deg"], res["scan_index"]
    max_roots = st.shape[-1]
    used = np.arange(max_roots) < np.minimum(nb, max_roots)[..., None]
    assert np.all(st[~used] == -1) and np.all(si[~used] == -1) and np.all(res["n_path"][~used] == 0)
    for k in ("elevation_deg",) + KEYS[:-1]:
        assert np.isnan(res[k][~used]).all(), k
    assert np.isin(st[used], (0, 1, 2)).all()
    hi = np.minimum(si + 1, scan.size - 1)
    assert np.all((e[used] >= scan[si[used]]) & (e[used] <= scan[hi[used]]))
    target = np.broadcast_to(np.asarray(t)[:, None], st.shape)
    ok = used & (st == 0)
    assert np.all(np.abs(res["ground_range_km"][ok] - target[ok]) <= tol)
    assert np.isfinite(res["ground_range_km"][used]).all()          # (the nearest ray tried: one that lands)
    return used


@pytest.mark.parametrize("geometry", [0, 1])
def test_against_the_reference_run_fixture(geometry):
    """G20 (tools/gen_golden_homing.py): per link the number of brackets, their scan intervals and their class -
    crossing (status 0) or jump (status 1) - are the reference's; a converged root lands within range_tol_km, and its
    elevation, group path and group delay lie within what the reference's own local slopes allow for two rays that are
    tol = range_tol_km + miss_ref apart in ground range: |e - e_ref| <= 2 tol / |dD/de| + 1e-9,
    |P' - P'_ref| <= 2 |dP'/dD| tol + 1e-10 P' (the tracers' stated parity), the same with dtau/dD for the delay; the
    factor 2 allows for the slope changing across the tolerance interval.  The worst ratios of error to bound are
    printed (profiles/homing_accuracy.md keeps them)."""
    g = load_golden("g20_homing.npz")
    worst = {"elevation": 0.0, "path": 0.0, "delay": 0.0}
    for case in range(len(CASES)):
        res = _g20_result(geometry, case)
        check_rows(res, TARGETS, g["scan_elevation_deg"])
        for ti in range(TARGETS.size):
            rows = np.nonzero((g["geometry"] == geometry) & (g["case"] == case) & (g["target"] == ti))[0]
            assert res["n_brackets"][0, ti] == g["n_brackets"][geometry, case, ti] == rows.size
            assert rows.size <= 4
            assert np.array_equal(res["scan_index"][0, ti, :rows.size], g["scan_index"][rows])
            assert np.array_equal(res["status"][0, ti, :rows.size], np.where(g["converged"][rows], 0, 1)), (case, ti)
            for k, r in enumerate(rows):
                if not g["converged"][r]:
                    continue
                assert abs(res["ground_range_km"][0, ti, k] - TARGETS[ti]) <= TOL
                tol = TOL + g["miss_km"][r]
                checks = (("elevation", res["elevation_deg"][0, ti, k] - g["root_elevation_deg"][r],
                           2.0 * tol / abs(g["dD_de"][r]) + 1e-9),
                          ("path", res["group_path_km"][0, ti, k] - g["group_path_km"][r],
                           2.0 * abs(g["dP_dD"][r]) * tol + 1e-10 * g["group_path_km"][r]),
                          ("delay", res["group_delay_sec"][0, ti, k] - g["group_delay_sec"][r],
                           2.0 * abs(g["dtau_dD"][r]) * tol + 1e-10 * g["group_delay_sec"][r]))
                for name, err, bound in checks:
                    worst[name] = max(worst[name], abs(err) / bound)
                    assert abs(err) <= bound, (name, geometry, case, ti, k, err, bound)
    print(f"homing vs G20, geometry {geometry}: worst error / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("mode", ["O", "X"])
@pytest.mark.parametrize("spherical", [False, True])
def test_every_returned_ray_is_the_tracers_ray(spherical, mode):
    """Self-consistency: every returned elevation traced again by the per-ray call in the reference's operation order
    gives the eight outputs of the row to 1e-12 relative (the fan-versus-per-ray parity), and status-0 rays land within
    range_tol_km - on the G8 columns and three Chapman profiles."""
    from pyrayhf_amd import _native, synth, tracers
    ray_fn = tracers.trace_rays_spherical_snells if spherical else tracers.trace_rays_cartesian_snells
    alt, den, bmag, bpsi = synth.chapman_profiles(3, 11)
    sets = ((_column("day"), np.array([6e6, 12e6])), (_column("gauss"), np.array([4e6, 5e6])),
            ([alt, den, bmag, bpsi], np.array([4e6, 7e6, 10e6])))
    scan = np.linspace(2.0, 88.0, 345)
    n_status = np.zeros(3, dtype=np.int64)
    for prof, f in sets:
        res = _home(spherical, f, TARGETS, *prof, mode)
        used = check_rows(res, TARGETS, scan)
        st = res["status"]
        n_status += np.bincount(st[used], minlength=3)
        many = prof[1].ndim == 2                                     # (P, F, T, max_roots), else (F, T, max_roots)
        ff = np.broadcast_to(f[:, None, None], st.shape)
        kw = {}
        if many:
            kw["profile_index"] = np.broadcast_to(np.arange(st.shape[0])[:, None, None, None], st.shape)[used]
        rays = ray_fn(ff[used], res["elevation_deg"][used], *prof, mode, math=_native.MATH_FAITHFUL, **kw)
        for key in KEYS:
            got, want = res[key][used], rays[key]
            if key == "n_path":
                assert np.array_equal(got, want)
            else:
                err = np.abs(got - want) / np.abs(want)
                print(f"homing vs per-ray, spherical={spherical} {mode} {key}: max rel {err.max():.2e}")
                assert np.all(err <= 1e-12), (key, err.max())
    assert n_status[0] > 0


@pytest.mark.parametrize("spherical", [False, True])
def test_brackets_are_those_of_a_fan_call_and_the_bracket_rule(spherical):
    """Host route equivalence: trace_fan_*_snells on the same scan grid, the bracket rule in NumPy; n_brackets and
    scan_index are exactly the GPU's (no scan node lies within 1e-9 km of a target: asserted first)."""
    from pyrayhf_amd import synth
    scan = np.linspace(2.0, 88.0, 345)
    for case in range(len(CASES)):
        name, f, mode = CASES[case]
        check_against_host_route(spherical, _g20_result(int(spherical), case), np.array([f]), TARGETS, _column(name), mode, scan)
    alt, den, bmag, bpsi = synth.chapman_profiles(3, 11)
    f = np.array([4e6, 7e6, 10e6])
    for mode in "OX":
        res = _home(spherical, f, TARGETS, alt, den, bmag, bpsi, mode)
        assert res["n_brackets"].shape == (3, 3, 3) and res["status"].shape == (3, 3, 3, 4)
        check_against_host_route(spherical, res, f, TARGETS, [alt, den, bmag, bpsi], mode, scan)


@pytest.mark.parametrize("n_scan", [2, 63, 64, 65, 129])
@pytest.mark.parametrize("spherical", [False, True])
def test_scan_grids_around_the_wavefront_size(spherical, n_scan):
    """The bracket kernel takes 64 intervals a trip: grids of 2, 63, 64, 65 and 129 nodes against the host route, and
    the rows' own conditions."""
    scan = np.linspace(2.0, 88.0, n_scan)
    f = np.array([5e6, 6e6, 12e6])
    for mode in "OX":
        res = _home(spherical, f, TARGETS, *_column("day"), mode, scan_elevation_deg=scan)
        check_against_host_route(spherical, res, f, TARGETS, _column("day"), mode, scan)
        check_rows(res, TARGETS, scan)


@pytest.mark.parametrize("spherical", [False, True])
def test_one_link_and_130_links(spherical):
    """1 link; 130 links (10 frequencies x 13 targets: more than two trips of anything sized 64) against the host route,
    and each of the 130 equal to the same link homed alone or in another batch - bit for bit."""
    scan = np.linspace(2.0, 88.0, 345)
    prof = _column("gauss")
    one = _home(spherical, np.array([4e6]), np.array([800.0]), *prof, "O")
    assert one["n_brackets"].shape == (1, 1) and one["status"].shape == (1, 1, 4)
    f = np.linspace(3e6, 5.25e6, 10)
    t = np.linspace(200.0, 1400.0, 13)
    res = _home(spherical, f, t, *prof, "O")
    assert res["n_brackets"].size == 130
    check_against_host_route(spherical, res, f, t, prof, "O", scan)
    check_rows(res, t, scan)
    assert res["n_brackets"].sum() > 0
    part = _home(spherical, f[4:5], t[6:7], *prof, "O")
    for k in ("n_brackets", "status", "scan_index", "elevation_deg") + KEYS:
        assert same_bits(part[k][0, 0], res[k][4, 6]), k


@pytest.mark.parametrize("spherical", [False, True])
def test_max_roots_keeps_the_lowest_brackets(spherical):
    """max_roots = 1 on the four-crossing link (day, 6 MHz O, 300 km): n_brackets is still 4 and the row is the lowest
    root's, bit for bit the first row of the max_roots = 4 call; max_roots = 2 likewise."""
    name, f, mode = CASES[0]
    full = _g20_result(int(spherical), 0)
    assert full["n_brackets"][0, 0] == 4 and np.all(full["status"][0, 0] >= 0)
    assert np.all(np.diff(full["elevation_deg"][0, 0]) > 0)
    for max_roots in (1, 2):
        res = _home(spherical, np.array([f]), TARGETS, *_column(name), mode, max_roots=max_roots)
        assert np.array_equal(res["n_brackets"], full["n_brackets"])
        for k in ("status", "scan_index", "elevation_deg") + KEYS:
            assert res[k].shape == (1, 3, max_roots)
            assert same_bits(res[k], full[k][..., :max_roots]), k


@pytest.mark.parametrize("spherical", [False, True])
def test_a_column_of_three_levels(spherical):
    """n_alt = 3 (one trip of everything; the ground level is inserted below the three)."""
    alt = np.array([60.0, 100.0, 250.0])
    den = np.array([0.0, 2e11, 1.2e12])
    bmag, bpsi = np.full(3, 4.5e-5), np.full(3, 60.0)
    f = np.array([5e6, 7e6])
    t = np.array([150.0, 400.0, 900.0])
    scan = np.linspace(2.0, 88.0, 345)
    res = _home(spherical, f, t, alt, den, bmag, bpsi, "O")
    check_against_host_route(spherical, res, f, t, [alt, den, bmag, bpsi], "O", scan)
    check_rows(res, t, scan)
    assert res["n_brackets"].sum() > 0


@pytest.mark.parametrize("spherical", [False, True])
def test_one_evaluation_per_bracket(spherical):
    """max_iter = 1: the loop's bound is the argument's - a status is 0 or 1 and the result stays inside its bracket."""
    scan = np.linspace(2.0, 88.0, 345)
    for case in (0, 1):
        name, f, mode = CASES[case]
        res = _home(spherical, np.array([f]), TARGETS, *_column(name), mode, max_iter=1)
        full = _g20_result(int(spherical), case)
        assert np.array_equal(res["n_brackets"], full["n_brackets"]) and np.array_equal(res["scan_index"], full["scan_index"])
        used = check_rows(res, TARGETS, scan)
        assert used.any() and np.isin(res["status"][used], (0, 1)).all()
        assert (res["status"][used] == 1).any()


@pytest.mark.parametrize("spherical", [False, True])
def test_links_without_a_bracket(spherical):
    """A target beyond every D_i, a NaN target, and a frequency at which every ray escapes: n_brackets 0, NaN rows,
    status -1 - beside a link that has roots."""
    prof = _column("gauss")
    t = np.array([800.0, 1e7, np.nan])
    res = _home(spherical, np.array([4e6, 30e6]), t, *prof, "O")
    assert res["n_brackets"][0, 0] >= 1 and np.all(res["n_brackets"][0, 1:] == 0) and np.all(res["n_brackets"][1] == 0)
    check_rows(res, t, np.linspace(2.0, 88.0, 345))
    assert np.all(res["status"][1] == -1) and np.isnan(res["elevation_deg"][1]).all()
    assert np.all(res["status"][0, 1:] == -1)


@pytest.mark.parametrize("spherical", [False, True])
def test_two_calls_give_identical_bits(spherical):
    from pyrayhf_amd import synth
    alt, den, bmag, bpsi = synth.chapman_profiles(3, 11)
    f = np.linspace(3e6, 12e6, 16)
    a = _home(spherical, f, TARGETS, alt, den, bmag, bpsi, "X")
    b = _home(spherical, f, TARGETS, alt, den, bmag, bpsi, "X")
    assert a["n_brackets"].sum() > 0
    for k in a:
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("geometry", [0, 1])
def test_device_resident_arrays(geometry):
    """PRHF_FLAG_DEVICE_PTRS: torch tensors through the binding; the rows and counts are bit for bit the host-buffer
    call's; a link_group out of range gives NaN rows, no bracket and PRHF_EINVAL, the other links their results."""
    import torch
    from pyrayhf_amd import _native
    name, f, mode = CASES[0]
    prof = _column(name)
    want = _g20_result(geometry, 0)
    dev = {k: torch.as_tensor(np.ascontiguousarray(v).reshape(1, -1), device="cuda") for k, v in zip(("alt", "den", "bmag", "bpsi"), prof)}
    n_alt = prof[0].size
    gf = torch.tensor([f], dtype=torch.float64, device="cuda")
    gp = torch.zeros(1, dtype=torch.int64, device="cuda")
    lr = torch.as_tensor(TARGETS, device="cuda")
    scan = torch.as_tensor(np.linspace(2.0, 88.0, 345), device="cuda")
    ctx = _native.host_context(0)
    for groups, want_rc in (([0, 0, 0], _native.OK), ([0, 3, 0], _native.EINVAL), ([-1, 0, 0], _native.EINVAL)):
        lg = torch.tensor(groups, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, 4, 11), dtype=torch.float64, device="cuda")
        nb = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        rc = ctx.snell_home(geometry, gf.data_ptr(), gp.data_ptr(), 1, lg.data_ptr(), lr.data_ptr(), 3, scan.data_ptr(), 345,
                            dev["den"].data_ptr(), dev["bmag"].data_ptr(), dev["bpsi"].data_ptr(), dev["alt"].data_ptr(), 1,
                            n_alt, 0, _native.MODE_O, 6371.0, 1.0, 200.0, 400, TOL, 64, 4, out.data_ptr(), nb.data_ptr(),
                            _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (groups, rc, _native.last_error())
        o, n = out.cpu().numpy(), nb.cpu().numpy()
        for l, grp in enumerate(groups):
            if grp == 0:
                assert n[l] == want["n_brackets"][0, l]
                assert same_bits(o[l, :, 0], want["elevation_deg"][0, l])
                assert np.array_equal(np.nan_to_num(o[l, :, 1], nan=-9).astype(np.int64), want["status"][0, l])
                for i, k in enumerate(KEYS[:-1]):
                    assert same_bits(o[l, :, 3 + i], want[k][0, l]), k
            else:
                assert n[l] == 0 and np.isnan(o[l, :, 0]).all() and np.all(o[l, :, 1] == -1) and np.isnan(o[l, :, 2:]).all()
