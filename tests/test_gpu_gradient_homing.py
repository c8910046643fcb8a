"""GPU: point-to-point homing for the gradient tracers (prhf_gradient_home_f64) against the
tracers' own calls, against a host restatement of the refine rule (tests/gradient_homing_rule.py) and against fixture
G21 (tools/gen_golden_gradient_homing.py: the reference's tracers driven by that restatement, and truth roots).

Inputs are G21's: the tilted (0.3) two-layer ionosphere of g18 on 121 x 201 nodes, 6 MHz O and 9 MHz X, launch point
(-400, 0), the bounded control set with max_step_km=2, the scan np.linspace(5, 85, 33), range_tol_km=0.05, max_iter=64.

Accuracy rule against G21, per status-0 bracket and per geometry (maxima over the fixture's roots of that geometry; the
factor 2 is the gradient tracers' rule: the same method at the same tolerances has truncation error of the same size
but not of the same sign):

    |e - e_truth|       <= de := (range_tol_km + 2 max err_D) / |dD/de|
    |P - P_truth|       <= 2 max err_P + |dP/de| de
    |tau - tau_truth|   <= 2 max err_T + |dT/de| de
"""

import functools

import numpy as np
import pytest

from conftest import load_golden, same_bits
from pyrayhf_amd import _native, gradient, synth
import gradient_homing_rule as rule

pytestmark = pytest.mark.gpu

R_E = gradient.constants()[2]
CASES = (("O", 6.0e6), ("X", 9.0e6))
X0, Z0 = -400.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TARGETS = np.array([300.0, 100.0, 700.0, 1500.0, np.nan])
TOL, MAX_ITER = 0.05, 64
CTL = (dict(s_max_km=4000.0, max_step_km=2.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0),
       dict(s_max_km=4000.0, max_step_km=2.0, r_max_km=R_E + 600.0, phi_min=-1000.0 / R_E, phi_max=1000.0 / R_E))
HOME = (gradient.home_rays_cartesian_gradient, gradient.home_rays_spherical_gradient)
FAN = (gradient.trace_fan_cartesian_gradient, gradient.trace_fan_spherical_gradient)
RAYS = (gradient.trace_rays_cartesian_gradient, gradient.trace_rays_spherical_gradient)
RAY_KEYS = gradient._KEYS
GEOS = [0, 1]


def _row_key(k):
    return "ray_status" if k == "status" else k


@functools.lru_cache(maxsize=None)
def _field(geo, tilt=0.3):
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, tilt, 18)
    name = "spherical" if geo else "cartesian"
    parts = [gradient.refractive_field([f], den, bmag, bpsi, z, x, mode, geometry=name) for mode, f in CASES]
    a0, a1 = (R_E + z, x / R_E) if geo else (z, x)
    return gradient.RefractiveField(a0, a1, np.concatenate([p.mu for p in parts]), np.concatenate([p.mup for p in parts]),
                                    geometry=name)


@functools.lru_cache(maxsize=None)
def _one_field(geo, fi):
    f = _field(geo)
    return gradient.RefractiveField(f.axis0, f.axis1, f.mu[fi], f.mup[fi], geometry=f.geometry)


@functools.lru_cache(maxsize=None)
def _g21_result(geo):
    """The call on G21's links: (field, target) = (2, 5), four rows each."""
    return HOME[geo](_field(geo), TARGETS, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])


@functools.lru_cache(maxsize=None)
def _fan(geo):
    return FAN[geo](_field(geo), SCAN, X0, Z0, **CTL[geo])


def _ray(geo, field, fi, e, x0=X0):
    return float(RAYS[geo](field, x0, Z0, np.float64(e), np.int64(fi), **CTL[geo])["ground_range_km"])


def _check_rows(geo, field, res, targets, tol, x0=X0, ctl=None):
    """Every used row is the tracer's row at the returned elevation; status-0 rows land within the tolerance; unused rows
    are NaN / -1 / 0.  Returns the number of used rows."""
    used = res["status"] >= 0
    fi = np.broadcast_to(np.arange(res["status"].shape[0])[:, None, None], used.shape)
    t = np.broadcast_to(np.asarray(targets)[None, :, None], used.shape)
    assert np.array_equal(used, np.arange(used.shape[2])[None, None, :] < np.minimum(res["n_brackets"], used.shape[2])[..., None])
    assert np.isin(res["status"][used], (0, 1, 2)).all() and np.all(res["scan_index"][used] >= 0)
    if used.any():
        again = RAYS[geo](field, x0, Z0, res["elevation_deg"][used], fi[used], **(CTL[geo] if ctl is None else ctl))
        for k in RAY_KEYS:
            assert same_bits(res[_row_key(k)][used], again[k]), k
        assert np.all(res["ray_status"][used] == 0)                  # the result of a bracket is a ray that lands
        ok = res["status"][used] == 0
        miss = np.abs(res["ground_range_km"][used] - t[used])
        assert np.all(miss[ok] <= tol), miss[ok].max()
    for k in RAY_KEYS:
        v = res[_row_key(k)][~used]
        assert np.all(v == (-1 if k == "status" else 0)) if k in gradient._INT_KEYS else np.isnan(v).all(), k
    assert np.isnan(res["elevation_deg"][~used]).all() and np.all(res["status"][~used] == -1)
    assert np.all(res["scan_index"][~used] == -1)
    return int(used.sum())


@pytest.mark.parametrize("geo", GEOS)
def test_scan_is_the_fan(geo):
    """Brackets computed in NumPy from trace_fan_*_gradient's ground ranges are the call's, for all of G21's links."""
    res, d = _g21_result(geo), _fan(geo)["ground_range_km"]
    for fi in range(2):
        for ti, t in enumerate(TARGETS):
            idx = rule.brackets(d[fi], float(t))
            assert res["n_brackets"][fi, ti] == len(idx)
            want = (idx + [-1] * 4)[:4]
            assert res["scan_index"][fi, ti].tolist() == want, (fi, ti)
    assert np.all(res["n_brackets"][:, 3:] == 0)                     # out of reach, NaN


@pytest.mark.parametrize("geo", GEOS)
def test_rows_are_tracer_rows(geo):
    n = _check_rows(geo, _field(geo), _g21_result(geo), TARGETS, TOL)
    assert n == _g21_result(geo)["n_brackets"].sum() >= 6


@pytest.mark.parametrize("geo", GEOS)
def test_the_rule(geo):
    """The refine rule restated on the host, stepping with one GPU ray per call, reproduces every elevation and status of
    the link with the most brackets (Cartesian, 6 MHz O, 300 km: three) bit for bit."""
    res, d = _g21_result(geo), _fan(geo)["ground_range_km"]
    fi, ti = 0, 0
    idx = rule.brackets(d[fi], float(TARGETS[ti]))
    assert len(idx) == (2 if geo else 3)
    for rank, i in enumerate(idx):
        r = rule.refine(lambda e: _ray(geo, _field(geo), fi, e), SCAN, d[fi], i, TARGETS[ti], TOL, MAX_ITER)
        print(f"geometry {geo} bracket {i}: status {r['status']}, {len(r['tried'])} rays, e = {r['elevation_deg']!r}")
        assert res["status"][fi, ti, rank] == r["status"]
        assert res["elevation_deg"][fi, ti, rank] == r["elevation_deg"]


@pytest.mark.parametrize("geo", GEOS)
def test_against_the_reference(geo):
    g = load_golden("g21_gradient_homing.npz")
    res = _g21_result(geo)
    here = g["bracket_case"] // 2 == geo
    conv = (g["bracket_status"] == 0) & here
    err = {k: np.abs(g["default_" + k][conv] - g["truth_" + k][conv]).max()
           for k in ("ground_range_km", "group_path_km", "group_delay_sec")}
    worst = dict(e=0.0, P=0.0, T=0.0)
    for fi in range(2):
        c = 2 * geo + fi
        assert np.array_equal(res["n_brackets"][fi], g["n_brackets"][c])
        for ti in range(TARGETS.size):
            rows = np.nonzero((g["bracket_case"] == c) & (g["bracket_target"] == ti))[0]
            assert res["scan_index"][fi, ti, :rows.size].tolist() == g["bracket_scan_index"][rows].tolist()
            for rank, b in enumerate(rows):
                st = int(res["status"][fi, ti, rank])
                assert (st == 0) == (g["bracket_status"][b] == 0), (c, ti, rank, st, int(g["bracket_status"][b]))
                if st != 0:
                    print(f"case {c} target {TARGETS[ti]} bracket {int(g['bracket_scan_index'][b])}: status {st} here, "
                          f"{int(g['bracket_status'][b])} in the reference")
                    continue
                de = (TOL + 2 * err["ground_range_km"]) / abs(g["dD_de"][b])
                miss_e = abs(res["elevation_deg"][fi, ti, rank] - g["e_truth"][b])
                bound_p = 2 * err["group_path_km"] + abs(g["dP_de"][b]) * de
                bound_t = 2 * err["group_delay_sec"] + abs(g["dT_de"][b]) * de
                miss_p = abs(res["group_path_km"][fi, ti, rank] - g["truth_group_path_km"][b])
                miss_t = abs(res["group_delay_sec"][fi, ti, rank] - g["truth_group_delay_sec"][b])
                print(f"case {c} target {TARGETS[ti]} bracket {int(g['bracket_scan_index'][b])}: |e - e_truth| = {miss_e:.3e} "
                      f"(bound {de:.3e}), |P - P_truth| = {miss_p:.3e} ({bound_p:.3e}), |tau - tau_truth| = {miss_t:.3e} "
                      f"({bound_t:.3e})")
                worst = dict(e=max(worst["e"], miss_e / de), P=max(worst["P"], miss_p / bound_p),
                             T=max(worst["T"], miss_t / bound_t))
                assert miss_e <= de and miss_p <= bound_p and miss_t <= bound_t
    print(f"geometry {geo}: reference errors {err}; worst error / bound: {worst}")


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("n_scan", [2, 63, 64, 65])
def test_scan_grid_sizes(geo, n_scan):
    """2, 63, 64 and 65 nodes on one group: brackets as NumPy finds them on the fan of that grid, rows as the tracer's."""
    scan = np.linspace(12.0, 58.0, n_scan)
    field = _one_field(geo, 0)
    t = np.array([300.0])
    res = HOME[geo](field, t, X0, Z0, scan_elevation_deg=scan, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    d = FAN[geo](field, scan, X0, Z0, **CTL[geo])["ground_range_km"][0]
    idx = rule.brackets(d, 300.0)
    assert res["n_brackets"][0, 0] == len(idx) >= 1
    assert res["scan_index"][0, 0].tolist() == (idx + [-1] * 4)[:4]
    _check_rows(geo, field, res, t, TOL)


@pytest.mark.parametrize("geo", GEOS)
def test_one_link_and_more_rows_than_a_wavefront(geo):
    many = np.linspace(-140.0, 680.0, 36)
    res = HOME[geo](_field(geo), many, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    n = _check_rows(geo, _field(geo), res, many, TOL)
    print(f"geometry {geo}: {n} used rows, counters {_native.host_context(None).gradient_home_counters()}")
    assert n >= 65
    for ti in (0, 17, 35):                                            # a link alone gets the rows it gets in company
        one = HOME[geo](_field(geo), many[ti:ti + 1], X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER,
                        **CTL[geo])
        for k in one:
            assert same_bits(one[k][:, 0], res[k][:, ti]), (k, ti)


def test_max_roots_gives_prefixes():
    """max_roots 1 / 2 / 4 on the three-bracket link: n_brackets unchanged, rows are prefixes of one another."""
    full = _g21_result(0)
    for max_roots in (1, 2):
        res = HOME[0](_field(0), TARGETS[:1], X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER,
                      max_roots=max_roots, **CTL[0])
        assert res["n_brackets"][0, 0] == full["n_brackets"][0, 0] == 3
        for k in res:
            if k != "n_brackets":
                assert res[k].shape == (2, 1, max_roots) and same_bits(res[k][:, 0], full[k][:, 0, :max_roots]), k


@pytest.mark.parametrize("geo", GEOS)
def test_max_iter_one_and_zero_tolerance(geo):
    full = _g21_result(geo)
    t = TARGETS[:3]
    one = HOME[geo](_field(geo), t, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=1, **CTL[geo])
    assert np.array_equal(one["n_brackets"], full["n_brackets"][:, :3])
    assert np.array_equal(one["scan_index"], full["scan_index"][:, :3])
    assert _check_rows(geo, _field(geo), one, t, TOL) == one["n_brackets"].sum()
    # range_tol_km = 0: no ray hits a target exactly, so no status 0; the best miss is no worse than with the default
    zero = HOME[geo](_field(geo), t, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=0.0, max_iter=MAX_ITER, **CTL[geo])
    _check_rows(geo, _field(geo), zero, t, 0.0)
    used = zero["status"] >= 0
    assert np.array_equal(used, full["status"][:, :3] >= 0)
    miss0 = np.abs(zero["ground_range_km"] - t[None, :, None])[used]
    miss = np.abs(full["ground_range_km"][:, :3] - t[None, :, None])[used]
    assert np.all((zero["status"][used] != 0) | (miss0 == 0.0))
    assert np.all(miss0 <= miss), (miss0, miss)
    print(f"geometry {geo}: statuses at tolerance 0: {zero['status'][used].tolist()}, best misses {miss0.tolist()}")


@pytest.mark.parametrize("geo", GEOS)
def test_vacuum_field_has_no_brackets(geo):
    """A 3 x 3 field of mu = 1: every ray leaves through the top; no bracket, every row unused."""
    z, x = np.array([0.0, 300.0, 600.0]), np.array([-1000.0, 0.0, 1000.0])
    one = np.ones((3, 3))
    field = (gradient.RefractiveField(R_E + z, x / R_E, one, one, geometry="spherical") if geo else
             gradient.RefractiveField(z, x, one, one))
    t = np.array([300.0, -200.0, 0.0])
    res = HOME[geo](field, t, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    fan = FAN[geo](field, SCAN, X0, Z0, **CTL[geo])
    assert np.all(fan["status"] == 1) and np.all(res["n_brackets"] == 0)
    assert _check_rows(geo, field, res, t, TOL) == 0


@pytest.mark.parametrize("geo", GEOS)
def test_scan_past_ninety_degrees_looks_behind(geo):
    scan = np.linspace(95.0, 175.0, 33)
    t = np.array([-500.0])
    res = HOME[geo](_one_field(geo, 0), t, 0.0, Z0, scan_elevation_deg=scan, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    ok = res["status"][0, 0] == 0
    print(f"geometry {geo}: elevations {res['elevation_deg'][0, 0].tolist()}, statuses {res['status'][0, 0].tolist()}")
    assert ok.any() and np.all(res["elevation_deg"][0, 0][ok] > 90.0)
    assert np.all(np.abs(res["ground_range_km"][0, 0][ok] + 500.0) <= TOL)
    _check_rows(geo, _one_field(geo, 0), res, t, TOL, x0=0.0)


@pytest.mark.parametrize("geo", GEOS)
def test_same_bits_again_and_two_transmitters_equal_two_calls(geo):
    full = _g21_result(geo)
    again = HOME[geo](_field(geo), TARGETS, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    for k in full:
        assert same_bits(full[k], again[k]), k
    for fi in range(2):
        alone = HOME[geo](_one_field(geo, fi), TARGETS, X0, Z0, scan_elevation_deg=SCAN, range_tol_km=TOL, max_iter=MAX_ITER,
                          **CTL[geo])
        for k in full:
            assert same_bits(full[k][fi], alone[k][0]), (k, fi)


@pytest.mark.parametrize("geo", GEOS)
def test_device_resident_arrays(geo):
    """PRHF_FLAG_DEVICE_PTRS: torch tensors through the binding; rows and counts are bit for bit the host-buffer call's; a
    link_group out of range gives NaN rows, no bracket and PRHF_EINVAL, the other links their results; a group_field out
    of range likewise for the links of that group."""
    import torch
    want = _g21_result(geo)
    field = _field(geo)
    ctx = field._ctx()
    c = CTL[geo]
    ctl = ((c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["r_max_km"], c["phi_min"], c["phi_max"], 50) if geo else
           (c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["z_max_km"], c["x_min_km"], c["x_max_km"], 50))
    gx = torch.full((2,), X0, dtype=torch.float64, device="cuda")
    gz = torch.full((2,), Z0, dtype=torch.float64, device="cuda")
    lt = torch.tensor([300.0, 700.0, 300.0], dtype=torch.float64, device="cuda")
    scan = torch.as_tensor(SCAN, device="cuda")
    for fields, groups, want_rc in (([0, 1], [0, 1, 1], _native.OK), ([0, 1], [0, 2, 1], _native.EINVAL),
                                    ([0, 1], [-1, 0, 1], _native.EINVAL), ([0, 2], [0, 1, 0], _native.EINVAL)):
        gf = torch.tensor(fields, dtype=torch.int64, device="cuda")
        lg = torch.tensor(groups, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, 4, 15), dtype=torch.float64, device="cuda")
        nb = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        rc = ctx.gradient_home(geo, field.records().data_ptr(), 2, field.axis0.size, field.axis1.size,
                               field.axis0.ctypes.data, field.axis1.ctypes.data, gf.data_ptr(), gx.data_ptr(), gz.data_ptr(), 2,
                               lg.data_ptr(), lt.data_ptr(), 3, scan.data_ptr(), SCAN.size, R_E if geo else 0.0, ctl,
                               field.fills, TOL, MAX_ITER, 4, out.data_ptr(), nb.data_ptr(), _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (fields, groups, rc, _native.last_error())
        o, n = out.cpu().numpy(), nb.cpu().numpy()
        for l, (grp, ti) in enumerate(zip(groups, (0, 2, 0))):
            if 0 <= grp < 2 and fields[grp] < 2:
                fi = fields[grp]
                assert n[l] == want["n_brackets"][fi, ti]
                assert same_bits(o[l, :, 0], want["elevation_deg"][fi, ti])
                assert np.array_equal(o[l, :, 1].astype(np.int64), want["status"][fi, ti])
                for i, k in enumerate(RAY_KEYS):
                    used = want["status"][fi, ti] >= 0
                    assert same_bits(o[l, used, 3 + i], want[_row_key(k)][fi, ti][used].astype(np.float64)), k
                    assert np.isnan(o[l, ~used, 3 + i]).all()
            else:
                assert n[l] == 0 and np.isnan(o[l, :, 0]).all() and np.all(o[l, :, 1] == -1) and np.isnan(o[l, :, 2:]).all()


@pytest.mark.parametrize("geo", GEOS)
def test_mirrored_links_on_the_zero_tilt_twin(geo):
    """Zero tilt, max_step_km=0.5 (the capped step sequence on which mirrored rays agree): homing
    from x0 = 0 to +t and, with the scan mirrored about 90 degrees, to -t finds mirrored elevations:
    |e + e' - 180| <= 2 range_tol_km / |dD/de|, the slope taken from the scan interval of the bracket."""
    field = _field(geo, 0.0)
    field = gradient.RefractiveField(field.axis0, field.axis1, field.mu[0], field.mup[0], geometry=field.geometry)
    ctl = dict(CTL[geo], max_step_km=0.5)
    scan = np.linspace(20.0, 60.0, 17)
    t = np.array([500.0])
    right = HOME[geo](field, t, 0.0, Z0, scan_elevation_deg=scan, range_tol_km=TOL, max_iter=MAX_ITER, max_roots=1, **ctl)
    left = HOME[geo](field, -t, 0.0, Z0, scan_elevation_deg=(180.0 - scan)[::-1].copy(), range_tol_km=TOL, max_iter=MAX_ITER,
                     max_roots=64, **ctl)
    assert right["status"][0, 0, 0] == 0 and right["n_brackets"][0, 0] == left["n_brackets"][0, 0] >= 1
    last = int(left["n_brackets"][0, 0]) - 1                          # ascending elevation: the mirror of the first is the last
    assert left["status"][0, 0, last] == 0
    i = int(right["scan_index"][0, 0, 0])
    d = FAN[geo](field, scan[i:i + 2], 0.0, Z0, **ctl)["ground_range_km"][0]
    slope = abs((d[1] - d[0]) / (scan[i + 1] - scan[i]))
    seen = abs(right["elevation_deg"][0, 0, 0] + left["elevation_deg"][0, 0, last] - 180.0)
    print(f"geometry {geo}: |e + e' - 180| = {seen:.3e}, bound {2 * TOL / slope:.3e} (|dD/de| = {slope:.3f} km/deg)")
    assert seen <= 2 * TOL / slope
    _check_rows(geo, field, right, t, TOL, x0=0.0, ctl=ctl)
