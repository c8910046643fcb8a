"""GPU: multi-hop gradient ray tracing and multi-hop homing (prhf_trace_gradient_hops_f64, prhf_gradient_hop_home_f64,
DESIGN.md section 4.12) against the one-hop tracers and homing calls, against the host restatement of the refine rule
(tests/gradient_homing_rule.py) and against fixture G24 (tools/gen_golden_gradient_hops.py: the reference's tracer chained
on the CPU in three runs, and truth roots of the two-hop homing).

Inputs are G24's: synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000), 6 MHz O and 9 MHz X, launch point
(-1800, 0), the elevations np.linspace(10, 70, 13), 3 hops, s_max_km=4000, max_step_km=1, z_max_km=600, x within
+-2000 km; homing on hop 1 with those elevations as scan grid, range_tol_km=0.05, max_iter=64.

Accuracy against G24 (Cartesian): per hop and per key max |GPU - truth| <= 2 max |reference default - truth| (G18's rule:
the same method at the same tolerances has truncation error of the same size but not of the same sign); the homing rows
under G21's rule with the totals of the chain in the places of a ray's range, path and delay.
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
X0, Z0 = -1800.0, 0.0
ELEV = np.linspace(10.0, 70.0, 13)
H = 3
TARGETS = np.array([-500.0, 0.0, -1100.0, 1900.0, np.nan])
HOME_H, TOL, MAX_ITER = 2, 0.05, 64
CTL = (dict(s_max_km=4000.0, max_step_km=1.0, z_max_km=600.0, x_min_km=-2000.0, x_max_km=2000.0),
       dict(s_max_km=4000.0, max_step_km=1.0, r_max_km=R_E + 600.0, phi_min=-2000.0 / R_E, phi_max=2000.0 / R_E))
RAYS = (gradient.trace_rays_cartesian_gradient, gradient.trace_rays_spherical_gradient)
HOPS = (gradient.trace_hops_cartesian_gradient, gradient.trace_hops_spherical_gradient)
HOP_FAN = (gradient.trace_hop_fan_cartesian_gradient, gradient.trace_hop_fan_spherical_gradient)
HOME = (gradient.home_rays_cartesian_gradient, gradient.home_rays_spherical_gradient)
HOME_HOPS = (gradient.home_hops_cartesian_gradient, gradient.home_hops_spherical_gradient)
RAY_KEYS = gradient._KEYS
LAUNCH = gradient._HOP_LAUNCH_KEYS
PATHS = (("t", "x", "z", "vx", "vz"), ("t", "r", "phi", "v_r", "v_phi"))
V_HORIZ, V_VERT = ("vx", "v_phi"), ("vz", "v_r")
TOTALS = ("n_landed", "total_group_path_km", "total_group_delay_sec", "total_ground_range_km")
GEOS = [0, 1]
ELEV_BUDGET_DEG = 8 * np.spacing(180.0)          # OpenCL's 6 ulp for atan2 and one for each conversion: 2.3e-13 degrees


@functools.lru_cache(maxsize=None)
def _field(geo):
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000.0)
    name = "spherical" if geo else "cartesian"
    parts = [gradient.refractive_field([f], den, bmag, bpsi, z, x, mode, geometry=name) for mode, f in CASES]
    a0, a1 = (R_E + z, x / R_E) if geo else (z, x)
    return gradient.RefractiveField(a0, a1, np.concatenate([p.mu for p in parts]), np.concatenate([p.mup for p in parts]),
                                    geometry=name)


@functools.lru_cache(maxsize=None)
def _fan_once(geo, n_hops, paths):
    return HOP_FAN[geo](_field(geo), ELEV, n_hops, X0, Z0, return_paths=paths, **CTL[geo])


def _fan(geo, n_hops=H, paths=False):
    """The call on G24's chains: (field, elevation, hop) = (2, 13, n_hops)."""
    return _fan_once(geo, n_hops, paths)


@functools.lru_cache(maxsize=None)
def _rows_again(geo, paths=False):
    """Every used hop row of _fan(geo) traced by the one-hop call at the row's launch columns."""
    res = _fan(geo, H, paths)
    used = res["status"] >= 0
    fi = np.broadcast_to(np.arange(2)[:, None, None], used.shape)
    return used, RAYS[geo](_field(geo), res["launch_x_km"][used], res["launch_z_km"][used], res["launch_elevation_deg"][used],
                           fi[used], return_paths=paths, **CTL[geo])


@functools.lru_cache(maxsize=None)
def _home(geo):
    """The call on G24's links, both fields: (field, target) = (2, 5), four rows of two hops each."""
    return HOME_HOPS[geo](_field(geo), TARGETS, HOME_H, X0, Z0, scan_elevation_deg=ELEV, range_tol_km=TOL, max_iter=MAX_ITER,
                          **CTL[geo])


def _chain_d(geo, fi, e, n_hops=HOME_H):
    return float(HOPS[geo](_field(geo), X0, Z0, np.float64(e), n_hops, np.int64(fi), **CTL[geo])["total_ground_range_km"])


def _assert_unused(res, unused, status_key="status"):
    for k in LAUNCH + RAY_KEYS:
        v = res[status_key if k == "status" else k][unused]
        assert np.all(v == (-1 if k == "status" else 0)) if k in gradient._INT_KEYS else np.isnan(v).all(), k


@pytest.mark.parametrize("geo", GEOS)
def test_rows_are_tracer_rows(geo):
    """Row composition: every used hop row equals trace_rays_*_gradient at its launch columns, all eleven keys."""
    res = _fan(geo)
    used, again = _rows_again(geo)
    assert res["status"].shape == (2, 13, H) and used.sum() >= 60
    for k in RAY_KEYS:
        assert same_bits(res[k][used], again[k]), k
    print(f"geometry {geo}: statuses", " ".join("".join(str(s) if s >= 0 else "-" for s in c) for c in res["status"].reshape(26, H)))


@pytest.mark.parametrize("geo", GEOS)
def test_launch_chaining(geo):
    res = _fan(geo)
    st = res["status"]
    used = st >= 0
    assert used[..., 0].all() and np.array_equal(used[..., 1:], st[..., :-1] == 0)       # unused right after the first non-landing hop
    assert (st[..., 0] != 0).any()                                        # chains that end on hop 0 ...
    assert geo or ((st[..., 0] == 0) & (st[..., 1] > 0)).any()            # ... and, over the flat Earth, one that ends on hop 1
    assert np.all(res["launch_x_km"][..., 0] == X0) and np.all(res["launch_z_km"][..., 0] == Z0)
    assert same_bits(res["launch_elevation_deg"][..., 0], np.broadcast_to(ELEV, (2, 13)))
    nxt = used[..., 1:]
    assert same_bits(res["launch_x_km"][..., 1:][nxt], res["ground_range_km"][..., :-1][nxt])
    assert np.all(res["launch_z_km"][..., 1:][nxt] == 0.0)
    _assert_unused(res, ~used)
    # a hop leaves the ground at the angle the hop before arrived with, mirrored: elevations stay within (0, 180)
    e = res["launch_elevation_deg"][..., 1:][nxt]
    assert np.all((e > 0.0) & (e < 180.0))


@pytest.mark.parametrize("geo", GEOS)
def test_a_raised_ground_is_the_launch_altitude(geo):
    """z_ground_km = 0.3: later hops launch at exactly 0.3 (not at (R_E + 0.3) - R_E), and rows still compose."""
    ctl = dict(CTL[geo], z_ground_km=0.3)
    e, fi = np.array([20.0, 35.0, 50.0]), np.array([0, 1, 1])
    res = HOPS[geo](_field(geo), X0, 0.3, e, H, fi, **ctl)
    used = res["status"] >= 0
    assert used[:, 1:].sum() >= 4 and np.all(res["launch_z_km"][:, 1:][used[:, 1:]] == 0.3)
    again = RAYS[geo](_field(geo), res["launch_x_km"][used], res["launch_z_km"][used], res["launch_elevation_deg"][used],
                      np.broadcast_to(fi[:, None], used.shape)[used], **ctl)
    for k in RAY_KEYS:
        assert same_bits(res[k][used], again[k]), k


@pytest.mark.parametrize("geo", GEOS)
def test_one_hop_is_the_tracer(geo):
    one = _fan(geo, 1)
    idx = np.arange(2, dtype=np.int64)[:, None]
    ray = RAYS[geo](_field(geo), X0, Z0, ELEV[None, :], idx, **CTL[geo])
    for k in RAY_KEYS:
        assert one[k].shape == (2, 13, 1) and same_bits(one[k][..., 0], ray[k]), k
    assert same_bits(one["total_ground_range_km"], ray["ground_range_km"])
    assert same_bits(one["total_group_path_km"], ray["group_path_km"]) and np.array_equal(one["n_landed"], ray["status"] == 0)
    # the chain of three starts with the chain of one
    for k in RAY_KEYS:
        assert same_bits(_fan(geo)[k][..., 0], one[k][..., 0]), k


@pytest.mark.parametrize("geo", GEOS)
def test_paths_and_reflected_elevation(geo):
    res = _fan(geo, H, True)
    plain = _fan(geo)
    for k in LAUNCH + RAY_KEYS + TOTALS:
        assert same_bits(res[k], plain[k]), k                              # asking for the paths changes nothing else
    used, again = _rows_again(geo, True)
    n = res["n_nodes"][used]
    assert res["t"].shape[:3] == (2, 13, H) and res["t"].shape[3] == res["n_nodes"].max() == again["t"].shape[1]
    for k in PATHS[geo] + (("x", "z") if geo else ()):
        assert same_bits(res[k][used], again[k]), k
        assert np.isnan(res[k][~used]).all(), k
        assert np.array_equal(np.isfinite(res[k][used]), np.arange(res[k].shape[3])[None, :] < n[:, None]), k
    # the elevation a hop is launched with is the mirror of the direction of the last node of the hop before
    last = np.maximum(res["n_nodes"] - 1, 0)[..., None]
    v_h = np.take_along_axis(res[V_HORIZ[geo]], last, axis=3)[..., 0]
    v_v = np.take_along_axis(res[V_VERT[geo]], last, axis=3)[..., 0]
    want = np.degrees(np.arctan2(-v_v, v_h))
    nxt = res["status"][..., 1:] >= 0
    miss = np.abs(res["launch_elevation_deg"][..., 1:][nxt] - want[..., :-1][nxt])
    print(f"geometry {geo}: max |launch elevation - degrees(arctan2(-v_vert, v_horiz))| = {miss.max():.3e} degrees "
          f"(budget {ELEV_BUDGET_DEG:.3e}), {int((miss > 0).sum())} of {miss.size} differ")
    assert miss.max() <= ELEV_BUDGET_DEG


@pytest.mark.parametrize("geo", GEOS)
def test_totals(geo):
    res = _fan(geo)
    st = res["status"]
    assert np.array_equal(res["n_landed"], (st == 0).sum(axis=-1))
    for k in ("group_path_km", "group_delay_sec"):
        total = np.zeros(st.shape[:2])
        for h in range(H):
            total = np.where(st[..., h] >= 0, total + res[k][..., h], total)
        assert same_bits(res["total_" + k], total), k
    assert same_bits(res["total_ground_range_km"], np.where(res["n_landed"] == H, res["ground_range_km"][..., H - 1], np.nan))
    assert np.isfinite(res["total_ground_range_km"]).sum() == (res["n_landed"] == H).sum() >= 20


def test_against_the_reference():
    """G24, Cartesian: statuses wherever the three runs agree; per hop and key the factor-2 rule against the truth run."""
    g = load_golden("g24_gradient_hops.npz")
    res = _fan(0)
    agree = (g["default_status"] == g["truth_status"]) & (g["default_status"] == g["check_status"])
    assert np.array_equal(res["status"][agree], g["default_status"][agree])
    pairs = (("group_path_km", res["group_path_km"]), ("group_delay_sec", res["group_delay_sec"]),
             ("ground_range_km", res["ground_range_km"]), ("z_apex_km", res["z_apex_km"]),
             ("next_elevation_deg", np.concatenate([res["launch_elevation_deg"][..., 1:], np.full((2, 13, 1), np.nan)], axis=2)))
    worst = 0.0
    for key, got in pairs:
        for h in range(H - 1 if key == "next_elevation_deg" else H):       # (the last hop of the call has no next hop)
            ok = agree[..., h] & (g["truth_status"][..., h] == 0)
            if key == "next_elevation_deg":
                ok &= agree[..., h + 1] & (g["truth_status"][..., h + 1] >= 0)
            truth = g["truth_" + key][..., h][ok]
            err_ref = np.abs(g["default_" + key][..., h][ok] - truth).max()
            err_gpu = np.abs(got[..., h][ok] - truth).max()
            print(f"{key} hop {h}: max|GPU - truth| = {err_gpu:.3e}, max|reference - truth| = {err_ref:.3e}, "
                  f"ratio {err_gpu / err_ref:.3f} over {int(ok.sum())} rows")
            worst = max(worst, err_gpu / err_ref)
            assert ok.sum() >= 20 and err_gpu <= 2.0 * err_ref, (key, h, err_gpu, err_ref)
    print(f"worst ratio {worst:.3f}")


def _check_home_rows(geo, res, n_hops, targets):
    """Used rows are trace_hops_* rows at the returned elevation, to the bit; status-0 rows land within the tolerance;
    unused rows are NaN / -1 / 0.  Returns the number of used rows."""
    used = res["status"] >= 0
    fi = np.broadcast_to(np.arange(used.shape[0])[:, None, None], used.shape)
    t = np.broadcast_to(np.asarray(targets)[None, :, None], used.shape)
    assert np.array_equal(used, np.arange(used.shape[2])[None, None, :] < np.minimum(res["n_brackets"], used.shape[2])[..., None])
    assert np.isin(res["status"][used], (0, 1, 2)).all() and np.all(res["scan_index"][used] >= 0)
    again = HOPS[geo](_field(geo), X0, Z0, res["elevation_deg"][used], n_hops, fi[used], **CTL[geo])
    for k in LAUNCH + RAY_KEYS + TOTALS:
        assert same_bits(res["ray_status" if k == "status" else k][used], again[k]), k
    assert np.all(res["n_landed"][used] == n_hops)                        # the result of a bracket is a chain that lands
    ok = res["status"][used] == 0
    miss = np.abs(res["total_ground_range_km"][used] - t[used])
    assert ok.any() and np.all(miss[ok] <= TOL), miss[ok].max()
    _assert_unused(res, ~used, "ray_status")
    assert np.isnan(res["elevation_deg"][~used]).all() and np.all(res["status"][~used] == -1)
    assert np.all(res["scan_index"][~used] == -1) and np.all(res["n_landed"][~used] == 0)
    for k in TOTALS[1:]:
        assert np.isnan(res[k][~used]).all(), k
    return int(used.sum())


@pytest.mark.parametrize("geo", GEOS)
def test_homing_rows_are_chain_rows(geo):
    res = _home(geo)
    assert res["status"].shape == (2, 5, 4) and res["ray_status"].shape == (2, 5, 4, HOME_H)
    n = _check_home_rows(geo, res, HOME_H, TARGETS)
    assert n == res["n_brackets"].sum() >= 5
    print(f"geometry {geo}: {n} used rows, n_brackets {res['n_brackets'].tolist()}, "
          f"counters {_native.host_context(None).gradient_home_counters()}")


@pytest.mark.parametrize("geo", GEOS)
def test_homing_scan_is_the_hop_fan(geo):
    res, d = _home(geo), _fan(geo, HOME_H)["total_ground_range_km"]
    for fi in range(2):
        for ti, t in enumerate(TARGETS):
            idx = rule.brackets(d[fi], float(t))
            assert res["n_brackets"][fi, ti] == len(idx)
            assert res["scan_index"][fi, ti].tolist() == (idx + [-1] * 4)[:4], (fi, ti)
    assert np.all(res["n_brackets"][:, 3:] == 0)                          # out of reach, NaN
    assert res["n_brackets"][0, 0] == 3 if geo == 0 else res["n_brackets"][0, 0] >= 1    # D(e) of two hops is not monotonic


@pytest.mark.parametrize("geo", GEOS)
def test_homing_follows_the_rule(geo):
    """The refine rule on the host, stepping with one GPU chain per call, reproduces every elevation and status of the
    link 6 MHz O to -500 km (over the flat Earth: three brackets)."""
    res, d = _home(geo), _fan(geo, HOME_H)["total_ground_range_km"]
    idx = rule.brackets(d[0], -500.0)
    assert len(idx) == 3 if geo == 0 else 1 <= len(idx) <= 4
    for rank, i in enumerate(idx):
        r = rule.refine(lambda e: _chain_d(geo, 0, e), ELEV, d[0], i, -500.0, TOL, MAX_ITER)
        print(f"geometry {geo} bracket {i}: status {r['status']}, {len(r['tried'])} chains, e = {r['elevation_deg']!r}")
        assert res["status"][0, 0, rank] == r["status"]
        assert res["elevation_deg"][0, 0, rank] == r["elevation_deg"]


@pytest.mark.parametrize("geo", GEOS)
def test_homing_on_one_hop_is_homing(geo):
    t = np.array([-1400.0, -1000.0, np.nan])
    kw = dict(scan_elevation_deg=ELEV, range_tol_km=TOL, max_iter=MAX_ITER, **CTL[geo])
    one = HOME_HOPS[geo](_field(geo), t, 1, X0, Z0, **kw)
    ray = HOME[geo](_field(geo), t, X0, Z0, **kw)
    assert ray["n_brackets"].sum() >= 2
    for k in ray:
        got = one[k] if one[k].ndim == ray[k].ndim else one[k][..., 0]
        assert same_bits(got, ray[k]), k
    assert same_bits(one["total_ground_range_km"], ray["ground_range_km"])


def test_homing_against_the_reference():
    """G21's accuracy rule on G24's truth roots (Cartesian, 6 MHz O, two hops): per status-0 bracket
    |e - e_truth| <= de := (range_tol_km + 2 max err_D) / |dD/de|, |P - P_truth| <= 2 max err_P + |dP/de| de and the same for
    the delay, with the chain's totals for D, P and tau and the maxima taken over the fixture's roots."""
    g = load_golden("g24_gradient_hops.npz")
    res = _home(0)
    conv = g["bracket_status"] == 0
    err = {k: np.abs(g["default_total_" + k][conv] - g["truth_total_" + k][conv]).max()
           for k in ("ground_range_km", "group_path_km", "group_delay_sec")}
    assert np.array_equal(res["n_brackets"][0], g["n_brackets"])
    for ti in range(TARGETS.size):
        rows = np.nonzero(g["bracket_target"] == ti)[0]
        assert res["scan_index"][0, ti, :rows.size].tolist() == g["bracket_scan_index"][rows].tolist()
        for rank, b in enumerate(rows):
            st = int(res["status"][0, ti, rank])
            assert (st == 0) == (g["bracket_status"][b] == 0), (ti, rank, st, int(g["bracket_status"][b]))
            if st != 0:
                continue
            de = (TOL + 2 * err["ground_range_km"]) / abs(g["dD_de"][b])
            miss_e = abs(res["elevation_deg"][0, ti, rank] - g["e_truth"][b])
            bound_p = 2 * err["group_path_km"] + abs(g["dP_de"][b]) * de
            bound_t = 2 * err["group_delay_sec"] + abs(g["dT_de"][b]) * de
            miss_p = abs(res["total_group_path_km"][0, ti, rank] - g["truth_total_group_path_km"][b])
            miss_t = abs(res["total_group_delay_sec"][0, ti, rank] - g["truth_total_group_delay_sec"][b])
            print(f"target {TARGETS[ti]} bracket {int(g['bracket_scan_index'][b])}: |e - e_truth| = {miss_e:.3e} (bound {de:.3e}), "
                  f"|P - P_truth| = {miss_p:.3e} ({bound_p:.3e}), |tau - tau_truth| = {miss_t:.3e} ({bound_t:.3e})")
            assert miss_e <= de and miss_p <= bound_p and miss_t <= bound_t
    print(f"reference errors {err}")


def _ctl_tuple(geo):
    c = CTL[geo]
    return ((c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["r_max_km"], c["phi_min"], c["phi_max"], 50) if geo else
            (c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["z_max_km"], c["x_min_km"], c["x_max_km"], 50))


@pytest.mark.parametrize("geo", GEOS)
def test_device_resident_rays(geo):
    """PRHF_FLAG_DEVICE_PTRS: rows are the host-buffer call's; a ray_field out of range gives that ray NaN rows and
    PRHF_EINVAL, the other rays their results - as in the one-hop tracer."""
    import torch
    want = _fan(geo)
    field = _field(geo)
    ctx = field._ctx()
    ei = [2, 6, 11]
    x0 = torch.full((3,), X0, dtype=torch.float64, device="cuda")
    z0 = torch.full((3,), Z0, dtype=torch.float64, device="cuda")
    e = torch.as_tensor(ELEV[ei], device="cuda")
    for fields, want_rc in (([0, 1, 1], _native.OK), ([0, 2, 1], _native.EINVAL), ([-1, 1, 0], _native.EINVAL)):
        rf = torch.tensor(fields, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, H, 15), dtype=torch.float64, device="cuda")
        rc = ctx.trace_gradient_hops(geo, field.records().data_ptr(), 2, field.axis0.size, field.axis1.size,
                                     field.axis0.ctypes.data, field.axis1.ctypes.data, x0.data_ptr(), z0.data_ptr(),
                                     e.data_ptr(), rf.data_ptr(), 3, R_E if geo else 0.0, _ctl_tuple(geo), field.fills, H,
                                     out.data_ptr(), None, 0, _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (fields, rc, _native.last_error())
        o = out.cpu().numpy()
        for r, (fi, i) in enumerate(zip(fields, ei)):
            if 0 <= fi < 2:
                for c, k in enumerate(LAUNCH + RAY_KEYS):
                    assert same_bits(o[r, :, c], want[k][fi, i].astype(np.float64)), (fields, r, k)
            else:
                assert np.isnan(o[r]).all()


@pytest.mark.parametrize("geo", GEOS)
def test_device_resident_homing(geo):
    """A group_field out of range gives the links of that group NaN rows, no bracket and PRHF_EINVAL, the other links
    their results - as in the one-hop homing."""
    import torch
    want = _home(geo)
    field = _field(geo)
    ctx = field._ctx()
    gx = torch.full((2,), X0, dtype=torch.float64, device="cuda")
    gz = torch.full((2,), Z0, dtype=torch.float64, device="cuda")
    lt = torch.tensor([-500.0, -1100.0, -500.0], dtype=torch.float64, device="cuda")
    lg = torch.tensor([0, 1, 1], dtype=torch.int64, device="cuda")
    scan = torch.as_tensor(ELEV, device="cuda")
    width = 3 + 15 * HOME_H
    for fields, want_rc in (([0, 1], _native.OK), ([0, 2], _native.EINVAL)):
        gf = torch.tensor(fields, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, 4, width), dtype=torch.float64, device="cuda")
        nb = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        rc = ctx.gradient_hop_home(geo, field.records().data_ptr(), 2, field.axis0.size, field.axis1.size,
                                   field.axis0.ctypes.data, field.axis1.ctypes.data, gf.data_ptr(), gx.data_ptr(), gz.data_ptr(), 2,
                                   lg.data_ptr(), lt.data_ptr(), 3, scan.data_ptr(), ELEV.size, R_E if geo else 0.0,
                                   _ctl_tuple(geo), field.fills, TOL, MAX_ITER, 4, HOME_H, out.data_ptr(), nb.data_ptr(),
                                   _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (fields, rc, _native.last_error())
        o, n = out.cpu().numpy(), nb.cpu().numpy()
        for l, (grp, ti) in enumerate(zip((0, 1, 1), (0, 2, 0))):
            hops = o[l, :, 3:].reshape(4, HOME_H, 15)
            if fields[grp] < 2:
                fi = fields[grp]
                assert n[l] == want["n_brackets"][fi, ti]
                assert same_bits(o[l, :, 0], want["elevation_deg"][fi, ti])
                assert np.array_equal(o[l, :, 1].astype(np.int64), want["status"][fi, ti])
                for c, k in enumerate(LAUNCH + RAY_KEYS):
                    assert same_bits(hops[..., c], want["ray_status" if k == "status" else k][fi, ti].astype(np.float64)), k
            else:
                assert n[l] == 0 and np.isnan(o[l, :, 0]).all() and np.all(o[l, :, 1] == -1) and np.isnan(o[l, :, 2]).all()
                assert np.isnan(hops[..., :10]).all() and np.all(hops[..., 10] == -1) and np.all(hops[..., 11:] == 0)
