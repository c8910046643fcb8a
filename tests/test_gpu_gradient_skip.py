"""GPU: fields built on the device (prhf_field_build_f64), skip distance (prhf_gradient_skip_f64) and MUF
(prhf_gradient_muf_f64) for the gradient tracers, DESIGN.md section 4.11: against the existing calls bit for bit
(find_mu_mup on array frequencies, the fan, one-ray traces), against the NumPy restatement of the rule
(tests/skip_rule.py) driven by those calls, and against fixture G23 (tools/gen_golden_gradient_skip.py: the reference's
tracers driven by the same restatement).

Inputs are G23's: the tilted (0.3) two-layer ionosphere of g18 on 121 x 201 nodes, 12 MHz O and 15 MHz X (case = 2
geometry + field), launch point (-400, 0), the bounded control set with max_step_km=2, the scan np.linspace(5, 85, 33),
elev_tol_deg=1e-3, max_iter=64.

Accuracy rule against G23: the same scan node and status, the elevation strictly between the node's neighbours, and
|skip_km - skip_km(truth)| <= 2 E_ref, E_ref the reference's own largest |skip_km(default) - skip_km(check or truth)|
over the four cases; the factor 2 is the gradient tracers' rule (the same method at the same tolerances has truncation
error of the same size but not of the same sign).  The elevation is not pinned tighter: the minimum is flat and D(e)
carries the step controller's sawtooth, which moves the reference's own elevation by 0.008 - 0.023 degrees between
control sets."""

import functools

import numpy as np
import pytest

from conftest import load_golden, same_bits
from pyrayhf_amd import _native, gradient, synth
from pyrayhf_amd.library import find_mu_mup, find_X, find_Y
import skip_rule as rule

pytestmark = pytest.mark.gpu

R_E = gradient.constants()[2]
NAME = ("cartesian", "spherical")
CASES = (("O", 12.0e6), ("X", 15.0e6))
X0, Z0 = -400.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TOL, MAX_ITER = 1e-3, 64
CTL = (dict(s_max_km=4000.0, max_step_km=2.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0),
       dict(s_max_km=4000.0, max_step_km=2.0, r_max_km=R_E + 600.0, phi_min=-1000.0 / R_E, phi_max=1000.0 / R_E))
SKIP = (gradient.skip_distance_cartesian_gradient, gradient.skip_distance_spherical_gradient)
MUF = (gradient.muf_cartesian_gradient, gradient.muf_spherical_gradient)
FAN = (gradient.trace_fan_cartesian_gradient, gradient.trace_fan_spherical_gradient)
RAYS = (gradient.trace_rays_cartesian_gradient, gradient.trace_rays_spherical_gradient)
RAY_KEYS = gradient._KEYS
HEAD = ("skip_km", "elevation_deg", "status", "scan_index", "bracket_deg", "n_evals")
GEOS = [0, 1]


def _row_key(k):
    return "ray_status" if k == "status" else k


@functools.lru_cache(maxsize=None)
def _iono(uniform=True):
    return synth.tilted_ionosphere(121, 201, 0.3, 18, uniform=uniform)


def _axes(geo, z, x):
    return (R_E + z, x / R_E) if geo else (z, x)


def _built(geo, mode, freqs, iono=None, **kw):
    z, x, den, bmag, bpsi = _iono() if iono is None else iono
    return gradient.refractive_field_device(np.asarray(freqs, dtype=np.float64), den, bmag, bpsi, z, x, mode,
                                            geometry=NAME[geo], **kw)


def _by_find_mu_mup(geo, mode, freqs, iono=None):
    """The field the issue defines: find_mu_mup on ARRAY frequencies, one call per frequency, then the records."""
    z, x, den, bmag, bpsi = _iono() if iono is None else iono
    parts = []
    with np.errstate(all="ignore"):
        for f in np.asarray(freqs, dtype=np.float64):
            fa = np.array([f])
            parts.append(find_mu_mup(find_X(den, fa), find_Y(fa, bmag), bpsi, mode))
    a0, a1 = _axes(geo, z, x)
    return gradient.RefractiveField(a0, a1, np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), geometry=NAME[geo])


def _same_field(got, want):
    assert got.geometry == want.geometry and got.R_E == want.R_E and got.same_grid(want)
    assert same_bits(got.mu, want.mu) and same_bits(got.mup, want.mup)
    assert got._rec is not None                                       # (it already holds its records)
    assert same_bits(got.records().cpu().numpy(), want.records().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _field(geo):
    """G23's two fields (12 MHz O, 15 MHz X) in one RefractiveField."""
    parts = [_built(geo, mode, [f]) for mode, f in CASES]
    return gradient.RefractiveField(parts[0].axis0, parts[0].axis1, np.concatenate([p.mu for p in parts]),
                                    np.concatenate([p.mup for p in parts]), geometry=NAME[geo])


@functools.lru_cache(maxsize=None)
def _one_field(geo, fi):
    f = _field(geo)
    return gradient.RefractiveField(f.axis0, f.axis1, f.mu[fi], f.mup[fi], geometry=f.geometry)


@functools.lru_cache(maxsize=None)
def _g23_result(geo):
    return SKIP[geo](_field(geo), X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])


class _Need(Exception):
    pass


def _rule_batched(geo, field, scan, x0, d, tol, max_iter):
    """skip_rule.skip_search for every field of `field` from (x0, Z0) on the scan ranges d (F, E), its rays traced by
    trace_rays_*_gradient: a golden-section step of all groups is one batched call (a search that needs a ray it does not
    have yet stops, the rays all searches wait for are traced together, and the searches run again)."""
    known = [dict() for _ in range(field.n_fields)]
    for _ in range(max_iter + 2):
        out, need = [], []
        for fi in range(field.n_fields):
            def ray(e, fi=fi):
                if e not in known[fi]:
                    need.append((fi, e))
                    raise _Need
                return known[fi][e]
            try:
                out.append(rule.skip_search(scan, d[fi], ray, tol, max_iter))
            except _Need:
                out.append(None)
        if not need:
            return out
        fis, es = np.array([n[0] for n in need], dtype=np.int64), np.array([n[1] for n in need])
        got = RAYS[geo](field, x0, Z0, es, fis, **CTL[geo])["ground_range_km"]
        for (fi, e), v in zip(need, got):
            known[fi][e] = float(v)
    raise AssertionError("the rule did not end")


def _check(geo, field, res, scan, x0s=(X0,), tol=TOL, max_iter=MAX_ITER):
    """Every group of `res` (F, T) is the NumPy rule's result on the fan's ground ranges, bit for bit; every row with a
    ray is the tracer's row at the returned elevation; rows without one are NaN / -1 / 0.  Returns the rule's dicts."""
    scan = np.atleast_1d(np.asarray(scan, dtype=np.float64))
    all_want = []
    for ti, x0 in enumerate(x0s):
        fan = FAN[geo](field, scan, x0, Z0, **CTL[geo])
        want = _rule_batched(geo, field, scan, x0, fan["ground_range_km"], tol, max_iter)
        all_want.append(want)
        for fi, w in enumerate(want):
            for k in HEAD:
                assert same_bits(res[k][fi, ti], w[k]), (k, fi, ti, res[k][fi, ti], w[k])
            if w["status"] >= 0:
                assert res["skip_km"][fi, ti] <= fan["ground_range_km"][fi, w["scan_index"]]
        has = res["status"][:, ti] >= 0
        if has.any():
            again = RAYS[geo](field, x0, Z0, res["elevation_deg"][has, ti], np.flatnonzero(has), **CTL[geo])
            for k in RAY_KEYS:
                assert same_bits(res[_row_key(k)][has, ti], again[k]), k
            assert np.all(res["ray_status"][has, ti] == 0)
            assert same_bits(res["ground_range_km"][has, ti], res["skip_km"][has, ti])
        for k in RAY_KEYS:
            v = res[_row_key(k)][~has, ti]
            assert np.all(v == (-1 if k == "status" else 0)) if k in gradient._INT_KEYS else np.isnan(v).all(), k
        for k in ("skip_km", "elevation_deg", "bracket_deg"):
            assert np.isnan(res[k][~has, ti]).all()
        assert np.all(res["scan_index"][~has, ti] == -1) and np.all(res["n_evals"][~has, ti] == 0)
    return all_want


# ---- part A: fields of many frequencies built on the device ------------------------------------------------------------

@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("mode", ["O", "X"])
def test_fields_are_find_mu_mup_on_array_frequencies(mode, geo, uniform):
    iono = _iono(uniform)
    rng = np.random.default_rng(23)
    for n_freq in (1, 3, 65):
        freqs = rng.uniform(3.0e6, 20.0e6, n_freq)
        _same_field(_built(geo, mode, freqs, iono), _by_find_mu_mup(geo, mode, freqs, iono))


@pytest.mark.parametrize("geo", GEOS)
def test_fields_equal_refractive_field_where_both_squares_are_exact(geo):
    z, x, den, bmag, bpsi = _iono()
    for mode in ("O", "X"):
        want = gradient.refractive_field([6.0e6, 9.0e6], den, bmag, bpsi, z, x, mode, geometry=NAME[geo])
        _same_field(_built(geo, mode, [6.0e6, 9.0e6]), want)


@pytest.mark.parametrize("mode", ["O", "X"])
def test_isotropic_decision_per_frequency(mode):
    z, x, den, bmag, bpsi = _iono()
    freqs = [4.0e6, 12.0e6, 15.0e6]
    zero = np.zeros_like(bmag)
    got = _built(0, mode, freqs, (z, x, den, zero, bpsi))
    _same_field(got, _by_find_mu_mup(0, mode, freqs, (z, x, den, zero, bpsi)))
    # the isotropic formulas know neither the mode nor the angle
    _same_field(got, _built(0, "X" if mode == "O" else "O", freqs, (z, x, den, zero, bpsi + 7.0)))
    one = zero.copy()
    one[60, 100] = 4.0e-5                                              # one magnetised node: every frequency is magnetised
    _same_field(_built(0, mode, freqs, (z, x, den, one, bpsi)), _by_find_mu_mup(0, mode, freqs, (z, x, den, one, bpsi)))
    tiny = np.full_like(bmag, 3.0e-16)                                 # g_p B / f straddles 1e-12 between 4 and 12 MHz
    assert 2.799249247e10 * 3.0e-16 / 12.0e6 < 1e-12 < 2.799249247e10 * 3.0e-16 / 4.0e6
    _same_field(_built(0, mode, freqs, (z, x, den, tiny, bpsi)), _by_find_mu_mup(0, mode, freqs, (z, x, den, tiny, bpsi)))
    nan = np.full_like(bmag, np.nan)                                   # all-NaN B counts as magnetised
    _same_field(_built(0, mode, freqs, (z, x, den, nan, bpsi)), _by_find_mu_mup(0, mode, freqs, (z, x, den, nan, bpsi)))


def test_nan_density_node_and_the_smallest_grid():
    z, x, den, bmag, bpsi = _iono()
    hole = den.copy()
    hole[40, 17] = np.nan
    got = _built(1, "O", [12.0e6, 5.0e6], (z, x, hole, bmag, bpsi))
    _same_field(got, _by_find_mu_mup(1, "O", [12.0e6, 5.0e6], (z, x, hole, bmag, bpsi)))
    assert np.isnan(got.mu[:, 40, 17]).all() and np.isfinite(got.mu[0]).sum() > 0
    z3, x3 = np.array([0.0, 250.0, 600.0]), np.array([-1000.0, 100.0, 1000.0])
    small = (z3, x3, den[::60, ::100].copy(), bmag[::60, ::100].copy(), bpsi[::60, ::100].copy())
    assert small[2].shape == (3, 3)
    for geo in GEOS:
        _same_field(_built(geo, "X", [9.0e6, 15.0e6], small), _by_find_mu_mup(geo, "X", [9.0e6, 15.0e6], small))


# ---- part B: skip distance ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo", GEOS)
def test_g23_links_against_the_rule_and_the_fixture(geo):
    g = load_golden("g23_gradient_skip.npz")
    res = _g23_result(geo)
    want = _check(geo, _field(geo), res, SCAN)[0]
    e_ref = float(g["e_ref_km"])
    for fi in range(2):
        c = 2 * geo + fi
        i = int(g["default_scan_index"][c])
        assert res["scan_index"][fi, 0] == i == want[fi]["scan_index"] and res["status"][fi, 0] == g["default_status"][c] == 0
        assert SCAN[i - 1] < res["elevation_deg"][fi, 0] < SCAN[i + 1]
        err = abs(res["skip_km"][fi, 0] - g["truth_skip_km"][c])
        print(f"case {c}: skip_km {res['skip_km'][fi, 0]!r} truth {g['truth_skip_km'][c]!r} |diff| / E_ref = {err / e_ref:.3f}; "
              f"elevation {res['elevation_deg'][fi, 0]!r} reference {g['default_elevation_deg'][c]!r}; "
              f"n_evals {res['n_evals'][fi, 0]} reference {g['default_n_evals'][c]}")
        assert err <= 2.0 * e_ref, (c, err, e_ref)
    ctx = _field(geo)._ctx()
    SKIP[geo](_field(geo), X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    groups, rays, slots, waves = ctx.gradient_skip_counters()
    print(f"geometry {geo}: counters {groups, rays, slots, waves}: lane utilisation {rays / slots:.3f}")
    assert groups == 2 and rays == res["n_evals"].sum() and waves == 1 and slots >= 64 * res["n_evals"].max()


@pytest.mark.parametrize("n_scan", [1, 2, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("geo", GEOS)
def test_scan_sizes(geo, n_scan):
    scan = np.array([30.0]) if n_scan == 1 else np.linspace(5.0, 85.0, n_scan)      # (5 and 85 degrees do not land)
    field = _one_field(geo, geo)                                       # (12 MHz O flat, 15 MHz X spherical)
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    want = _check(geo, field, res, scan)[0][0]
    assert want["status"] == (1 if n_scan == 1 else -1 if n_scan == 2 else 0 if n_scan >= 63 else want["status"])
    assert want["status"] in (-1, 0, 1)


@pytest.mark.parametrize("n_groups", [1, 65, 130])
@pytest.mark.parametrize("geo", GEOS)
def test_more_groups_than_a_wavefront_has_lanes(geo, n_groups):
    freqs = [13.0e6] if n_groups == 1 else np.linspace(11.0e6, 16.0e6, n_groups)
    field = _built(geo, "O", freqs)
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    want = _check(geo, field, res, SCAN)[0]
    groups, rays, slots, waves = field._ctx().gradient_skip_counters()
    n_refined = sum(w["status"] in (0, 2, 3) for w in want)
    assert groups == n_refined and rays == sum(w["n_evals"] for w in want) and waves == (n_refined + 63) // 64
    print(f"geometry {geo}, {n_groups} groups: {n_refined} refined, lane utilisation {rays / max(slots, 1):.3f}")
    assert n_refined >= n_groups // 2


@pytest.mark.parametrize("geo", GEOS)
def test_edge_and_empty_rows(geo):
    z, x, den, bmag, bpsi = _iono()
    # 6 MHz O, below the layer's critical frequency: D(e) falls into the rays that fail - status 1, no ray counted
    field = _built(geo, "O", [6.0e6])
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert field._ctx().gradient_skip_counters() == (0, 0, 0, 0)
    want = _check(geo, field, res, SCAN)[0][0]
    assert res["status"][0, 0] == 1 == want["status"] and res["n_evals"][0, 0] == 0 and np.isnan(res["bracket_deg"][0, 0])
    fan = FAN[geo](field, SCAN, X0, Z0, **CTL[geo])
    assert same_bits(res["skip_km"][0, 0], fan["ground_range_km"][0, res["scan_index"][0, 0]])
    # a 3 x 3 vacuum: no ray comes back - status -1, a NaN row
    z3, x3 = np.array([0.0, 300.0, 600.0]), np.array([-1000.0, 0.0, 1000.0])
    a0, a1 = _axes(geo, z3, x3)
    vacuum = gradient.RefractiveField(a0, a1, np.ones((3, 3)), np.ones((3, 3)), geometry=NAME[geo])
    res = SKIP[geo](vacuum, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert res["status"][0, 0] == -1 and np.isnan(res["skip_km"][0, 0])
    _check(geo, vacuum, res, SCAN)
    # a scan node whose neighbour leaves through the top of the domain: status 1
    field = _one_field(geo, 0)
    fan = FAN[geo](field, SCAN, X0, Z0, **CTL[geo])
    i = int(_g23_result(geo)["scan_index"][0, 0])
    domain = i + 1 + np.flatnonzero(fan["status"][0, i + 1:] == 1)
    assert domain.size, fan["status"][0]
    scan = np.array([SCAN[i - 2], SCAN[i], SCAN[domain[0]]])
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert res["status"][0, 0] == 1 and res["scan_index"][0, 0] == 1 and res["n_evals"][0, 0] == 0
    assert same_bits(res["skip_km"][0, 0], fan["ground_range_km"][0, i])
    _check(geo, field, res, scan)


@pytest.mark.parametrize("geo", GEOS)
def test_iteration_limits(geo):
    field = _field(geo)
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=1, **CTL[geo])
    assert np.all(res["status"] == 3) and np.all(res["n_evals"] == 1)
    _check(geo, field, res, SCAN, max_iter=1)
    res = SKIP[geo](field, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=0.0, max_iter=128, **CTL[geo])
    assert np.isin(res["status"], (0, 3)).all()
    _check(geo, field, res, SCAN, tol=0.0, max_iter=128)
    print(f"geometry {geo}: elev_tol_deg=0: statuses {res['status'].ravel().tolist()}, n_evals {res['n_evals'].ravel().tolist()}, "
          f"brackets {res['bracket_deg'].ravel().tolist()}")


@pytest.mark.parametrize("geo", GEOS)
def test_same_bits_again_and_two_transmitters_equal_two_calls(geo):
    full = _g23_result(geo)
    again = SKIP[geo](_field(geo), X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    for k in full:
        assert same_bits(full[k], again[k]), k
    x0s = np.array([X0, -300.0])
    both = SKIP[geo](_field(geo), x0s, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert both["skip_km"].shape == (2, 2)
    for ti, x0 in enumerate(x0s):
        alone = full if ti == 0 else SKIP[geo](_field(geo), x0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL,
                                               max_iter=MAX_ITER, **CTL[geo])
        for k in full:
            assert same_bits(both[k][:, ti], alone[k][:, 0]), (k, ti)
    for fi in range(2):
        alone = SKIP[geo](_one_field(geo, fi), X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
        for k in full:
            assert same_bits(full[k][fi], alone[k][0]), (k, fi)


@pytest.mark.parametrize("geo", GEOS)
def test_device_resident_arrays(geo):
    """PRHF_FLAG_DEVICE_PTRS: torch tensors through the binding; rows are bit for bit the host-buffer call's; a
    group_field out of range gives that group a NaN row and PRHF_EINVAL at the synchronisation, the other groups their
    results."""
    import torch
    want = _g23_result(geo)
    field = _field(geo)
    ctx = field._ctx()
    c = CTL[geo]
    ctl = ((c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["r_max_km"], c["phi_min"], c["phi_max"], 50) if geo else
           (c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["z_max_km"], c["x_min_km"], c["x_max_km"], 50))
    gx = torch.full((3,), X0, dtype=torch.float64, device="cuda")
    gz = torch.full((3,), Z0, dtype=torch.float64, device="cuda")
    scan = torch.as_tensor(SCAN, device="cuda")
    for fields, want_rc in (([1, 0, 1], _native.OK), ([0, 2, 1], _native.EINVAL), ([-1, 1, 0], _native.EINVAL)):
        gf = torch.tensor(fields, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, 18), dtype=torch.float64, device="cuda")
        rc = ctx.gradient_skip(geo, field.records().data_ptr(), 2, field.axis0.size, field.axis1.size,
                               field.axis0.ctypes.data, field.axis1.ctypes.data, gf.data_ptr(), gx.data_ptr(), gz.data_ptr(), 3,
                               scan.data_ptr(), SCAN.size, R_E if geo else 0.0, ctl, field.fills, TOL, MAX_ITER,
                               out.data_ptr(), _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (fields, rc, _native.last_error())
        o = out.cpu().numpy()
        for g, fi in enumerate(fields):
            if 0 <= fi < 2:
                for j, k in enumerate(HEAD):
                    assert same_bits(o[g, j], np.float64(want[k][fi, 0])), (k, g)
                for j, k in enumerate(RAY_KEYS):
                    assert same_bits(o[g, 6 + j], np.float64(want[_row_key(k)][fi, 0])), (k, g)
            else:
                assert o[g, 2] == -1 and o[g, 3] == -1 and o[g, 5] == 0 and np.isnan(o[g, [0, 1, 4]]).all()
                assert np.isnan(o[g, 6:]).all()


# ---- part C: MUF -------------------------------------------------------------------------------------------------------

F_LO, F_HI = 12.0e6, 15.0e6
MUF_SCAN = np.linspace(25.0, 65.0, 9)


@functools.lru_cache(maxsize=None)
def _skip_at(geo, mode, f, scan_key, tol):
    """The skip call's result (the dict, shapes (1, 1)) on the device-built field at f."""
    scan = SCAN if scan_key == "g23" else MUF_SCAN
    return SKIP[geo](_built(geo, mode, [f]), X0, Z0, scan_elevation_deg=scan, elev_tol_deg=tol, max_iter=MAX_ITER, **CTL[geo])


def _s(geo, mode, scan_key, tol):
    def s(f):
        r = _skip_at(geo, mode, float(f), scan_key, tol)
        return rule.INF if r["status"][0, 0] == -1 else float(r["skip_km"][0, 0])
    return s


def _muf(geo, t, mode="O", f_lo=F_LO, f_hi=F_HI, scan_key="g23", tol=TOL, **kw):
    z, x, den, bmag, bpsi = _iono()
    return MUF[geo](t, den, bmag, bpsi, z, x, mode, f_lo, f_hi, X0, Z0, max_iter=MAX_ITER, elev_tol_deg=tol,
                    scan_elevation_deg=SCAN if scan_key == "g23" else MUF_SCAN, **CTL[geo], **kw)


def _check_muf(geo, res, targets, n_bisect, mode="O", f_lo=F_LO, f_hi=F_HI, scan_key="g23", tol=TOL):
    """Every link is skip_rule.muf_search driven by the two GPU calls, bit for bit; status 0 keeps the invariant; the row
    at muf_hz is the skip call's row on the device-built field at muf_hz."""
    s = _s(geo, mode, scan_key, tol)
    targets = np.atleast_1d(targets)
    assert res["muf_hz"].shape == targets.shape
    for l, t in enumerate(targets):
        w = rule.muf_search(s, float(t), f_lo, f_hi, n_bisect)
        assert res["status"][l] == w["status"], (l, t, res["status"][l], w["status"])
        assert same_bits(res["muf_hz"][l], w["muf_hz"]) and same_bits(res["f_above_hz"][l], w["f_above_hz"]), (l, t)
        if w["status"] == 0:
            assert s(res["muf_hz"][l]) <= t < s(res["f_above_hz"][l])
        if w["status"] in (0, 1):
            row = _skip_at(geo, mode, float(res["muf_hz"][l]), scan_key, tol)
            for k in row:
                assert same_bits(res["skip_status" if k == "status" else k][l], row[k][0, 0]), (k, l)
        else:
            for k in ("skip_km", "elevation_deg", "bracket_deg", "ground_range_km", "group_path_km"):
                assert np.isnan(res[k][l]), k
            assert res["skip_status"][l] == -1 and res["ray_status"][l] == -1 and res["n_evals"][l] == 0


@pytest.mark.parametrize("n_bisect", [1, 6])
@pytest.mark.parametrize("geo", GEOS)
def test_muf_is_the_rule_on_the_gpu_calls_and_the_four_statuses(geo, n_bisect):
    s = _s(geo, "O", "g23", TOL)
    s_lo, s_hi = s(F_LO), s(F_HI)
    assert np.isfinite(s_lo) and np.isfinite(s_hi) and s_lo < 300.0 < s_hi, (s_lo, s_hi)
    targets = np.array([np.nan, s_lo - 50.0, s_hi + 50.0, 300.0, 0.5 * (s_lo + s_hi)])
    res = _muf(geo, targets, n_bisect=n_bisect)
    assert res["status"].tolist() == [-1, 2, 1, 0, 0]
    _check_muf(geo, res, targets, n_bisect)
    again = _muf(geo, targets, n_bisect=n_bisect)
    for k in res:
        assert same_bits(res[k], again[k]), k                          # identical bits on a second call
    groups, rays, slots, waves = _native.host_context(None).gradient_skip_counters()
    print(f"geometry {geo}, n_bisect {n_bisect}: S(f_lo) {s_lo!r} S(f_hi) {s_hi!r}; muf {res['muf_hz'][3]!r}; "
          f"counters {groups, rays, slots, waves}: lane utilisation {rays / max(slots, 1):.3f}")


@pytest.mark.parametrize("geo", GEOS)
def test_muf_bisection_outlasts_the_doubles(geo):
    res = _muf(geo, np.array([300.0]), n_bisect=64, scan_key="muf", tol=0.05)
    _check_muf(geo, res, [300.0], 64, scan_key="muf", tol=0.05)
    assert res["status"][0] == 0 and np.nextafter(res["muf_hz"][0], np.inf) == res["f_above_hz"][0]


@pytest.mark.parametrize("geo", GEOS)
def test_muf_against_the_fixture(geo):
    """With n_bisect = muf_safe_trips the bracket is the reference's after that many trips, bit for bit: the midpoints
    are deterministic and those decisions are clear by ten times the reference's own error."""
    g = load_golden("g23_gradient_skip.npz")
    n = int(g["muf_safe_trips"][geo])
    assert 4 <= n <= 10
    f_lo, f_hi = float(g["muf_f_lo_hz"][geo]), float(g["muf_f_hi_hz"][geo])
    res = _muf(geo, np.array([float(g["muf_target_km"])]), f_lo=f_lo, f_hi=f_hi, n_bisect=n)
    want_lo = g["muf_trip_lo_hz"][geo, n] if n < 10 else g["muf_hz"][geo]
    want_hi = g["muf_trip_hi_hz"][geo, n] if n < 10 else g["muf_f_above_hz"][geo]
    print(f"geometry {geo}: {n} safe trips: bracket {res['muf_hz'][0]!r} .. {res['f_above_hz'][0]!r}; the reference's final "
          f"{g['muf_hz'][geo]!r} .. {g['muf_f_above_hz'][geo]!r}")
    assert res["status"][0] == 0 and res["muf_hz"][0] == want_lo and res["f_above_hz"][0] == want_hi


@pytest.mark.parametrize("geo", GEOS)
def test_muf_many_links_slabs_and_x_mode(geo):
    s = _s(geo, "O", "g23", TOL)
    targets = np.linspace(s(F_LO) - 5.0, s(F_HI) + 5.0, 65)
    res = _muf(geo, targets, n_bisect=3)
    _check_muf(geo, res, targets, 3)
    assert set(res["status"].tolist()) == {0, 1, 2}
    one = _muf(geo, targets[31:32], n_bisect=3)
    for k in res:
        assert same_bits(one[k][0], res[k][31]), k                     # 1 link
    slabs = _muf(geo, targets[28:33], n_bisect=3, _slab_links=2)
    for k in res:
        assert same_bits(slabs[k], res[k][28:33]), k                   # forced slabs of 2 equal one slab
    sx = _s(geo, "X", "g23", TOL)
    tx = np.array([0.5 * (sx(F_LO) + sx(F_HI))])
    assert np.isfinite(tx[0])
    rx = _muf(geo, tx, mode="X", n_bisect=4)
    _check_muf(geo, rx, tx, 4, mode="X")
    assert rx["status"][0] == 0
