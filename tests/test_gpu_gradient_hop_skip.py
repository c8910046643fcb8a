"""GPU: multi-hop skip distance (prhf_gradient_hop_skip_f64) and MUF (prhf_gradient_hop_muf_f64) for the gradient
tracers, DESIGN.md section 4.13: against the NumPy restatement of the rule (tests/skip_rule.py) driven by the hop fan and
by one trace_hops_*_gradient call per trial chain, bit for bit - both sides run the same device chain, so the arctangent
of section 4.12 does not come between them -, against trace_hops_*_gradient on every hop row, against the one-hop calls
at H = 1, and (Cartesian) against fixture G25 (tools/gen_golden_gradient_hop_skip.py: the reference's tracer chained on
the CPU and driven by the same restatement).

Inputs are G25's: G24's tilted (0.3) ionosphere on 121 x 401 nodes, 12 MHz O and 15 MHz X, launch point (-1800, 0), the
bounded control set with max_step_km=2, the scan np.linspace(5, 85, 33), elev_tol_deg=1e-3, max_iter=64, H = 2 and 3.

Accuracy rule against G25 (Cartesian; G25 is Cartesian only, as G24 is): the same scan node and status, the elevation
strictly between the node's neighbours, and |skip_km - skip_km(truth)| <= 2 E_ref, E_ref read from the fixture: the
reference's own largest |skip_km(default) - skip_km(truth)| over the four cases; the factor 2 is the gradient tracers'
rule (the same method at the same tolerances has truncation error of the same size but not of the same sign).  The
measured ratios are recorded in profiles/gradient_hop_skip_accuracy.md."""

import functools

import numpy as np
import pytest

from conftest import load_golden, same_bits
from pyrayhf_amd import _native, gradient, synth
import skip_rule as rule

pytestmark = pytest.mark.gpu

R_E = gradient.constants()[2]
NAME = ("cartesian", "spherical")
CASES = (("O", 12.0e6), ("X", 15.0e6))
X0, Z0 = -1800.0, 0.0
SCAN = np.linspace(5.0, 85.0, 33)
TOL, MAX_ITER = 1e-3, 64
X_LIM = 2000.0


def _ctl(geo, x_max=X_LIM, x_min=-X_LIM, **kw):
    c = (dict(s_max_km=4000.0, max_step_km=2.0, r_max_km=R_E + 600.0, phi_min=x_min / R_E, phi_max=x_max / R_E) if geo else
         dict(s_max_km=4000.0, max_step_km=2.0, z_max_km=600.0, x_min_km=x_min, x_max_km=x_max))
    c.update(kw)
    return c


CTL = (_ctl(0), _ctl(1))
SKIP = (gradient.skip_distance_hops_cartesian_gradient, gradient.skip_distance_hops_spherical_gradient)
SKIP1 = (gradient.skip_distance_cartesian_gradient, gradient.skip_distance_spherical_gradient)
MUF = (gradient.muf_hops_cartesian_gradient, gradient.muf_hops_spherical_gradient)
MUF1 = (gradient.muf_cartesian_gradient, gradient.muf_spherical_gradient)
FAN = (gradient.trace_hop_fan_cartesian_gradient, gradient.trace_hop_fan_spherical_gradient)
HOPS = (gradient.trace_hops_cartesian_gradient, gradient.trace_hops_spherical_gradient)
HEAD = ("skip_km", "elevation_deg", "status", "scan_index", "bracket_deg", "n_evals")
HOP_KEYS = gradient._HOP_LAUNCH_KEYS + tuple("ray_status" if k == "status" else k for k in gradient._KEYS)
TOTALS = ("n_landed", "total_group_path_km", "total_group_delay_sec", "total_ground_range_km")
GEOS = [0, 1]
N_HOPS = [2, 3]


@functools.lru_cache(maxsize=None)
def _iono():
    return synth.tilted_ionosphere(121, 401, 0.3, 24, x_half_km=2000)


def _built(geo, mode, freqs):
    z, x, den, bmag, bpsi = _iono()
    return gradient.refractive_field_device(np.asarray(freqs, dtype=np.float64), den, bmag, bpsi, z, x, mode,
                                            geometry=NAME[geo])


@functools.lru_cache(maxsize=None)
def _field(geo):
    """G25's two fields (12 MHz O, 15 MHz X) in one RefractiveField."""
    parts = [_built(geo, mode, [f]) for mode, f in CASES]
    return gradient.RefractiveField(parts[0].axis0, parts[0].axis1, np.concatenate([p.mu for p in parts]),
                                    np.concatenate([p.mup for p in parts]), geometry=NAME[geo])


@functools.lru_cache(maxsize=None)
def _one_field(geo, fi):
    f = _field(geo)
    return gradient.RefractiveField(f.axis0, f.axis1, f.mu[fi], f.mup[fi], geometry=f.geometry)


@functools.lru_cache(maxsize=None)
def _low_field(geo):
    """6 MHz O, below the layer's critical frequency: every ray comes back."""
    return _built(geo, "O", [6.0e6])


@functools.lru_cache(maxsize=None)
def _g25_result(geo, n_hops):
    return SKIP[geo](_field(geo), n_hops, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])


class _Need(Exception):
    pass


def _rule_batched(geo, field, n_hops, scan, x0, z0, d, tol, max_iter, ctl):
    """skip_rule.skip_search for every field of `field` from (x0, z0) on the scan ranges d (F, E), its trial chains traced
    by trace_hops_*_gradient: a golden-section step of all groups is one batched call (a search that needs a chain it
    does not have yet stops, the chains all searches wait for are traced together, and the searches run again)."""
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
        got = HOPS[geo](field, x0, z0, es, n_hops, fis, **ctl)["total_ground_range_km"]
        for (fi, e), v in zip(need, got):
            known[fi][e] = float(v)
    raise AssertionError("the rule did not end")


def _check(geo, field, n_hops, res, scan, x0s=(X0,), z0=Z0, tol=TOL, max_iter=MAX_ITER, ctl=None):
    """Every group of `res` (F, T) is the NumPy rule's result on the hop fan's total ground ranges, bit for bit; every
    row with a chain is trace_hops_*_gradient's at the returned elevation on every key; rows without one are unused as
    that call writes them.  Returns the rule's dicts and the fans."""
    ctl = CTL[geo] if ctl is None else ctl
    scan = np.atleast_1d(np.asarray(scan, dtype=np.float64))
    all_want, fans = [], []
    for ti, x0 in enumerate(x0s):
        fan = FAN[geo](field, scan, n_hops, x0, z0, **ctl)
        d = fan["total_ground_range_km"]
        want = _rule_batched(geo, field, n_hops, scan, x0, z0, d, tol, max_iter, ctl)
        all_want.append(want)
        fans.append(fan)
        for fi, w in enumerate(want):
            for k in HEAD:
                assert same_bits(res[k][fi, ti], w[k]), (k, fi, ti, res[k][fi, ti], w[k])
            if w["status"] >= 0:
                assert res["skip_km"][fi, ti] <= d[fi, w["scan_index"]]
        has = res["status"][:, ti] >= 0
        if has.any():
            again = HOPS[geo](field, x0, z0, res["elevation_deg"][has, ti], n_hops, np.flatnonzero(has), **ctl)
            for k in HOP_KEYS + TOTALS:
                assert same_bits(res[k][has, ti], again["status" if k == "ray_status" else k]), k
            assert np.all(res["ray_status"][has, ti] == 0) and np.all(res["n_landed"][has, ti] == n_hops)
            assert same_bits(res["total_ground_range_km"][has, ti], res["skip_km"][has, ti])
            assert same_bits(res["ground_range_km"][has, ti, n_hops - 1], res["skip_km"][has, ti])
        none = ~has
        for k in HOP_KEYS:
            v = res[k][none, ti]
            want_v = -1 if k == "ray_status" else 0
            assert np.all(v == want_v) if k in ("ray_status", "n_nodes", "n_rhs", "n_rejected") else np.isnan(v).all(), k
        for k in ("skip_km", "elevation_deg", "bracket_deg", "total_ground_range_km"):
            assert np.isnan(res[k][none, ti]).all()
        assert np.all(res["scan_index"][none, ti] == -1) and np.all(res["n_evals"][none, ti] == 0)
        assert np.all(res["n_landed"][none, ti] == 0)
    return all_want, fans


# ---- part A: skip distance ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_hops", N_HOPS)
@pytest.mark.parametrize("geo", GEOS)
def test_g25_cases_against_the_rule_and_the_fixture(geo, n_hops):
    res = _g25_result(geo, n_hops)
    assert res["skip_km"].shape == (2, 1) and res["ground_range_km"].shape == (2, 1, n_hops)
    want = _check(geo, _field(geo), n_hops, res, SCAN)[0][0]
    assert [w["status"] for w in want] == [0, 0]
    ctx = _field(geo)._ctx()
    SKIP[geo](_field(geo), n_hops, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    groups, rays, slots, waves, hop_rays = ctx.gradient_hop_skip_counters()
    print(f"geometry {geo} H {n_hops}: counters {groups, rays, slots, waves, hop_rays}: lane utilisation {rays / slots:.3f}")
    assert (groups, rays, slots, waves) == ctx.gradient_skip_counters()
    assert groups == 2 and rays == res["n_evals"].sum() and waves == 1 and slots >= 64 * res["n_evals"].max()
    assert hop_rays == n_hops * rays                                      # (status 0: every trial chain landed)
    if geo:
        return
    g = load_golden("g25_gradient_hop_skip.npz")
    e_ref = float(g["e_ref_km"])
    for fi in range(2):
        c = 2 * fi + n_hops - 2
        i = int(g["default_scan_index"][c])
        assert res["scan_index"][fi, 0] == i and res["status"][fi, 0] == g["default_status"][c] == 0
        assert SCAN[i - 1] < res["elevation_deg"][fi, 0] < SCAN[i + 1]
        err = abs(res["skip_km"][fi, 0] - g["truth_skip_km"][c])
        print(f"case {c}: skip_km {res['skip_km'][fi, 0]!r} truth {g['truth_skip_km'][c]!r} |diff| / E_ref = {err / e_ref:.3f} "
              f"(E_ref {e_ref!r}); elevation {res['elevation_deg'][fi, 0]!r} reference {g['default_elevation_deg'][c]!r}; "
              f"n_evals {res['n_evals'][fi, 0]} reference {g['default_n_evals'][c]}")
        assert err <= 2.0 * e_ref, (c, err, e_ref)


@pytest.mark.parametrize("geo", GEOS)
def test_one_hop_equals_the_one_hop_call(geo):
    one = SKIP1[geo](_field(geo), X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    res = SKIP[geo](_field(geo), 1, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert (one["status"] >= 0).all()
    for k in one:
        got = res[k][..., 0] if res[k].ndim == 3 else res[k]
        assert same_bits(got, one[k]), k
    assert same_bits(res["launch_x_km"][..., 0], np.full((2, 1), X0)) and same_bits(res["launch_elevation_deg"][..., 0], one["elevation_deg"])
    _check(geo, _field(geo), 1, res, SCAN)


@pytest.mark.parametrize("n_scan", [1, 2, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("geo", GEOS)
def test_scan_sizes(geo, n_scan):
    scan = np.array([30.0]) if n_scan == 1 else np.linspace(5.0, 85.0, n_scan)      # (5 and 85 degrees do not land)
    field = _one_field(geo, geo)                                       # (12 MHz O flat, 15 MHz X spherical)
    res = SKIP[geo](field, 2, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    want = _check(geo, field, 2, res, scan)[0][0][0]
    assert want["status"] == (1 if n_scan == 1 else -1 if n_scan == 2 else want["status"])
    print(f"geometry {geo}, {n_scan} nodes: status {want['status']}, node {want['scan_index']}, n_evals {want['n_evals']}")


@pytest.mark.parametrize("n_groups", [1, 65, 130])
@pytest.mark.parametrize("geo", GEOS)
def test_more_groups_than_a_wavefront_has_lanes(geo, n_groups):
    freqs = [13.0e6] if n_groups == 1 else np.linspace(11.0e6, 16.0e6, n_groups)
    field = _built(geo, "O", freqs)
    res = SKIP[geo](field, 2, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    groups, rays, slots, waves, hop_rays = field._ctx().gradient_hop_skip_counters()
    want = _check(geo, field, 2, res, SCAN)[0][0]
    n_refined = sum(w["status"] in (0, 2, 3) for w in want)
    assert groups == n_refined and rays == sum(w["n_evals"] for w in want) and waves == (n_refined + 63) // 64
    failed = sum(w["status"] == 2 for w in want)                         # (a search ends with its first chain that fails)
    assert hop_rays == 2 * (rays - failed)
    print(f"geometry {geo}, {n_groups} groups: {n_refined} refined, lane utilisation {rays / max(slots, 1):.3f}, "
          f"statuses {sorted(set(w['status'] for w in want))}")
    assert n_refined >= 1


@pytest.mark.parametrize("geo", GEOS)
def test_hop_one_lands_nowhere(geo):
    """Hop 0 lands at some scan nodes, hop 1 at none: status -1, a NaN row, the hop rows unused."""
    field = _low_field(geo)
    scan = np.linspace(20.0, 40.0, 9)
    first = FAN[geo](field, scan, 1, X0, Z0, **CTL[geo])["ground_range_km"][0, :, 0]
    assert np.isfinite(first).all(), first
    ctl = _ctl(geo, x_max=float(first.min()) + 50.0)                  # (a second hop is some hundred km long)
    fan = FAN[geo](field, scan, 2, X0, Z0, **ctl)
    assert (fan["n_landed"][0] == 1).any() and (fan["n_landed"][0] < 2).all(), fan["n_landed"]
    res = SKIP[geo](field, 2, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **ctl)
    assert field._ctx().gradient_hop_skip_counters() == (0, 0, 0, 0, 0)
    assert res["status"][0, 0] == -1 and np.isnan(res["skip_km"][0, 0]) and (res["ray_status"][0, 0] == -1).all()
    _check(geo, field, 2, res, scan, ctl=ctl)
    # the same rays with one hop: a result
    one = SKIP[geo](field, 1, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **ctl)
    assert one["status"][0, 0] >= 0


@pytest.mark.parametrize("geo", GEOS)
def test_minimum_beside_a_chain_that_fails_on_a_later_hop(geo):
    """Status 1, no chain counted: the neighbour's hop 0 lands, its hop 1 does not - D is not finite all the same."""
    field = _one_field(geo, 0)
    fan = FAN[geo](field, SCAN, 2, X0, Z0, **CTL[geo])
    d, landed = fan["total_ground_range_km"][0], fan["n_landed"][0]
    pick = None
    for j in np.flatnonzero(landed == 1)[::-1]:
        for k in range(int(j) + 1, SCAN.size - 1):                        # (j, k, k + 1): the minimum in the middle
            if pick is None and np.isfinite(d[k]) and np.isfinite(d[k + 1]) and d[k] < d[k + 1]:
                pick = (int(j), k)
    assert pick is not None, (landed, d)
    j, k = pick
    scan = np.array([SCAN[j], SCAN[k], SCAN[k + 1]])
    res = SKIP[geo](field, 2, X0, Z0, scan_elevation_deg=scan, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert field._ctx().gradient_hop_skip_counters() == (0, 0, 0, 0, 0)
    assert res["status"][0, 0] == 1 and res["scan_index"][0, 0] == 1 and res["n_evals"][0, 0] == 0
    assert np.isnan(res["bracket_deg"][0, 0]) and same_bits(res["skip_km"][0, 0], d[k])
    _check(geo, field, 2, res, scan)


@pytest.mark.parametrize("n_hops", N_HOPS)
@pytest.mark.parametrize("geo", GEOS)
def test_iteration_limits(geo, n_hops):
    field = _field(geo)
    res = SKIP[geo](field, n_hops, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=1, **CTL[geo])
    assert np.all(res["status"] == 3) and np.all(res["n_evals"] == 1)
    _check(geo, field, n_hops, res, SCAN, max_iter=1)
    res = SKIP[geo](field, n_hops, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=0.0, max_iter=128, **CTL[geo])
    assert np.isin(res["status"], (0, 2, 3)).all()
    _check(geo, field, n_hops, res, SCAN, tol=0.0, max_iter=128)
    print(f"geometry {geo} H {n_hops}: elev_tol_deg=0: statuses {res['status'].ravel().tolist()}, n_evals "
          f"{res['n_evals'].ravel().tolist()}, brackets {res['bracket_deg'].ravel().tolist()}")


@pytest.mark.parametrize("geo", GEOS)
def test_raised_ground(geo):
    """z_ground_km = 0.3: the hops after the first launch from it."""
    ctl = dict(CTL[geo], z_ground_km=0.3)
    field = _field(geo)
    res = SKIP[geo](field, 3, X0, 0.3, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **ctl)
    assert (res["status"] >= 0).all() and np.all(res["launch_z_km"] == 0.3)
    _check(geo, field, 3, res, SCAN, z0=0.3, ctl=ctl)
    flat = _g25_result(geo, 3)
    assert not same_bits(res["skip_km"], flat["skip_km"])


@pytest.mark.parametrize("geo", GEOS)
def test_same_bits_again_and_two_transmitters_equal_two_calls(geo):
    full = _g25_result(geo, 2)
    again = SKIP[geo](_field(geo), 2, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    for k in full:
        assert same_bits(full[k], again[k]), k
    x0s = np.array([X0, -1700.0])
    both = SKIP[geo](_field(geo), 2, x0s, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
    assert both["skip_km"].shape == (2, 2) and both["ground_range_km"].shape == (2, 2, 2)
    for ti, x0 in enumerate(x0s):
        alone = full if ti == 0 else SKIP[geo](_field(geo), 2, x0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL,
                                               max_iter=MAX_ITER, **CTL[geo])
        for k in full:
            assert same_bits(both[k][:, ti], alone[k][:, 0]), (k, ti)
    for fi in range(2):
        alone = SKIP[geo](_one_field(geo, fi), 2, X0, Z0, scan_elevation_deg=SCAN, elev_tol_deg=TOL, max_iter=MAX_ITER, **CTL[geo])
        for k in full:
            assert same_bits(full[k][fi], alone[k][0]), (k, fi)


@pytest.mark.parametrize("geo", GEOS)
def test_device_resident_arrays(geo):
    """PRHF_FLAG_DEVICE_PTRS: torch tensors through the binding; rows are bit for bit the host-buffer call's; a
    group_field out of range gives that group a NaN row and PRHF_EINVAL at the synchronisation, the other groups their
    results."""
    import torch
    n_hops = 2
    want = _g25_result(geo, n_hops)
    field = _field(geo)
    ctx = field._ctx()
    c = CTL[geo]
    ctl = ((c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["r_max_km"], c["phi_min"], c["phi_max"], 50) if geo else
           (c["s_max_km"], 1e-7, 1e-9, c["max_step_km"], 0.0, c["z_max_km"], c["x_min_km"], c["x_max_km"], 50))
    gx = torch.full((3,), X0, dtype=torch.float64, device="cuda")
    gz = torch.full((3,), Z0, dtype=torch.float64, device="cuda")
    scan = torch.as_tensor(SCAN, device="cuda")
    width = 6 + 15 * n_hops
    for fields, want_rc in (([1, 0, 1], _native.OK), ([0, 2, 1], _native.EINVAL), ([-1, 1, 0], _native.EINVAL)):
        gf = torch.tensor(fields, dtype=torch.int64, device="cuda")
        out = torch.zeros((3, width), dtype=torch.float64, device="cuda")
        rc = ctx.gradient_hop_skip(geo, field.records().data_ptr(), 2, field.axis0.size, field.axis1.size,
                                   field.axis0.ctypes.data, field.axis1.ctypes.data, gf.data_ptr(), gx.data_ptr(),
                                   gz.data_ptr(), 3, scan.data_ptr(), SCAN.size, R_E if geo else 0.0, ctl, field.fills, TOL,
                                   MAX_ITER, n_hops, out.data_ptr(), _native.FLAG_DEVICE_PTRS)
        assert rc == want_rc, (fields, rc, _native.last_error())
        o = out.cpu().numpy()
        for g, fi in enumerate(fields):
            if 0 <= fi < 2:
                for j, k in enumerate(HEAD):
                    assert same_bits(o[g, j], np.float64(want[k][fi, 0])), (k, g)
                rows = o[g, 6:].reshape(n_hops, 15)
                for j, k in enumerate(HOP_KEYS):
                    assert same_bits(rows[:, j], want[k][fi, 0].astype(np.float64)), (k, g)
            else:
                assert o[g, 2] == -1 and o[g, 3] == -1 and o[g, 5] == 0 and np.isnan(o[g, [0, 1, 4]]).all()
                rows = o[g, 6:].reshape(n_hops, 15)
                assert np.isnan(rows[:, :10]).all() and np.all(rows[:, 10] == -1) and np.all(rows[:, 11:] == 0)


# ---- part B: MUF -------------------------------------------------------------------------------------------------------

F_LO, F_HI = 12.0e6, 15.0e6


@functools.lru_cache(maxsize=None)
def _skip_at(geo, mode, n_hops, f, x0=X0, scan_key="fwd"):
    """The hop-skip call's result (the dict, shapes (1, 1)) on the device-built field at f."""
    return SKIP[geo](_built(geo, mode, [f]), n_hops, x0, Z0, scan_elevation_deg=_scan(scan_key), elev_tol_deg=TOL,
                     max_iter=MAX_ITER, **CTL[geo])


def _scan(scan_key):
    # "back": 120 .. 160 degrees, the rays that look behind the transmitter
    return SCAN if scan_key == "fwd" else np.linspace(120.0, 160.0, 17)


def _s(geo, mode, n_hops, x0=X0, scan_key="fwd"):
    def s(f):
        r = _skip_at(geo, mode, n_hops, float(f), x0, scan_key)
        return rule.INF if r["status"][0, 0] == -1 else float(r["skip_km"][0, 0])
    return s


def _muf(geo, t, n_hops, mode="O", f_lo=F_LO, f_hi=F_HI, x0=X0, scan_key="fwd", **kw):
    z, x, den, bmag, bpsi = _iono()
    return MUF[geo](t, n_hops, den, bmag, bpsi, z, x, mode, f_lo, f_hi, x0, Z0, max_iter=MAX_ITER, elev_tol_deg=TOL,
                    scan_elevation_deg=_scan(scan_key), **CTL[geo], **kw)


def _check_muf(geo, res, targets, n_hops, n_bisect, mode="O", f_lo=F_LO, f_hi=F_HI, x0=X0, scan_key="fwd"):
    """Every link is skip_rule.muf_search driven by the two GPU calls, bit for bit; status 0 keeps the invariant; the row
    at muf_hz is the hop-skip call's row on the device-built field at muf_hz."""
    s = _s(geo, mode, n_hops, x0, scan_key)
    targets = np.atleast_1d(targets)
    assert res["muf_hz"].shape == targets.shape and res["ground_range_km"].shape == targets.shape + (n_hops,)
    for l, t in enumerate(targets):
        w = rule.muf_search(s, float(t), f_lo, f_hi, n_bisect)
        assert res["status"][l] == w["status"], (l, t, res["status"][l], w["status"])
        assert same_bits(res["muf_hz"][l], w["muf_hz"]) and same_bits(res["f_above_hz"][l], w["f_above_hz"]), (l, t)
        if w["status"] == 0:
            assert s(res["muf_hz"][l]) <= t < s(res["f_above_hz"][l])
        if w["status"] in (0, 1):
            row = _skip_at(geo, mode, n_hops, float(res["muf_hz"][l]), x0, scan_key)
            for k in row:
                assert same_bits(res["skip_status" if k == "status" else k][l], row[k][0, 0]), (k, l)
        else:
            for k in ("skip_km", "elevation_deg", "bracket_deg", "total_ground_range_km"):
                assert np.isnan(res[k][l]), k
            assert np.isnan(res["ground_range_km"][l]).all() and (res["ray_status"][l] == -1).all()
            assert res["skip_status"][l] == -1 and res["n_evals"][l] == 0 and res["n_landed"][l] == 0


@pytest.mark.parametrize("n_bisect", [1, 6])
@pytest.mark.parametrize("geo", GEOS)
def test_muf_is_the_rule_on_the_gpu_calls_and_the_four_statuses(geo, n_bisect):
    s = _s(geo, "O", 2)
    s_lo, s_hi = s(F_LO), s(F_HI)
    assert np.isfinite(s_lo) and np.isfinite(s_hi) and s_lo < s_hi, (s_lo, s_hi)
    targets = np.array([np.nan, s_lo - 50.0, s_hi + 50.0, 0.25 * s_lo + 0.75 * s_hi, 0.5 * (s_lo + s_hi)])
    res = _muf(geo, targets, 2, n_bisect=n_bisect)
    assert res["status"].tolist() == [-1, 2, 1, 0, 0]
    _check_muf(geo, res, targets, 2, n_bisect)
    again = _muf(geo, targets, 2, n_bisect=n_bisect)
    for k in res:
        assert same_bits(res[k], again[k]), k                          # identical bits on a second call
    groups, rays, slots, waves, hop_rays = _native.host_context(None).gradient_hop_skip_counters()
    print(f"geometry {geo}, n_bisect {n_bisect}: S(f_lo) {s_lo!r} S(f_hi) {s_hi!r}; muf {res['muf_hz'][3]!r}; "
          f"counters {groups, rays, slots, waves, hop_rays}: lane utilisation {rays / max(slots, 1):.3f}")


@pytest.mark.parametrize("geo", GEOS)
def test_muf_with_one_hop_equals_the_one_hop_call(geo):
    z, x, den, bmag, bpsi = _iono()
    targets = np.array([np.nan, -1500.0, -1000.0, -800.0, 1900.0])
    kw = dict(n_bisect=4, max_iter=MAX_ITER, elev_tol_deg=TOL, scan_elevation_deg=SCAN, **CTL[geo])
    one = MUF1[geo](targets, den, bmag, bpsi, z, x, "O", F_LO, F_HI, X0, Z0, **kw)
    res = MUF[geo](targets, 1, den, bmag, bpsi, z, x, "O", F_LO, F_HI, X0, Z0, **kw)
    print(f"geometry {geo}: one-hop statuses {one['status'].tolist()}")
    assert len(set(one["status"].tolist())) >= 3
    for k in one:
        got = res[k][..., 0] if res[k].ndim == 2 else res[k]
        assert same_bits(got, one[k]), k


def test_muf_against_the_fixture():
    """With n_bisect = muf_safe_trips the bracket is the reference's after that many trips, bit for bit: the midpoints
    are deterministic and those decisions are clear by ten times the reference's own error."""
    g = load_golden("g25_gradient_hop_skip.npz")
    n = int(g["muf_safe_trips"])
    assert 4 <= n <= 10
    f_lo, f_hi = float(g["muf_f_lo_hz"]), float(g["muf_f_hi_hz"])
    res = _muf(0, np.array([float(g["muf_target_km"])]), int(g["muf_hops"]), f_lo=f_lo, f_hi=f_hi, n_bisect=n)
    want_lo = g["muf_trip_lo_hz"][n] if n < 10 else g["muf_hz"]
    want_hi = g["muf_trip_hi_hz"][n] if n < 10 else g["muf_f_above_hz"]
    print(f"{n} safe trips: bracket {res['muf_hz'][0]!r} .. {res['f_above_hz'][0]!r}; the reference's final "
          f"{g['muf_hz']!r} .. {g['muf_f_above_hz']!r}")
    assert res["status"][0] == 0 and res["muf_hz"][0] == want_lo and res["f_above_hz"][0] == want_hi


@pytest.mark.parametrize("geo", GEOS)
def test_two_hops_bracket_a_link_the_one_hop_call_cannot_reach(geo):
    """The feature's reason.  S(f) is the LEAST landing coordinate of the scan, so "no one-hop ray reaches that far" is a
    statement about a scan that looks behind the transmitter (elevations beyond 90 degrees), where the least coordinate
    is the farthest landing: from x0 = 1800 km with the scan 120 .. 160 degrees the one-hop call answers a target beyond
    its farthest landing with status 2 - S(f_lo) > target, nothing found - and the two-hop call brackets the MUF."""
    x0, f_hi = 1800.0, 40.0e6
    z, x, den, bmag, bpsi = _iono()
    s1 = SKIP1[geo](_built(geo, "O", [F_LO]), x0, Z0, scan_elevation_deg=_scan("back"), elev_tol_deg=TOL, max_iter=MAX_ITER,
                    **CTL[geo])
    s2 = _s(geo, "O", 2, x0, "back")
    s1_lo, s2_lo, s2_hi = float(s1["skip_km"][0, 0]), s2(F_LO), s2(f_hi)
    print(f"geometry {geo}: one hop S(f_lo) {s1_lo!r}; two hops S(f_lo) {s2_lo!r} S(f_hi) {s2_hi!r}")
    assert s1["status"][0, 0] >= 0 and s2_lo < s1_lo
    t = np.array([0.5 * (s1_lo + s2_lo)])
    assert s2_hi > t[0]
    kw = dict(n_bisect=5, max_iter=MAX_ITER, elev_tol_deg=TOL, scan_elevation_deg=_scan("back"), **CTL[geo])
    one = MUF1[geo](t, den, bmag, bpsi, z, x, "O", F_LO, f_hi, x0, Z0, **kw)
    assert one["status"][0] == 2 and np.isnan(one["muf_hz"][0])
    two = _muf(geo, t, 2, f_hi=f_hi, x0=x0, scan_key="back", n_bisect=5)
    assert two["status"][0] == 0 and F_LO <= two["muf_hz"][0] < two["f_above_hz"][0] <= f_hi
    _check_muf(geo, two, t, 2, 5, f_hi=f_hi, x0=x0, scan_key="back")


@pytest.mark.parametrize("geo", GEOS)
def test_muf_many_links_slabs_and_x_mode(geo):
    s = _s(geo, "O", 2)
    targets = np.linspace(s(F_LO) - 5.0, s(F_HI) + 5.0, 65)
    res = _muf(geo, targets, 2, n_bisect=3)
    _check_muf(geo, res, targets, 2, 3)
    assert set(res["status"].tolist()) == {0, 1, 2}
    one = _muf(geo, targets[31:32], 2, n_bisect=3)
    for k in res:
        assert same_bits(one[k][0], res[k][31]), k                     # 1 link
    slabs = _muf(geo, targets[28:33], 2, n_bisect=3, _slab_links=2)
    for k in res:
        assert same_bits(slabs[k], res[k][28:33]), k                   # forced slabs of 2 equal one slab
    sx = _s(geo, "X", 3)
    lo, hi = sx(F_LO), sx(F_HI)
    assert np.isfinite(lo) and lo < hi, (lo, hi)
    tx = np.array([0.5 * (lo + hi) if np.isfinite(hi) else lo + 100.0])
    rx = _muf(geo, tx, 3, mode="X", n_bisect=4)
    _check_muf(geo, rx, tx, 3, 4, mode="X")
    assert rx["status"][0] == 0
