"""The spherical Snell kernels under the caller's controls (R_E, dz_target_km, apex_boost, max_substeps) and both Snell
kernels on rays whose bracket sits at the edge of a 64-level chunk, against fixture G29 (the reference's tracers run by
oracle/gen_golden.py gen_snell_controls); and the controls through every entry point that takes them: the per-ray, the
single-ray and the grouped call, homing, skip distance and MUF.

The bounds are those of tests/test_gpu_tracers.py (TIERS, and the grouped call against the per-ray call at 1e-13)."""

import numpy as np
import pytest

import skip_rule
import snell_g29
from conftest import same_bits
from test_gpu_tracers import TIERS

pytestmark = pytest.mark.gpu

SETS = ("fine", "coarse", "flat_count", "cap1", "cap15", "cap16", "cap17", "cap65", "beyond", "mars", "small", "mixed")
KEYS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_turn_km", "z_turn_km",
        "n_path")
# absolute floors beside the tiers' relative bounds, as test_gpu_tracers.py has them: (ground range, x nodes) per geometry
FLOORS = ((1e-12, 1e-10), (1e-10, 1e-9))


def _math(tier):
    from pyrayhf_amd import library
    return library.MATH_FAITHFUL if tier == "faithful" else None


def _rays_fn(geometry):
    from pyrayhf_amd import tracers
    return tracers.trace_rays_spherical_snells if geometry else tracers.trace_rays_cartesian_snells


def _fan_fn(geometry):
    from pyrayhf_amd import tracers
    return tracers.trace_fan_spherical_snells if geometry else tracers.trace_fan_cartesian_snells


class Worst:
    """The largest ratio of error to bound seen, per quantity"""

    def __init__(self):
        self.ratio = {}

    def hold(self, name, got, want, rtol, atol=0.0, where=None):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape and np.isfinite(want).all(), (name, where)
        with np.errstate(all="ignore"):
            ratio = np.abs(got - want) / (rtol * np.abs(want) + atol)
        ratio = np.where(got == want, 0.0, ratio)                   # (0 against 0 without a floor is no error)
        self.ratio[name] = max(self.ratio.get(name, 0.0), float(np.max(ratio, initial=0.0)))
        assert np.all(ratio <= 1.0), (name, where, float(np.nanmax(ratio)))

    def __str__(self):
        return ", ".join(f"{k} {v:.1e}" for k, v in self.ratio.items())


def _hold_rows_to_g29(part, rows, got, geometry, rtol, worst, column):
    """The per-ray call's result `got` for the rows `rows` of G29's part `part`, in their order: the same rays turn, the
    paths have the same nodes, and every stored value is within the tier's bound; the midpoint is the node before the
    apex (tracers.trace_rays_cartesian_snells) - of the call's own path bit for bit, and so of the reference's."""
    from oracle import snell_numpy as sn
    g = snell_g29.fixture()
    want, n_ref = g[f"{part}_scalars"][rows], g[f"{part}_n_path"][rows]
    floor_range, floor_x = FLOORS[geometry]
    assert np.array_equal(np.isfinite(got["group_path_km"]), n_ref > 0), part            # the same rays turn
    assert np.array_equal(got["n_path"], n_ref), (part, got["n_path"], n_ref)
    t = n_ref > 0
    for key in ("ground_range_km", "x_turn_km", "z_turn_km", "x_midpoint", "z_midpoint"):
        assert np.isnan(got[key][~t]).all(), key
    assert np.isfinite(want[t][:, [0, 1, 4]]).all()                                       # (every ray of G29 that turns lands)
    worst.hold("path", got["group_path_km"][t], want[t, 0], rtol)
    worst.hold("delay", got["group_delay_sec"][t], want[t, 1], rtol)
    worst.hold("range", got["ground_range_km"][t], want[t, 4], rtol, floor_range)
    worst.hold("x_turn", got["x_turn_km"][t], g[f"{part}_x_turn"][rows][t], rtol, floor_x)
    worst.hold("z_turn", got["z_turn_km"][t], g[f"{part}_z_turn"][rows][t], max(rtol / 10, 1e-13))
    grounded = sn.with_ground(*column)
    for k, i in enumerate(rows):
        n = int(n_ref[k])
        if n == 0:
            assert np.isnan(got["x"][k]).all() and np.isnan(got["z"][k]).all()
            continue
        worst.hold("x", got["x"][k, :n], snell_g29.x_path(part, i), rtol, floor_x, where=(part, int(i)))
        assert np.isnan(got["x"][k, n:]).all() and np.isnan(got["z"][k, n:]).all()
        apex = n // 2
        assert same_bits(got["x_turn_km"][k], got["x"][k, apex]) and same_bits(got["z_turn_km"][k], got["z"][k, apex])
        assert same_bits(got["x_midpoint"][k], got["x"][k, apex - 1]) and same_bits(got["z_midpoint"][k], got["z"][k, apex - 1])
        # the nodes below the apex are the column's levels, the ground level included, less those whose refractive index
        # is blanked (library.py:1184-1189; G8 / G9 pin the z arrays)
        mode_i, f_hz = g[f"{part}_rays"][i, :2]
        levels = grounded[0][np.isfinite(sn.level_indices(f_hz, *grounded[1:], "OX"[int(mode_i)])[0])]
        np.testing.assert_allclose(got["z"][k, :apex], levels[:apex], rtol=max(rtol / 10, 1e-13), atol=1e-12)
        assert same_bits(got["z"][k, apex + 1:n], got["z"][k, :apex][::-1])


def _hold_fan_to_rays(fan, rays, where):
    """The grouped call against the per-ray call in the reference's operation order on the same rays: equal NaN masks
    and node counts, values to rtol 1e-13 / atol 1e-12 (test_fan_shares_the_levels_and_changes_nothing)."""
    for key in KEYS + ("x", "z"):
        got, want = fan[key].reshape(rays[key].shape), rays[key]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (where, key)
        if key == "n_path":
            assert np.array_equal(got, want), (where, key)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-12, equal_nan=True, err_msg=f"{where} {key}")


@pytest.mark.parametrize("tier", ["faithful", "default"])
@pytest.mark.parametrize("name", SETS)
def test_controls_against_reference_rays(name, tier):
    """trace_rays_spherical_snells with the controls of one set of G29 part A against the reference run with the same
    keyword arguments, in both arithmetic settings: the same rays turn, the same node counts; group path, group delay,
    ground range, the apex and every x node within the tier's spherical bound (1e-11 faithful, 1e-10 default), the apex
    altitude within a tenth of it.  The worst ratio of error to bound is printed
    (profiles/snell_controls_parity.md keeps them)."""
    g = snell_g29.fixture()
    s = snell_g29.set_names().index(name)
    kw = snell_g29.controls(s)
    rtol = TIERS[tier][1]
    worst = Worst()
    turned = 0
    for col_i in (0, 1):
        column = snell_g29.control_column(col_i)
        for mode_i, mode in enumerate("OX"):
            rows = np.nonzero((g["a_set"] == s) & (g["a_column"] == col_i) & (g["a_rays"][:, 0] == mode_i))[0]
            got = _rays_fn(1)(g["a_rays"][rows, 1], g["a_rays"][rows, 2], *column, mode, return_paths=True, math=_math(tier),
                              **kw)
            _hold_rows_to_g29("a", rows, got, 1, rtol, worst, column)
            turned += int((got["n_path"] > 0).sum())
    assert turned >= 25
    print(f"controls vs G29, per-ray call, set {name}, {tier}: {turned} rays turn; worst error / bound {worst}")


@pytest.mark.parametrize("name", SETS)
def test_fan_under_controls(name):
    """trace_fan_spherical_snells with a set's controls on the set's frequencies and elevations against the per-ray call
    in the reference's operation order with the same controls: the existing fan-versus-ray bound.  That holds the grouped
    kernel to G29 through the test above; its group path is held to the fixture directly as well, at the faithful
    tier's bound."""
    g = snell_g29.fixture()
    s = snell_g29.set_names().index(name)
    kw = snell_g29.controls(s)
    freqs = np.array([5e6, 10e6, 12.5e6])
    elevs = np.array(sorted(set(g["a_rays"][g["a_set"] == s][:, 2])))
    assert elevs[-1] == 90.0 and elevs.size >= 4
    ff, ee = np.meshgrid(freqs, elevs, indexing="ij")
    worst = Worst()
    held = 0
    for col_i in (0, 1):
        column = snell_g29.control_column(col_i)
        for mode_i, mode in enumerate("OX"):
            fan = _fan_fn(1)(freqs, elevs, *column, mode, return_paths=True, **kw)
            rays = _rays_fn(1)(ff.ravel(), ee.ravel(), *column, mode, return_paths=True, math=_math("faithful"), **kw)
            assert fan["group_path_km"].shape == (freqs.size, elevs.size)
            _hold_fan_to_rays(fan, rays, (name, col_i, mode))
            for i in np.nonzero((g["a_set"] == s) & (g["a_column"] == col_i) & (g["a_rays"][:, 0] == mode_i))[0]:
                fi, ei = np.nonzero(freqs == g["a_rays"][i, 1])[0][0], np.nonzero(elevs == g["a_rays"][i, 2])[0][0]
                assert fan["n_path"][fi, ei] == g["a_n_path"][i]
                if g["a_n_path"][i]:
                    worst.hold("path", fan["group_path_km"][fi, ei], g["a_scalars"][i, 0], TIERS["faithful"][1])
                    held += 1
    assert held >= 25
    print(f"controls vs G29, grouped call, set {name}: {held} rays turn; worst error / bound {worst}")


def test_single_ray_call_takes_the_controls():
    """trace_ray_spherical_snells hands every control on: with the `mixed` set (none at its default, all four distinct)
    its dict is row 0 of the batch call with the same controls bit for bit, and not the default call's."""
    from pyrayhf_amd import tracers
    kw = snell_g29.controls(SETS.index("mixed"))
    column = snell_g29.control_column(0)
    one = tracers.trace_ray_spherical_snells(10e6, 45.0, *column, "O", **kw)
    row = tracers.trace_rays_spherical_snells(np.array([10e6]), np.array([45.0]), *column, "O", return_paths=True, **kw)
    n = int(row["n_path"][0])
    assert n > 0 and one["x"].size == n
    assert same_bits(one["x"], row["x"][0, :n]) and same_bits(one["z"], row["z"][0, :n])
    for key in ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km"):
        assert same_bits(one[key], row[key][0]), key
    plain = tracers.trace_ray_spherical_snells(10e6, 45.0, *column, "O")
    assert abs(plain["group_path_km"] - one["group_path_km"]) > 1e-6 * plain["group_path_km"]
    # each control on its own moves the ray too: one dropped on the way would not go unnoticed
    for key, value in kw.items():
        alone = tracers.trace_ray_spherical_snells(10e6, 45.0, *column, "O", **{key: value})
        assert not same_bits(alone["group_path_km"], plain["group_path_km"]), key
        assert not same_bits(alone["group_path_km"], one["group_path_km"]), key


@pytest.mark.parametrize("tier", ["faithful", "default"])
@pytest.mark.parametrize("geometry", [0, 1])
def test_chunk_edge_brackets(geometry, tier):
    """Every ray of G29 part B - brackets in the last interval of a chunk of 64 levels, across two chunks, in the first of
    the next, a column's lowest and last, with and without the inserted ground level, and the column with a repeated
    altitude - through trace_rays_*_snells against the reference at the tier's bounds (flat 1e-12 / 1e-10, spherical
    1e-11 / 1e-10), with paths.  Under the faithful tier the same rays go through trace_fan_*_snells, one fan per column
    and mode with that column's stored elevations, against the per-ray call at 1e-13."""
    g = snell_g29.fixture()
    rtol = TIERS[tier][geometry]
    worst = Worst()
    seen = set()
    for col_i in range(g["b_columns"].shape[0]):
        column = snell_g29.edge_column(col_i)
        for mode_i, mode in enumerate("OX"):
            rows = np.nonzero((g["b_geometry"] == geometry) & (g["b_column"] == col_i) & (g["b_rays"][:, 0] == mode_i))[0]
            assert rows.size >= 3
            elevs = g["b_rays"][rows, 2]
            got = _rays_fn(geometry)(np.full(rows.size, 10e6), elevs, *column, mode, return_paths=True, math=_math(tier))
            _hold_rows_to_g29("b", rows, got, geometry, rtol, worst, column)
            seen |= set(((got["n_path"] - 3) // 2).tolist())
            if tier == "faithful":
                order = np.argsort(elevs)
                assert np.all(np.diff(elevs[order]) > 0)
                fan = _fan_fn(geometry)(np.array([10e6]), elevs[order], *column, mode, return_paths=True)
                _hold_fan_to_rays(fan, {k: v[order] for k, v in got.items()}, (geometry, col_i, mode))
    assert {62, 63, 64, 126, 127, 128} <= seen
    print(f"chunk edges vs G29, {'spherical' if geometry else 'flat'}, {tier}: {int((g['b_geometry'] == geometry).sum())} rays; "
          f"worst error / bound {worst}")


def _retrace(freq, elev, column, mode, kw):
    return _rays_fn(1)(np.atleast_1d(freq), np.atleast_1d(elev), *column, mode, math=_math("faithful"), **kw)


def _hold_rows_to_retrace(rows, again, where):
    """The eight outputs of result rows against the per-ray call at the rows' elevations: 1e-12 relative and equal node
    counts (test_gpu_homing.test_every_returned_ray_is_the_tracers_ray)."""
    for key in KEYS:
        got, want = np.atleast_1d(rows[key]), again[key]
        if key == "n_path":
            assert np.array_equal(got, want), (where, key)
        else:
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (where, key, got, want)


def test_controls_reach_homing_skip_and_muf():
    """home_rays_, skip_distance_ and muf_spherical_snells under the `mixed` controls on the day and gauss columns of G8.
    Homing (targets 300, 800 and 1500 km, the default scan) and skip distance: every row, traced again by the per-ray
    call at its elevation with the same controls in the reference's operation order, gives the row's eight outputs to
    1e-12 and the same node count - and with the default controls a group path more than 1e-6 relative away, so that a
    call that ignored the controls fails.  MUF (n_bisect = 12, one link per column): bit for bit the bisection of
    tests/skip_rule.py driven by skip-distance calls with the same controls, and not the MUF of the default controls."""
    from pyrayhf_amd import tracers
    kw = snell_g29.controls(SETS.index("mixed"))
    targets = np.array([300.0, 800.0, 1500.0])
    # (the day column's skip distance passes 450 km near 14.4 MHz where it grows by 0.3 km per kHz, the gauss column's 800 km
    #  near 12.5 MHz: the two radii put these crossings tens of kHz apart, 6 MHz / 2^12 is 1.5 kHz)
    for col_i, f_home, mode_home, f_skip, t_muf in ((1, 6.0e6, "O", 10e6, 450.0), (0, 5.0e6, "X", 12e6, 800.0)):
        column = snell_g29.control_column(col_i)
        res = tracers.home_rays_spherical_snells(np.array([f_home]), targets, *column, mode_home, **kw)
        used = np.arange(4) < np.minimum(res["n_brackets"], 4)[..., None]
        assert used.sum() >= 2 and np.all(res["status"][used] >= 0)
        rows = {k: res[k][used] for k in KEYS}
        elev = res["elevation_deg"][used]
        _hold_rows_to_retrace(rows, _retrace(np.full(elev.size, f_home), elev, column, mode_home, kw), ("home", col_i))
        plain = _retrace(np.full(elev.size, f_home), elev, column, mode_home, {})
        assert (np.abs(plain["group_path_km"] - rows["group_path_km"]) > 1e-6 * rows["group_path_km"]).any()

        skip = tracers.skip_distance_spherical_snells(np.array([f_skip]), *column, "O", **kw)
        assert skip["status"][0] == 0 and skip["n_evals"][0] > 0
        rows = {k: skip[k][0] for k in KEYS}
        _hold_rows_to_retrace(rows, _retrace(f_skip, skip["elevation_deg"][0], column, "O", kw), ("skip", col_i))
        plain = _retrace(f_skip, skip["elevation_deg"][0], column, "O", {})
        assert abs(plain["group_path_km"][0] - rows["group_path_km"]) > 1e-6 * rows["group_path_km"]

        f_lo, f_hi, n_bisect = 9e6, 15e6, 12
        muf = tracers.muf_spherical_snells(np.array([t_muf]), f_lo, f_hi, *column, "O", n_bisect=n_bisect, **kw)

        def s_of(f):
            r = tracers.skip_distance_spherical_snells(np.array([f]), *column, "O", **kw)
            return np.inf if r["status"][0] == -1 else float(r["skip_km"][0])
        want = skip_rule.muf_search(s_of, t_muf, f_lo, f_hi, n_bisect)
        assert want["status"] == 0 == muf["status"][0] and len(want["trips"]) == n_bisect
        assert same_bits(want["muf_hz"], muf["muf_hz"][0]) and same_bits(want["f_above_hz"], muf["f_above_hz"][0])
        plain = tracers.muf_spherical_snells(np.array([t_muf]), f_lo, f_hi, *column, "O", n_bisect=n_bisect)
        assert plain["status"][0] == 0 and plain["muf_hz"][0] != muf["muf_hz"][0]


def test_bad_controls_raise_from_every_entry_point():
    """snell_controls (prhf_api.cpp) refuses a radius that is not positive and finite, a dz_target_km that is not
    positive, an apex_boost that is negative or NaN and max_substeps below 1 - from each of the entry points."""
    from pyrayhf_amd import tracers
    column = snell_g29.control_column(0)
    f, e, t = np.array([10e6]), np.array([50.0]), np.array([800.0])
    calls = (lambda **kw: tracers.trace_ray_spherical_snells(10e6, 50.0, *column, "O", **kw),
             lambda **kw: tracers.trace_rays_spherical_snells(f, e, *column, "O", **kw),
             lambda **kw: tracers.trace_fan_spherical_snells(f, e, *column, "O", **kw),
             lambda **kw: tracers.home_rays_spherical_snells(f, t, *column, "O", **kw),
             lambda **kw: tracers.skip_distance_spherical_snells(f, *column, "O", **kw),
             lambda **kw: tracers.muf_spherical_snells(t, 9e6, 15e6, *column, "O", n_bisect=4, **kw))
    for kw in ({"R_E": np.inf}, {"R_E": -6371.0}, {"R_E": np.nan}, {"dz_target_km": 0.0}, {"max_substeps": 0},
               {"apex_boost": -1.0}, {"apex_boost": np.nan}):
        for call in calls:
            with pytest.raises(ValueError, match="spherical tracer controls"):
                call(**kw)
    for call in calls:                                               # the calls themselves are sound
        call()
