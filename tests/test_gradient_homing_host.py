"""Host-side checks of point-to-point homing for the gradient tracers: the C symbol and the two
functions are exported, arguments are validated before any device call, fixture G21
(tools/gen_golden_gradient_homing.py, reference-run) satisfies the invariants its generator asserts - the ones the GPU
tests of tests/test_gpu_gradient_homing.py rest on - and the plain-Python restatement of the refine rule
(tests/gradient_homing_rule.py) behaves as the rule says on synthetic D(e)."""

import math
import os
import re

import numpy as np
import pytest

from conftest import load_golden
import gradient_homing_rule as rule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_TOL_KM, NODE_GAP_KM, JUMP_KM = 0.05, 1.0, 5.0


def test_symbol_and_functions_are_exported():
    import pyrayhf_amd
    from pyrayhf_amd import _native, gradient
    for name in ("home_rays_cartesian_gradient", "home_rays_spherical_gradient"):
        assert name in pyrayhf_amd.__all__ and name in gradient.__all__
        assert getattr(pyrayhf_amd, name) is getattr(gradient, name)
    lib = _native.load()
    for name in ("prhf_gradient_home_f64", "prhf_gradient_home_counters"):
        assert name in _native.exported_symbols() and hasattr(lib, name)
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    header = sorted(set(re.findall(r"\b(prhf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert header == _native.exported_symbols()
    assert lib.prhf_abi_version() == 4 == _native.ABI_VERSION


def test_native_call_rejects_a_null_context_before_anything_else():
    from pyrayhf_amd import _native
    lib = _native.load()
    rc = lib.prhf_gradient_home_f64(None, 7, None, 0, 0, 0, None, None, None, None, None, 0, None, None, 0, None, 0,
                                    -1.0, -1.0, 1e-7, 1e-9, 2.0, 0.0, 600.0, -1000.0, 1000.0, 50, np.nan, 0.0, np.nan,
                                    -1.0, 0, 0, None, None, 0)
    assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()
    assert lib.prhf_gradient_home_counters(None, None) == _native.EINVAL


@pytest.mark.parametrize("spherical", [False, True])
def test_arguments_are_validated_before_any_device_call(monkeypatch, spherical):
    from pyrayhf_amd import _native, gradient

    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    monkeypatch.setattr(gradient.RefractiveField, "records", no_native_call)
    z, x = np.linspace(0.0, 400.0, 5), np.linspace(-500.0, 500.0, 7)
    mu = np.ones((z.size, x.size))
    r_e = 6371.0
    cart = gradient.RefractiveField(z, x, mu, mu)
    sph = gradient.RefractiveField(r_e + z, x / r_e, mu, mu, geometry="spherical", R_E=r_e)
    home, field, other = ((gradient.home_rays_spherical_gradient, sph, cart) if spherical else
                          (gradient.home_rays_cartesian_gradient, cart, sph))
    t = np.array([300.0, 100.0])
    with pytest.raises(TypeError):
        home(mu, t)                                                       # not a field
    with pytest.raises(ValueError, match="needs a"):
        home(other, t)                                                    # a field of the other geometry
    bad = (dict(scan_elevation_deg=[10.0]), dict(scan_elevation_deg=[10.0, 10.0]), dict(scan_elevation_deg=[20.0, 10.0, 30.0]),
           dict(scan_elevation_deg=[10.0, np.nan, 30.0]), dict(scan_elevation_deg=np.ones((2, 3))),
           dict(max_roots=0), dict(max_roots=65), dict(max_iter=0), dict(max_iter=129),
           dict(range_tol_km=-1e-9), dict(range_tol_km=np.nan), dict(range_tol_km=np.inf), dict(max_step_km=0.0))
    for kw in bad:
        with pytest.raises(ValueError):
            home(field, t, **kw)
    for targets in (t.reshape(2, 1), t.reshape(1, 2), np.empty(0)):
        with pytest.raises(ValueError, match="target_x_km"):
            home(field, targets)
    with pytest.raises(ValueError, match="strictly increasing"):
        home(field, t, scan_elevation_deg=[30.0, 20.0])
    with pytest.raises(ValueError, match="max_roots is 1 .. 64"):
        home(field, t, max_roots=65)
    with pytest.raises(ValueError, match="max_iter is 1 .. 128"):
        home(field, t, max_iter=0)
    with pytest.raises(ValueError, match="range_tol_km must be finite and not negative"):
        home(field, t, range_tol_km=-1.0)
    if spherical:
        with pytest.raises(ValueError, match="R_E"):
            home(field, t, R_E=6400.0)


def test_fixture_satisfies_the_generators_invariants():
    g = load_golden("g21_gradient_homing.npz")
    assert np.array_equal(g["scan_elevation_deg"], np.linspace(5.0, 85.0, 33))
    assert np.array_equal(g["target_km"][:4], [300.0, 100.0, 700.0, 1500.0]) and np.isnan(g["target_km"][4])
    assert np.array_equal(g["freq_hz"], [6e6, 9e6]) and np.array_equal(g["mode_is_x"], [False, True])
    assert np.array_equal(g["launch_km"], [-400.0, 0.0]) and g["range_tol_km"] == RANGE_TOL_KM and g["max_iter"] == 64
    d, st = g["scan_ground_range_km"], g["scan_status"]
    assert d.shape == st.shape == (4, 33)
    # default and check scans agree in status at every node; a ray has a ground range exactly when it lands
    assert np.array_equal(st, g["check_status"])
    assert np.array_equal(np.isfinite(d), st == 0)
    # no scan node within 1 km (50 x the recorded range error) of a target
    gap = np.abs(d[:, None, :] - g["target_km"][None, :, None])
    assert np.nanmin(gap) >= NODE_GAP_KM
    # the stored brackets are the rule applied to the stored scan, in (case, target, elevation) order
    nb = g["n_brackets"]
    want = [(c, ti, i) for c in range(4) for ti, t in enumerate(g["target_km"]) for i in rule.brackets(d[c], float(t))]
    got = list(zip(g["bracket_case"].tolist(), g["bracket_target"].tolist(), g["bracket_scan_index"].tolist()))
    assert got == want
    for c in range(4):
        for ti in range(5):
            assert nb[c, ti] == sum(1 for k in want if k[:2] == (c, ti))
    assert nb.max() >= 3 and np.all(nb[:, 3:] == 0)              # out of reach, NaN: no bracket
    # every reference-refined bracket is a crossing, a bracket with a ray that does not land, or a jump
    bst, miss = g["bracket_status"], g["bracket_miss_km"]
    assert np.all(((bst == 0) & (miss <= RANGE_TOL_KM)) | (bst == 2) | ((bst == 1) & (miss >= JUMP_KM)))
    assert (bst != 0).any()
    conv = bst == 0
    scan = g["scan_elevation_deg"]
    for name in ("bracket_elevation_deg", "e_truth"):
        e = g[name][conv]
        assert np.all((e >= scan[g["bracket_scan_index"][conv]]) & (e <= scan[g["bracket_scan_index"][conv] + 1]))
    assert np.all(np.isnan(g["e_truth"][~conv]))
    for name in ("dD_de", "dP_de", "dT_de", "truth_group_path_km", "truth_group_delay_sec", "default_ground_range_km"):
        assert np.all(np.isfinite(g[name][conv])), name
    assert np.all(g["dD_de"][conv] != 0.0)
    # the truth run's root is a root: its own ground range is the target to well below the tolerance
    t = g["target_km"][g["bracket_target"][conv]]
    assert np.max(np.abs(g["truth_ground_range_km"][conv] - t)) <= 1e-3 * RANGE_TOL_KM
    # the reference's own range error at the roots (default run - truth run) stays below the jumps by a factor 40;
    # next to the E -> F transition (Cartesian, 6 MHz O, 700 km at 25.02 degrees) it is 0.12 km, elsewhere <= 2e-2 km
    err_d = np.abs(g["default_ground_range_km"][conv] - g["truth_ground_range_km"][conv])
    assert err_d.max() <= JUMP_KM / 40 and np.sort(err_d)[-2] <= 2.3e-2


def _drive(fn, scan, t, tol, max_iter):
    d = np.array([fn(e) for e in scan])
    return d, [rule.refine(fn, scan, d, i, t, tol, max_iter) for i in rule.brackets(d, t)]


def test_the_rule_on_synthetic_ranges():
    scan = np.linspace(0.0, 10.0, 11)
    # a cubic with three crossings of 0.3: every bracket converges, on rays inside its bracket
    cubic = lambda e: 0.05 * (e - 1.5) * (e - 5.2) * (e - 8.7) + 0.3          # noqa: E731
    d, res = _drive(cubic, scan, 0.3, 1e-9, 64)
    assert [r["status"] for r in res] == [0, 0, 0]
    for r, i in zip(res, rule.brackets(d, 0.3)):
        assert abs(cubic(r["elevation_deg"]) - 0.3) <= 1e-9 and r["miss_km"] == abs(cubic(r["elevation_deg"]) - 0.3)
        assert all(scan[i] < x < scan[i + 1] for x in r["tried"]) and len(r["tried"]) <= 12
    # a scan node within the tolerance is a root without a ray; D_i == t and the bracket of no width at the last node
    hit = lambda e: e - 4.0                                                    # noqa: E731
    d = np.array([hit(e) for e in scan])
    assert rule.brackets(d, 0.0) == [4] and rule.brackets(d, 6.0) == [10] and rule.brackets(d, float("nan")) == []
    for i, t in ((4, 0.0), (10, 6.0)):
        r = rule.refine(hit, scan, d, i, t, 0.0, 64)
        assert r["status"] == 0 and r["tried"] == [] and r["is_node"] and r["elevation_deg"] == scan[i]
    # a jump across the target: status 1 once no float64 is left between the ends (tolerance 0, max_iter at its cap)
    jump = lambda e: 100.0 + e if e < 3.3 else 50.0 - e                        # noqa: E731
    d, res = _drive(jump, scan, 75.0, 0.0, 128)
    assert len(res) == 1 and res[0]["status"] == 1 and res[0]["miss_km"] >= 20.0
    assert abs(res[0]["tried"][-1] - 3.3) < 1e-12 and len(res[0]["tried"]) < 128       # the ends closed in on the jump
    assert res[0]["elevation_deg"] == 3.0 and res[0]["is_node"] and res[0]["miss_km"] == 28.0  # no ray beat the lower node
    # ... and with few rays: max_iter spent, the bracket halved at least max_iter / 2 times, the best ray kept
    for max_iter in (1, 7, 16):
        r = rule.refine(jump, scan, d, 3, 75.0, 0.0, max_iter)
        assert r["status"] == 1 and len(r["tried"]) == max_iter and r["halved"] >= max_iter // 2
        assert r["miss_km"] == min([abs(d[3] - 75.0), abs(d[4] - 75.0)] + [abs(jump(x) - 75.0) for x in r["tried"]])
    # a hole of NaN inside the bracket: status 2, the best of the rays that landed
    hole = lambda e: float("nan") if 6.2 < e < 6.9 else 10.0 * (e - 6.5)       # noqa: E731
    d, res = _drive(hole, scan, 0.0, 1e-6, 64)
    assert len(res) == 1 and res[0]["status"] == 2 and math.isnan(hole(res[0]["tried"][-1]))
    assert math.isfinite(res[0]["miss_km"]) and res[0]["miss_km"] <= 5.0
    # NaN nodes bracket nothing
    assert rule.brackets(np.array([1.0, np.nan, -1.0, np.nan]), 0.0) == []
