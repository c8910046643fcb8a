"""Host-side checks of the multi-hop skip distance and MUF for the gradient tracers: the C
symbols and the four functions are exported, both entry points reject a null context before anything else, arguments
are validated before any device call, and fixture G25 (tools/gen_golden_gradient_hop_skip.py: the reference's Cartesian
tracer chained by section 4.12's rule and driven by tests/skip_rule.py) satisfies the invariants its generator asserts -
the ones the GPU tests of tests/test_gpu_gradient_hop_skip.py rest on."""

import os
import re

import numpy as np
import pytest

from conftest import load_golden
import skip_rule as rule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prhf_gradient_hop_skip_f64", "prhf_gradient_hop_muf_f64", "prhf_gradient_hop_skip_counters")
FUNCTIONS = ("skip_distance_hops_cartesian_gradient", "skip_distance_hops_spherical_gradient",
             "muf_hops_cartesian_gradient", "muf_hops_spherical_gradient")
G25 = "g25_gradient_hop_skip.npz"


def test_symbols_and_functions_are_exported():
    import pyrayhf_amd
    from pyrayhf_amd import _native, gradient
    for name in FUNCTIONS:
        assert name in pyrayhf_amd.__all__ and name in gradient.__all__
        assert getattr(pyrayhf_amd, name) is getattr(gradient, name)
    lib = _native.load()
    for name in SYMBOLS:
        assert name in _native.exported_symbols() and hasattr(lib, name)
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    header = sorted(set(re.findall(r"\b(prhf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert header == _native.exported_symbols()
    assert lib.prhf_abi_version() == 4 == _native.ABI_VERSION


def test_native_calls_reject_a_null_context_before_anything_else():
    from pyrayhf_amd import _native
    lib = _native.load()
    ctl = (-1.0, -1.0, 1e-7, 1e-9, 2.0, 0.0, 600.0, -1000.0, 1000.0, 50, np.nan, 0.0, np.nan)   # (R_E, s_max_km bad too)
    for n_hops in (2, 0, 17):                                             # (a bad n_hops comes after the context)
        rc = lib.prhf_gradient_hop_skip_f64(None, 7, None, 0, 0, 0, None, None, None, None, None, 0, None, 0, *ctl, -1.0, 0,
                                            n_hops, None, 0xff)
        assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()
        rc = lib.prhf_gradient_hop_muf_f64(None, 7, None, None, None, 0, 0, None, None, 7, 9, None, None, None, 0, -1.0, -2.0,
                                           0, None, 0, *ctl, -1.0, 0, n_hops, None, 0xff)
        assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()
    assert lib.prhf_gradient_hop_skip_counters(None, None) == _native.EINVAL


def _no_native_call(monkeypatch):
    from pyrayhf_amd import _native, gradient

    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    monkeypatch.setattr(gradient.RefractiveField, "records", no_native_call)


@pytest.mark.parametrize("spherical", [False, True])
def test_skip_arguments_are_validated_before_any_device_call(monkeypatch, spherical):
    from pyrayhf_amd import gradient
    _no_native_call(monkeypatch)
    z, x = np.linspace(0.0, 400.0, 5), np.linspace(-500.0, 500.0, 7)
    mu = np.ones((z.size, x.size))
    r_e = 6371.0
    cart = gradient.RefractiveField(z, x, mu, mu)
    sph = gradient.RefractiveField(r_e + z, x / r_e, mu, mu, geometry="spherical", R_E=r_e)
    skip, field, other = ((gradient.skip_distance_hops_spherical_gradient, sph, cart) if spherical else
                          (gradient.skip_distance_hops_cartesian_gradient, cart, sph))
    with pytest.raises(TypeError):
        skip(mu, 2)                                                       # not a field
    with pytest.raises(ValueError, match="needs a"):
        skip(other, 2)                                                    # a field of the other geometry
    for n_hops in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_hops is an integer in 1 .. 16"):
            skip(field, n_hops)
    bad = (dict(scan_elevation_deg=[]), dict(scan_elevation_deg=[10.0, 10.0]), dict(scan_elevation_deg=[20.0, 10.0, 30.0]),
           dict(scan_elevation_deg=[10.0, np.nan, 30.0]), dict(scan_elevation_deg=np.ones((2, 3))),
           dict(scan_elevation_deg=[np.nan]), dict(max_iter=0), dict(max_iter=129), dict(elev_tol_deg=-1e-9),
           dict(elev_tol_deg=np.nan), dict(elev_tol_deg=np.inf), dict(max_step_km=0.0), dict(x0_km=np.zeros((2, 2))),
           dict(x0_km=np.zeros(2), z0_km=np.zeros(3)), dict(x0_km=np.empty(0)))
    for kw in bad:
        with pytest.raises(ValueError):
            skip(field, 2, **kw)
    with pytest.raises(ValueError, match="strictly increasing"):
        skip(field, 3, scan_elevation_deg=[30.0, 20.0])
    with pytest.raises(ValueError, match="max_iter is 1 .. 128"):
        skip(field, 3, max_iter=0)
    with pytest.raises(ValueError, match="elev_tol_deg must be finite and not negative"):
        skip(field, 3, elev_tol_deg=-1.0)
    if spherical:
        with pytest.raises(ValueError, match="R_E"):
            skip(field, 2, R_E=6400.0)


@pytest.mark.parametrize("spherical", [False, True])
def test_muf_arguments_are_validated_before_any_device_call(monkeypatch, spherical):
    from pyrayhf_amd import gradient
    _no_native_call(monkeypatch)
    z, x = np.linspace(0.0, 400.0, 5), np.linspace(-500.0, 500.0, 7)
    ne = np.full((z.size, x.size), 1e11)
    b = np.full_like(ne, 4e-5)
    psi = np.full_like(ne, 30.0)
    muf = gradient.muf_hops_spherical_gradient if spherical else gradient.muf_hops_cartesian_gradient
    neg = ne.copy()
    neg[2, 3] = -1.0

    def search(t=300.0, n_hops=2, ne=ne, b=b, psi=psi, z=z, x=x, mode="O", f_lo=5e6, f_hi=9e6, **kw):
        return muf(t, n_hops, ne, b, psi, z, x, mode, f_lo, f_hi, **kw)

    for n_hops in (0, 17, 1.5):
        with pytest.raises(ValueError, match="n_hops is an integer in 1 .. 16"):
            search(n_hops=n_hops)
    bad = (dict(mode="Z"), dict(z=z[::-1]), dict(x=np.zeros(7)), dict(ne=neg), dict(ne=ne[:, :-1]), dict(b=b[:-1]),
           dict(psi=psi.ravel()), dict(z=z[:4]), dict(edge_order=3), dict(ne=ne[:2], b=b[:2], psi=psi[:2], z=z[:2]),
           dict(n_bisect=0), dict(n_bisect=65), dict(f_lo=9e6, f_hi=9e6), dict(f_lo=9e6, f_hi=5e6), dict(f_lo=0.0),
           dict(f_lo=-1e6), dict(f_hi=np.inf), dict(f_lo=np.nan), dict(max_iter=0), dict(max_iter=129),
           dict(elev_tol_deg=-1.0), dict(elev_tol_deg=np.nan), dict(scan_elevation_deg=[20.0, 10.0]),
           dict(scan_elevation_deg=[10.0, np.nan]), dict(max_step_km=-1.0), dict(t=np.empty(0)),
           dict(t=np.zeros(2), x0_km=np.zeros(3)), dict(_slab_links=0))
    for kw in bad:
        with pytest.raises(ValueError):
            search(**kw)
    with pytest.raises(ValueError, match="n_bisect is 1 .. 64"):
        search(n_bisect=65)
    with pytest.raises(ValueError, match="0 < f_lo_hz < f_hi_hz"):
        search(f_lo=9e6, f_hi=5e6)
    with pytest.raises(ValueError, match="a slab holds at least one link"):
        search(_slab_links=0)


def test_hop_rows_of_a_row_without_a_frequency_read_as_unused():
    """The MUF calls leave the row NaN throughout for status -1 and 2: the dict shows unused hops, not garbage."""
    from pyrayhf_amd import gradient
    out = np.full((2, 6 + 15 * 3), np.nan)
    out[1, :6] = [100.0, 30.0, 0.0, 7.0, 1e-4, 18.0]
    out[1, 6:] = np.tile(np.r_[np.arange(10.0), 0.0, 5.0, 30.0, 1.0, 0.0], 3)
    res = gradient._hop_skip_rows(out, (2,), 3)
    assert res["status"].tolist() == [-1, 0] and res["scan_index"].tolist() == [-1, 7] and res["n_evals"].tolist() == [0, 18]
    assert res["ray_status"].tolist() == [[-1] * 3, [0] * 3] and res["n_landed"].tolist() == [0, 3]
    assert res["n_nodes"][0].tolist() == [0] * 3 and np.isnan(res["ground_range_km"][0]).all()
    assert np.isnan(res["total_ground_range_km"][0]) and res["total_ground_range_km"][1] == 7.0


def test_fixture_satisfies_the_generators_invariants():
    g = load_golden(G25)
    scan = g["scan_elevation_deg"]
    assert np.array_equal(scan, np.linspace(5.0, 85.0, 33))
    assert np.array_equal(g["freq_hz"], [12.0e6, 15.0e6]) and np.array_equal(g["mode_is_x"], [False, True])
    assert np.array_equal(g["n_hops"], [2, 3]) and np.array_equal(g["launch_km"], [-1800.0, 0.0])
    assert np.array_equal(g["controls"], [4000.0, 600.0, 2000.0]) and g["elev_tol_deg"] == 1e-3 and g["max_iter"] == 64
    for c in range(4):
        d = g["scan_ground_range_km"][c]
        i, edge = rule.scan_node(d)
        # an interior minimum with finite neighbours on both sides, and the rule's result on it
        assert not edge and 0 < i < d.size - 1 and np.isfinite(d[i - 1:i + 2]).all()
        assert i == g["default_scan_index"][c] and g["default_status"][c] == 0
        assert scan[i - 1] < g["default_elevation_deg"][c] < scan[i + 1]
        assert g["default_skip_km"][c] <= d[i] and g["default_bracket_deg"][c] <= 1e-3
        assert 1 <= g["default_n_evals"][c] <= 64
    # the nodes the issue records for these inputs
    assert g["default_scan_index"].tolist() == [13, 13, 10, 10]
    e_ref = np.abs(g["default_skip_km"] - g["truth_skip_km"]).max()
    assert e_ref == g["e_ref_km"] and e_ref > 0.0
    ratio = np.abs(g["check_skip_km"] - g["truth_skip_km"]).max() / e_ref
    assert ratio <= 0.1, ratio
    # the MUF link: bracketed, ten trips, and at least four of them decided by ten margins
    t = float(g["muf_target_km"])
    assert g["muf_n_bisect"] == 10 and g["muf_hops"] == 2
    assert g["muf_s_lo_km"] <= t < g["muf_s_hi_km"] and g["muf_status"] == 0
    n = int(g["muf_n_trips"])
    assert n == 10
    lo, hi = float(g["muf_f_lo_hz"]), float(g["muf_f_hi_hz"])
    for k in range(n):                                                   # the stored trips are the bisection's
        assert g["muf_trip_lo_hz"][k] == lo and g["muf_trip_hi_hz"][k] == hi
        m = lo + 0.5 * (hi - lo)
        assert g["muf_trip_m_hz"][k] == m
        lo, hi = (m, hi) if g["muf_trip_s_km"][k] <= t else (lo, m)
    assert g["muf_hz"] == lo and g["muf_f_above_hz"] == hi
    margins = np.abs(g["muf_trip_s_km"][:n] - t) >= 10.0 * e_ref
    safe = n if margins.all() else int(np.argmin(margins))
    assert safe == g["muf_safe_trips"] and safe >= 4


def test_the_muf_rule_replays_the_stored_search():
    """skip_rule.muf_search on S_ref(f) looked up from the fixture's trips returns the fixture's trips and bracket."""
    g = load_golden(G25)
    known = {float(g["muf_f_lo_hz"]): float(g["muf_s_lo_km"]), float(g["muf_f_hi_hz"]): float(g["muf_s_hi_km"])}
    known.update(zip(g["muf_trip_m_hz"].tolist(), g["muf_trip_s_km"].tolist()))
    r = rule.muf_search(known.__getitem__, float(g["muf_target_km"]), float(g["muf_f_lo_hz"]), float(g["muf_f_hi_hz"]), 10)
    assert r["status"] == 0 and r["muf_hz"] == g["muf_hz"] and r["f_above_hz"] == g["muf_f_above_hz"]
    assert len(r["trips"]) == 10
    for k, trip in enumerate(r["trips"]):
        assert tuple(trip) == (g["muf_trip_m_hz"][k], g["muf_trip_s_km"][k], g["muf_trip_lo_hz"][k], g["muf_trip_hi_hz"][k])
