"""CPU-side checks of the spherical gradient tracer: the C symbol resolves, is listed by header and binding alike and
validates before it touches a device; the Python wrappers raise their argument errors before any native call; the
fixture g19 loads as plain arrays and satisfies the assertions its generator made (tools/gen_golden_spherical.py)."""

import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from pyrayhf_amd import _native, gradient

SYMBOL = "prhf_trace_gradient_spherical_f64"
RULE_KEYS = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km")


def _grids():
    z = np.linspace(0.0, 400.0, 9)
    x = np.linspace(-100.0, 100.0, 5)
    n = np.ones((9, 5))
    return z, x, n


@pytest.fixture
def no_native(monkeypatch):
    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)


def test_the_three_functions_exist_and_are_exported():
    import pyrayhf_amd
    for name in ("trace_ray_spherical_gradient", "trace_rays_spherical_gradient", "trace_fan_spherical_gradient"):
        assert callable(getattr(gradient, name)), name
        assert name in gradient.__all__ and name in pyrayhf_amd.__all__
        assert getattr(pyrayhf_amd, name) is getattr(gradient, name)


def test_header_and_binding_list_the_symbol_and_the_abi_stays_4():
    header = os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "prhf.h")
    with open(header) as fh:
        text = fh.read()
    assert re.search(r"^int " + SYMBOL + r"\(", text, re.M)
    assert SYMBOL in _native.exported_symbols()
    lib = _native.load()
    assert hasattr(lib, SYMBOL)
    assert lib.prhf_abi_version() == _native.ABI_VERSION == 4


def test_null_context_is_einval():
    lib = _native.load()
    rc = getattr(lib, SYMBOL)(None, None, 0, 0, 0, None, None, None, None, None, None, 0, 6371.0, 1.0, 1e-7, 1e-9, 1.0,
                              0.0, 7000.0, -1.0, 1.0, 50, 0.0, 0.0, 0.0, None, None, None, None, None, None, 0, 0)
    assert rc == _native.EINVAL
    assert b"context" in lib.prhf_last_error()


def test_single_ray_argument_errors_before_any_native_call(no_native):
    z, x, n = _grids()
    sph = gradient.build_refractive_index_interpolator_spherical(z, x, n)
    mup = gradient.build_mup_function(n, x, z, geometry="spherical")
    with pytest.raises(ValueError, match=r"mup_func must be provided — build it with "
                                         r"build_mup_function\(\.\.\., geometry='spherical'\)\."):
        gradient.trace_ray_spherical_gradient(sph, None, 0.0, 0.0, 45.0)             # reference library.py:2216-2219
    with pytest.raises(TypeError):
        gradient.trace_ray_spherical_gradient(lambda p, r: (p, p, p), mup, 0.0, 0.0, 45.0)
    with pytest.raises(TypeError):
        gradient.trace_ray_spherical_gradient(sph, lambda xx, zz: xx, 0.0, 0.0, 45.0)
    cart = gradient.build_refractive_index_interpolator_cartesian(z, x, n)
    with pytest.raises(ValueError, match="spherical"):
        gradient.trace_ray_spherical_gradient(cart, mup, 0.0, 0.0, 45.0)
    with pytest.raises(ValueError, match="spherical"):
        gradient.trace_ray_spherical_gradient(sph, gradient.build_mup_function(n, x, z), 0.0, 0.0, 45.0)
    other = gradient.build_mup_function(np.ones((9, 7)), np.linspace(-100.0, 100.0, 7), z, geometry="spherical")
    with pytest.raises(ValueError, match="same z_grid and x_grid"):
        gradient.trace_ray_spherical_gradient(sph, other, 0.0, 0.0, 45.0)
    with pytest.raises(ValueError, match="same R_E"):
        gradient.trace_ray_spherical_gradient(sph, gradient.build_mup_function(n, x, z, geometry="spherical", R_E=6400.0),
                                              0.0, 0.0, 45.0)
    with pytest.raises(ValueError, match="max_step"):
        gradient.trace_ray_spherical_gradient(sph, mup, 0.0, 0.0, 45.0, max_step_km=0.0)
    with pytest.raises(ValueError, match="max_step"):
        gradient.trace_ray_spherical_gradient(sph, mup, 0.0, 0.0, 45.0, max_step_km=-2.0)
    with pytest.raises(ValueError, match="R_E"):
        gradient.trace_ray_spherical_gradient(sph, mup, 0.0, 0.0, 45.0, R_E=6400.0)


def test_batch_argument_errors_before_any_native_call(no_native):
    z, x, n = _grids()
    r_e = gradient.constants()[2]
    two = np.ones((2, 9, 5))
    field = gradient.RefractiveField(r_e + z, x / r_e, two, two, geometry="spherical")
    assert field.geometry == "spherical" and field.R_E == r_e
    flat = gradient.RefractiveField(z, x, two, two)
    assert flat.geometry == "cartesian" and flat.R_E is None
    with pytest.raises(ValueError, match="geometry"):
        gradient.RefractiveField(z, x, two, two, geometry="polar")
    # a field of the other geometry
    with pytest.raises(ValueError, match="spherical field"):
        gradient.trace_rays_spherical_gradient(flat, 0.0, 0.0, [10.0, 20.0], [0, 1])
    with pytest.raises(ValueError, match="spherical field"):
        gradient.trace_fan_spherical_gradient(flat, [10.0, 20.0])
    with pytest.raises(ValueError, match="cartesian field"):
        gradient.trace_rays_cartesian_gradient(field, 0.0, 0.0, [10.0, 20.0], [0, 1])
    with pytest.raises(ValueError, match="cartesian field"):
        gradient.trace_fan_cartesian_gradient(field, [10.0, 20.0])
    with pytest.raises(TypeError):
        gradient.trace_rays_spherical_gradient(gradient.build_refractive_index_interpolator_spherical(z, x, n), 0.0, 0.0,
                                               [10.0, 20.0])                         # (a RefractiveField is wanted)
    with pytest.raises(ValueError, match="field_index"):
        gradient.trace_rays_spherical_gradient(field, 0.0, 0.0, [10.0, 20.0])
    with pytest.raises(ValueError, match="field_index"):
        gradient.trace_rays_spherical_gradient(field, 0.0, 0.0, [10.0, 20.0], field_index=[0, 2])
    with pytest.raises(ValueError, match="field_index"):
        gradient.trace_rays_spherical_gradient(field, 0.0, 0.0, [10.0, 20.0], field_index=[-1, 0])
    with pytest.raises(ValueError, match="max_step"):
        gradient.trace_fan_spherical_gradient(field, [10.0, 20.0], max_step_km=0.0)
    with pytest.raises(ValueError, match="R_E"):
        gradient.trace_fan_spherical_gradient(field, [10.0, 20.0], R_E=6400.0)
    with pytest.raises(ValueError, match="1-D"):
        gradient.trace_fan_spherical_gradient(field, [[10.0, 20.0]])
    # the builders and refractive_field record the geometry
    assert gradient.build_refractive_index_interpolator_spherical(z, x, n, R_E=6400.0).field.R_E == 6400.0
    assert gradient.build_refractive_index_interpolator_cartesian(z, x, n).field.geometry == "cartesian"
    assert gradient.build_mup_function(n, x, z, geometry="spherical").field.geometry == "spherical"


def test_fixture_is_plain_arrays_and_keeps_its_generators_assertions():
    path = os.path.join(GOLDEN, "g19_spherical_rays.npz")
    assert os.path.getsize(path) < 200000                              # (g17 is about 1.2 MB)
    with np.load(path, allow_pickle=False) as zf:
        for k in zf.files:
            assert zf[k].dtype.kind in "fib", k
    g = load_golden("g19_spherical_rays.npz")
    e = g["elevation_deg"]
    assert e.size == 16 and e[0] == 5.0 and e[-1] == 85.0
    shape = (2, 2, 2, 16)
    for run in ("default", "truth", "check"):
        assert g[run + "_status"].shape == shape
        assert g[run + "_bouguer_drift"].shape == shape[1:]
        for key in RULE_KEYS + ("x_apex_km", "x_midpoint", "z_midpoint"):
            assert g[f"{run}_{key}"].shape == shape
    agree = g["agree"]
    # (-1: a run the reference did not finish, see tools/gen_golden_spherical.py; such a ray is not compared)
    assert np.array_equal(agree, (g["default_status"] == g["truth_status"]) & (g["default_status"] == g["check_status"]) &
                          (g["default_status"] >= 0))
    assert all((g[run + "_status"] >= -1).all() and (g[run + "_status"] <= 3).all() for run in ("default", "truth", "check"))
    assert agree.mean() >= 0.9
    for si in range(2):
        m = agree[:, :, si]
        assert (g["default_status"][:, :, si][m] == 0).sum() >= 8
        for key in RULE_KEYS:
            d = np.abs(g["default_" + key] - g["truth_" + key])[:, :, si][m]
            c = np.abs(g["check_" + key] - g["truth_" + key])[:, :, si][m]
            ok = np.isfinite(d) & np.isfinite(c)
            assert ok.sum() >= 8
            assert c[ok].max() <= 0.1 * d[ok].max(), (si, key, c[ok].max(), d[ok].max())
