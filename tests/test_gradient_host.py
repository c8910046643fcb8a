"""CPU-side checks of the 2-D field layer and the gradient tracer: the three C symbols resolve and validate their
arguments before touching a device, the Python wrappers raise the reference's errors without a GPU, and the fixtures
g17 / g18 load as plain arrays."""

import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from pyrayhf_amd import _native, gradient, synth

NEW_SYMBOLS = ("prhf_field_pack_f64", "prhf_field_sample_f64", "prhf_trace_gradient_f64")


def _grids():
    z = np.linspace(0.0, 400.0, 9)
    x = np.linspace(-100.0, 100.0, 5)
    n = np.ones((9, 5))
    return z, x, n


def test_new_symbols_resolve_and_abi_is_4():
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _native.exported_symbols()
    assert lib.prhf_abi_version() == _native.ABI_VERSION == 4


def test_null_context_is_einval():
    lib = _native.load()
    assert lib.prhf_field_pack_f64(None, None, None, 0, 0, 0, None, None, 2, None, 0) == _native.EINVAL
    assert b"context" in lib.prhf_last_error()
    assert lib.prhf_field_sample_f64(None, None, 0, 0, 0, None, None, None, None, None, 0, 0.0, 0.0, 0.0, None, None, None,
                                     None, 0) == _native.EINVAL
    assert lib.prhf_trace_gradient_f64(None, None, 0, 0, 0, None, None, None, None, None, None, 0, 1.0, 1e-7, 1e-9, 1.0,
                                       0.0, 1.0, 0.0, 1.0, 50, 0.0, 0.0, 0.0, None, None, None, None, None, None, 0,
                                       0) == _native.EINVAL
    assert b"context" in lib.prhf_last_error()


def test_builders_raise_the_references_errors_without_a_gpu():
    z, x, n = _grids()
    with pytest.raises(ValueError, match=r"`n_field` must have shape \(len\(z_grid\)=9, len\(x_grid\)=5\), got \(5, 9\)\."):
        gradient.build_refractive_index_interpolator_cartesian(z, x, n.T)                  # library.py:1805-1810
    with pytest.raises(ValueError, match="`z_grid` and `x_grid` must be strictly increasing."):
        gradient.build_refractive_index_interpolator_cartesian(z[::-1], x, n)              # :1812-1813
    zz = z.copy()
    zz[3] = zz[2]
    with pytest.raises(ValueError, match="`z_grid` and `x_grid` must be strictly increasing."):
        gradient.build_refractive_index_interpolator_cartesian(zz, x, n)
    with pytest.raises(ValueError, match=r"`n_field` shape \(5, 9\) must be \(len\(r_grid\)=9, len\(phi_grid\)=5\)\."):
        gradient.build_refractive_index_interpolator_spherical(z, x, n.T)                  # :1890-1894
    with pytest.raises(ValueError, match="`r_grid` and `phi_grid` must be strictly increasing."):
        gradient.build_refractive_index_interpolator_spherical(z, x[::-1], n)              # :1896-1898
    with pytest.raises(ValueError, match="geometry must be 'cartesian' or 'spherical'"):
        gradient.build_mup_function(n, x, z, geometry="polar")                             # :2017
    with pytest.raises(ValueError):
        gradient.build_mup_function(n.T, x, z)
    with pytest.raises(ValueError):
        gradient.refractive_field([6e6], n, n, n, z, x, "Q")
    with pytest.raises(ValueError):
        gradient.refractive_field([6e6], n.T, n.T, n.T, z, x, "O")


def test_tracer_argument_errors_without_a_gpu():
    z, x, n = _grids()
    n_and_grad = gradient.build_refractive_index_interpolator_cartesian(z, x, n)      # (packed on first use: no GPU needed)
    mup_func = gradient.build_mup_function(n, x, z)
    with pytest.raises(ValueError, match="mup_func must be provided, build it with build_mup_function."):
        gradient.trace_ray_cartesian_gradient(n_and_grad, None, 0.0, 0.0, 45.0)       # library.py:1349-1351
    with pytest.raises(TypeError):
        gradient.trace_ray_cartesian_gradient(lambda xx, zz: (xx, xx, xx), mup_func, 0.0, 0.0, 45.0)
    with pytest.raises(TypeError):
        gradient.trace_ray_cartesian_gradient(n_and_grad, lambda xx, zz: xx, 0.0, 0.0, 45.0)
    other = gradient.build_mup_function(np.ones((9, 7)), np.linspace(-100.0, 100.0, 7), z)
    with pytest.raises(ValueError, match="same z_grid and x_grid"):
        gradient.trace_ray_cartesian_gradient(n_and_grad, other, 0.0, 0.0, 45.0)
    sph = gradient.build_refractive_index_interpolator_spherical(z, x, n)
    with pytest.raises(ValueError):
        gradient.trace_ray_cartesian_gradient(sph, mup_func, 0.0, 0.0, 45.0)
    with pytest.raises(TypeError):
        gradient.trace_rays_cartesian_gradient(n_and_grad, 0.0, 0.0, [10.0, 20.0])    # (a RefractiveField is wanted)
    field = gradient.RefractiveField(z, x, np.ones((2, 9, 5)), np.ones((2, 9, 5)))
    with pytest.raises(ValueError, match="field_index"):
        gradient.trace_rays_cartesian_gradient(field, 0.0, 0.0, [10.0, 20.0])
    with pytest.raises(ValueError, match="field_index"):
        gradient.trace_rays_cartesian_gradient(field, 0.0, 0.0, [10.0, 20.0], field_index=[0, 2])
    with pytest.raises(ValueError, match="max_step"):
        gradient.trace_fan_cartesian_gradient(field, [10.0, 20.0], max_step_km=0.0)


def test_bounds_error_is_scipys_without_a_gpu():
    z, x, n = _grids()
    n_and_grad = gradient.build_refractive_index_interpolator_cartesian(z, x, n, bounds_error=True)
    with pytest.raises(ValueError, match="One of the requested xi is out of bounds in dimension 0"):
        n_and_grad(0.0, 401.0)
    with pytest.raises(ValueError, match="One of the requested xi is out of bounds in dimension 1"):
        n_and_grad(-100.5, 10.0)
    mup_func = gradient.build_mup_function(n, x, z, bounds_error=True)
    with pytest.raises(ValueError, match="out of bounds in dimension 1"):
        mup_func(np.array([0.0, 101.0]), np.array([1.0, 1.0]))


def test_exports():
    import pyrayhf_amd
    for name in ("build_refractive_index_interpolator_cartesian", "build_refractive_index_interpolator_spherical",
                 "build_mup_function", "refractive_field", "trace_ray_cartesian_gradient",
                 "trace_rays_cartesian_gradient", "trace_fan_cartesian_gradient", "STATUS_NAMES"):
        assert hasattr(pyrayhf_amd, name), name
    assert pyrayhf_amd.STATUS_NAMES == ("ground", "domain", "length", "failure")


def test_fixtures_are_plain_arrays():
    for name in ("g17_fields.npz", "g18_gradient_rays.npz"):
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 1300000
        with np.load(path, allow_pickle=False) as zf:
            for k in zf.files:
                assert zf[k].dtype.kind in "fib", (name, k)
    g = load_golden("g17_fields.npz")
    for grid in ("nonuniform", "uniform"):
        for mode in "OX":
            key = f"{grid}_{mode}"
            assert g[key + "_mu"].shape == (41, 33) and np.isnan(g[key + "_mu"]).any()
            assert g[key + "_points"].shape == (2000, 2) and g[key + "_rgi"].shape == (4, 2000)
            for geo in ("cartesian", "spherical"):
                for order in (1, 2):
                    assert g[f"{key}_{geo}_e{order}_d0"].shape == (41, 33)
    r = load_golden("g18_gradient_rays.npz")
    assert r["elevation_deg"].size >= 16 and r["elevation_deg"][0] == 5.0 and r["elevation_deg"][-1] == 85.0
    shape = (2, 2, 2, r["elevation_deg"].size)
    for run in ("default", "truth", "check"):
        assert r[run + "_status"].shape == shape
        for key in ("group_path_km", "group_delay_sec", "ground_range_km", "x_apex_km", "z_apex_km"):
            assert r[f"{run}_{key}"].shape == shape
    assert r["agree"].mean() >= 0.9


def test_synthetic_ionosphere_is_what_the_fixtures_were_made_from():
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.0, 18)
    assert np.array_equal(-x[::-1], x) and np.all(np.diff(x) == 10.0) and np.all(np.diff(z) == 5.0)
    assert (den == den[:, :1]).all() and (bmag == bmag[:, :1]).all() and (bpsi == bpsi[:, :1]).all()
    z, x, den, _, _ = synth.tilted_ionosphere(41, 33, 0.3, 17, uniform=False)
    assert np.all(np.diff(z) > 0) and np.all(np.diff(x) > 0) and len(set(np.diff(z))) == 40
    assert den[:, -1].max() > den[:, 0].max()                     # NmF2 grows to the right
    assert ctypes.sizeof(ctypes.c_double) == 8
