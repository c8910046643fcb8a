"""Host-side checks of point-to-point homing: the two functions are exported, their arguments
are validated before any native call, and fixture G20 (tools/gen_golden_homing.py, reference-run) satisfies the
invariants its generator asserts - the ones the GPU tests of tests/test_gpu_homing.py rest on."""

import numpy as np
import pytest

from conftest import load_golden

CONVERGED_KM, JUMP_KM, NODE_KM = 1e-7, 1.0, 1e-6


def test_both_functions_are_exported():
    import pyrayhf_amd
    from pyrayhf_amd import _native, tracers
    for name in ("home_rays_cartesian_snells", "home_rays_spherical_snells"):
        assert name in pyrayhf_amd.__all__ and name in tracers.__all__
        assert getattr(pyrayhf_amd, name) is getattr(tracers, name)
    assert "prhf_snell_home_f64" in _native.exported_symbols()
    assert hasattr(_native.load(), "prhf_snell_home_f64")
    assert np.array_equal(tracers.default_scan_elevations(), np.linspace(2.0, 88.0, 345))


@pytest.mark.parametrize("spherical", [False, True])
def test_arguments_are_validated_before_any_native_call(monkeypatch, spherical):
    from pyrayhf_amd import _native, tracers

    def no_native_call(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", no_native_call)
    monkeypatch.setattr(_native, "context", no_native_call)
    g = load_golden("g8_snell.npz")
    cols = [g[f"gauss_{k}"] for k in ("alt", "den", "bmag", "bpsi")]
    home = tracers.home_rays_spherical_snells if spherical else tracers.home_rays_cartesian_snells
    f, t = np.array([4e6, 5e6]), np.array([300.0, 800.0])
    with pytest.raises(ValueError, match="Mode must be O or X"):
        home(f, t, *cols, "Z")
    bad = (dict(scan_elevation_deg=[10.0]), dict(scan_elevation_deg=[10.0, 10.0]), dict(scan_elevation_deg=[20.0, 10.0, 30.0]),
           dict(scan_elevation_deg=[10.0, np.nan, 30.0]), dict(scan_elevation_deg=np.ones((2, 3))),
           dict(max_roots=0), dict(max_roots=65), dict(max_iter=0), dict(max_iter=129),
           dict(range_tol_km=-1e-9), dict(range_tol_km=np.nan), dict(range_tol_km=np.inf))
    for kw in bad:
        with pytest.raises(ValueError):
            home(f, t, *cols, "O", **kw)
    with pytest.raises(ValueError):
        home(f.reshape(1, 2), t, *cols, "O")                          # frequencies and targets are 1-D
    with pytest.raises(ValueError):
        home(f, t.reshape(2, 1), *cols, "O")
    with pytest.raises(ValueError):
        home(f, t, cols[0], cols[1][:-1], cols[2], cols[3], "O")      # columns of different lengths
    with pytest.raises(ValueError):
        home(f, t, cols[0][:-1], cols[1], cols[2], cols[3], "O")      # one altitude per level
    with pytest.raises(ValueError):
        home(f, t, np.tile(cols[0], (3, 1)), *(np.tile(c, (2, 1)) for c in cols[1:]), "O")


def test_native_call_validates_without_a_gpu():
    """prhf_snell_home_f64 rejects a null context before anything else: PRHF_EINVAL with a message, no device touched."""
    from pyrayhf_amd import _native
    lib = _native.load()
    rc = lib.prhf_snell_home_f64(None, 0, None, None, 0, None, None, 0, None, 0, None, None, None, None, 0, 0, 0, 0,
                                 6371.0, 1.0, 200.0, 400, 1e-6, 64, 4, None, None, 0)
    assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()


def test_fixture_satisfies_the_generators_invariants():
    g = load_golden("g20_homing.npz")
    g8 = load_golden("g8_snell.npz")
    assert np.array_equal(g["scan_elevation_deg"], np.linspace(2.0, 88.0, 345))
    assert np.array_equal(g["target_km"], [300.0, 800.0, 1500.0])
    assert np.array_equal(g["freq_hz"], [6e6, 12e6, 4e6, 5e6]) and np.array_equal(g["mode_is_x"], [False, True, False, True])
    assert np.array_equal(g["column_is_day"], [True, True, False, False]) and "day_den" in g8 and "gauss_den" in g8
    miss, conv, nb = g["miss_km"], g["converged"], g["n_brackets"]
    assert nb.shape == (2, 4, 3) and nb.sum() == miss.size
    # every bracket is a crossing (the reference lands within 1e-7 km) or a jump (it stays a kilometre or more away)
    assert np.all((miss <= CONVERGED_KM) | (miss >= JUMP_KM))
    assert np.array_equal(conv, miss <= CONVERGED_KM)
    assert nb.max() >= 3 and nb.min() == 0 and (~conv).any()
    assert nb[0, 0, 0] == 4 and nb[0, 2, 2] == 0               # day, flat, 6 MHz O, 300 km; gauss, flat, 4 MHz O, 1500 km
    # no scan node within 1e-6 km of a target: bracket membership cannot hinge on the last bits
    d = g["scan_ground_range_km"]
    gap = np.abs(d[:, :, None, :] - g["target_km"][None, None, :, None])
    assert np.nanmin(gap) >= NODE_KM
    # the stored brackets are the bracket rule applied to the stored scan, in (geometry, case, target, elevation) order
    want = []
    for geo in range(2):
        for case in range(4):
            for ti, t in enumerate(g["target_km"]):
                f = d[geo, case] - t
                with np.errstate(invalid="ignore"):
                    is_b = np.isfinite(f[:-1]) & np.isfinite(f[1:]) & (f[:-1] * f[1:] < 0)
                idx = np.nonzero(is_b)[0]
                assert idx.size == nb[geo, case, ti]
                want += [(geo, case, ti, int(i)) for i in idx]
    got = list(zip(g["geometry"].tolist(), g["case"].tolist(), g["target"].tolist(), g["scan_index"].tolist()))
    assert got == want
    # a root lies inside its bracket; converged roots carry usable slopes
    e, scan = g["root_elevation_deg"], g["scan_elevation_deg"]
    assert np.all((e >= scan[g["scan_index"]]) & (e <= scan[g["scan_index"] + 1]))
    assert np.all(np.isfinite(g["dD_de"][conv]) & (g["dD_de"][conv] != 0.0))
    assert np.all(np.isfinite(g["dP_dD"][conv]) & np.isfinite(g["dtau_dD"][conv]))
    assert np.all(np.isnan(g["dD_de"][~conv]))
    assert np.allclose(g["ground_range_km"][conv], g["target_km"][g["target"][conv]], rtol=0, atol=CONVERGED_KM)
