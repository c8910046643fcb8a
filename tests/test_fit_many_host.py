"""Host-side checks of the many-ionogram fit (DESIGN.md 4.5 "many ionograms"): the two new entry points are declared,
bound and exported alike; their argument checks answer before any device is touched (through the real library with a
null context, and through the Python layer); the common grid is sorted once and the observation columns with it."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from pyrayhf_amd import _native, fitting

NEW = ("prhf_residual_many_f64", "prhf_vfo_residual_many_f64")
_CTYPE = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}


def _header_prototype(name):
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, name
    args = []
    for decl in m.group(1).split(","):
        decl = " ".join(decl.split())
        args.append(ctypes.c_void_p if "*" in decl else _CTYPE[decl.rsplit(" ", 1)[0]])
    return args


@pytest.mark.parametrize("name", NEW)
def test_binding_matches_the_header(name):
    res, args = _native._PROTOTYPES[name]
    assert res is ctypes.c_int and args == _header_prototype(name)
    assert hasattr(_native.load(), name)
    assert _native.load().prhf_abi_version() == 4          # a new symbol changes nothing for callers of the others


def _ptr(x):
    return x.ctypes.data


def _stage(lib, ion, n_iono=2, n_freq=3, residual=True, n_rows=None):
    """prhf_residual_many_f64 on host arrays with a null context: the argument checks come first."""
    n_rows = len(ion) if ion is not None and n_rows is None else n_rows
    model, obs = np.zeros((max(n_rows, 1), n_freq)), np.zeros((n_iono, n_freq))
    res, cost = np.zeros_like(model), np.zeros(max(n_rows, 1) * n_iono)
    best, best_cost = np.zeros(n_iono, dtype=np.int64), np.zeros(n_iono)
    ion = None if ion is None else np.ascontiguousarray(ion, dtype=np.int32)
    rc = lib.prhf_residual_many_f64(None, _ptr(model), n_rows, _ptr(obs), n_iono, n_freq,
                                    None if ion is None else _ptr(ion), _ptr(res) if residual else None, _ptr(cost),
                                    _ptr(best), _ptr(best_cost), 0)
    return rc, lib.prhf_last_error().decode()


def test_stage_entry_checks_its_arguments_before_the_device():
    lib = _native.load()
    rc, msg = _stage(lib, [0, 1, 0])
    assert rc == _native.EINVAL and "ionogram_of_row[2] decreases" in msg
    rc, msg = _stage(lib, [0, 1, 2])
    assert rc == _native.EINVAL and "ionogram_of_row[2] outside" in msg
    rc, msg = _stage(lib, [-1, 0, 1])
    assert rc == _native.EINVAL and "ionogram_of_row[0] outside" in msg
    rc, msg = _stage(lib, None, n_rows=3)                       # shared candidates have no dense residual
    assert rc == _native.EINVAL and "shared candidates" in msg
    rc, msg = _stage(lib, [0, 0, 1], n_freq=4097)
    assert rc == _native.EINVAL and "4096" in msg
    rc, msg = _stage(lib, [0, 0, 1], n_iono=0)
    assert rc == _native.EINVAL and "shape" in msg
    # ... and arguments that pass every check reach the context, which is null here: ragged groups, an empty one
    for ion, kw in (([0, 0, 2], dict(n_iono=3)), ([], dict(n_iono=2)), (None, dict(n_rows=3, residual=False))):
        rc, msg = _stage(lib, ion, **kw)
        assert rc == _native.EINVAL and "null context" in msg, (ion, msg)
    model = np.zeros((2, 3))
    assert lib.prhf_residual_many_f64(None, _ptr(model), 2, None, 1, 3, None, None, None, None, None, 0) == _native.EINVAL
    assert "null array pointer" in lib.prhf_last_error().decode()


def test_fused_entry_refuses_a_non_finite_grid_and_bad_rows():
    lib = _native.load()
    n_alt, n_freq, n_prof, n_iono = 5, 3, 3, 2
    den, field, alt = np.ones((n_prof, n_alt)), np.ones(n_alt), np.arange(1.0, 1.0 + n_alt)
    mult, obs = np.linspace(0.0, 1.0, 4), np.zeros((n_iono, n_freq))
    cost, best, best_cost = np.zeros(n_prof), np.zeros(n_iono, dtype=np.int64), np.zeros(n_iono)

    def call(freq, ion):
        freq, ion = np.asarray(freq, dtype=np.float64), np.asarray(ion, dtype=np.int32)
        rc = lib.prhf_vfo_residual_many_f64(None, _ptr(freq), n_freq, _ptr(den), _ptr(field), _ptr(field), _ptr(alt), n_prof,
                                            n_alt, n_alt, 0, _ptr(mult), 4, _native.MODE_O, _ptr(obs), n_iono, _ptr(ion),
                                            None, None, _ptr(cost), _ptr(best), _ptr(best_cost), _native.FLAG_SHARED_FIELD)
        return rc, lib.prhf_last_error().decode()

    for bad in (np.nan, np.inf):
        rc, msg = call([1.0, bad, 3.0], [0, 0, 1])
        assert rc == _native.EINVAL and "freq_mhz[1] is not finite" in msg
    rc, msg = call([1.0, 2.0, 3.0], [1, 0, 1])
    assert rc == _native.EINVAL and "decreases" in msg
    rc, msg = call([1.0, 2.0, 3.0], [0, 1, 5])
    assert rc == _native.EINVAL and "outside" in msg
    rc, msg = call([1.0, 2.0, 3.0], [0, 0, 1])
    assert rc == _native.EINVAL and "null context" in msg


@pytest.fixture
def no_native_call(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_native, "host_context", refuse)
    monkeypatch.setattr(_native, "context", refuse)


def test_python_layer_validates_before_any_native_call(no_native_call):
    n_alt = 6
    alt, field = np.arange(100.0, 100.0 + n_alt), np.full(n_alt, 4e-5)
    den, freq = np.ones((4, n_alt)), np.array([2.0, 3.0, 4.0])
    obs = np.full((2, 3), 200.0)

    def call(freq=freq, obs=obs, den=den, bmag=field, bpsi=field, **kw):
        return fitting.residual_VH_many(freq, obs, den, bmag, bpsi, alt, "O", 10, **kw)

    with pytest.raises(ValueError, match="non-decreasing"):
        call(ionogram_of_row=[0, 1, 0, 1])
    with pytest.raises(ValueError, match=r"outside \[0, I\)"):
        call(ionogram_of_row=[0, 0, 1, 2])
    with pytest.raises(ValueError, match=r"outside \[0, I\)"):
        call(ionogram_of_row=[-1, 0, 1, 1])
    with pytest.raises(ValueError, match="one entry per candidate row"):
        call(ionogram_of_row=[0, 0, 1])
    with pytest.raises(ValueError, match="integers"):
        call(ionogram_of_row=[0.0, 0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="ionogram_of_row must be None"):
        call(ionogram_of_row=[0, 0, 1, 1], shared=True)
    with pytest.raises(ValueError, match="no dense residual"):
        call(shared=True, return_residual=True)
    with pytest.raises(ValueError, match="ionogram_of_row is required"):
        call()
    with pytest.raises(ValueError, match="finite and positive"):
        call(freq=np.array([2.0, np.nan, 4.0]), ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="finite and positive"):
        call(freq=np.array([2.0, 0.0, 4.0]), ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match=r"vh_obs must be \(I, F\)"):
        call(obs=np.full((2, 4), 200.0), ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="common frequency grid"):
        call(freq=np.ones((3, 1)), ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="one value per density level"):
        call(bmag=field[:-1], ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="one row per candidate"):
        call(bmag=np.ones((3, n_alt)), bpsi=np.ones((3, n_alt)), ionogram_of_row=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="mode must be 'O' or 'X'"):
        fitting.residual_VH_many(freq, obs, den, field, field, alt, "Z", 10, ionogram_of_row=[0, 0, 1, 1])


def test_minimize_parameters_many_batches_the_brute_search_only(no_native_call):
    one = lambda v: np.array([[[v]]])                                          # noqa: E731
    F2 = {"Nm": one(1e12), "hm": one(300.0), "B_bot": one(40.0)}
    alt = np.arange(100.0, 400.0, 5.0)
    args = ([F2, F2], [{}, {}], [{}, {}], np.array([2.0, 3.0]), np.full((2, 2), 250.0), alt, np.full(alt.size, 4e-5),
            np.full(alt.size, 30.0))
    for method in ("leastsq", "nelder", "differential_evolution"):
        with pytest.raises(NotImplementedError, match="minimize_parameters per ionogram"):
            fitting.minimize_parameters_many(*args, method=method, edp_builder=lambda *a: alt)
    with pytest.raises(ValueError, match="one entry per ionogram"):
        fitting.minimize_parameters_many([F2], [{}, {}], [{}, {}], *args[3:], edp_builder=lambda *a: alt)
    with pytest.raises(ValueError, match="ionogram 1: no finite observation"):
        obs = np.array([[250.0, 260.0], [np.nan, np.nan]])
        fitting.minimize_parameters_many(*args[:4], obs, *args[5:], edp_builder=lambda *a: alt)
    with pytest.raises(ValueError, match="B0 and B1 are not provided"):
        fitting.minimize_parameters_many(*args, bottom_type="B0_B1", edp_builder=lambda *a: alt)


def test_the_grid_is_sorted_once_and_the_observations_with_it():
    rng = np.random.default_rng(5)
    freq = rng.permutation(np.arange(1.0, 14.0, 0.5))
    obs = rng.uniform(100.0, 400.0, (5, freq.size))
    obs[rng.random(obs.shape) < 0.3] = np.nan
    f, o, order = fitting._common_grid(freq, obs)
    assert np.array_equal(f, np.sort(freq)) and np.array_equal(order, np.argsort(freq, kind="stable"))
    assert f.flags.c_contiguous and o.flags.c_contiguous and o.dtype == np.float64
    # the direct statement: the observation that was made at frequency f[k] sits in column k
    for k, fk in enumerate(f):
        assert np.array_equal(o[:, k], obs[:, int(np.nonzero(freq == fk)[0][0])], equal_nan=True)
    # per ionogram, what minimize_parameters' filter-and-sort gives is the kept part of the sorted row
    for i in range(obs.shape[0]):
        fi, oi = fitting._sorted_finite(freq, obs[i])
        keep = np.isfinite(o[i])
        assert np.array_equal(fi, f[keep]) and np.array_equal(oi, o[i][keep])
    # a grid that is sorted already is left alone; one trace is one ionogram
    f2, o2, order2 = fitting._common_grid(f, o[0])
    assert np.array_equal(f2, f) and o2.shape == (1, f.size) and np.array_equal(order2, np.arange(f.size))
