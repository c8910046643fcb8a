"""Readers of fixture G29 (oracle/gen_golden.py gen_snell_controls): a helper of tests/test_oracle_golden.py and
tests/test_gpu_snell_controls.py, not a test."""

import numpy as np

from conftest import load_golden

SCALARS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km")
_cache = {}


def fixture():
    """G29 and the gauss and day columns of G8 it refers to: loaded once, shared, not modified"""
    if "g" not in _cache:
        _cache["g"] = load_golden("g29_snell_controls.npz")
        _cache["g8"] = load_golden("g8_snell.npz")
    return _cache["g"]


def set_names():
    return [str(s) for s in fixture()["a_set_names"]]


def controls(set_i):
    """The keyword arguments the reference was run with for control set `set_i`: only those the set names (NaN in the
    fixture: left at the default), max_substeps as an int"""
    g = fixture()
    kw = {}
    for name, v in zip(g["a_control_order"], g["a_controls"][set_i]):
        if not np.isnan(v):
            kw[str(name)] = int(v) if name == "max_substeps" else float(v)
    return kw


def control_column(col_i):
    """alt, den, bmag, bpsi of part A's column `col_i` (0 gauss, 1 day): G8's"""
    fixture()
    name = str(_cache["g"]["a_column_names"][col_i])
    return [_cache["g8"][f"{name}_{k}"] for k in ("alt", "den", "bmag", "bpsi")]


def edge_column(col_i):
    """alt, den, bmag, bpsi of part B's column `col_i`: the Gaussian layer of G8 cut at its peak, n levels from z0 to
    250 km, with alt[31] = alt[30] where the table says so (oracle/gen_golden.py snell_edge_column)"""
    z0, n, repeat = fixture()["b_columns"][col_i]
    alt = np.linspace(float(z0), 250.0, int(n))
    if repeat:
        alt[31] = alt[30]
    return [alt, 1e12 * np.exp(-(alt - 250) ** 2 / (2 * 60 ** 2)), np.full_like(alt, 4e-5), np.full_like(alt, 45.0)]


def x_path(part, i):
    g = fixture()
    return g[f"{part}_x"][g[f"{part}_offsets"][i]:g[f"{part}_offsets"][i + 1]]
