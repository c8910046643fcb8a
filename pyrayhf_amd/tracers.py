"""Stratified Snell's-law ray tracing on the GPU.

``trace_ray_cartesian_snells`` and ``trace_ray_spherical_snells`` keep the reference's signatures
and result dictionaries (reference ``PyRayHF/library.py:1096-1268``, ``:1460-1713``);
``trace_rays_cartesian_snells`` / ``trace_rays_spherical_snells`` trace a batch of
(frequency, elevation[, profile]) rays in one launch, one wavefront per ray;
``trace_fan_cartesian_snells`` / ``trace_fan_spherical_snells`` trace every elevation of a fan for every
frequency (and profile): the refractive-index levels, which depend on the profile and the frequency only, are
computed once per (profile, frequency) and shared by the fan's rays;
``home_rays_cartesian_snells`` / ``home_rays_spherical_snells`` find, for every (profile, frequency) and every ground
range, the rays that land there (point-to-point homing, the oblique ionogram of a link);
``skip_distance_cartesian_snells`` / ``skip_distance_spherical_snells`` find the smallest ground range a
(profile, frequency) reaches, and ``muf_cartesian_snells`` / ``muf_spherical_snells`` the frequency at which that skip
distance equals a link's range.

There is no multi-hop call here: over a stratified ionosphere n hops are n copies of one hop (n times its ground range,
path and delay at the same elevation), so these tracers need nothing new.  Through a horizontally varying ionosphere a
hop is not a copy of the one before it; ``pyrayhf_amd.gradient.trace_hops_cartesian_gradient`` and its kin chain them
(DESIGN.md section 4.12).
"""

from __future__ import annotations

import numpy as np

from . import _native
from .library import MATH_AUTO, _as_rows, constants

__all__ = ["trace_ray_cartesian_snells", "trace_rays_cartesian_snells", "trace_ray_spherical_snells",
           "trace_rays_spherical_snells", "trace_fan_cartesian_snells", "trace_fan_spherical_snells",
           "home_rays_cartesian_snells", "home_rays_spherical_snells", "skip_distance_cartesian_snells",
           "skip_distance_spherical_snells", "muf_cartesian_snells", "muf_spherical_snells", "tan_from_mu_scalar",
           "find_turning_point"]

_KEYS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_turn_km",
         "z_turn_km", "n_path")
_DICT_KEYS = ("x", "z", "group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km")


def _trace_rays(spherical, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, profile_index, return_paths, device,
                controls=None, math=None):
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")                     # find_mu_mup, reference library.py:225-226
    f, e = np.broadcast_arrays(np.asarray(f0_Hz, dtype=np.float64), np.asarray(elevation_deg, dtype=np.float64))
    f = np.ascontiguousarray(f).reshape(-1)
    e = np.ascontiguousarray(e).reshape(-1)
    d2, b2, p2 = (np.atleast_2d(_as_rows(n, x)) for n, x in (("Ne", Ne), ("Babs", Babs), ("bpsi", bpsi)))
    if not (d2.shape == b2.shape == p2.shape):
        raise ValueError("Ne, Babs and bpsi must have the same shape")
    n_prof, n_alt = d2.shape
    a = _as_rows("alt_km", alt_km)
    if a.shape[-1] != n_alt or (a.ndim == 2 and a.shape[0] != n_prof):
        raise ValueError("alt_km must have one value per level")
    idx = None
    if profile_index is not None:
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(profile_index, dtype=np.int64), f.shape))
    elif n_prof != 1:
        raise ValueError("profile_index is needed when several profiles are given")
    out = np.empty((f.size, 8), dtype=np.float64)
    stride = 2 * n_alt + 1
    px = np.empty((f.size, stride), dtype=np.float64) if return_paths else None
    pz = np.empty((f.size, stride), dtype=np.float64) if return_paths else None
    ctx = _native.host_context(device)
    ctx.set_math(MATH_AUTO if math is None else int(math))
    common = (f.ctypes.data, e.ctypes.data, idx.ctypes.data if idx is not None else None, f.size, d2.ctypes.data,
              b2.ctypes.data, p2.ctypes.data, a.ctypes.data, n_prof, n_alt, n_alt if a.ndim == 2 else 0,
              _native.MODE_O if mode == "O" else _native.MODE_X)
    tail = (out.ctypes.data, px.ctypes.data if return_paths else None, pz.ctypes.data if return_paths else None,
            stride, 0)
    rc = ctx.snell_spherical(*common, *controls, *tail) if spherical else ctx.snell_cartesian(*common, *tail)
    _native.raise_for(rc)
    res = {k: out[:, i].copy() for i, k in enumerate(_KEYS)}
    res["n_path"] = res["n_path"].astype(np.int64)
    if return_paths:
        res["x"], res["z"] = px, pz
    return res


def _trace_fan(spherical, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, return_paths, device, controls, math=None):
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")
    f = np.ascontiguousarray(np.atleast_1d(np.asarray(f0_Hz, dtype=np.float64)))
    e = np.ascontiguousarray(np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64)))
    if f.ndim != 1 or e.ndim != 1:
        raise ValueError("f0_Hz and elevation_deg must be 1-D (frequencies, elevations of the fan)")
    single = np.ndim(Ne) == 1
    d2, b2, p2 = (np.atleast_2d(_as_rows(n, x)) for n, x in (("Ne", Ne), ("Babs", Babs), ("bpsi", bpsi)))
    if not (d2.shape == b2.shape == p2.shape):
        raise ValueError("Ne, Babs and bpsi must have the same shape")
    n_prof, n_alt = d2.shape
    a = _as_rows("alt_km", alt_km)
    if a.shape[-1] != n_alt or (a.ndim == 2 and a.shape[0] != n_prof):
        raise ValueError("alt_km must have one value per level")
    # groups: (profile, frequency) in C order; rays: (profile, frequency, elevation) in C order
    group_f = np.ascontiguousarray(np.tile(f, n_prof))
    group_p = np.ascontiguousarray(np.repeat(np.arange(n_prof, dtype=np.int64), f.size))
    n_groups = group_f.size
    ray_group = np.ascontiguousarray(np.repeat(np.arange(n_groups, dtype=np.int64), e.size))
    ray_e = np.ascontiguousarray(np.tile(e, n_groups))
    n_rays = ray_e.size
    out = np.empty((n_rays, 8), dtype=np.float64)
    stride = 2 * n_alt + 1
    px = np.empty((n_rays, stride), dtype=np.float64) if return_paths else None
    pz = np.empty((n_rays, stride), dtype=np.float64) if return_paths else None
    r_e, dz_t, boost, nsub = controls if spherical else (6371.0, 1.0, 200.0, 400)
    ctx = _native.host_context(device)
    ctx.set_math(MATH_AUTO if math is None else int(math))
    rc = ctx.snell_fan(1 if spherical else 0, group_f.ctypes.data, group_p.ctypes.data, n_groups, ray_group.ctypes.data,
                       ray_e.ctypes.data, n_rays, d2.ctypes.data, b2.ctypes.data, p2.ctypes.data, a.ctypes.data, n_prof,
                       n_alt, n_alt if a.ndim == 2 else 0, _native.MODE_O if mode == "O" else _native.MODE_X,
                       r_e, dz_t, boost, nsub, out.ctypes.data, px.ctypes.data if return_paths else None,
                       pz.ctypes.data if return_paths else None, stride, 0)
    _native.raise_for(rc)
    shape = (f.size, e.size) if single else (n_prof, f.size, e.size)
    res = {k: out[:, i].reshape(shape).copy() for i, k in enumerate(_KEYS)}
    res["n_path"] = res["n_path"].astype(np.int64)
    if return_paths:
        res["x"], res["z"] = px.reshape(shape + (stride,)), pz.reshape(shape + (stride,))
    return res


def trace_fan_cartesian_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, *, return_paths=False, device=None,
                               math=None):
    """Every elevation of ``elevation_deg`` ``(E,)`` for every frequency of ``f0_Hz`` ``(F,)`` (and every profile
    when ``Ne, Babs, bpsi`` are ``(P, N_alt)``), flat Earth.  Returns the dict of ``trace_rays_cartesian_snells``
    with arrays of shape ``(F, E)`` (or ``(P, F, E)``): the values the per-ray call gives for the same rays in the
    reference's operation order (``math=library.MATH_FAITHFUL``), to 1e-13; the level-by-level refractive index is evaluated once per (profile, frequency) instead of once
    per ray (``prhf_snell_fan_f64``)."""
    return _trace_fan(False, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, return_paths, device, None, math)


def trace_fan_spherical_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode="O", *, dz_target_km=1.0,
                               apex_boost=200.0, max_substeps=400, R_E=None, return_paths=False, device=None, math=None):
    """The same over a spherical Earth, with the reference's apex-refinement controls (library.py:1470-1473)."""
    r_e = constants()[2] if R_E is None else float(R_E)
    return _trace_fan(True, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, return_paths, device,
                      (r_e, dz_target_km, apex_boost, max_substeps), math)


HOME_STATUS_NAMES = {0: "converged", 1: "discontinuity", 2: "escapes inside", -1: "unused"}


def default_scan_elevations():
    """The homing calls' default scan grid: 2 to 88 degrees in steps of 0.25."""
    return np.linspace(2.0, 88.0, 345)


def _home_rays(spherical, f0_Hz, ground_range_km, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, max_roots,
               range_tol_km, max_iter, device, controls):
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")
    f = np.ascontiguousarray(np.atleast_1d(np.asarray(f0_Hz, dtype=np.float64)))
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(ground_range_km, dtype=np.float64)))
    if f.ndim != 1 or t.ndim != 1 or f.size == 0 or t.size == 0:
        raise ValueError("f0_Hz and ground_range_km must be 1-D and not empty (frequencies, target ranges)")
    scan = default_scan_elevations() if scan_elevation_deg is None else \
        np.ascontiguousarray(np.asarray(scan_elevation_deg, dtype=np.float64))
    if scan.ndim != 1 or scan.size < 2:
        raise ValueError("scan_elevation_deg needs at least 2 elevations")
    if not np.all(np.diff(scan) > 0):
        raise ValueError("scan_elevation_deg must be strictly increasing")
    max_roots, max_iter, range_tol_km = int(max_roots), int(max_iter), float(range_tol_km)
    if not 1 <= max_roots <= 64:
        raise ValueError("max_roots is 1 .. 64")
    if not 1 <= max_iter <= 128:
        raise ValueError("max_iter is 1 .. 128")
    if not (np.isfinite(range_tol_km) and range_tol_km >= 0.0):
        raise ValueError("range_tol_km must be finite and not negative")
    single = np.ndim(Ne) == 1
    d2, b2, p2 = (np.atleast_2d(_as_rows(n, x)) for n, x in (("Ne", Ne), ("Babs", Babs), ("bpsi", bpsi)))
    if not (d2.shape == b2.shape == p2.shape):
        raise ValueError("Ne, Babs and bpsi must have the same shape")
    n_prof, n_alt = d2.shape
    a = _as_rows("alt_km", alt_km)
    if a.shape[-1] != n_alt or (a.ndim == 2 and a.shape[0] != n_prof):
        raise ValueError("alt_km must have one value per level")
    if n_alt < 2:
        raise ValueError("a profile needs at least 2 levels")
    # groups: (profile, frequency) in C order; links: (profile, frequency, target) in C order
    group_f = np.ascontiguousarray(np.tile(f, n_prof))
    group_p = np.ascontiguousarray(np.repeat(np.arange(n_prof, dtype=np.int64), f.size))
    n_groups = group_f.size
    link_g = np.ascontiguousarray(np.repeat(np.arange(n_groups, dtype=np.int64), t.size))
    link_t = np.ascontiguousarray(np.tile(t, n_groups))
    n_links = link_g.size
    out = np.empty((n_links, max_roots, 11), dtype=np.float64)
    n_br = np.empty(n_links, dtype=np.int64)
    r_e, dz_t, boost, nsub = controls if spherical else (6371.0, 1.0, 200.0, 400)
    ctx = _native.host_context(device)
    rc = ctx.snell_home(1 if spherical else 0, group_f.ctypes.data, group_p.ctypes.data, n_groups, link_g.ctypes.data,
                        link_t.ctypes.data, n_links, scan.ctypes.data, scan.size, d2.ctypes.data, b2.ctypes.data,
                        p2.ctypes.data, a.ctypes.data, n_prof, n_alt, n_alt if a.ndim == 2 else 0,
                        _native.MODE_O if mode == "O" else _native.MODE_X, r_e, dz_t, boost, nsub, range_tol_km, max_iter,
                        max_roots, out.ctypes.data, n_br.ctypes.data, 0)
    _native.raise_for(rc)
    lead = (f.size, t.size) if single else (n_prof, f.size, t.size)
    out = out.reshape(lead + (max_roots, 11))
    res = {"n_brackets": n_br.reshape(lead), "elevation_deg": out[..., 0].copy(),
           "status": out[..., 1].astype(np.int64)}
    idx = out[..., 2]
    res["scan_index"] = np.where(np.isfinite(idx), idx, -1.0).astype(np.int64)
    for i, k in enumerate(_KEYS):
        res[k] = out[..., 3 + i].copy()
    n_path = res["n_path"]
    res["n_path"] = np.where(np.isfinite(n_path), n_path, 0.0).astype(np.int64)
    return res


def home_rays_cartesian_snells(f0_Hz, ground_range_km, alt_km, Ne, Babs, bpsi, mode, *, scan_elevation_deg=None,
                               max_roots=4, range_tol_km=1e-6, max_iter=64, device=None):
    """Point-to-point homing over a flat Earth: for every frequency of ``f0_Hz`` ``(F,)`` (and every profile when
    ``Ne, Babs, bpsi`` are ``(P, N_alt)``) and every target of ``ground_range_km`` ``(T,)``, the rays that land at that
    range - the oblique ionogram of the link (``prhf_snell_home_f64``).

    The fan of ``scan_elevation_deg`` (strictly increasing, default ``np.linspace(2, 88, 345)``) is traced once per
    (profile, frequency); an interval of the scan whose two rays land on either side of the target (or whose lower ray
    lands on it) is a bracket, and each of the first ``max_roots`` brackets in ascending elevation is narrowed with at
    most ``max_iter`` further rays.  What is found is a function of the scan grid: a tangential contact that causes no
    sign change on it is not found.

    Returns a dict: ``n_brackets`` ``([P,] F, T)`` - every bracket of the link, those beyond ``max_roots`` included -
    and, with shape ``([P,] F, T, max_roots)``, ``elevation_deg``, ``status``, ``scan_index`` (the bracket's interval)
    and the eight keys of ``trace_rays_cartesian_snells`` for the result ray.  ``status`` 0: the ray lands within
    ``range_tol_km`` of the target; 1: the ground range jumps across the target inside the bracket (a ray stops
    reflecting from a lower layer) - the ray given is the nearest one tried; 2: a ray inside the bracket does not
    turn; -1: unused slot (NaN everywhere, ``scan_index`` -1, ``n_path`` 0)."""
    return _home_rays(False, f0_Hz, ground_range_km, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, max_roots,
                      range_tol_km, max_iter, device, None)


def home_rays_spherical_snells(f0_Hz, ground_range_km, alt_km, Ne, Babs, bpsi, mode="O", *, scan_elevation_deg=None,
                               max_roots=4, range_tol_km=1e-6, max_iter=64, dz_target_km=1.0, apex_boost=200.0,
                               max_substeps=400, R_E=None, device=None):
    """The same over a spherical Earth, with the reference's apex-refinement controls (library.py:1470-1473)."""
    r_e = constants()[2] if R_E is None else float(R_E)
    return _home_rays(True, f0_Hz, ground_range_km, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, max_roots,
                      range_tol_km, max_iter, device, (r_e, dz_target_km, apex_boost, max_substeps))


SKIP_STATUS_NAMES = {0: "converged", 1: "edge of the scan", 2: "escapes inside", 3: "max_iter spent", -1: "no ray lands"}
MUF_STATUS_NAMES = {0: "bracketed", 1: "open at f_hi", 2: "unreachable at f_lo", -1: "no target"}


def _skip_arguments(alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, elev_tol_deg, max_iter):
    """The checks and conversions the skip-distance and MUF calls share; all before any native call."""
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")
    scan = default_scan_elevations() if scan_elevation_deg is None else \
        np.ascontiguousarray(np.asarray(scan_elevation_deg, dtype=np.float64))
    if scan.ndim != 1 or scan.size < 1:
        raise ValueError("scan_elevation_deg needs at least 1 elevation")
    if not (np.all(np.isfinite(scan)) and np.all(np.diff(scan) > 0)):
        raise ValueError("scan_elevation_deg must be finite and strictly increasing")
    max_iter, elev_tol_deg = int(max_iter), float(elev_tol_deg)
    if not 1 <= max_iter <= 128:
        raise ValueError("max_iter is 1 .. 128")
    if not (np.isfinite(elev_tol_deg) and elev_tol_deg >= 0.0):
        raise ValueError("elev_tol_deg must be finite and not negative")
    d2, b2, p2 = (np.atleast_2d(_as_rows(n, x)) for n, x in (("Ne", Ne), ("Babs", Babs), ("bpsi", bpsi)))
    if not (d2.shape == b2.shape == p2.shape):
        raise ValueError("Ne, Babs and bpsi must have the same shape")
    n_prof, n_alt = d2.shape
    a = _as_rows("alt_km", alt_km)
    if a.shape[-1] != n_alt or (a.ndim == 2 and a.shape[0] != n_prof):
        raise ValueError("alt_km must have one value per level")
    if n_alt < 2:
        raise ValueError("a profile needs at least 2 levels")
    return scan, elev_tol_deg, max_iter, a, d2, b2, p2


def _skip_row(out, res, first):
    """The 13 values of a skip row, out[..., first:first + 13], into the dict under the public names."""
    res["elevation_deg"] = out[..., first].copy()
    idx, n_evals = out[..., first + 2], out[..., first + 4]
    res["scan_index"] = np.where(np.isfinite(idx), idx, -1.0).astype(np.int64)
    res["bracket_deg"] = out[..., first + 3].copy()
    res["n_evals"] = np.where(np.isfinite(n_evals), n_evals, 0.0).astype(np.int64)
    for i, k in enumerate(_KEYS):
        res[k] = out[..., first + 5 + i].copy()
    res["skip_km"] = res["ground_range_km"].copy()
    n_path = res["n_path"]
    res["n_path"] = np.where(np.isfinite(n_path), n_path, 0.0).astype(np.int64)
    status = out[..., first + 1]
    return np.where(np.isfinite(status), status, -1.0).astype(np.int64)


def _skip_distance(spherical, f0_Hz, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, elev_tol_deg, max_iter, device,
                   controls):
    scan, elev_tol_deg, max_iter, a, d2, b2, p2 = _skip_arguments(alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg,
                                                                   elev_tol_deg, max_iter)
    f = np.ascontiguousarray(np.atleast_1d(np.asarray(f0_Hz, dtype=np.float64)))
    if f.ndim != 1 or f.size == 0:
        raise ValueError("f0_Hz must be 1-D and not empty (frequencies)")
    single = np.ndim(Ne) == 1
    n_prof, n_alt = d2.shape
    # groups: (profile, frequency) in C order
    group_f = np.ascontiguousarray(np.tile(f, n_prof))
    group_p = np.ascontiguousarray(np.repeat(np.arange(n_prof, dtype=np.int64), f.size))
    out = np.empty((group_f.size, 13), dtype=np.float64)
    r_e, dz_t, boost, nsub = controls if spherical else (6371.0, 1.0, 200.0, 400)
    ctx = _native.host_context(device)
    rc = ctx.snell_skip(1 if spherical else 0, group_f.ctypes.data, group_p.ctypes.data, group_f.size, scan.ctypes.data,
                        scan.size, d2.ctypes.data, b2.ctypes.data, p2.ctypes.data, a.ctypes.data, n_prof, n_alt,
                        n_alt if a.ndim == 2 else 0, _native.MODE_O if mode == "O" else _native.MODE_X, r_e, dz_t, boost,
                        nsub, elev_tol_deg, max_iter, out.ctypes.data, 0)
    _native.raise_for(rc)
    out = out.reshape(((f.size,) if single else (n_prof, f.size)) + (13,))
    res = {}
    res["status"] = _skip_row(out, res, 0)
    return res


def skip_distance_cartesian_snells(f0_Hz, alt_km, Ne, Babs, bpsi, mode, *, scan_elevation_deg=None, elev_tol_deg=1e-6,
                                   max_iter=64, device=None):
    """Skip distance over a flat Earth: for every frequency of ``f0_Hz`` ``(F,)`` (and every profile when
    ``Ne, Babs, bpsi`` are ``(P, N_alt)``) the smallest ground range any ray of the scan reaches, refined
    (``prhf_snell_skip_f64``).

    The fan of ``scan_elevation_deg`` (strictly increasing, at least one elevation, default ``np.linspace(2, 88, 345)``)
    is traced once per (profile, frequency); ``scan_index`` is the first node that attains the smallest finite ground
    range.  A node at either end of the scan, or beside a ray that does not turn, is returned as it stands (``status``
    1: no skip zone inside the scan, or the minimum sits beside penetration).  Otherwise a golden-section search between
    the node's two neighbours traces at most ``max_iter`` further rays until the bracket is ``elev_tol_deg`` wide or
    cannot be split in float64 (``status`` 0), ``max_iter`` is spent (3) or a ray inside the bracket escapes (2); the
    result is the ray with the smallest ground range seen.  ``status`` -1: no ray of the scan lands (NaN everywhere,
    ``scan_index`` -1, ``n_path`` 0).  What is found is a function of the scan grid.

    Returns a dict of ``([P,] F)`` arrays: ``skip_km``, ``elevation_deg``, ``status`` (``SKIP_STATUS_NAMES``),
    ``scan_index``, ``bracket_deg`` (width of the final bracket, NaN for status 1), ``n_evals`` (rays the search traced)
    and the eight keys of ``trace_rays_cartesian_snells`` for the result ray - bit for bit what the fan call gives at
    ``elevation_deg``; ``skip_km`` is its ``ground_range_km``."""
    return _skip_distance(False, f0_Hz, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, elev_tol_deg, max_iter, device,
                          None)


def skip_distance_spherical_snells(f0_Hz, alt_km, Ne, Babs, bpsi, mode="O", *, scan_elevation_deg=None, elev_tol_deg=1e-6,
                                   max_iter=64, dz_target_km=1.0, apex_boost=200.0, max_substeps=400, R_E=None,
                                   device=None):
    """The same over a spherical Earth, with the reference's apex-refinement controls (library.py:1470-1473)."""
    r_e = constants()[2] if R_E is None else float(R_E)
    return _skip_distance(True, f0_Hz, alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg, elev_tol_deg, max_iter, device,
                          (r_e, dz_target_km, apex_boost, max_substeps))


def _muf(spherical, ground_range_km, f_lo_Hz, f_hi_Hz, alt_km, Ne, Babs, bpsi, mode, n_bisect, scan_elevation_deg,
         elev_tol_deg, max_iter, device, controls):
    scan, elev_tol_deg, max_iter, a, d2, b2, p2 = _skip_arguments(alt_km, Ne, Babs, bpsi, mode, scan_elevation_deg,
                                                                   elev_tol_deg, max_iter)
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(ground_range_km, dtype=np.float64)))
    if t.ndim != 1 or t.size == 0:
        raise ValueError("ground_range_km must be 1-D and not empty (target ranges)")
    f_lo, f_hi, n_bisect = float(f_lo_Hz), float(f_hi_Hz), int(n_bisect)
    if not (np.isfinite(f_lo) and np.isfinite(f_hi) and 0.0 < f_lo < f_hi):
        raise ValueError("the frequency bracket needs 0 < f_lo_Hz < f_hi_Hz, both finite")
    if not 1 <= n_bisect <= 64:
        raise ValueError("n_bisect is 1 .. 64")
    single = np.ndim(Ne) == 1
    n_prof, n_alt = d2.shape
    # links: (profile, target) in C order
    link_p = np.ascontiguousarray(np.repeat(np.arange(n_prof, dtype=np.int64), t.size))
    link_t = np.ascontiguousarray(np.tile(t, n_prof))
    out = np.empty((link_t.size, 16), dtype=np.float64)
    r_e, dz_t, boost, nsub = controls if spherical else (6371.0, 1.0, 200.0, 400)
    ctx = _native.host_context(device)
    rc = ctx.snell_muf(1 if spherical else 0, link_p.ctypes.data, link_t.ctypes.data, link_t.size, f_lo, f_hi, n_bisect,
                       scan.ctypes.data, scan.size, d2.ctypes.data, b2.ctypes.data, p2.ctypes.data, a.ctypes.data, n_prof,
                       n_alt, n_alt if a.ndim == 2 else 0, _native.MODE_O if mode == "O" else _native.MODE_X, r_e, dz_t,
                       boost, nsub, elev_tol_deg, max_iter, out.ctypes.data, 0)
    _native.raise_for(rc)
    out = out.reshape(((t.size,) if single else (n_prof, t.size)) + (16,))
    res = {"muf_hz": out[..., 0].copy(), "f_above_hz": out[..., 1].copy(), "status": out[..., 2].astype(np.int64)}
    res["skip_status"] = _skip_row(out, res, 3)
    return res


def muf_cartesian_snells(ground_range_km, f_lo_Hz, f_hi_Hz, alt_km, Ne, Babs, bpsi, mode, *, n_bisect=40,
                         scan_elevation_deg=None, elev_tol_deg=1e-6, max_iter=64, device=None):
    """MUF (junction frequency) of links over a flat Earth: for every target of ``ground_range_km`` ``(T,)`` (and
    every profile when ``Ne, Babs, bpsi`` are ``(P, N_alt)``) the frequency in ``[f_lo_Hz, f_hi_Hz]`` at which the skip
    distance ``S(f)`` of ``skip_distance_cartesian_snells`` (same column, mode, scan and controls; +inf when no ray
    lands) reaches the target (``prhf_snell_muf_f64``).

    ``status`` (``MUF_STATUS_NAMES``) -1: the target is NaN; 2: ``S(f_lo) > t``, the link is unreachable even at
    ``f_lo_Hz`` (both: NaN everywhere else); 1: ``S(f_hi) <= t``, the link is open at ``f_hi_Hz``, which is returned with
    its skip row (``f_above_hz`` NaN); 0: ``S(f_lo) <= t < S(f_hi)`` and ``n_bisect`` (1 .. 64) halvings of the frequency
    bracket, ``m = lo + 0.5 (hi - lo)``, ``lo = m`` when ``S(m) <= t`` and ``hi = m`` otherwise, give ``muf_hz = lo`` and
    ``f_above_hz = hi`` with ``S(muf_hz) <= t < S(f_above_hz)`` - also where ``S`` is not monotone: the rule says which
    crossing is found.

    Returns a dict of ``([P,] T)`` arrays: ``muf_hz``, ``f_above_hz``, ``status`` and the skip call's results at
    ``muf_hz`` (``skip_km``, ``elevation_deg``, ``skip_status``, ``scan_index``, ``bracket_deg``, ``n_evals`` and the
    eight ray keys).  All trips run inside one native call; with few links few wavefronts are resident and the call is
    bound by the latency of its chain of kernels."""
    return _muf(False, ground_range_km, f_lo_Hz, f_hi_Hz, alt_km, Ne, Babs, bpsi, mode, n_bisect, scan_elevation_deg,
                elev_tol_deg, max_iter, device, None)


def muf_spherical_snells(ground_range_km, f_lo_Hz, f_hi_Hz, alt_km, Ne, Babs, bpsi, mode="O", *, n_bisect=40,
                         scan_elevation_deg=None, elev_tol_deg=1e-6, max_iter=64, dz_target_km=1.0, apex_boost=200.0,
                         max_substeps=400, R_E=None, device=None):
    """The same over a spherical Earth, with the reference's apex-refinement controls (library.py:1470-1473)."""
    r_e = constants()[2] if R_E is None else float(R_E)
    return _muf(True, ground_range_km, f_lo_Hz, f_hi_Hz, alt_km, Ne, Babs, bpsi, mode, n_bisect, scan_elevation_deg,
                elev_tol_deg, max_iter, device, (r_e, dz_target_km, apex_boost, max_substeps))


def _single(r, apex_keys):
    n = int(r["n_path"][0])
    if n == 0:
        return {k: np.nan for k in _DICT_KEYS + (("x_apex_km", "z_apex_km") if apex_keys else ())}
    return {"x": r["x"][0, :n].copy(), "z": r["z"][0, :n].copy(),
            "group_path_km": float(r["group_path_km"][0]), "group_delay_sec": float(r["group_delay_sec"][0]),
            "x_midpoint": float(r["x_midpoint"][0]), "z_midpoint": float(r["z_midpoint"][0]),
            "ground_range_km": float(r["ground_range_km"][0]),
            "x_apex_km": float(r["x_midpoint"][0]), "z_apex_km": float(r["z_midpoint"][0])}


def trace_rays_cartesian_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, *, profile_index=None,
                                return_paths=False, device=None, math=None):
    """Trace ``R`` rays over a flat Earth; ``f0_Hz`` and ``elevation_deg`` broadcast to ``(R,)``.

    ``Ne, Babs, bpsi`` are ``(N_alt,)`` or ``(P, N_alt)`` with ``profile_index`` ``(R,)`` choosing the
    column of each ray; ``alt_km`` ``(N_alt,)`` or ``(P, N_alt)``.  Returns a dict of ``(R,)`` arrays:
    the reference's ``group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km`` plus the
    turning point ``x_turn_km, z_turn_km`` and ``n_path``; NaN for rays that never turn.  With
    ``return_paths`` also ``x`` and ``z``: ``(R, 2 N_alt + 1)`` padded with NaN.

    ``x_midpoint, z_midpoint``: the reference's search (library.py:1248-1252) lands on the path node before the apex
    or - one rounding away, for one ray in three - on the apex; here always the node before the apex, its
    exact-arithmetic answer (the apex itself is ``x_turn_km, z_turn_km``).

    ``math``: None (default) evaluates the refractive index of a level in the reduced algebra where that cannot move a
    result - far from reflection and from the ray's turning point - and in the reference's operation order elsewhere
    (within 1e-10 of ``library.MATH_FAITHFUL`` - on a spherical Earth one ray in a few million, at the edge of a skip
    zone, up to 3e-10 - which keeps the reference's order at every level and agrees with reference-run rays to 1e-12;
    about three times the time).  Fans always read faithful level tables.
    """
    return _trace_rays(False, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, profile_index, return_paths,
                       device, math=math)


def trace_rays_spherical_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode="O", *, dz_target_km=1.0,
                                apex_boost=200.0, max_substeps=400, R_E=None, profile_index=None,
                                return_paths=False, device=None, math=None):
    """The same over a spherical Earth (Bouguer's law), with the reference's apex-refinement controls
    (library.py:1470-1473); ``x`` is the ground distance ``R_E * phi``."""
    r_e = constants()[2] if R_E is None else float(R_E)
    return _trace_rays(True, f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, profile_index, return_paths, device,
                       controls=(r_e, dz_target_km, apex_boost, max_substeps), math=math)


def trace_ray_cartesian_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode, *, device=None, math=None):
    """One ray; the reference's signature and result dict (library.py:1096-1268):
    ``x, z`` (path arrays), ``group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km,
    x_apex_km, z_apex_km`` (the apex entries repeat the midpoint, as in the reference).  A ray that
    never turns returns NaN for every entry."""
    r = trace_rays_cartesian_snells(np.float64(f0_Hz), np.float64(elevation_deg), alt_km, Ne, Babs, bpsi, mode,
                                    return_paths=True, device=device, math=math)
    return _single(r, apex_keys=True)


def trace_ray_spherical_snells(f0_Hz, elevation_deg, alt_km, Ne, Babs, bpsi, mode="O", *, dz_target_km=1.0,
                               apex_boost=200.0, max_substeps=400, R_E=None, device=None, math=None):
    """One ray over a spherical Earth; the reference's signature and result dict (library.py:1460-1713).
    A ray that never turns returns the reference's seven-key NaN dict (library.py:1577-1583)."""
    r = trace_rays_spherical_snells(np.float64(f0_Hz), np.float64(elevation_deg), alt_km, Ne, Babs, bpsi, mode,
                                    dz_target_km=dz_target_km, apex_boost=apex_boost, max_substeps=max_substeps,
                                    R_E=R_E, return_paths=True, device=device, math=math)
    return _single(r, apex_keys=False)


def tan_from_mu_scalar(mu_val, p):
    """Tangent of the ray's angle to the vertical where the phase index is ``mu_val`` and the Snell invariant ``p``
    (reference ``library.py:1034-1062``): ``p / sqrt(max(mu_val**2 - p**2, 1e-10))``.  A host helper beside the
    tracers, which apply the same rule inside the kernel; array arguments broadcast."""
    mu_val = np.asarray(mu_val, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    out = p / np.sqrt(np.maximum(mu_val * mu_val - p * p, 1e-10))
    return float(out) if out.ndim == 0 else out


def find_turning_point(z, mu, p):
    """Altitude at which ``mu`` falls through the Snell invariant ``p``: the first pair of neighbouring nodes with
    ``mu[i] >= p >= mu[i + 1]``, linear in between, NaN when there is none (reference ``library.py:1065-1093``)."""
    z = np.asarray(z, dtype=np.float64).ravel()
    mu = np.asarray(mu, dtype=np.float64).ravel()
    hit = np.nonzero((mu[:-1] >= p) & (mu[1:] <= p))[0]
    if hit.size == 0:
        return float("nan")
    i = int(hit[0])
    if mu[i] == mu[i + 1]:
        return float(z[i])
    return float(z[i] + ((mu[i] - p) / (mu[i] - mu[i + 1])) * (z[i + 1] - z[i]))
