"""2-D refractive-index fields and the gradient ray tracers of both geometries on the GPU (SURVEY.md section 2, rows 10
and 11).

``build_refractive_index_interpolator_cartesian``, ``build_refractive_index_interpolator_spherical`` and
``build_mup_function`` keep the reference's signatures, defaults and error messages (reference
``PyRayHF/library.py:1755-2017``) and return callable objects with the reference's call conventions that evaluate on
the GPU: the grid values live on the device as node records {mu, d mu/d a1, d mu/d a0, mu'} (``prhf_field_pack_f64``:
``np.gradient`` bit for bit) and a call samples them with ``RegularGridInterpolator``'s linear rule
(``prhf_field_sample_f64``).  ``refractive_field`` builds the records of many frequencies in one go from the existing
GPU ``find_mu_mup``.

``trace_ray_cartesian_gradient`` is the reference's single-ray call (``:1270-1457``; the dict lacks ``'sol'``);
``trace_rays_cartesian_gradient`` / ``trace_fan_cartesian_gradient`` trace a batch / a fan of elevations for every field
in one launch, one ray per lane (``prhf_trace_gradient_f64``).  ``trace_ray_spherical_gradient``,
``trace_rays_spherical_gradient`` and ``trace_fan_spherical_gradient`` are the same over a spherical Earth
(``:2128-2337``, ``prhf_trace_gradient_spherical_f64``) with the stop conditions DESIGN.md section 4.7 defines: the
reference's own wiring of its event helpers cannot fire.

Limitations: a tracer reads mu and mu' from ONE set of records, so the ``n_and_grad`` and ``mup_func`` objects given to
``trace_ray_cartesian_gradient`` / ``trace_ray_spherical_gradient`` must have been built on the same ``z_grid`` and
``x_grid`` - and the same ``R_E`` - (``ValueError`` otherwise), and both must come from this module (``TypeError``
otherwise: there is no CPU path).  A field knows its geometry; a tracer refuses a field of the other one.
"""

from __future__ import annotations

import numpy as np

from . import _native
from .library import constants, find_mu_mup, find_X, find_Y

_MODE_CODE = {"O": _native.MODE_O, "X": _native.MODE_X}

__all__ = ["build_refractive_index_interpolator_cartesian", "build_refractive_index_interpolator_spherical",
           "build_mup_function", "refractive_field", "RefractiveField", "trace_ray_cartesian_gradient",
           "trace_rays_cartesian_gradient", "trace_fan_cartesian_gradient", "trace_ray_spherical_gradient",
           "trace_rays_spherical_gradient", "trace_fan_spherical_gradient", "home_rays_cartesian_gradient",
           "home_rays_spherical_gradient", "refractive_field_device", "skip_distance_cartesian_gradient",
           "skip_distance_spherical_gradient", "muf_cartesian_gradient", "muf_spherical_gradient", "STATUS_NAMES",
           "trace_hops_cartesian_gradient", "trace_hops_spherical_gradient", "trace_hop_fan_cartesian_gradient",
           "trace_hop_fan_spherical_gradient", "home_hops_cartesian_gradient", "home_hops_spherical_gradient",
           "skip_distance_hops_cartesian_gradient", "skip_distance_hops_spherical_gradient",
           "muf_hops_cartesian_gradient", "muf_hops_spherical_gradient"]

STATUS_NAMES = ("ground", "domain", "length", "failure")          # reference library.py:1391-1398
_KEYS = ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_apex_km", "z_apex_km",
         "status", "n_nodes", "n_rhs", "n_rejected")
_INT_KEYS = ("status", "n_nodes", "n_rhs", "n_rejected")
_PATH_KEYS = ("t", "x", "z", "vx", "vz")
_PATH_KEYS_SPHERICAL = ("t", "r", "phi", "v_r", "v_phi")
_MAX_AXES = 8000
_MAX_HOPS = 16
_HOP_LAUNCH_KEYS = ("launch_x_km", "launch_z_km", "launch_elevation_deg")


class RefractiveField:
    """``F`` fields mu, mu' on one grid: the device-resident node records the sampler and the tracer read.

    ``mu, mup``: ``(F, n0, n1)`` (or ``(n0, n1)``) on ``axis0`` (altitude, or radius) and ``axis1`` (distance, or
    angle).  ``geometry`` says which: ``"cartesian"`` (the default), or ``"spherical"`` with the Earth radius ``R_E``
    (default ``constants()[2]``) that made the axes ``R_E + z`` and ``x / R_E``; the tracers check it, the sampler does
    not care.  The records are packed on first use, so that building a field needs no GPU."""

    def __init__(self, axis0, axis1, mu, mup, *, edge_order=2, device=None, fill_n=np.nan, fill_grad=0.0,
                 fill_mup=np.nan, geometry="cartesian", R_E=None):
        if geometry not in ("cartesian", "spherical"):
            raise ValueError("geometry must be 'cartesian' or 'spherical'")
        self.geometry = geometry
        self.R_E = None if geometry == "cartesian" else float(constants()[2] if R_E is None else R_E)
        self.axis0 = np.ascontiguousarray(axis0, dtype=np.float64)
        self.axis1 = np.ascontiguousarray(axis1, dtype=np.float64)
        mu = np.asarray(mu, dtype=np.float64)
        mup = np.asarray(mup, dtype=np.float64)
        if mu.ndim == 2:
            mu, mup = mu[None], mup[None]
        if mu.ndim != 3 or mu.shape != mup.shape or mu.shape[1:] != (self.axis0.size, self.axis1.size):
            raise ValueError("mu and mup must have shape (F, len(axis0), len(axis1))")
        if edge_order not in (1, 2):
            raise ValueError("'edge_order' greater than 2 not supported")          # np.gradient's message
        if min(mu.shape[1:]) < edge_order + 1:
            raise ValueError("Shape of array too small to calculate a numerical gradient, "
                             "at least (edge_order + 1) elements are required.")
        if self.axis0.size + self.axis1.size > _MAX_AXES:
            raise ValueError(f"the two axes hold at most {_MAX_AXES} values together")
        self.mu = np.ascontiguousarray(mu)
        self.mup = np.ascontiguousarray(mup)
        self.edge_order = int(edge_order)
        self.device = device
        self.fills = (float(fill_n), float(fill_grad), float(fill_mup))
        self._rec = None

    @property
    def n_fields(self):
        return self.mu.shape[0]

    def _ctx(self):
        return _native.host_context(self.device)

    def records(self):
        """The ``(F, n0, n1, 4)`` records as a device tensor (packed on first use)."""
        if self._rec is None:
            import torch
            ctx = self._ctx()
            rec = torch.empty(self.mu.shape + (4,), dtype=torch.float64, device=f"cuda:{ctx.device}")
            _native.raise_for(ctx.field_pack(self.mu.ctypes.data, self.mup.ctypes.data, self.n_fields, self.axis0.size,
                                             self.axis1.size, self.axis0.ctypes.data, self.axis1.ctypes.data,
                                             self.edge_order, rec.data_ptr(), 0))
            self._rec = rec
        return self._rec

    def sample(self, p0, p1, field_index=None, want=(True, True, True, True), fills=None):
        """mu, d mu/d a1, d mu/d a0, mu' (those asked for, else None) at the points ``(p0, p1)`` (flat arrays)."""
        p0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1)
        p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1)
        idx = None
        if field_index is not None:
            idx = np.ascontiguousarray(np.broadcast_to(np.asarray(field_index, dtype=np.int64), p0.shape))
        outs = [np.empty(p0.size, dtype=np.float64) if w else None for w in want]
        if p0.size:
            rec = self.records()
            _native.raise_for(self._ctx().field_sample(
                rec.data_ptr(), self.n_fields, self.axis0.size, self.axis1.size, self.axis0.ctypes.data,
                self.axis1.ctypes.data, p0.ctypes.data, p1.ctypes.data, idx.ctypes.data if idx is not None else None,
                p0.size, self.fills if fills is None else fills, [o.ctypes.data if o is not None else None for o in outs], 0))
        return outs

    def same_grid(self, other):
        return np.array_equal(self.axis0, other.axis0) and np.array_equal(self.axis1, other.axis1)


def _check_bounds(grids, pts):
    """``bounds_error=True``: RegularGridInterpolator's test and message."""
    for i, (g, p) in enumerate(zip(grids, pts)):
        if not np.logical_and(np.all(g[0] <= p), np.all(p <= g[-1])):
            raise ValueError("One of the requested xi is out of bounds in dimension %d" % i)


class _NAndGrad:
    """``(x, z) -> (n, dndx, dndz)`` (Cartesian) or ``(phi, r) -> (mu, dmu/dr, dmu/dphi)`` (spherical)."""

    def __init__(self, field, geometry, bounds_error, z_grid, x_grid):
        self.field = field
        self.geometry = geometry
        self.bounds_error = bool(bounds_error)
        self.z_grid, self.x_grid = z_grid, x_grid
        self._with_mup = {}

    def __call__(self, first, second):
        a1 = np.atleast_1d(np.asarray(first, dtype=float))
        a0 = np.atleast_1d(np.asarray(second, dtype=float))
        a1, a0 = np.broadcast_arrays(a1, a0)
        if self.bounds_error:
            _check_bounds((self.field.axis0, self.field.axis1), (a0.ravel(), a1.ravel()))
        n, d1, d0, _ = self.field.sample(a0, a1, want=(True, True, True, False))
        shape = a1.shape
        if self.geometry == "cartesian":
            return n.reshape(shape), d1.reshape(shape), d0.reshape(shape)
        return n.reshape(shape), d0.reshape(shape), d1.reshape(shape)


class _MupFunction:
    """``(x, z) -> mu'``."""

    def __init__(self, field, geometry, bounds_error, R_E, z_grid, x_grid):
        self.field = field
        self.geometry = geometry
        self.bounds_error = bool(bounds_error)
        self.R_E = R_E
        self.z_grid, self.x_grid = z_grid, x_grid

    def __call__(self, x, z):
        if self.geometry == "cartesian":
            a0, a1 = np.ravel(z), np.ravel(x)
        else:
            a0, a1 = (self.R_E + np.asarray(z)).ravel(), (np.asarray(x) / self.R_E).ravel()
        a0 = np.asarray(a0, dtype=float)
        a1 = np.asarray(a1, dtype=float)
        if a0.shape != a1.shape:
            raise ValueError("x and z must have the same number of elements")
        if self.bounds_error:
            _check_bounds((self.field.axis0, self.field.axis1), (a0, a1))
        mup = self.field.sample(a0, a1, want=(False, False, False, True))[3]
        return mup.reshape(np.shape(x))


def build_refractive_index_interpolator_cartesian(z_grid, x_grid, n_field, *, fill_value_n=np.nan, fill_value_grad=0.0,
                                                  bounds_error=False, edge_order=2, device=None):
    """The reference's builder (library.py:1755-1835): a callable ``(x, z) -> (n, dndx, dndz)`` that samples mu and
    ``np.gradient(n_field, z_grid, x_grid, edge_order=edge_order)`` linearly on the GPU."""
    z_grid = np.asarray(z_grid, dtype=float)
    x_grid = np.asarray(x_grid, dtype=float)
    n_field = np.asarray(n_field, dtype=float)
    if n_field.shape != (z_grid.size, x_grid.size):
        raise ValueError(f"`n_field` must have shape (len(z_grid)={z_grid.size}, len(x_grid)={x_grid.size}), "
                         f"got {n_field.shape}.")
    if not (np.all(np.diff(z_grid) > 0) and np.all(np.diff(x_grid) > 0)):
        raise ValueError("`z_grid` and `x_grid` must be strictly increasing.")
    field = RefractiveField(z_grid, x_grid, n_field, np.full_like(n_field, np.nan), edge_order=edge_order, device=device,
                            fill_n=fill_value_n, fill_grad=fill_value_grad, geometry="cartesian")
    return _NAndGrad(field, "cartesian", bounds_error, z_grid, x_grid)


def build_refractive_index_interpolator_spherical(z_grid, x_grid, n_field, *, fill_value_n=np.nan, fill_value_grad=0.0,
                                                  bounds_error=False, R_E=None, edge_order=2, device=None):
    """The reference's builder (library.py:1838-1927): a callable ``(phi, r) -> (mu, dmu/dr, dmu/dphi)`` on the grid
    ``r = R_E + z_grid``, ``phi = x_grid / R_E``."""
    x_grid = np.asarray(x_grid, dtype=float)
    z_grid = np.asarray(z_grid, dtype=float)
    n_field = np.asarray(n_field, dtype=float)
    if R_E is None:
        R_E = constants()[2]
    r_grid = R_E + z_grid
    phi_grid = x_grid / R_E
    if n_field.shape != (r_grid.size, phi_grid.size):
        raise ValueError(f"`n_field` shape {n_field.shape} must be "
                         f"(len(r_grid)={r_grid.size}, len(phi_grid)={phi_grid.size}).")
    if not (np.all(np.diff(r_grid) > 0) and np.all(np.diff(phi_grid) > 0)):
        raise ValueError("`r_grid` and `phi_grid` must be strictly increasing.")
    field = RefractiveField(r_grid, phi_grid, n_field, np.full_like(n_field, np.nan), edge_order=edge_order,
                            device=device, fill_n=fill_value_n, fill_grad=fill_value_grad, geometry="spherical", R_E=R_E)
    return _NAndGrad(field, "spherical", bounds_error, z_grid, x_grid)


def build_mup_function(mup_field, x_grid, z_grid, *, geometry="cartesian", R_E=None, bounds_error=False,
                       fill_value=np.nan, device=None):
    """The reference's builder (library.py:1930-2017): a callable ``(x, z) -> mu'`` (both geometries take x and z in km)."""
    if R_E is None:
        R_E = constants()[2]
    if geometry not in ("cartesian", "spherical"):
        raise ValueError("geometry must be 'cartesian' or 'spherical'")
    x_grid = np.asarray(x_grid, dtype=float)
    z_grid = np.asarray(z_grid, dtype=float)
    mup_field = np.asarray(mup_field, dtype=float)
    axis0, axis1 = (z_grid, x_grid) if geometry == "cartesian" else (R_E + z_grid, x_grid / R_E)
    # RegularGridInterpolator's own checks (it is what the reference hands the grids to)
    for i, g in enumerate((axis0, axis1)):
        if g.ndim != 1 or not np.all(np.diff(g) > 0):
            raise ValueError(f"The points in dimension {i} must be strictly ascending")
    if mup_field.ndim != 2:
        raise ValueError(f"There are 2 point arrays, but values has {mup_field.ndim} dimensions")
    for i, g in enumerate((axis0, axis1)):
        if mup_field.shape[i] != g.size:
            raise ValueError(f"There are {g.size} points and {mup_field.shape[i]} values in dimension {i}")
    field = RefractiveField(axis0, axis1, mup_field, mup_field, edge_order=1, device=device, fill_mup=fill_value,
                            geometry=geometry, R_E=R_E)
    return _MupFunction(field, geometry, bounds_error, R_E, z_grid, x_grid)


def refractive_field(f0_Hz, Ne, Babs, bpsi, z_grid, x_grid, mode, geometry="cartesian", *, R_E=None, edge_order=2,
                     fill_value_n=np.nan, fill_value_grad=0.0, fill_value_mup=np.nan, device=None):
    """``F`` fields for the frequencies ``f0_Hz`` ``(F,)`` from one 2-D ionosphere ``Ne, Babs, bpsi`` ``(nz, nx)``:
    mu and mu' by the GPU ``find_mu_mup`` (one call per frequency, so that the reference's isotropic rule
    ``nanmax|Y| < 1e-12`` applies per frequency as it would to that frequency's arrays), then the records.
    Returns a ``RefractiveField`` on ``(z_grid, x_grid)`` - or ``(R_E + z_grid, x_grid / R_E)`` for
    ``geometry="spherical"`` - for ``trace_rays_cartesian_gradient`` / ``trace_fan_cartesian_gradient`` - or
    ``trace_rays_spherical_gradient`` / ``trace_fan_spherical_gradient`` - and the ``sample`` method."""
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")
    if geometry not in ("cartesian", "spherical"):
        raise ValueError("geometry must be 'cartesian' or 'spherical'")
    f = np.atleast_1d(np.asarray(f0_Hz, dtype=np.float64))
    z_grid = np.asarray(z_grid, dtype=float)
    x_grid = np.asarray(x_grid, dtype=float)
    Ne, Babs, bpsi = (np.asarray(v, dtype=np.float64) for v in (Ne, Babs, bpsi))
    if f.ndim != 1 or not (Ne.shape == Babs.shape == bpsi.shape == (z_grid.size, x_grid.size)):
        raise ValueError("f0_Hz must be 1-D and Ne, Babs, bpsi of shape (len(z_grid), len(x_grid))")
    if not (np.all(np.diff(z_grid) > 0) and np.all(np.diff(x_grid) > 0)):
        raise ValueError("`z_grid` and `x_grid` must be strictly increasing.")
    mu = np.empty((f.size,) + Ne.shape)
    mup = np.empty_like(mu)
    for k, fk in enumerate(f):
        mu[k], mup[k] = find_mu_mup(find_X(Ne, fk), find_Y(fk, Babs), bpsi, mode, device=device)
    if geometry == "spherical":
        if R_E is None:
            R_E = constants()[2]
        axis0, axis1 = R_E + z_grid, x_grid / R_E
    else:
        axis0, axis1 = z_grid, x_grid
    return RefractiveField(axis0, axis1, mu, mup, edge_order=edge_order, device=device, fill_n=fill_value_n,
                           fill_grad=fill_value_grad, fill_mup=fill_value_mup, geometry=geometry, R_E=R_E)


def _ionosphere(Ne, Babs, bpsi, z_grid, x_grid, mode, geometry, R_E, edge_order):
    """The checks and the axes that ``refractive_field_device`` and the MUF calls share; nothing here needs a GPU."""
    if mode not in ("O", "X"):
        raise ValueError("Mode must be O or X")
    if geometry not in ("cartesian", "spherical"):
        raise ValueError("geometry must be 'cartesian' or 'spherical'")
    if edge_order not in (1, 2):
        raise ValueError("'edge_order' greater than 2 not supported")          # np.gradient's message
    z_grid = np.asarray(z_grid, dtype=float)
    x_grid = np.asarray(x_grid, dtype=float)
    Ne, Babs, bpsi = (np.ascontiguousarray(v, dtype=np.float64) for v in (Ne, Babs, bpsi))
    if z_grid.ndim != 1 or x_grid.ndim != 1 or not (Ne.shape == Babs.shape == bpsi.shape == (z_grid.size, x_grid.size)):
        raise ValueError("Ne, Babs, bpsi must have shape (len(z_grid), len(x_grid))")
    if not (np.all(np.diff(z_grid) > 0) and np.all(np.diff(x_grid) > 0)):
        raise ValueError("`z_grid` and `x_grid` must be strictly increasing.")
    if min(Ne.shape) < edge_order + 1:
        raise ValueError("Shape of array too small to calculate a numerical gradient, "
                         "at least (edge_order + 1) elements are required.")
    if z_grid.size + x_grid.size > _MAX_AXES:
        raise ValueError(f"the two axes hold at most {_MAX_AXES} values together")
    if np.any(Ne < 0):
        raise ValueError("Density must be non-negative")                       # den2freq's
    if geometry == "spherical":
        R_E = float(constants()[2] if R_E is None else R_E)
        axis0, axis1 = R_E + z_grid, x_grid / R_E
    else:
        R_E, axis0, axis1 = None, z_grid, x_grid
    return Ne, Babs, bpsi, np.ascontiguousarray(axis0), np.ascontiguousarray(axis1), R_E


def refractive_field_device(f0_Hz, Ne, Babs, bpsi, z_grid, x_grid, mode, geometry="cartesian", *, R_E=None, edge_order=2,
                            fill_value_n=np.nan, fill_value_grad=0.0, fill_value_mup=np.nan, device=None):
    """``refractive_field`` built on the device in one call with no host round trip inside it
    (``prhf_field_build_f64``): X, Y, mu and mu' of every frequency of ``f0_Hz`` ``(F,)`` and the
    records, from one upload of ``Ne, Babs, bpsi`` ``(nz, nx)``.  Returns a ``RefractiveField`` that already holds its
    records; its ``.mu`` and ``.mup`` are copied back once.

    Per frequency the fields are bit for bit those of ``find_mu_mup(find_X(Ne, np.array([f])), find_Y(np.array([f]),
    Babs), bpsi, mode)``, the isotropic rule ``nanmax|Y| < 1e-12`` applied per frequency.  f squared is the PRODUCT
    ``f * f``, which is what ``find_X`` gives for an ARRAY of frequencies.  ``refractive_field`` hands ``find_X`` a NumPy
    scalar, whose ``f ** 2`` is libm's ``pow`` and differs from the product in the last bit for about one frequency in a
    thousand: for those frequencies the two functions differ by a rounding of X.  ``ValueError`` for a negative
    density."""
    Ne, Babs, bpsi, axis0, axis1, R_E = _ionosphere(Ne, Babs, bpsi, z_grid, x_grid, mode, geometry, R_E, edge_order)
    f = np.ascontiguousarray(np.atleast_1d(np.asarray(f0_Hz, dtype=np.float64)))
    if f.ndim != 1 or f.size == 0:
        raise ValueError("f0_Hz must be 1-D and not empty")
    import torch
    ctx = _native.host_context(device)
    rec = torch.empty((f.size,) + Ne.shape + (4,), dtype=torch.float64, device=f"cuda:{ctx.device}")
    mu = np.empty((f.size,) + Ne.shape)
    mup = np.empty_like(mu)
    _native.raise_for(ctx.field_build(Ne.ctypes.data, Babs.ctypes.data, bpsi.ctypes.data, axis0.size, axis1.size,
                                      axis0.ctypes.data, axis1.ctypes.data, f.ctypes.data, f.size, _MODE_CODE[mode],
                                      edge_order, rec.data_ptr(), mu.ctypes.data, mup.ctypes.data, 0))
    field = RefractiveField(axis0, axis1, mu, mup, edge_order=edge_order, device=device, fill_n=fill_value_n,
                            fill_grad=fill_value_grad, fill_mup=fill_value_mup, geometry=geometry, R_E=R_E)
    field._rec = rec
    return field


def _need_geometry(field, geometry, name):
    if not isinstance(field, RefractiveField):
        raise TypeError("field must be a RefractiveField (refractive_field, or the .field of a builder's callable)")
    if field.geometry != geometry:
        raise ValueError(f"{name} needs a {geometry} field, this one is {field.geometry}")


def _trace(field, x0, z0, elev, idx, controls, return_paths, earth_radius=None):
    """Rays in the caller's order; the launch gets them sorted by (field, elevation) so that a wave shares a field and
    neighbouring lanes take similar numbers of steps.  A lane's result does not depend on its neighbours.
    ``earth_radius``: the spherical tracer, whose ``controls`` hold ``r_max_km, phi_min, phi_max`` in the places of
    ``z_max_km, x_min_km, x_max_km``."""
    path_keys = _PATH_KEYS if earth_radius is None else _PATH_KEYS_SPHERICAL
    s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every = controls
    max_step = np.inf if max_step_km is None else float(max_step_km)
    if max_step <= 0:
        raise ValueError("`max_step` must be positive.")                   # solve_ivp's message
    n = x0.size
    if idx is None:
        if field.n_fields != 1:
            raise ValueError("field_index is needed when the field holds several frequencies")
        idx = np.zeros(n, dtype=np.int64)
    if n and (idx.min() < 0 or idx.max() >= field.n_fields):
        raise ValueError("field_index outside [0, n_fields)")
    order = np.lexsort((elev, idx))
    xs, zs, es, fs = (np.ascontiguousarray(v[order]) for v in (x0, z0, elev, idx))
    ctl = (s_max_km, rtol, atol, max_step, z_ground_km, z_max_km, x_min_km, x_max_km,
           int(renormalize_every) if renormalize_every else 0)
    out = np.empty((n, 12), dtype=np.float64)
    res = {}
    if n:
        rec = field.records()
        ctx = field._ctx()

        def launch(paths, stride):
            grid = (rec.data_ptr(), field.n_fields, field.axis0.size, field.axis1.size, field.axis0.ctypes.data,
                    field.axis1.ctypes.data, xs.ctypes.data, zs.ctypes.data, es.ctypes.data, fs.ctypes.data, n)
            tail = (ctl, field.fills, out.ctypes.data, paths, stride, 0)
            if earth_radius is None:
                _native.raise_for(ctx.trace_gradient(*grid, *tail))
            else:
                _native.raise_for(ctx.trace_gradient_spherical(*grid, earth_radius, *tail))
        launch(None, 0)
        if return_paths:
            # the same rays again, now that the longest path is known: the steps are deterministic
            stride = int(out[:, 8].max())
            bufs = [np.empty((n, stride), dtype=np.float64) for _ in path_keys]
            launch([b.ctypes.data for b in bufs], stride)
            for k, b in zip(path_keys, bufs):
                unsorted = np.empty_like(b)
                unsorted[order] = b
                res[k] = unsorted
    elif return_paths:
        for k in path_keys:
            res[k] = np.empty((0, 0))
    back = np.empty_like(out)
    back[order] = out
    for i, k in enumerate(_KEYS):
        res[k] = back[:, i].astype(np.int64) if k in _INT_KEYS else back[:, i].copy()
    return res


def _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every):
    return (float(s_max_km), float(rtol), float(atol), max_step_km, float(z_ground_km), float(z_max_km), float(x_min_km),
            float(x_max_km), renormalize_every)


def _broadcast_rays(x0_km, z0_km, elevation_deg, field_index):
    arrs = [np.asarray(v, dtype=np.float64) for v in (x0_km, z0_km, elevation_deg)]
    if field_index is not None:
        arrs.append(np.asarray(field_index, dtype=np.int64))
    arrs = np.broadcast_arrays(*arrs)
    flat = [np.ascontiguousarray(v).reshape(-1) for v in arrs]
    return arrs[0].shape, flat, flat[3] if field_index is not None else None


def trace_rays_cartesian_gradient(field, x0_km, z0_km, elevation_deg, field_index=None, s_max_km=5000.0, *, rtol=1e-7,
                                  atol=1e-9, max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0,
                                  x_min_km=-1e6, x_max_km=1e6, renormalize_every=50, return_paths=False):
    """Trace ``R`` rays through ``field`` (a ``RefractiveField``, Cartesian) in one launch; ``x0_km, z0_km,
    elevation_deg`` and ``field_index`` broadcast to ``(R,)``.  The controls are the reference's (library.py:1278-1291;
    ``z_min_km`` is accepted and, as there, unused).  Returns a dict of ``(R,)`` arrays: the reference's
    ``group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km, x_apex_km, z_apex_km`` and ``status``
    (index into ``STATUS_NAMES``), ``n_nodes``, ``n_rhs``, ``n_rejected``; with ``return_paths`` also ``t, x, z, vx,
    vz``: ``(R, max n_nodes)`` padded with NaN."""
    _need_geometry(field, "cartesian", "trace_rays_cartesian_gradient")
    shape, flat, idx = _broadcast_rays(x0_km, z0_km, elevation_deg, field_index)
    res = _trace(field, flat[0], flat[1], flat[2], idx,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                 return_paths)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}


def trace_fan_cartesian_gradient(field, elevation_deg, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, *, rtol=1e-7, atol=1e-9,
                                 max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6,
                                 x_max_km=1e6, renormalize_every=50, return_paths=False):
    """Every elevation of ``elevation_deg`` ``(E,)`` from ``(x0_km, z0_km)`` in every field of ``field``: the dict of
    ``trace_rays_cartesian_gradient`` with arrays of shape ``(F, E)``, one launch."""
    e = np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64))
    if e.ndim != 1:
        raise ValueError("elevation_deg must be 1-D (the elevations of the fan)")
    _need_geometry(field, "cartesian", "trace_fan_cartesian_gradient")
    idx = np.arange(field.n_fields, dtype=np.int64)[:, None]
    return trace_rays_cartesian_gradient(field, x0_km, z0_km, e[None, :], idx, s_max_km, rtol=rtol, atol=atol,
                                         max_step_km=max_step_km, z_ground_km=z_ground_km, z_min_km=z_min_km,
                                         z_max_km=z_max_km, x_min_km=x_min_km, x_max_km=x_max_km,
                                         renormalize_every=renormalize_every, return_paths=return_paths)


def _merged(n_and_grad, mup_func):
    """One field with the mu of ``n_and_grad`` and the mu' of ``mup_func`` (same grids)."""
    nf, mf = n_and_grad.field, mup_func.field
    return RefractiveField(nf.axis0, nf.axis1, nf.mu, mf.mup, edge_order=nf.edge_order, device=nf.device,
                           fill_n=nf.fills[0], fill_grad=nf.fills[1], fill_mup=mf.fills[2], geometry=nf.geometry,
                           R_E=nf.R_E)


def trace_ray_cartesian_gradient(n_and_grad, mup_func, x0_km, z0_km, elevation_deg, s_max_km=5000.0, *, rtol=1e-7,
                                 atol=1e-9, max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0,
                                 x_min_km=-1e6, x_max_km=1e6, renormalize_every=50):
    """One ray; the reference's signature and result dict (library.py:1270-1457) without ``'sol'``: ``t, x, z, vx, vz``
    (path arrays), ``status`` (str), ``group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km,
    x_apex_km, z_apex_km``.  ``n_and_grad`` and ``mup_func`` must be the objects this module's builders return, in
    Cartesian geometry and on the same grids."""
    if mup_func is None:
        raise ValueError("mup_func must be provided, build it with build_mup_function.")      # :1349-1351
    if not isinstance(n_and_grad, _NAndGrad) or not isinstance(mup_func, _MupFunction):
        raise TypeError("n_and_grad and mup_func must be built with this module's "
                        "build_refractive_index_interpolator_cartesian and build_mup_function: there is no CPU path")
    if n_and_grad.geometry != "cartesian" or mup_func.geometry != "cartesian":
        raise ValueError("trace_ray_cartesian_gradient needs Cartesian n_and_grad and mup_func")
    if not n_and_grad.field.same_grid(mup_func.field):
        raise ValueError("n_and_grad and mup_func must be built on the same z_grid and x_grid")
    field = n_and_grad._with_mup.get(id(mup_func))
    if field is None or field[0] is not mup_func:
        nf, mf = n_and_grad.field, mup_func.field
        n_and_grad._with_mup = {id(mup_func): (mup_func, _merged(n_and_grad, mup_func))}
        field = n_and_grad._with_mup[id(mup_func)]
    r = trace_rays_cartesian_gradient(field[1], np.float64(x0_km), np.float64(z0_km), np.float64(elevation_deg), None,
                                      s_max_km, rtol=rtol, atol=atol, max_step_km=max_step_km, z_ground_km=z_ground_km,
                                      z_min_km=z_min_km, z_max_km=z_max_km, x_min_km=x_min_km, x_max_km=x_max_km,
                                      renormalize_every=renormalize_every, return_paths=True)
    n = int(r["n_nodes"])
    out = {k: r[k][:n].copy() for k in _PATH_KEYS}
    out["status"] = STATUS_NAMES[int(r["status"])]
    for k in _KEYS[:7]:
        out[k] = float(r[k])
    return out


def trace_rays_spherical_gradient(field, x0_km, z0_km, elevation_deg, field_index=None, s_max_km=6000.0, *, R_E=None,
                                  z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9,
                                  max_step_km=2.0, renormalize_every=50, return_paths=False):
    """Trace ``R`` rays through ``field`` (a ``RefractiveField``, spherical) in one launch; ``x0_km`` (surface arc),
    ``z0_km`` (altitude), ``elevation_deg`` and ``field_index`` broadcast to ``(R,)``.  The controls are the reference's
    (library.py:2135-2145; ``max_step_km=None``: no limit; ``r_max_km=None``: ``R_E + 1200``); ``R_E`` defaults to the
    field's and must equal it.  The rays stop at ``r <= R_E + z_ground_km + 1e-3``, ``r >= r_max_km``, ``phi <= phi_min``
    or ``phi >= phi_max``.  Returns the dict of ``trace_rays_cartesian_gradient`` with
    ``x = R_E phi`` and ``z = r - R_E`` in every x and z entry; with ``return_paths`` also ``t, r, phi, v_r, v_phi, x,
    z``: ``(R, max n_nodes)`` padded with NaN."""
    _need_geometry(field, "spherical", "trace_rays_spherical_gradient")
    if R_E is None:
        R_E = field.R_E
    if float(R_E) != field.R_E:
        raise ValueError(f"R_E={R_E} is not the field's ({field.R_E})")
    R_E = field.R_E
    if r_max_km is None:
        r_max_km = R_E + 1200.0                                             # :2226-2227
    shape, flat, idx = _broadcast_rays(x0_km, z0_km, elevation_deg, field_index)
    res = _trace(field, flat[0], flat[1], flat[2], idx,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                 return_paths, earth_radius=R_E)
    if return_paths:
        res["x"] = R_E * res["phi"]                                         # :2277-2278
        res["z"] = res["r"] - R_E
    return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}


def trace_fan_spherical_gradient(field, elevation_deg, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, *, R_E=None,
                                 z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9,
                                 max_step_km=2.0, renormalize_every=50, return_paths=False):
    """Every elevation of ``elevation_deg`` ``(E,)`` from ``(x0_km, z0_km)`` in every field of ``field``: the dict of
    ``trace_rays_spherical_gradient`` with arrays of shape ``(F, E)``, one launch."""
    e = np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64))
    if e.ndim != 1:
        raise ValueError("elevation_deg must be 1-D (the elevations of the fan)")
    _need_geometry(field, "spherical", "trace_fan_spherical_gradient")
    idx = np.arange(field.n_fields, dtype=np.int64)[:, None]
    return trace_rays_spherical_gradient(field, x0_km, z0_km, e[None, :], idx, s_max_km, R_E=R_E, z_ground_km=z_ground_km,
                                         r_max_km=r_max_km, phi_min=phi_min, phi_max=phi_max, rtol=rtol, atol=atol,
                                         max_step_km=max_step_km, renormalize_every=renormalize_every,
                                         return_paths=return_paths)


def _home(field, geometry, name, target_x_km, x0_km, z0_km, controls, scan_elevation_deg, max_roots, range_tol_km, max_iter,
          earth_radius, n_hops=None):
    """Both homing calls: every field of ``field`` is a group launched from ``(x0_km, z0_km)``, the links are
    (field, target) in C order.  ``controls``: the tracer's, as ``_trace`` takes them.  ``n_hops``: homing on the landing
    of hop ``n_hops - 1`` (``prhf_gradient_hop_home_f64``), whose rows hold every hop."""
    from .tracers import default_scan_elevations
    _need_geometry(field, geometry, name)
    if n_hops is not None:
        n_hops = _check_hops(n_hops)
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(target_x_km, dtype=np.float64)))
    if t.ndim != 1 or t.size == 0:
        raise ValueError("target_x_km must be 1-D and not empty (the targets)")
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
    s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right, renormalize_every = controls
    max_step = np.inf if max_step_km is None else float(max_step_km)
    if max_step <= 0:
        raise ValueError("`max_step` must be positive.")                   # solve_ivp's message
    ctl = (s_max_km, rtol, atol, max_step, z_ground_km, top, left, right, int(renormalize_every) if renormalize_every else 0)
    n_groups = field.n_fields
    group_f = np.arange(n_groups, dtype=np.int64)
    group_x = np.full(n_groups, float(x0_km))
    group_z = np.full(n_groups, float(z0_km))
    link_g = np.ascontiguousarray(np.repeat(group_f, t.size))
    link_t = np.ascontiguousarray(np.tile(t, n_groups))
    width = 15 if n_hops is None else 3 + 15 * n_hops
    out = np.empty((link_g.size, max_roots, width), dtype=np.float64)
    n_br = np.empty(link_g.size, dtype=np.int64)
    rec = field.records()
    ctx = field._ctx()
    head = (0 if earth_radius is None else 1, rec.data_ptr(), n_groups, field.axis0.size, field.axis1.size,
            field.axis0.ctypes.data, field.axis1.ctypes.data, group_f.ctypes.data, group_x.ctypes.data, group_z.ctypes.data,
            n_groups, link_g.ctypes.data, link_t.ctypes.data, link_g.size, scan.ctypes.data, scan.size,
            0.0 if earth_radius is None else earth_radius, ctl, field.fills, range_tol_km, max_iter, max_roots)
    if n_hops is None:
        _native.raise_for(ctx.gradient_home(*head, out.ctypes.data, n_br.ctypes.data, 0))
    else:
        _native.raise_for(ctx.gradient_hop_home(*head, n_hops, out.ctypes.data, n_br.ctypes.data, 0))
    lead = (n_groups, t.size)
    out = out.reshape(lead + (max_roots, width))
    res = {"n_brackets": n_br.reshape(lead), "elevation_deg": out[..., 0].copy(), "status": out[..., 1].astype(np.int64)}
    idx = out[..., 2]
    res["scan_index"] = np.where(np.isfinite(idx), idx, -1.0).astype(np.int64)
    if n_hops is not None:
        res.update(_hop_dict(out[..., 3:].reshape(lead + (max_roots, n_hops, 15)), "ray_status"))
        return res
    unused = res["status"] < 0
    for i, k in enumerate(_KEYS):
        v = out[..., 3 + i]
        # (the tracer's integer keys: its status under its own name would collide with the bracket's)
        if k == "status":
            res["ray_status"] = np.where(unused, -1.0, v).astype(np.int64)
        elif k in _INT_KEYS:
            res[k] = np.where(unused, 0.0, v).astype(np.int64)
        else:
            res[k] = v.copy()
    return res


def home_rays_cartesian_gradient(field, target_x_km, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, *, scan_elevation_deg=None,
                                 max_roots=4, range_tol_km=0.05, max_iter=64, rtol=1e-7, atol=1e-9, max_step_km=None,
                                 z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6, x_max_km=1e6,
                                 renormalize_every=50):
    """Point-to-point homing through a horizontally varying ionosphere over a flat Earth: for every field of ``field``
    (a ``RefractiveField``, Cartesian; ``F`` of them), launched from ``(x0_km, z0_km)``, and every target of
    ``target_x_km`` ``(T,)``, the rays that land at that x - the oblique ionogram of the link
    (``prhf_gradient_home_f64``).  The controls are ``trace_rays_cartesian_gradient``'s.

    The fan of ``scan_elevation_deg`` (strictly increasing, default ``tracers.default_scan_elevations()``; elevations
    beyond 90 degrees look behind the transmitter) is traced once per field; an interval of the scan whose two rays land
    on either side of the target (or whose lower ray lands on it) is a bracket, and each of the first ``max_roots``
    brackets in ascending elevation is narrowed with at most ``max_iter`` further rays.  What is found is a function of
    the scan grid.

    ``range_tol_km`` defaults to 0.05 km: twice the reference tracer's own recorded range error at the default
    tolerances (2.3e-2 km).  The landing coordinate of these tracers is not continuous in the
    elevation down to rounding - the step-size controller turns last-bit differences into other step sequences, a
    sawtooth of about 3e-3 km at the default controls - so a tolerance below the sawtooth of D(e) under the chosen
    controls yields status 1, not a better ray.

    Returns a dict: ``n_brackets`` ``(F, T)`` - every bracket of the link, those beyond ``max_roots`` included - and,
    with shape ``(F, T, max_roots)``, ``elevation_deg``, ``status``, ``scan_index`` (the bracket's interval) and the
    keys of ``trace_rays_cartesian_gradient`` for the result ray, bit for bit what that call returns at
    ``elevation_deg`` (the tracer's own ``status`` is ``ray_status`` here).  ``status`` 0: the ray lands within
    ``range_tol_km`` of the target; 1: the landing coordinate jumps across the target inside the bracket, or
    ``max_iter`` is spent - the ray given is the nearest one tried; 2: a ray inside the bracket does not land; -1: unused
    slot (NaN everywhere, ``scan_index`` and ``ray_status`` -1, the counts 0)."""
    return _home(field, "cartesian", "home_rays_cartesian_gradient", target_x_km, x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                 scan_elevation_deg, max_roots, range_tol_km, max_iter, None)


def home_rays_spherical_gradient(field, target_x_km, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, *, R_E=None,
                                 scan_elevation_deg=None, max_roots=4, range_tol_km=0.05, max_iter=64, z_ground_km=0.0,
                                 r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9, max_step_km=2.0,
                                 renormalize_every=50):
    """The same over a spherical Earth: ``field`` is spherical, the controls and their defaults are
    ``trace_rays_spherical_gradient``'s, and a target is compared with that tracer's ``ground_range_km``, the surface arc
    ``R_E phi`` of the landing node (``x0_km`` is a surface arc as well)."""
    _need_geometry(field, "spherical", "home_rays_spherical_gradient")
    if R_E is None:
        R_E = field.R_E
    if float(R_E) != field.R_E:
        raise ValueError(f"R_E={R_E} is not the field's ({field.R_E})")
    R_E = field.R_E
    if r_max_km is None:
        r_max_km = R_E + 1200.0                                             # :2226-2227
    return _home(field, "spherical", "home_rays_spherical_gradient", target_x_km, x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                 scan_elevation_deg, max_roots, range_tol_km, max_iter, R_E)


def _check_hops(n_hops):
    if isinstance(n_hops, bool) or int(n_hops) != n_hops or not 1 <= int(n_hops) <= _MAX_HOPS:
        raise ValueError(f"n_hops is an integer in 1 .. {_MAX_HOPS}")
    return int(n_hops)


def _hop_dict(rows, status_key="status"):
    """The per-hop arrays and the totals from hop rows ``(..., H, 15)`` (include/prhf.h: launch x, z, elevation, then
    the tracer's twelve; an unused row is NaN with status -1 and counters 0)."""
    n_hops = rows.shape[-2]
    res = {k: rows[..., i].copy() for i, k in enumerate(_HOP_LAUNCH_KEYS)}
    for i, k in enumerate(_KEYS):
        v = rows[..., 3 + i]
        res[status_key if k == "status" else k] = v.astype(np.int64) if k in _INT_KEYS else v.copy()
    st = res[status_key]
    res["n_landed"] = (st == 0).sum(axis=-1)
    for k in ("group_path_km", "group_delay_sec"):
        total = np.zeros(rows.shape[:-2])
        for h in range(n_hops):                                             # in hop order, over the used hops
            total = np.where(st[..., h] >= 0, total + res[k][..., h], total)
        res["total_" + k] = np.where(st[..., 0] >= 0, total, np.nan)         # (an unused slot of a homing call: NaN)
    res["total_ground_range_km"] = np.where(res["n_landed"] == n_hops, res["ground_range_km"][..., n_hops - 1], np.nan)
    return res


def _trace_hops(field, x0, z0, elev, idx, controls, n_hops, return_paths, earth_radius=None):
    """``_trace`` for chains of ``n_hops`` hops (``prhf_trace_gradient_hops_f64``): arrays ``(R, H)``, paths
    ``(R, H, max n_nodes)``."""
    path_keys = _PATH_KEYS if earth_radius is None else _PATH_KEYS_SPHERICAL
    s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right, renormalize_every = controls
    max_step = np.inf if max_step_km is None else float(max_step_km)
    if max_step <= 0:
        raise ValueError("`max_step` must be positive.")                   # solve_ivp's message
    n = x0.size
    if idx is None:
        if field.n_fields != 1:
            raise ValueError("field_index is needed when the field holds several frequencies")
        idx = np.zeros(n, dtype=np.int64)
    if n and (idx.min() < 0 or idx.max() >= field.n_fields):
        raise ValueError("field_index outside [0, n_fields)")
    order = np.lexsort((elev, idx))
    xs, zs, es, fs = (np.ascontiguousarray(v[order]) for v in (x0, z0, elev, idx))
    ctl = (s_max_km, rtol, atol, max_step, z_ground_km, top, left, right, int(renormalize_every) if renormalize_every else 0)
    out = np.empty((n, n_hops, 15), dtype=np.float64)
    paths = {}
    if n:
        rec = field.records()
        ctx = field._ctx()

        def launch(bufs, stride):
            _native.raise_for(ctx.trace_gradient_hops(
                0 if earth_radius is None else 1, rec.data_ptr(), field.n_fields, field.axis0.size, field.axis1.size,
                field.axis0.ctypes.data, field.axis1.ctypes.data, xs.ctypes.data, zs.ctypes.data, es.ctypes.data,
                fs.ctypes.data, n, 0.0 if earth_radius is None else earth_radius, ctl, field.fills, n_hops, out.ctypes.data,
                bufs, stride, 0))
        launch(None, 0)
        if return_paths:
            # the same chains again, now that the longest path is known: the steps are deterministic
            stride = max(int(out[:, :, 11].max()), 1)
            bufs = [np.empty((n, n_hops, stride), dtype=np.float64) for _ in path_keys]
            launch([b.ctypes.data for b in bufs], stride)
            for k, b in zip(path_keys, bufs):
                unsorted = np.empty_like(b)
                unsorted[order] = b
                paths[k] = unsorted
    elif return_paths:
        for k in path_keys:
            paths[k] = np.empty((0, n_hops, 0))
    back = np.empty_like(out)
    back[order] = out
    res = _hop_dict(back)
    res.update(paths)
    return res


def trace_hops_cartesian_gradient(field, x0_km, z0_km, elevation_deg, n_hops, field_index=None, s_max_km=5000.0, *,
                                  rtol=1e-7, atol=1e-9, max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0,
                                  x_min_km=-1e6, x_max_km=1e6, renormalize_every=50, return_paths=False):
    """Multi-hop rays through ``field`` (a ``RefractiveField``, Cartesian): ``R`` chains of ``n_hops`` (1 .. 16) hops in
    one launch, a chain per lane (``prhf_trace_gradient_hops_f64``).  The arguments are
    ``trace_rays_cartesian_gradient``'s and every hop runs under them.  A hop that lands (status 0) is reflected off the
    ground: the next hop launches at ``(ground_range_km, z_ground_km)`` with the elevation
    ``degrees(arctan2(-vz, vx))`` of the landing node; a chain ends with its first hop that does not land.

    Returns that call's keys with a trailing hop axis, ``(R, H)`` - every used hop bit for bit what
    ``trace_rays_cartesian_gradient`` returns for the hop's ``launch_x_km``, ``launch_z_km``, ``launch_elevation_deg``,
    which are returned as well; unused hops are NaN with ``status`` -1 and the counts 0 -, and per chain ``n_landed``,
    ``total_group_path_km`` and ``total_group_delay_sec`` (summed in hop order over the used hops) and
    ``total_ground_range_km`` (the landing x of the last hop, NaN unless all ``n_hops`` hops landed).  With
    ``return_paths`` also ``t, x, z, vx, vz``: ``(R, H, max n_nodes)`` padded with NaN."""
    _need_geometry(field, "cartesian", "trace_hops_cartesian_gradient")
    n_hops = _check_hops(n_hops)
    shape, flat, idx = _broadcast_rays(x0_km, z0_km, elevation_deg, field_index)
    res = _trace_hops(field, flat[0], flat[1], flat[2], idx,
                      _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km,
                                renormalize_every), n_hops, return_paths)
    return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}


def trace_hop_fan_cartesian_gradient(field, elevation_deg, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, **controls):
    """Every elevation of ``elevation_deg`` ``(E,)`` from ``(x0_km, z0_km)`` in every field of ``field``: the dict of
    ``trace_hops_cartesian_gradient`` (whose keyword controls these are) with arrays of shape ``(F, E, H)``, one launch."""
    e = np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64))
    if e.ndim != 1:
        raise ValueError("elevation_deg must be 1-D (the elevations of the fan)")
    _need_geometry(field, "cartesian", "trace_hop_fan_cartesian_gradient")
    idx = np.arange(field.n_fields, dtype=np.int64)[:, None]
    return trace_hops_cartesian_gradient(field, x0_km, z0_km, e[None, :], n_hops, idx, s_max_km, **controls)


def _spherical_controls(field, R_E, r_max_km):
    if R_E is None:
        R_E = field.R_E
    if float(R_E) != field.R_E:
        raise ValueError(f"R_E={R_E} is not the field's ({field.R_E})")
    return field.R_E, field.R_E + 1200.0 if r_max_km is None else r_max_km                      # :2226-2227


def trace_hops_spherical_gradient(field, x0_km, z0_km, elevation_deg, n_hops, field_index=None, s_max_km=6000.0, *,
                                  R_E=None, z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7,
                                  atol=1e-9, max_step_km=2.0, renormalize_every=50, return_paths=False):
    """The same over a spherical Earth: the arguments are ``trace_rays_spherical_gradient``'s, the reflected elevation is
    ``degrees(arctan2(-v_r, v_phi))`` of the landing node, and the next hop launches at the surface arc
    ``ground_range_km = R_E phi`` of the landing, altitude ``z_ground_km``.  With ``return_paths`` also ``t, r, phi, v_r,
    v_phi, x, z``: ``(R, H, max n_nodes)``."""
    _need_geometry(field, "spherical", "trace_hops_spherical_gradient")
    n_hops = _check_hops(n_hops)
    R_E, r_max_km = _spherical_controls(field, R_E, r_max_km)
    shape, flat, idx = _broadcast_rays(x0_km, z0_km, elevation_deg, field_index)
    res = _trace_hops(field, flat[0], flat[1], flat[2], idx,
                      _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                      n_hops, return_paths, earth_radius=R_E)
    if return_paths:
        res["x"] = R_E * res["phi"]                                         # :2277-2278
        res["z"] = res["r"] - R_E
    return {k: v.reshape(shape + v.shape[1:]) for k, v in res.items()}


def trace_hop_fan_spherical_gradient(field, elevation_deg, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, **controls):
    """Every elevation of ``elevation_deg`` ``(E,)`` from ``(x0_km, z0_km)`` in every field of ``field``: the dict of
    ``trace_hops_spherical_gradient`` (whose keyword controls these are) with arrays of shape ``(F, E, H)``, one launch."""
    e = np.atleast_1d(np.asarray(elevation_deg, dtype=np.float64))
    if e.ndim != 1:
        raise ValueError("elevation_deg must be 1-D (the elevations of the fan)")
    _need_geometry(field, "spherical", "trace_hop_fan_spherical_gradient")
    idx = np.arange(field.n_fields, dtype=np.int64)[:, None]
    return trace_hops_spherical_gradient(field, x0_km, z0_km, e[None, :], n_hops, idx, s_max_km, **controls)


def home_hops_cartesian_gradient(field, target_x_km, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, *,
                                 scan_elevation_deg=None, max_roots=4, range_tol_km=0.05, max_iter=64, rtol=1e-7, atol=1e-9,
                                 max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6,
                                 x_max_km=1e6, renormalize_every=50):
    """Homing on the landing of hop ``n_hops - 1`` (the 2F, 3F .. modes of a long link through a tilted ionosphere):
    ``home_rays_cartesian_gradient`` with the landing coordinate of a ray replaced by ``total_ground_range_km`` of
    ``trace_hops_cartesian_gradient``'s chain (``prhf_gradient_hop_home_f64``); scan, brackets,
    refinement, statuses and arguments are that call's.

    Returns ``n_brackets`` ``(F, T)``, with shape ``(F, T, max_roots)`` ``elevation_deg``, ``status``, ``scan_index``,
    ``n_landed`` and the three totals, and with shape ``(F, T, max_roots, H)`` the per-hop keys of
    ``trace_hops_cartesian_gradient`` for the result chain, bit for bit what that call returns at ``elevation_deg`` (the
    tracer's own ``status`` is ``ray_status`` here).  Unused slots are NaN with ``status``, ``scan_index`` and
    ``ray_status`` -1 and the counts 0."""
    return _home(field, "cartesian", "home_hops_cartesian_gradient", target_x_km, x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                 scan_elevation_deg, max_roots, range_tol_km, max_iter, None, n_hops=n_hops)


def home_hops_spherical_gradient(field, target_x_km, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, *, R_E=None,
                                 scan_elevation_deg=None, max_roots=4, range_tol_km=0.05, max_iter=64, z_ground_km=0.0,
                                 r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9, max_step_km=2.0,
                                 renormalize_every=50):
    """The same over a spherical Earth: ``home_rays_spherical_gradient``'s arguments, ``trace_hops_spherical_gradient``'s
    chains."""
    _need_geometry(field, "spherical", "home_hops_spherical_gradient")
    R_E, r_max_km = _spherical_controls(field, R_E, r_max_km)
    return _home(field, "spherical", "home_hops_spherical_gradient", target_x_km, x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                 scan_elevation_deg, max_roots, range_tol_km, max_iter, R_E, n_hops=n_hops)


def _search_controls(scan_elevation_deg, elev_tol_deg, max_iter, controls):
    """The scan grid, the rule's controls and the tracer's, checked (no GPU needed)."""
    from .tracers import default_scan_elevations
    scan = default_scan_elevations() if scan_elevation_deg is None else \
        np.ascontiguousarray(np.atleast_1d(np.asarray(scan_elevation_deg, dtype=np.float64)))
    if scan.ndim != 1 or scan.size < 1:
        raise ValueError("scan_elevation_deg needs at least 1 elevation")
    if not np.all(np.diff(scan) > 0) or not np.all(np.isfinite(scan)):
        raise ValueError("scan_elevation_deg must be strictly increasing")
    max_iter, elev_tol_deg = int(max_iter), float(elev_tol_deg)
    if not 1 <= max_iter <= 128:
        raise ValueError("max_iter is 1 .. 128")
    if not (np.isfinite(elev_tol_deg) and elev_tol_deg >= 0.0):
        raise ValueError("elev_tol_deg must be finite and not negative")
    s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right, renormalize_every = controls
    max_step = np.inf if max_step_km is None else float(max_step_km)
    if max_step <= 0:
        raise ValueError("`max_step` must be positive.")                   # solve_ivp's message
    ctl = (s_max_km, rtol, atol, max_step, z_ground_km, top, left, right, int(renormalize_every) if renormalize_every else 0)
    return scan, elev_tol_deg, max_iter, ctl


def _skip_head(out):
    """The six rule keys from rows ``(..., >= 6)`` (include/prhf.h)."""
    res = {"skip_km": out[..., 0].copy(), "elevation_deg": out[..., 1].copy()}
    res["status"] = np.where(np.isfinite(out[..., 2]), out[..., 2], -1.0).astype(np.int64)
    res["scan_index"] = np.where(np.isfinite(out[..., 3]), out[..., 3], -1.0).astype(np.int64)
    res["bracket_deg"] = out[..., 4].copy()
    res["n_evals"] = np.where(np.isfinite(out[..., 5]), out[..., 5], 0.0).astype(np.int64)
    return res


_HOP_UNUSED_ROW = np.array([np.nan] * 10 + [-1.0, 0.0, 0.0, 0.0, 0.0])


def _hop_skip_rows(out, lead, n_hops):
    """The dict of the multi-hop skip calls from rows of ``6 + 15 n_hops``, reshaped to ``lead``: the rule keys, then
    ``_hop_dict``'s.  A row that a MUF call left NaN throughout (no frequency found) reads as unused hops."""
    out = out.reshape(lead + (6 + 15 * n_hops,))
    res = _skip_head(out)
    rows = out[..., 6:].reshape(lead + (n_hops, 15)).copy()
    rows[~np.isfinite(out[..., 2])] = _HOP_UNUSED_ROW
    res.update(_hop_dict(rows, "ray_status"))
    return res


def _skip_rows(out, lead):
    """The dict of the skip calls from rows of 18 (include/prhf.h), reshaped to ``lead``."""
    out = out.reshape(lead + (18,))
    res = _skip_head(out)
    status = res["status"]
    none = status < 0
    for i, k in enumerate(_KEYS):
        v = out[..., 6 + i]
        # (the tracer's integer keys: its status under its own name would collide with the rule's)
        if k == "status":
            res["ray_status"] = np.where(none | ~np.isfinite(v), -1.0, v).astype(np.int64)
        elif k in _INT_KEYS:
            res[k] = np.where(none | ~np.isfinite(v), 0.0, v).astype(np.int64)
        else:
            res[k] = v.copy()
    return res


def _skip(field, geometry, name, x0_km, z0_km, controls, scan_elevation_deg, elev_tol_deg, max_iter, earth_radius,
          n_hops=None):
    """Both skip calls: the groups are (field, transmitter) in C order.  ``n_hops``: the skip distance of the landing of
    hop ``n_hops - 1`` (``prhf_gradient_hop_skip_f64``), whose rows hold every hop."""
    _need_geometry(field, geometry, name)
    if n_hops is not None:
        n_hops = _check_hops(n_hops)
    scan, elev_tol_deg, max_iter, ctl = _search_controls(scan_elevation_deg, elev_tol_deg, max_iter, controls)
    x0 = np.atleast_1d(np.asarray(x0_km, dtype=np.float64))
    z0 = np.atleast_1d(np.asarray(z0_km, dtype=np.float64))
    if x0.ndim != 1 or z0.ndim != 1:
        raise ValueError("x0_km and z0_km are scalars or 1-D (the transmitters)")
    x0, z0 = np.broadcast_arrays(x0, z0)
    n_tx = x0.size
    if n_tx == 0:
        raise ValueError("x0_km and z0_km must not be empty")
    n_fields = field.n_fields
    group_f = np.ascontiguousarray(np.repeat(np.arange(n_fields, dtype=np.int64), n_tx))
    group_x = np.ascontiguousarray(np.tile(x0, n_fields))
    group_z = np.ascontiguousarray(np.tile(z0, n_fields))
    out = np.empty((group_f.size, 18 if n_hops is None else 6 + 15 * n_hops), dtype=np.float64)
    rec = field.records()
    ctx = field._ctx()
    head = (0 if earth_radius is None else 1, rec.data_ptr(), n_fields, field.axis0.size, field.axis1.size,
            field.axis0.ctypes.data, field.axis1.ctypes.data, group_f.ctypes.data, group_x.ctypes.data, group_z.ctypes.data,
            group_f.size, scan.ctypes.data, scan.size, 0.0 if earth_radius is None else earth_radius, ctl, field.fills,
            elev_tol_deg, max_iter)
    if n_hops is None:
        _native.raise_for(ctx.gradient_skip(*head, out.ctypes.data, 0))
        return _skip_rows(out, (n_fields, n_tx))
    _native.raise_for(ctx.gradient_hop_skip(*head, n_hops, out.ctypes.data, 0))
    return _hop_skip_rows(out, (n_fields, n_tx), n_hops)


def skip_distance_cartesian_gradient(field, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, *, scan_elevation_deg=None,
                                     elev_tol_deg=1e-3, max_iter=64, rtol=1e-7, atol=1e-9, max_step_km=None,
                                     z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6, x_max_km=1e6,
                                     renormalize_every=50):
    """Skip distance through a horizontally varying ionosphere over a flat Earth: for every field of ``field`` (a
    ``RefractiveField``, Cartesian; ``F`` of them) and every transmitter ``(x0_km, z0_km)`` (scalars or ``(T,)``), the
    least ``ground_range_km`` over the elevations of that transmitter's rays (``prhf_gradient_skip_f64``, DESIGN.md
    section 4.11; the rule is section 4.10's, ``skip_distance_cartesian``'s).  The controls are
    ``trace_rays_cartesian_gradient``'s.

    ``skip_km`` is the tracer's ``ground_range_km`` of the ray found: the LANDING COORDINATE x.  For a scan that looks
    forward the skip distance is ``skip_km - x0_km``.

    The fan of ``scan_elevation_deg`` (strictly increasing, default ``tracers.default_scan_elevations()``) is traced
    once per group; the first scan node that attains the least finite landing coordinate is refined by a golden-section
    search between its neighbours, with at most ``max_iter`` (1 .. 128) further rays, until the bracket is no wider than
    ``elev_tol_deg``.  The default, 1e-3 degrees, costs 18 - 19 rays from a 2.5 degree scan; the step controller's
    sawtooth in D(e) already moves the elevation of so flat a minimum by about 1e-2 degrees, so ``elevation_deg`` is not a
    robust output - ``skip_km`` is.

    Returns a dict of ``(F, T)`` arrays: ``skip_km``, ``elevation_deg``, ``status``, ``scan_index``, ``bracket_deg``,
    ``n_evals`` and the keys of ``trace_rays_cartesian_gradient`` for the ray at ``elevation_deg``, bit for bit what that
    call returns there (the tracer's own ``status`` is ``ray_status`` here).  ``status`` 0: the bracket is within
    ``elev_tol_deg`` (or no float64 is left inside it); 1: the minimum of the scan lies at either end of it or beside a
    ray that does not land - the node as it stands, no further ray; 2: a ray inside the bracket does not land; 3:
    ``max_iter`` is spent; -1: no ray of the scan lands (NaN everywhere, ``scan_index`` and ``ray_status`` -1, the counts
    0)."""
    return _skip(field, "cartesian", "skip_distance_cartesian_gradient", x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                 scan_elevation_deg, elev_tol_deg, max_iter, None)


def _spherical_defaults(R_E, field_R_E, r_max_km):
    if R_E is None:
        R_E = field_R_E
    if float(R_E) != field_R_E:
        raise ValueError(f"R_E={R_E} is not the field's ({field_R_E})")
    return field_R_E, (field_R_E + 1200.0 if r_max_km is None else r_max_km)      # :2226-2227


def skip_distance_spherical_gradient(field, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, *, R_E=None, scan_elevation_deg=None,
                                     elev_tol_deg=1e-3, max_iter=64, z_ground_km=0.0, r_max_km=None, phi_min=-np.pi,
                                     phi_max=np.pi, rtol=1e-7, atol=1e-9, max_step_km=2.0, renormalize_every=50):
    """The same over a spherical Earth: ``field`` is spherical, the controls and their defaults are
    ``trace_rays_spherical_gradient``'s, and ``skip_km`` is that tracer's ``ground_range_km``, the surface arc ``R_E phi``
    of the landing node (``x0_km`` is a surface arc as well)."""
    _need_geometry(field, "spherical", "skip_distance_spherical_gradient")
    R_E, r_max_km = _spherical_defaults(R_E, field.R_E, r_max_km)
    return _skip(field, "spherical", "skip_distance_spherical_gradient", x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                 scan_elevation_deg, elev_tol_deg, max_iter, R_E)


_MUF_SCRATCH_BYTES = 1 << 30      # the MUF calls cut their links into slabs whose fields stay under this


def _muf(geometry, target_x_km, x0_km, z0_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, n_bisect, controls,
         scan_elevation_deg, elev_tol_deg, max_iter, R_E, edge_order, fills, device, slab_links, n_hops=None):
    if n_hops is not None:
        n_hops = _check_hops(n_hops)
    Ne, Babs, bpsi, axis0, axis1, R_E = _ionosphere(Ne, Babs, bpsi, z_grid, x_grid, mode, geometry, R_E, edge_order)
    scan, elev_tol_deg, max_iter, ctl = _search_controls(scan_elevation_deg, elev_tol_deg, max_iter, controls)
    n_bisect, f_lo_hz, f_hi_hz = int(n_bisect), float(f_lo_hz), float(f_hi_hz)
    if not 1 <= n_bisect <= 64:
        raise ValueError("n_bisect is 1 .. 64")
    if not (0.0 < f_lo_hz < f_hi_hz < np.inf):
        raise ValueError("the frequency bracket needs 0 < f_lo_hz < f_hi_hz, both finite")
    arrs = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (target_x_km, x0_km, z0_km)))
    shape = arrs[0].shape
    t, x0, z0 = (np.ascontiguousarray(v).reshape(-1) for v in arrs)
    if t.size == 0:
        raise ValueError("target_x_km must not be empty")
    if slab_links is None:
        slab_links = max(1, _MUF_SCRATCH_BYTES // (48 * Ne.size))
    slab_links = int(slab_links)
    if slab_links < 1:
        raise ValueError("a slab holds at least one link")
    out = np.empty((t.size, 21 if n_hops is None else 9 + 15 * n_hops), dtype=np.float64)
    ctx = _native.host_context(device)
    for lo in range(0, t.size, slab_links):
        n = min(slab_links, t.size - lo)
        # (contiguous 1-D arrays: a slice's address is its first element's)
        head = (0 if geometry == "cartesian" else 1, Ne.ctypes.data, Babs.ctypes.data, bpsi.ctypes.data, axis0.size,
                axis1.size, axis0.ctypes.data, axis1.ctypes.data, _MODE_CODE[mode], edge_order, x0[lo:].ctypes.data,
                z0[lo:].ctypes.data, t[lo:].ctypes.data, n, f_lo_hz, f_hi_hz, n_bisect, scan.ctypes.data, scan.size,
                0.0 if R_E is None else R_E, ctl, fills, elev_tol_deg, max_iter)
        if n_hops is None:
            _native.raise_for(ctx.gradient_muf(*head, out[lo:].ctypes.data, 0))
        else:
            _native.raise_for(ctx.gradient_hop_muf(*head, n_hops, out[lo:].ctypes.data, 0))
    res = {"muf_hz": out[:, 0].reshape(shape).copy(), "f_above_hz": out[:, 1].reshape(shape).copy(),
           "status": out[:, 2].astype(np.int64).reshape(shape)}
    row = np.ascontiguousarray(out[:, 3:])
    for k, v in (_skip_rows(row, shape) if n_hops is None else _hop_skip_rows(row, shape, n_hops)).items():
        res["skip_status" if k == "status" else k] = v
    return res


def muf_cartesian_gradient(target_x_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, x0_km=0.0, z0_km=0.0,
                           s_max_km=5000.0, *, n_bisect=40, scan_elevation_deg=None, elev_tol_deg=1e-3, max_iter=64,
                           edge_order=2, fill_value_n=np.nan, fill_value_grad=0.0, fill_value_mup=np.nan, rtol=1e-7,
                           atol=1e-9, max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6,
                           x_max_km=1e6, renormalize_every=50, device=None, _slab_links=None):
    """MUF of links through a tilted ionosphere over a flat Earth: for every link - ``target_x_km``, ``x0_km`` and
    ``z0_km`` broadcast against each other - the highest frequency in ``[f_lo_hz, f_hi_hz]`` whose skip distance through
    the ionosphere ``Ne, Babs, bpsi`` ``(nz, nx)`` on ``z_grid, x_grid`` still reaches the target
    (``prhf_gradient_muf_f64``).  S(f) is ``skip_distance_cartesian_gradient``'s ``skip_km`` (the
    landing coordinate) on ``refractive_field_device``'s field at f, +inf where no ray of the scan lands; the semantics,
    statuses and the bisection are ``muf_cartesian``'s (section 4.10): ``n_bisect`` (1 .. 64) halvings of the bracket, m =
    lo + 0.5 (hi - lo).  The fields of the frequencies tried are built on the device (f squared is the product f f), the
    whole search is one call with one synchronisation, and it is latency-bound: 3 + ``n_bisect`` dependent rounds.

    The fields of a call's links take 48 bytes per node and link; the links go in slabs that keep that under 1 GiB, and
    no result depends on the slabs.

    Returns a dict of arrays of the links' broadcast shape: ``muf_hz``, ``f_above_hz``, ``status`` and the keys of
    ``skip_distance_cartesian_gradient`` for the field at ``muf_hz``, bit for bit what that call returns on
    ``refractive_field_device([muf_hz], ...)`` (its ``status`` is ``skip_status`` here).  ``status`` 0: S(muf_hz) <=
    target < S(f_above_hz); 1: S(f_hi_hz) <= target, ``muf_hz`` is ``f_hi_hz`` and ``f_above_hz`` NaN; 2: S(f_lo_hz) >
    target, nothing found; -1: a NaN target."""
    return _muf("cartesian", target_x_km, x0_km, z0_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, n_bisect,
                _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                scan_elevation_deg, elev_tol_deg, max_iter, None, edge_order,
                (float(fill_value_n), float(fill_value_grad), float(fill_value_mup)), device, _slab_links)


def muf_spherical_gradient(target_x_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, x0_km=0.0, z0_km=0.0,
                           s_max_km=6000.0, *, R_E=None, n_bisect=40, scan_elevation_deg=None, elev_tol_deg=1e-3,
                           max_iter=64, edge_order=2, fill_value_n=np.nan, fill_value_grad=0.0, fill_value_mup=np.nan,
                           z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9,
                           max_step_km=2.0, renormalize_every=50, device=None, _slab_links=None):
    """The same over a spherical Earth of radius ``R_E`` (default ``constants()[2]``): the controls and their defaults are
    ``trace_rays_spherical_gradient``'s, targets and ``x0_km`` are surface arcs."""
    R_E = float(constants()[2] if R_E is None else R_E)
    if r_max_km is None:
        r_max_km = R_E + 1200.0                                             # :2226-2227
    return _muf("spherical", target_x_km, x0_km, z0_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, n_bisect,
                _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                scan_elevation_deg, elev_tol_deg, max_iter, R_E, edge_order,
                (float(fill_value_n), float(fill_value_grad), float(fill_value_mup)), device, _slab_links)


def skip_distance_hops_cartesian_gradient(field, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=5000.0, *, scan_elevation_deg=None,
                                          elev_tol_deg=1e-3, max_iter=64, rtol=1e-7, atol=1e-9, max_step_km=None,
                                          z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0, x_min_km=-1e6, x_max_km=1e6,
                                          renormalize_every=50):
    """Skip distance of the ``n_hops``-hop mode (2F, 3F ..) through a tilted ionosphere: where that mode starts to be
    heard.  ``skip_distance_cartesian_gradient`` with the landing coordinate of a ray replaced by
    ``total_ground_range_km`` of ``trace_hops_cartesian_gradient``'s chain - NaN unless all ``n_hops`` (1 .. 16) hops
    land - in one call (``prhf_gradient_hop_skip_f64``); scan, the first index of the minimum,
    refinement, statuses and keyword arguments are that call's.  D(e) of a chain jumps between layers and is not
    unimodal: what is found is the minimum next to the first scan node that attains the least landing coordinate.

    Returns a dict of ``(F, T)`` arrays ``skip_km``, ``elevation_deg``, ``status``, ``scan_index``, ``bracket_deg``,
    ``n_evals`` (chains, not hops), ``n_landed`` and the three totals, and with shape ``(F, T, H)`` the per-hop keys of
    ``trace_hops_cartesian_gradient`` for the chain at ``elevation_deg``, bit for bit what that call returns there (the
    tracer's own ``status`` is ``ray_status`` here); ``skip_km`` has the bits of ``total_ground_range_km``.  ``status``
    -1: no chain of the scan lands - NaN, the hops unused (``ray_status`` -1, the counts 0)."""
    return _skip(field, "cartesian", "skip_distance_hops_cartesian_gradient", x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                 scan_elevation_deg, elev_tol_deg, max_iter, None, n_hops=n_hops)


def skip_distance_hops_spherical_gradient(field, n_hops, x0_km=0.0, z0_km=0.0, s_max_km=6000.0, *, R_E=None,
                                          scan_elevation_deg=None, elev_tol_deg=1e-3, max_iter=64, z_ground_km=0.0,
                                          r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9,
                                          max_step_km=2.0, renormalize_every=50):
    """The same over a spherical Earth: ``skip_distance_spherical_gradient``'s arguments,
    ``trace_hops_spherical_gradient``'s chains."""
    _need_geometry(field, "spherical", "skip_distance_hops_spherical_gradient")
    R_E, r_max_km = _spherical_defaults(R_E, field.R_E, r_max_km)
    return _skip(field, "spherical", "skip_distance_hops_spherical_gradient", x0_km, z0_km,
                 _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                 scan_elevation_deg, elev_tol_deg, max_iter, R_E, n_hops=n_hops)


def muf_hops_cartesian_gradient(target_x_km, n_hops, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, x0_km=0.0,
                                z0_km=0.0, s_max_km=5000.0, *, n_bisect=40, scan_elevation_deg=None, elev_tol_deg=1e-3,
                                max_iter=64, edge_order=2, fill_value_n=np.nan, fill_value_grad=0.0, fill_value_mup=np.nan,
                                rtol=1e-7, atol=1e-9, max_step_km=None, z_ground_km=0.0, z_min_km=-1.0, z_max_km=1000.0,
                                x_min_km=-1e6, x_max_km=1e6, renormalize_every=50, device=None, _slab_links=None):
    """MUF of the ``n_hops``-hop mode of links through a tilted ionosphere - the 2F or 3F MUF of a link that no one-hop
    ray reaches, which ``muf_cartesian_gradient`` can only answer with status 2: that call with S(f) the ``skip_km`` of
    ``skip_distance_hops_cartesian_gradient`` on ``refractive_field_device``'s field at f (``prhf_gradient_hop_muf_f64``,
    DESIGN.md section 4.13).  Arguments, statuses, the bisection and the slabs under 1 GiB are ``muf_cartesian_gradient``'s.

    Returns a dict of arrays of the links' broadcast shape: ``muf_hz``, ``f_above_hz``, ``status`` and the keys of
    ``skip_distance_hops_cartesian_gradient`` for the field at ``muf_hz`` (per-hop keys with a trailing hop axis), bit
    for bit what that call returns on ``refractive_field_device([muf_hz], ...)`` (its ``status`` is ``skip_status``
    here)."""
    return _muf("cartesian", target_x_km, x0_km, z0_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, n_bisect,
                _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every),
                scan_elevation_deg, elev_tol_deg, max_iter, None, edge_order,
                (float(fill_value_n), float(fill_value_grad), float(fill_value_mup)), device, _slab_links, n_hops=n_hops)


def muf_hops_spherical_gradient(target_x_km, n_hops, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, x0_km=0.0,
                                z0_km=0.0, s_max_km=6000.0, *, R_E=None, n_bisect=40, scan_elevation_deg=None,
                                elev_tol_deg=1e-3, max_iter=64, edge_order=2, fill_value_n=np.nan, fill_value_grad=0.0,
                                fill_value_mup=np.nan, z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi,
                                rtol=1e-7, atol=1e-9, max_step_km=2.0, renormalize_every=50, device=None, _slab_links=None):
    """The same over a spherical Earth of radius ``R_E`` (default ``constants()[2]``): ``muf_spherical_gradient``'s
    arguments, ``skip_distance_hops_spherical_gradient``'s S(f)."""
    R_E = float(constants()[2] if R_E is None else R_E)
    if r_max_km is None:
        r_max_km = R_E + 1200.0                                             # :2226-2227
    return _muf("spherical", target_x_km, x0_km, z0_km, Ne, Babs, bpsi, z_grid, x_grid, mode, f_lo_hz, f_hi_hz, n_bisect,
                _controls(s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every),
                scan_elevation_deg, elev_tol_deg, max_iter, R_E, edge_order,
                (float(fill_value_n), float(fill_value_grad), float(fill_value_mup)), device, _slab_links, n_hops=n_hops)


def trace_ray_spherical_gradient(n_and_grad_rphi, mup_func, x0_km, z0_km, elevation_deg, s_max_km=6000.0, *, R_E=None,
                                 z_ground_km=0.0, r_max_km=None, phi_min=-np.pi, phi_max=np.pi, rtol=1e-7, atol=1e-9,
                                 max_step_km=2.0, renormalize_every=50):
    """One ray; the reference's signature and result dict (library.py:2128-2337): ``t, r, phi, v_r, v_phi, x, z`` (path
    arrays), ``status`` (str), ``group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km, x_apex_km,
    z_apex_km``.  ``n_and_grad_rphi`` and ``mup_func`` must be the objects this module's builders return, in spherical
    geometry, on the same grids and with the same ``R_E``."""
    if mup_func is None:
        raise ValueError("mup_func must be provided \u2014 build it with "
                         "build_mup_function(..., geometry='spherical').")                     # :2216-2219
    if not isinstance(n_and_grad_rphi, _NAndGrad) or not isinstance(mup_func, _MupFunction):
        raise TypeError("n_and_grad_rphi and mup_func must be built with this module's "
                        "build_refractive_index_interpolator_spherical and build_mup_function: there is no CPU path")
    if n_and_grad_rphi.geometry != "spherical" or mup_func.geometry != "spherical":
        raise ValueError("trace_ray_spherical_gradient needs spherical n_and_grad_rphi and mup_func")
    if n_and_grad_rphi.field.R_E != mup_func.field.R_E:
        raise ValueError("n_and_grad_rphi and mup_func must be built with the same R_E")
    if not n_and_grad_rphi.field.same_grid(mup_func.field):
        raise ValueError("n_and_grad_rphi and mup_func must be built on the same z_grid and x_grid")
    field = n_and_grad_rphi._with_mup.get(id(mup_func))
    if field is None or field[0] is not mup_func:
        n_and_grad_rphi._with_mup = {id(mup_func): (mup_func, _merged(n_and_grad_rphi, mup_func))}
        field = n_and_grad_rphi._with_mup[id(mup_func)]
    r = trace_rays_spherical_gradient(field[1], np.float64(x0_km), np.float64(z0_km), np.float64(elevation_deg), None,
                                      s_max_km, R_E=R_E, z_ground_km=z_ground_km, r_max_km=r_max_km, phi_min=phi_min,
                                      phi_max=phi_max, rtol=rtol, atol=atol, max_step_km=max_step_km,
                                      renormalize_every=renormalize_every, return_paths=True)
    n = int(r["n_nodes"])
    out = {k: r[k][:n].copy() for k in _PATH_KEYS_SPHERICAL + ("x", "z")}
    out["status"] = STATUS_NAMES[int(r["status"])]
    for k in _KEYS[:7]:
        out[k] = float(r[k])
    return out
