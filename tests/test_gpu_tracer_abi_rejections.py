"""What the C entry points of the tracers and of the derivatives refuse, which rejection wins where two apply, and that a
refused call leaves the context usable.  tracers.py, gradient.py and library.py validate before they call, so these
rejections are reached through the raw ``Context`` only.

Per entry point: one small fully valid host-buffer call, then a table of cases.  A case changes the named arguments of
the valid call and states ``(rc, part of prhf_last_error)``; every case returns before the library touches the device or
dereferences an array it was not given.  A case with two faults pins the order of the checks.  After its table the entry
point makes the valid call once more: OK and a finite first output."""

import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

BIG = 1 << 31
NAN, INF = float("nan"), float("inf")
BAD_FLAG = 1 << 9


def _native():
    from pyrayhf_amd import _native
    return _native


def _ptr(v):
    """The raw address of an array argument: None stays a null pointer."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    return v.data_ptr()


@pytest.fixture(scope="module")
def ctx():
    return _native().host_context(0)


@pytest.fixture(scope="module")
def null_ctx():
    """A Context whose handle is the null pointer: what a caller of the C ABI passes by mistake."""
    n = _native()
    c = n.Context.__new__(n.Context)
    c._lib = n.load()
    c._h = ctypes.c_void_p()
    c.device = 0
    yield c
    c._h = None


def _run(call, base, cases, ctx, null_ctx, first):
    """The valid call, every case of the table, the valid call again."""
    n = _native()
    rc = call(ctx, base)
    assert rc == n.OK, n.last_error()
    for change, want_rc, text in cases:
        a = dict(base)
        a.update(change)
        c = null_ctx if a.pop("null_ctx", False) else ctx
        rc = call(c, a)
        msg = n.last_error()
        assert rc == want_rc and text in msg, (sorted(change), rc, msg, text)
    out = first(base)
    out[...] = -7.0
    rc = call(ctx, base)
    assert rc == n.OK, n.last_error()
    assert np.isfinite(out.ravel()[0]), out.ravel()[:4]


# ---------------------------------------------------------------------------------------------------------------------
# the Snell family: one Gaussian profile of g8_snell.npz, 2 groups, 2 links, 3 scan elevations, 3 rays
# ---------------------------------------------------------------------------------------------------------------------

def _snell_base():
    n = _native()
    g = load_golden("g8_snell.npz")
    n_alt = g["gauss_alt"].size
    return dict(
        den=np.ascontiguousarray(g["gauss_den"]).reshape(1, -1), bmag=np.ascontiguousarray(g["gauss_bmag"]).reshape(1, -1),
        bpsi=np.ascontiguousarray(g["gauss_bpsi"]).reshape(1, -1), alt=np.ascontiguousarray(g["gauss_alt"]),
        n_prof=1, n_alt=n_alt, alt_stride=0, mode=n.MODE_O, flags=0,
        freq=np.full(3, 5e6), elev=np.array([30.0, 45.0, 60.0]), prof_idx=np.zeros(3, dtype=np.int64), n_rays=3,
        out=np.zeros((3, 8)), path_x=None, path_z=None, path_stride=0,
        geometry=1, r_e=6371.0, dz=1.0, boost=200.0, substeps=400,
        group_freq=np.array([5e6, 6e6]), group_prof=np.zeros(2, dtype=np.int64), n_groups=2,
        ray_group=np.array([0, 1, 1], dtype=np.int64),
        link_group=np.array([0, 1], dtype=np.int64), link_range=np.array([500.0, 600.0]), n_links=2,
        scan=np.array([20.0, 40.0, 60.0]), n_scan=3, range_tol=0.01, max_iter=40, max_roots=2,
        home_out=np.zeros((2, 2, 11)), n_brackets=np.zeros(2, dtype=np.int64),
        elev_tol=1e-6, skip_out=np.zeros((2, 13)),
        link_prof=np.zeros(2, dtype=np.int64), f_lo=2e6, f_hi=2e7, n_bisect=8, muf_out=np.zeros((2, 16)))


def _snell_cartesian(c, a):
    return c.snell_cartesian(_ptr(a["freq"]), _ptr(a["elev"]), _ptr(a["prof_idx"]), a["n_rays"], _ptr(a["den"]), _ptr(a["bmag"]),
                             _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"], a["n_alt"], a["alt_stride"], a["mode"], _ptr(a["out"]),
                             _ptr(a["path_x"]), _ptr(a["path_z"]), a["path_stride"], a["flags"])


def _snell_spherical(c, a):
    return c.snell_spherical(_ptr(a["freq"]), _ptr(a["elev"]), _ptr(a["prof_idx"]), a["n_rays"], _ptr(a["den"]), _ptr(a["bmag"]),
                             _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"], a["n_alt"], a["alt_stride"], a["mode"], a["r_e"], a["dz"],
                             a["boost"], a["substeps"], _ptr(a["out"]), _ptr(a["path_x"]), _ptr(a["path_z"]), a["path_stride"],
                             a["flags"])


def _snell_fan(c, a):
    return c.snell_fan(a["geometry"], _ptr(a["group_freq"]), _ptr(a["group_prof"]), a["n_groups"], _ptr(a["ray_group"]),
                       _ptr(a["elev"]), a["n_rays"], _ptr(a["den"]), _ptr(a["bmag"]), _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"],
                       a["n_alt"], a["alt_stride"], a["mode"], a["r_e"], a["dz"], a["boost"], a["substeps"], _ptr(a["out"]),
                       _ptr(a["path_x"]), _ptr(a["path_z"]), a["path_stride"], a["flags"])


def _snell_home(c, a):
    return c.snell_home(a["geometry"], _ptr(a["group_freq"]), _ptr(a["group_prof"]), a["n_groups"], _ptr(a["link_group"]),
                        _ptr(a["link_range"]), a["n_links"], _ptr(a["scan"]), a["n_scan"], _ptr(a["den"]), _ptr(a["bmag"]),
                        _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"], a["n_alt"], a["alt_stride"], a["mode"], a["r_e"], a["dz"],
                        a["boost"], a["substeps"], a["range_tol"], a["max_iter"], a["max_roots"], _ptr(a["home_out"]),
                        _ptr(a["n_brackets"]), a["flags"])


def _snell_skip(c, a):
    return c.snell_skip(a["geometry"], _ptr(a["group_freq"]), _ptr(a["group_prof"]), a["n_groups"], _ptr(a["scan"]), a["n_scan"],
                        _ptr(a["den"]), _ptr(a["bmag"]), _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"], a["n_alt"], a["alt_stride"],
                        a["mode"], a["r_e"], a["dz"], a["boost"], a["substeps"], a["elev_tol"], a["max_iter"], _ptr(a["skip_out"]),
                        a["flags"])


def _snell_muf(c, a):
    return c.snell_muf(a["geometry"], _ptr(a["link_prof"]), _ptr(a["link_range"]), a["n_links"], a["f_lo"], a["f_hi"], a["n_bisect"],
                       _ptr(a["scan"]), a["n_scan"], _ptr(a["den"]), _ptr(a["bmag"]), _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"],
                       a["n_alt"], a["alt_stride"], a["mode"], a["r_e"], a["dz"], a["boost"], a["substeps"], a["elev_tol"],
                       a["max_iter"], _ptr(a["muf_out"]), a["flags"])


I64 = lambda *v: np.array(v, dtype=np.int64)          # noqa: E731
F64 = lambda *v: np.array(v, dtype=np.float64)        # noqa: E731
_PATH = np.zeros((3, 401))

# (the lines and the function names - snell_run, skip_run, grad_*_run, grad_search_check, check_field_shape - are those of
# prhf_api.cpp before the drivers were assembled from shared steps)
# snell_run, :1728-1758: context, arrays, [groups], level tables, shape, [profiles], paths, stride, mode, alt stride, flags,
# n_rays == 0, then the two host range loops
_SNELL_RUN = [
    (dict(null_ctx=True), "EINVAL", "null context"),                                             # :1728
    (dict(den=None), "EINVAL", "null array pointer"),                                            # :1729
    (dict(out=None), "EINVAL", "null array pointer"),
    (dict(n_rays=-1), "EINVAL", "bad shape"),                                                    # :1741
    (dict(n_prof=0), "EINVAL", "bad shape"),
    (dict(n_alt=1), "EINVAL", "bad shape"),
    (dict(n_alt=3001), "EINVAL", "bad shape"),
    (dict(path_x=_PATH), "EINVAL", "path_x and path_z go together"),                             # :1743
    (dict(path_x=_PATH, path_z=_PATH, path_stride=400), "EINVAL", "path_stride must hold"),      # :1744
    (dict(mode=7), "EINVAL", "Mode must be O or X"),                                             # :1746
    (dict(alt_stride=5), "EINVAL", "alt stride is 0 or n_alt"),                                  # :1747
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                       # :1748
    # two at once
    (dict(null_ctx=True, den=None), "EINVAL", "null context"),
    (dict(bpsi=None, n_alt=1), "EINVAL", "null array pointer"),
    (dict(n_alt=1, mode=7), "EINVAL", "bad shape"),
    (dict(path_x=_PATH, mode=7), "EINVAL", "path_x and path_z go together"),
    (dict(mode=7, alt_stride=5), "EINVAL", "Mode must be O or X"),
    (dict(alt_stride=5, flags=BAD_FLAG), "EINVAL", "alt stride is 0 or n_alt"),
    (dict(n_rays=0, flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                             # (a zero-size call is checked too)
]
_SNELL_PER_RAY = _SNELL_RUN + [
    (dict(freq=None), "EINVAL", "null array pointer"),                                           # :1729
    (dict(elev=None, n_alt=1), "EINVAL", "null array pointer"),
    (dict(prof_idx=I64(0, 1, 0)), "EINVAL", "profile_index[1] outside [0, n_prof)"),             # :1754
    (dict(prof_idx=I64(0, 0, -1)), "EINVAL", "profile_index[2] outside [0, n_prof)"),
    (dict(prof_idx=I64(0, 1, 0), flags=BAD_FLAG), "EINVAL", "unknown flag bits"),
    (dict(n_rays=0, prof_idx=I64(5, 5, 5)), "OK", ""),                                           # :1749 comes before the loops
]
_SPHERICAL_CONTROLS = [                                                                          # :1921, :1936, :1957, :2102
    (dict(r_e=0.0), "EINVAL", "bad spherical tracer controls"),
    (dict(r_e=NAN), "EINVAL", "bad spherical tracer controls"),
    (dict(r_e=INF), "EINVAL", "bad spherical tracer controls"),
    (dict(dz=0.0), "EINVAL", "bad spherical tracer controls"),
    (dict(boost=-1.0), "EINVAL", "bad spherical tracer controls"),
    (dict(substeps=0), "EINVAL", "bad spherical tracer controls"),
]
_GEOMETRY = [
    (dict(geometry=2), "EINVAL", "geometry is 0 (flat Earth) or 1 (spherical Earth)"),
    (dict(geometry=-1), "EINVAL", "geometry is 0 (flat Earth) or 1 (spherical Earth)"),
    (dict(geometry=0, r_e=0.0, dz=0.0, boost=-1.0, substeps=0), "OK", ""),                       # (flat Earth ignores the controls)
]

SNELL = {
    "snell_cartesian": (_snell_cartesian, _SNELL_PER_RAY, "out"),
    # prhf_snell_spherical_f64 checks its controls first (:1921), then snell_run
    "snell_spherical": (_snell_spherical, _SPHERICAL_CONTROLS + _SNELL_PER_RAY + [
        (dict(null_ctx=True, r_e=0.0), "EINVAL", "bad spherical tracer controls"),
        (dict(freq=None, dz=-1.0), "EINVAL", "bad spherical tracer controls"),
    ], "out"),
    # prhf_snell_fan_f64: geometry, ray_group, controls (:1934-1938), then snell_run with its grouped checks
    "snell_fan": (_snell_fan, _GEOMETRY + _SPHERICAL_CONTROLS + _SNELL_RUN + [
        (dict(ray_group=None), "EINVAL", "null array pointer"),                                  # :1935
        (dict(n_groups=0), "EINVAL", "a grouped launch needs at least one group"),               # :1732
        (dict(n_groups=BIG), "EINVAL", "level tables of 2147483648 groups exceed 64 GiB (or 2^31 - 1 groups / rays): "
                                       "trace in batches"),                                      # :1738
        (dict(n_groups=BIG, n_rays=0), "EINVAL", "(or 2^31 - 1 groups / rays): trace in batches"),   # (:1738 before :1749)
        (dict(n_rays=BIG), "EINVAL", "level tables of 2 groups exceed 64 GiB (or 2^31 - 1 groups / rays): trace in batches"),
        (dict(n_prof=BIG), "EINVAL", "a grouped launch takes at most 2^31 - 1 profiles"),        # :1742
        (dict(group_freq=None), "EINVAL", "null array pointer"),                                 # :1729
        (dict(group_prof=I64(0, 3)), "EINVAL", "profile_index[1] outside [0, n_prof)"),          # :1754
        (dict(ray_group=I64(0, 2, 1)), "EINVAL", "ray_group[1] outside [0, n_groups)"),          # :1758
        (dict(ray_group=I64(-1, 0, 1)), "EINVAL", "ray_group[0] outside [0, n_groups)"),
        (dict(null_ctx=True, geometry=2), "EINVAL", "geometry is 0"),
        (dict(geometry=2, ray_group=None), "EINVAL", "geometry is 0"),
        (dict(ray_group=None, r_e=0.0), "EINVAL", "null array pointer"),
        (dict(r_e=0.0, null_ctx=True), "EINVAL", "bad spherical tracer controls"),
        (dict(n_groups=0, den=None), "EINVAL", "null array pointer"),
        (dict(n_groups=BIG, n_alt=1), "EINVAL", "level tables of"),
        (dict(group_prof=I64(0, 3), ray_group=I64(0, 2, 1)), "EINVAL", "profile_index[1]"),
    ], "out"),
    # prhf_snell_home_f64, :1952-1992
    "snell_home": (_snell_home, _GEOMETRY + _SPHERICAL_CONTROLS + [
        (dict(null_ctx=True), "EINVAL", "null context"),                                         # :1952
        (dict(group_freq=None), "EINVAL", "null array pointer"),                                 # :1953
        (dict(n_brackets=None), "EINVAL", "null array pointer"),
        (dict(link_group=None), "EINVAL", "null array pointer"),
        (dict(n_scan=1), "EINVAL", "the scan grid needs at least 2 elevations"),                 # :1960
        (dict(max_iter=0), "EINVAL", "max_iter is 1 .. 128"),                                    # :1961
        (dict(max_iter=129), "EINVAL", "max_iter is 1 .. 128"),
        (dict(max_roots=0), "EINVAL", "max_roots is 1 .. 64"),                                   # :1962
        (dict(max_roots=65), "EINVAL", "max_roots is 1 .. 64"),
        (dict(range_tol=-1.0), "EINVAL", "range_tol_km must be finite and not negative"),        # :1963
        (dict(range_tol=INF), "EINVAL", "range_tol_km must be finite and not negative"),
        (dict(n_groups=0), "EINVAL", "homing needs at least one group"),                         # :1965
        (dict(n_groups=BIG), "EINVAL", "level tables of 2147483648 groups exceed 64 GiB (or 2^31 - 1 groups): home in batches"),
        (dict(n_links=-1), "EINVAL", "bad shape"),                                               # :1973
        (dict(n_prof=0), "EINVAL", "bad shape"),
        (dict(n_prof=BIG), "EINVAL", "bad shape"),
        (dict(n_alt=1), "EINVAL", "bad shape"),
        (dict(n_alt=3001), "EINVAL", "bad shape"),
        (dict(n_scan=BIG), "EINVAL", "more than 2^31 - 1 scan rays or result rows: home in batches"),      # :1974
        (dict(n_links=BIG), "EINVAL", "more than 2^31 - 1 scan rays or result rows: home in batches"),
        (dict(mode=7), "EINVAL", "Mode must be O or X"),                                         # :1976
        (dict(alt_stride=5), "EINVAL", "alt stride is 0 or n_alt"),                              # :1977
        (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                   # :1978
        (dict(scan=F64(20.0, 20.0, 60.0)), "EINVAL", "scan_elevation_deg must be strictly increasing"),    # :1983
        (dict(scan=F64(20.0, NAN, 60.0)), "EINVAL", "scan_elevation_deg must be strictly increasing"),
        (dict(group_prof=I64(0, 1)), "EINVAL", "profile_index[1] outside [0, n_prof)"),          # :1987
        (dict(link_group=I64(0, 2)), "EINVAL", "link_group[1] outside [0, n_groups)"),           # :1990
        (dict(link_group=I64(-1, 0)), "EINVAL", "link_group[0] outside [0, n_groups)"),
        (dict(n_links=0, link_group=I64(9, 9)), "OK", ""),                                       # :1992 (no link: no loop, no launch)
        (dict(n_links=0, group_prof=I64(0, 1)), "EINVAL", "profile_index[1]"),                   # (a zero-size call is checked)
        (dict(null_ctx=True, den=None), "EINVAL", "null context"),
        (dict(den=None, geometry=2), "EINVAL", "null array pointer"),
        (dict(geometry=2, n_scan=1), "EINVAL", "geometry is 0"),
        (dict(r_e=0.0, n_scan=1), "EINVAL", "bad spherical tracer controls"),
        (dict(n_scan=1, max_iter=0), "EINVAL", "the scan grid needs"),
        (dict(max_iter=0, max_roots=0), "EINVAL", "max_iter is"),
        (dict(max_roots=0, range_tol=-1.0), "EINVAL", "max_roots is"),
        (dict(range_tol=NAN, n_groups=0), "EINVAL", "range_tol_km"),
        (dict(n_groups=BIG, n_alt=1), "EINVAL", "level tables of"),
        (dict(n_alt=1, n_scan=BIG), "EINVAL", "bad shape"),
        (dict(n_scan=BIG, mode=7), "EINVAL", "more than 2^31 - 1"),
        (dict(mode=7, alt_stride=5), "EINVAL", "Mode must be"),
        (dict(alt_stride=5, flags=BAD_FLAG), "EINVAL", "alt stride"),
        (dict(flags=BAD_FLAG, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "unknown flag bits"),
        (dict(scan=F64(3.0, 2.0, 1.0), group_prof=I64(0, 1)), "EINVAL", "strictly increasing"),
        (dict(group_prof=I64(0, 1), link_group=I64(0, 2)), "EINVAL", "profile_index[1]"),
    ], "home_out"),
}

# skip_run, :2098-2137, behind the wrappers' own checks (:2248, :2260-2261)
_SKIP_RUN = _GEOMETRY + _SPHERICAL_CONTROLS + [
    (dict(null_ctx=True), "EINVAL", "null context"),                                             # :2098
    (dict(scan=None), "EINVAL", "null array pointer"),                                           # :2099
    (dict(alt=None), "EINVAL", "null array pointer"),
    (dict(n_scan=0), "EINVAL", "the scan grid needs at least 1 elevation"),                      # :2105
    (dict(max_iter=0), "EINVAL", "max_iter is 1 .. 128"),                                        # :2106
    (dict(max_iter=129), "EINVAL", "max_iter is 1 .. 128"),
    (dict(elev_tol=-1.0), "EINVAL", "elev_tol_deg must be finite and not negative"),             # :2107
    (dict(elev_tol=NAN), "EINVAL", "elev_tol_deg must be finite and not negative"),
    (dict(n_prof=0), "EINVAL", "bad shape"),                                                     # :2114
    (dict(n_prof=BIG), "EINVAL", "bad shape"),
    (dict(n_alt=1), "EINVAL", "bad shape"),
    (dict(n_alt=3001), "EINVAL", "bad shape"),
    (dict(n_scan=BIG), "EINVAL", "more than 2^31 - 1 scan rays: search in batches"),            # :2122
    (dict(mode=7), "EINVAL", "Mode must be O or X"),                                             # :2123
    (dict(alt_stride=5), "EINVAL", "alt stride is 0 or n_alt"),                                  # :2124
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                       # :2125
    (dict(scan=F64(20.0, 20.0, 60.0)), "EINVAL", "scan_elevation_deg must be strictly increasing"),        # :2130
    (dict(scan=F64(NAN), n_scan=1), "EINVAL", "scan_elevation_deg must be finite"),              # :2131
    (dict(scan=F64(INF), n_scan=1), "EINVAL", "scan_elevation_deg must be finite"),
    (dict(null_ctx=True, scan=None), "EINVAL", "null context"),
    (dict(scan=None, geometry=2), "EINVAL", "null array pointer"),
    (dict(geometry=2, flags=BAD_FLAG), "EINVAL", "geometry is 0"),
    (dict(r_e=0.0, n_scan=0), "EINVAL", "bad spherical tracer controls"),
    (dict(n_scan=0, max_iter=0), "EINVAL", "the scan grid needs"),
    (dict(max_iter=0, elev_tol=-1.0), "EINVAL", "max_iter is"),
    (dict(n_alt=1, n_scan=BIG), "EINVAL", "bad shape"),
    (dict(n_scan=BIG, mode=7), "EINVAL", "more than 2^31 - 1 scan rays"),
    (dict(mode=7, alt_stride=5), "EINVAL", "Mode must be"),
    (dict(alt_stride=5, flags=BAD_FLAG), "EINVAL", "alt stride"),
    (dict(flags=BAD_FLAG, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "unknown flag bits"),
    (dict(max_iter=0, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "max_iter is"),
]
SNELL["snell_skip"] = (_snell_skip, _SKIP_RUN + [
    (dict(n_groups=0), "EINVAL", "the search needs at least one group"),                         # :2248
    (dict(n_groups=-1), "EINVAL", "the search needs at least one group"),
    (dict(group_freq=None), "EINVAL", "null array pointer"),                                     # :2099
    (dict(n_groups=BIG), "EINVAL", "level tables of 2147483648 groups exceed 64 GiB (or 2^31 - 1 groups): search in batches"),
    (dict(group_prof=I64(0, 1)), "EINVAL", "profile_index[1] outside [0, n_prof)"),              # :2135
    (dict(n_groups=0, null_ctx=True), "EINVAL", "null context"),                                 # (:2248 asks for a context)
    (dict(n_groups=0, scan=None), "EINVAL", "the search needs at least one group"),
    (dict(elev_tol=-1.0, n_groups=BIG), "EINVAL", "elev_tol_deg"),
    (dict(n_groups=BIG, n_alt=1), "EINVAL", "bad shape"),                                        # (:2114 before :2119)
    (dict(n_groups=BIG, mode=7), "EINVAL", "level tables of"),
    (dict(scan=F64(3.0, 2.0, 1.0), group_prof=I64(0, 1)), "EINVAL", "strictly increasing"),
], "skip_out")
SNELL["snell_muf"] = (_snell_muf, _SKIP_RUN + [
    (dict(link_range=None), "EINVAL", "null array pointer"),                                     # :2260
    (dict(n_links=0), "EINVAL", "the search needs at least one link"),                           # :2261
    (dict(n_bisect=0), "EINVAL", "n_bisect is 1 .. 64"),                                         # :2110
    (dict(n_bisect=65), "EINVAL", "n_bisect is 1 .. 64"),
    (dict(f_lo=0.0), "EINVAL", "the frequency bracket needs 0 < f_lo_hz < f_hi_hz, both finite"),          # :2111
    (dict(f_hi=1e6), "EINVAL", "the frequency bracket needs"),
    (dict(f_hi=INF), "EINVAL", "the frequency bracket needs"),
    (dict(f_lo=NAN), "EINVAL", "the frequency bracket needs"),
    (dict(n_links=BIG), "EINVAL", "level tables of 2147483648 groups exceed 64 GiB (or 2^31 - 1 groups): search in batches"),
    (dict(link_prof=I64(0, 1)), "EINVAL", "profile_index[1] outside [0, n_prof)"),               # :2135
    (dict(link_range=None, n_links=0), "EINVAL", "null array pointer"),
    (dict(n_links=0, geometry=2), "EINVAL", "the search needs at least one link"),
    (dict(elev_tol=-1.0, n_bisect=0), "EINVAL", "elev_tol_deg"),
    (dict(n_bisect=0, f_lo=0.0), "EINVAL", "n_bisect is"),
    (dict(f_lo=0.0, n_alt=1), "EINVAL", "the frequency bracket needs"),
], "muf_out")


@pytest.mark.parametrize("name", sorted(SNELL))
def test_snell_entry_point_rejections(name, ctx, null_ctx):
    n = _native()
    call, cases, out_key = SNELL[name]
    base = _snell_base()
    _run(call, base, [(ch, getattr(n, rc), text) for ch, rc, text in cases], ctx, null_ctx, lambda a: a[out_key])


# ---------------------------------------------------------------------------------------------------------------------
# the gradient family: a 4 x 4 field of two frequencies built with field_build, 2 groups, 2 links, 3 scan elevations, 3 rays
# ---------------------------------------------------------------------------------------------------------------------

R_E = 6371.0
N_HOPS = 2


def _grad_base(geo):
    """Per geometry: a horizontally uniform layer on a 4 x 4 grid whose density grows linearly with height, X = 0.9 at the
    top for 10 MHz, and its records for 10 and 11 MHz on the device.  A ray of elevation e through such a layer turns at
    about 500 sin(e)^2 km (605 at 11 MHz) and lands about 1000 sin(2 e) km away (1210): 643, 866 and 985 km for the scan
    below, inside the grid, so the links at 750 and 900 km have a bracket each and the searches a finite skip; the
    two-hop calls land further out and have targets of their own."""
    import torch
    n = _native()
    z = np.array([0.0, 150.0, 300.0, 450.0])
    x = np.array([-2000.0, -500.0, 1000.0, 2500.0])
    den = np.ascontiguousarray(np.repeat((0.9 * 1e14 / 80.6 * z / 450.0)[:, None], 4, axis=1))
    bmag = np.full((4, 4), 4.5e-5)
    bpsi = np.full((4, 4), 60.0)
    axis0, axis1 = (R_E + z, x / R_E) if geo else (z, x)
    freq = np.array([10e6, 11e6])
    rec = torch.empty((2, 4, 4, 4), dtype=torch.float64, device="cuda")
    c = n.host_context(0)
    n.raise_for(c.field_build(den.ctypes.data, bmag.ctypes.data, bpsi.ctypes.data, 4, 4, axis0.ctypes.data, axis1.ctypes.data,
                              freq.ctypes.data, 2, n.MODE_O, 2, rec.data_ptr(), None, None, 0))
    top, left, right = (R_E + 450.0, -2000.0 / R_E, 2500.0 / R_E) if geo else (450.0, -2000.0, 2500.0)
    # the two-hop homing call aims between the landings of the second hop at the first two scan elevations of its group
    hops, origin, elev, field = np.zeros((4, N_HOPS, 15)), np.zeros(4), np.array([20.0, 30.0, 20.0, 30.0]), I64(0, 0, 1, 1)
    n.raise_for(c.trace_gradient_hops(geo, rec.data_ptr(), 2, 4, 4, axis0.ctypes.data, axis1.ctypes.data, origin.ctypes.data,
                                      origin.ctypes.data, elev.ctypes.data, field.ctypes.data, 4, R_E if geo else 0.0,
                                      (3000.0, 1e-6, 1e-9, 10.0, 0.0, top, left, right, 50), (NAN, 0.0, NAN), N_HOPS,
                                      hops.ctypes.data, None, 0, 0))
    landing = hops[:, N_HOPS - 1, 3 + 4].reshape(2, 2)                   # (group, scan node): ground_range_km of the last hop
    return dict(
        geometry=geo, records=rec, n_fields=2, n0=4, n1=4, axis0=np.ascontiguousarray(axis0), axis1=np.ascontiguousarray(axis1),
        r_e=R_E if geo else 0.0, s_max=3000.0, rtol=1e-6, atol=1e-9, max_step=10.0, z_ground=0.0, top=top, left=left, right=right,
        renorm=50, fills=(NAN, 0.0, NAN), flags=0,
        x0=np.zeros(3), z0=np.zeros(3), elev=np.array([30.0, 45.0, 60.0]), ray_field=I64(0, 1, 0), n_rays=3,
        out=np.zeros((3, 12)), hops_out=np.zeros((3, N_HOPS, 15)), paths=None, path_stride=0, n_hops=N_HOPS,
        group_field=I64(0, 1), group_x0=np.zeros(2), group_z0=np.zeros(2), n_groups=2,
        link_group=I64(0, 1), link_target=np.array([750.0, 900.0]), hop_link_target=landing.mean(axis=1), hop_landing=landing, n_links=2,
        scan=np.array([20.0, 30.0, 40.0]), n_scan=3, range_tol=0.01, max_iter=30, max_roots=2,
        home_out=np.zeros((2, 2, 15)), hop_home_out=np.zeros((2, 2, 3 + 15 * N_HOPS)), n_brackets=np.zeros(2, dtype=np.int64),
        elev_tol=1e-4, skip_out=np.zeros((2, 18)), hop_skip_out=np.zeros((2, 6 + 15 * N_HOPS)),
        den=den, bmag=bmag, bpsi=bpsi, mode=n.MODE_O, edge_order=2, link_x0=np.zeros(2), link_z0=np.zeros(2),
        muf_target=np.array([900.0, 1100.0]), hop_muf_target=np.array([1800.0, 2100.0]),
        f_lo=10e6, f_hi=20e6, n_bisect=4, muf_out=np.zeros((2, 21)), hop_muf_out=np.zeros((2, 3 + 6 + 15 * N_HOPS)))


def _ctl(a):
    return (a["s_max"], a["rtol"], a["atol"], a["max_step"], a["z_ground"], a["top"], a["left"], a["right"], a["renorm"])


def _paths(a):
    return None if a["paths"] is None else [_ptr(p) for p in a["paths"]]


def _grid(a):
    return (_ptr(a["records"]), a["n_fields"], a["n0"], a["n1"], _ptr(a["axis0"]), _ptr(a["axis1"]))


def _rays(a):
    return (_ptr(a["x0"]), _ptr(a["z0"]), _ptr(a["elev"]), _ptr(a["ray_field"]), a["n_rays"])


def _groups(a):
    return (_ptr(a["group_field"]), _ptr(a["group_x0"]), _ptr(a["group_z0"]), a["n_groups"])


def _trace_gradient(c, a):
    return c.trace_gradient(*_grid(a), *_rays(a), _ctl(a), a["fills"], _ptr(a["out"]), _paths(a), a["path_stride"], a["flags"])


def _trace_gradient_spherical(c, a):
    return c.trace_gradient_spherical(*_grid(a), *_rays(a), a["r_e"], _ctl(a), a["fills"], _ptr(a["out"]), _paths(a),
                                      a["path_stride"], a["flags"])


def _trace_gradient_hops(c, a):
    return c.trace_gradient_hops(a["geometry"], *_grid(a), *_rays(a), a["r_e"], _ctl(a), a["fills"], a["n_hops"],
                                 _ptr(a["hops_out"]), _paths(a), a["path_stride"], a["flags"])


def _gradient_home(c, a):
    return c.gradient_home(a["geometry"], *_grid(a), *_groups(a), _ptr(a["link_group"]), _ptr(a["link_target"]), a["n_links"],
                           _ptr(a["scan"]), a["n_scan"], a["r_e"], _ctl(a), a["fills"], a["range_tol"], a["max_iter"],
                           a["max_roots"], _ptr(a["home_out"]), _ptr(a["n_brackets"]), a["flags"])


def _gradient_hop_home(c, a):
    return c.gradient_hop_home(a["geometry"], *_grid(a), *_groups(a), _ptr(a["link_group"]), _ptr(a["hop_link_target"]), a["n_links"],
                               _ptr(a["scan"]), a["n_scan"], a["r_e"], _ctl(a), a["fills"], a["range_tol"], a["max_iter"],
                               a["max_roots"], a["n_hops"], _ptr(a["hop_home_out"]), _ptr(a["n_brackets"]), a["flags"])


def _gradient_skip(c, a):
    return c.gradient_skip(a["geometry"], *_grid(a), *_groups(a), _ptr(a["scan"]), a["n_scan"], a["r_e"], _ctl(a), a["fills"],
                           a["elev_tol"], a["max_iter"], _ptr(a["skip_out"]), a["flags"])


def _gradient_hop_skip(c, a):
    return c.gradient_hop_skip(a["geometry"], *_grid(a), *_groups(a), _ptr(a["scan"]), a["n_scan"], a["r_e"], _ctl(a), a["fills"],
                               a["elev_tol"], a["max_iter"], a["n_hops"], _ptr(a["hop_skip_out"]), a["flags"])


def _muf_head(a, target="muf_target"):
    return (a["geometry"], _ptr(a["den"]), _ptr(a["bmag"]), _ptr(a["bpsi"]), a["n0"], a["n1"], _ptr(a["axis0"]), _ptr(a["axis1"]),
            a["mode"], a["edge_order"], _ptr(a["link_x0"]), _ptr(a["link_z0"]), _ptr(a[target]), a["n_links"], a["f_lo"],
            a["f_hi"], a["n_bisect"], _ptr(a["scan"]), a["n_scan"], a["r_e"], _ctl(a), a["fills"], a["elev_tol"], a["max_iter"])


def _gradient_muf(c, a):
    return c.gradient_muf(*_muf_head(a), _ptr(a["muf_out"]), a["flags"])


def _gradient_hop_muf(c, a):
    return c.gradient_hop_muf(*_muf_head(a, "hop_muf_target"), a["n_hops"], _ptr(a["hop_muf_out"]), a["flags"])


_P5 = [np.zeros((3 * N_HOPS, 8)) for _ in range(5)]
_DOWN = F64(0.0, 300.0, 150.0, 450.0)

# what every gradient entry point says of the tracer's controls (:2398-2401, :2535-2538, :2684-2687), in this order
_TRACER_CONTROLS = [
    (dict(s_max=0.0), "EINVAL", "s_max_km must be positive and finite"),
    (dict(s_max=INF), "EINVAL", "s_max_km must be positive and finite"),
    (dict(s_max=NAN), "EINVAL", "s_max_km must be positive and finite"),
    (dict(max_step=0.0), "EINVAL", "`max_step` must be positive."),
    (dict(max_step=NAN), "EINVAL", "`max_step` must be positive."),
    (dict(rtol=-1.0), "EINVAL", "`atol` must be positive."),
    (dict(atol=-1.0), "EINVAL", "`atol` must be positive."),
    (dict(atol=NAN), "EINVAL", "`atol` must be positive."),
    (dict(renorm=-1), "EINVAL", "renormalize_every must not be negative"),
    (dict(s_max=0.0, max_step=0.0), "EINVAL", "s_max_km"),
    (dict(max_step=0.0, rtol=-1.0), "EINVAL", "`max_step`"),
    (dict(atol=-1.0, renorm=-1), "EINVAL", "`atol`"),
]
# check_field_shape, :2283-2288; least: what check_axis asks of either axis
def _field_shape(least):
    return [
        (dict(axis0=None), "EINVAL", "null array pointer"),
        (dict(axis1=None), "EINVAL", "null array pointer"),
        (dict(n0=0), "EINVAL", "bad shape (the two axes hold at most 8000 values together)"),
        (dict(n1=0), "EINVAL", "bad shape (the two axes hold at most"),
        (dict(n0=8000), "EINVAL", "bad shape (the two axes hold at most"),
        (dict(n0=least - 1), "EINVAL", "axis 0 needs at least %d values" % least),
        (dict(n1=least - 1), "EINVAL", "axis 1 needs at least %d values" % least),
        (dict(axis0=_DOWN), "EINVAL", "axis 0 must be strictly increasing"),
        (dict(axis1=_DOWN), "EINVAL", "axis 1 must be strictly increasing"),
        (dict(axis0=F64(0.0, NAN, 300.0, 450.0)), "EINVAL", "axis 0 must be strictly increasing"),
        (dict(axis0=None, n0=0), "EINVAL", "null array pointer"),
        (dict(n0=least - 1, axis1=_DOWN), "EINVAL", "axis 0 needs"),
        (dict(axis0=_DOWN, axis1=_DOWN), "EINVAL", "axis 0 must be"),
    ]


_N_FIELDS = [
    (dict(n_fields=0), "EINVAL", "bad shape (the two axes hold at most"),
    (dict(n_fields=(1 << 24) + 1), "EINVAL", "bad shape (the two axes hold at most"),
]
# grad_trace_run, :2391-2410
_GRAD_TRACE = [
    (dict(null_ctx=True), "EINVAL", "null context"),                                             # :2391
    (dict(records=None), "EINVAL", "null array pointer"),                                        # :2392
    (dict(elev=None), "EINVAL", "null array pointer"),
    (dict(n_rays=-1), "EINVAL", "bad shape"),                                                    # :2393
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                       # :2394
    (dict(paths=_P5[:4] + [None]), "EINVAL", "the five path arrays go together"),                # :2396
    (dict(paths=[None] + _P5[1:]), "EINVAL", "the five path arrays go together"),
    (dict(paths=_P5, path_stride=0), "EINVAL", "path_stride must hold at least the launch point"),         # :2397
] + _TRACER_CONTROLS + _field_shape(2) + _N_FIELDS + [
    (dict(ray_field=I64(0, 2, 0)), "EINVAL", "ray_field[1] outside [0, n_fields)"),              # :2409
    (dict(ray_field=I64(0, 0, -1)), "EINVAL", "ray_field[2] outside [0, n_fields)"),
    (dict(n_rays=0, ray_field=I64(9, 9, 9)), "OK", ""),                                          # :2410
    (dict(n_rays=0, axis0=_DOWN), "EINVAL", "axis 0 must be"),                                   # (a zero-size call is checked)
    (dict(null_ctx=True, records=None), "EINVAL", "null context"),
    (dict(x0=None, n_rays=-1), "EINVAL", "null array pointer"),
    (dict(n_rays=-1, flags=BAD_FLAG), "EINVAL", "bad shape"),
    (dict(flags=BAD_FLAG, paths=_P5[:4] + [None]), "EINVAL", "unknown flag bits"),
    (dict(paths=_P5, path_stride=0, s_max=0.0), "EINVAL", "path_stride must hold"),
    (dict(renorm=-1, axis0=None), "EINVAL", "renormalize_every"),
    (dict(axis1=_DOWN, ray_field=I64(0, 2, 0)), "EINVAL", "axis 1 must be"),
]
_RADIUS = [
    (dict(r_e=0.0), "EINVAL", "earth_radius_km must be positive and finite"),
    (dict(r_e=INF), "EINVAL", "earth_radius_km must be positive and finite"),
    (dict(r_e=NAN), "EINVAL", "earth_radius_km must be positive and finite"),
]
_GRAD_GEOMETRY = [
    (dict(geometry=2), "EINVAL", "geometry is 0 (Cartesian) or 1 (spherical)"),
    (dict(geometry=-1), "EINVAL", "geometry is 0 (Cartesian) or 1 (spherical)"),
]
_N_HOPS = [
    (dict(n_hops=0), "EINVAL", "n_hops is 1 .. 16"),
    (dict(n_hops=17), "EINVAL", "n_hops is 1 .. 16"),
    (dict(null_ctx=True, n_hops=0), "EINVAL", "null context"),
]
# grad_home_run, :2527-2564, behind the wrappers' null context and n_hops (:2644, :2660-2661)
_GRAD_HOME = _GRAD_GEOMETRY + [
    (dict(null_ctx=True), "EINVAL", "null context"),
    (dict(records=None), "EINVAL", "null array pointer"),                                        # :2527
    (dict(group_field=None), "EINVAL", "null array pointer"),
    (dict(n_brackets=None), "EINVAL", "null array pointer"),
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                       # :2534
] + _TRACER_CONTROLS + [
    (dict(n_scan=1), "EINVAL", "the scan grid needs at least 2 elevations"),                     # :2539
    (dict(max_iter=0), "EINVAL", "max_iter is 1 .. 128"),                                        # :2540
    (dict(max_iter=129), "EINVAL", "max_iter is 1 .. 128"),
    (dict(max_roots=0), "EINVAL", "max_roots is 1 .. 64"),                                       # :2541
    (dict(max_roots=65), "EINVAL", "max_roots is 1 .. 64"),
    (dict(range_tol=-1.0), "EINVAL", "range_tol_km must be finite and not negative"),            # :2542
    (dict(range_tol=INF), "EINVAL", "range_tol_km must be finite and not negative"),
    (dict(n_groups=0), "EINVAL", "homing needs at least one group"),                             # :2544
    (dict(n_links=-1), "EINVAL", "bad shape"),                                                   # :2545
    (dict(n_scan=BIG), "EINVAL", "more than 2^31 - 1 scan rays or result rows: home in batches"),          # :2546
    (dict(n_links=BIG), "EINVAL", "more than 2^31 - 1 scan rays or result rows: home in batches"),
    (dict(n_groups=1 << 40), "EINVAL", "more than 2^31 - 1 scan rays or result rows: home in batches"),
] + _field_shape(2) + _N_FIELDS + [
    (dict(scan=F64(20.0, 20.0, 60.0)), "EINVAL", "scan_elevation_deg must be strictly increasing"),        # :2555
    (dict(group_field=I64(0, 2)), "EINVAL", "group_field[1] outside [0, n_fields)"),             # :2558
    (dict(link_group=I64(0, 2)), "EINVAL", "link_group[1] outside [0, n_groups)"),               # :2561
    (dict(link_group=I64(-1, 0)), "EINVAL", "link_group[0] outside [0, n_groups)"),
    (dict(n_links=0, link_group=I64(9, 9)), "OK", ""),                                           # :2564
    (dict(n_links=0, group_field=I64(0, 2)), "EINVAL", "group_field[1]"),
    (dict(records=None, geometry=2), "EINVAL", "null array pointer"),
    (dict(geometry=2, flags=BAD_FLAG), "EINVAL", "geometry is 0"),
    (dict(flags=BAD_FLAG, s_max=0.0), "EINVAL", "unknown flag bits"),
    (dict(renorm=-1, n_scan=1), "EINVAL", "renormalize_every"),
    (dict(n_scan=1, max_iter=0), "EINVAL", "the scan grid needs"),
    (dict(max_iter=0, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "max_iter is"),
    (dict(max_roots=0, range_tol=-1.0), "EINVAL", "max_roots is"),
    (dict(range_tol=-1.0, n_groups=0), "EINVAL", "range_tol_km"),
    (dict(n_groups=0, n_links=-1), "EINVAL", "homing needs"),
    (dict(n_links=-1, axis0=None), "EINVAL", "bad shape"),
    (dict(n_scan=BIG, axis0=_DOWN), "EINVAL", "more than 2^31 - 1"),
    (dict(axis0=_DOWN, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "axis 0 must be"),
    (dict(scan=F64(3.0, 2.0, 1.0), group_field=I64(0, 2)), "EINVAL", "strictly increasing"),
    (dict(group_field=I64(0, 2), link_group=I64(0, 2)), "EINVAL", "group_field[1]"),
]
# grad_search_check (:2679-2691) as grad_skip_run and grad_muf_run use it
def _grad_search(least):
    return _GRAD_GEOMETRY + [
    (dict(null_ctx=True), "EINVAL", "null context"),
    (dict(scan=None), "EINVAL", "null array pointer"),
    (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                       # :2683
] + _TRACER_CONTROLS + [
    (dict(n_scan=0), "EINVAL", "the scan grid needs at least 1 elevation"),                      # :2688
    (dict(n_scan=BIG), "EINVAL", "the scan grid needs at least 1 elevation"),
    (dict(max_iter=0), "EINVAL", "max_iter is 1 .. 128"),                                        # :2689
    (dict(max_iter=129), "EINVAL", "max_iter is 1 .. 128"),
    (dict(elev_tol=-1.0), "EINVAL", "elev_tol_deg must be finite and not negative"),             # :2690
    (dict(elev_tol=INF), "EINVAL", "elev_tol_deg must be finite and not negative"),
] + _field_shape(least) + [
    (dict(scan=F64(20.0, 20.0, 60.0)), "EINVAL", "scan_elevation_deg must be strictly increasing"),        # :2697
    (dict(scan=F64(NAN), n_scan=1), "EINVAL", "scan_elevation_deg must be finite"),              # :2698
    (dict(scan=None, geometry=2), "EINVAL", "null array pointer"),
    (dict(geometry=2, flags=BAD_FLAG), "EINVAL", "geometry is 0"),
    (dict(flags=BAD_FLAG, s_max=0.0), "EINVAL", "unknown flag bits"),
    (dict(renorm=-1, n_scan=0), "EINVAL", "renormalize_every"),
    (dict(n_scan=0, max_iter=0), "EINVAL", "the scan grid needs"),
    (dict(max_iter=0, elev_tol=-1.0), "EINVAL", "max_iter is"),
    (dict(max_iter=0, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "max_iter is"),
    (dict(axis0=_DOWN, scan=F64(3.0, 2.0, 1.0)), "EINVAL", "axis 0 must be"),
]
# grad_skip_run, :2794-2812
_GRAD_SKIP = _grad_search(2) + _N_FIELDS + [
    (dict(records=None), "EINVAL", "null array pointer"),                                        # :2794
    (dict(group_z0=None), "EINVAL", "null array pointer"),
    (dict(n_groups=0), "EINVAL", "the search needs at least one group"),                         # :2799
    (dict(n_groups=BIG), "EINVAL", "more than 2^31 - 1 groups or scan wavefronts: search in batches"),     # :2800
    (dict(group_field=I64(0, 2)), "EINVAL", "group_field[1] outside [0, n_fields)"),             # :2811
    (dict(group_field=I64(-1, 0)), "EINVAL", "group_field[0] outside [0, n_fields)"),
    (dict(elev_tol=-1.0, n_groups=0), "EINVAL", "elev_tol_deg"),
    (dict(n_groups=0, axis0=None), "EINVAL", "the search needs"),
    (dict(n_groups=BIG, n0=1), "EINVAL", "more than 2^31 - 1 groups"),
    (dict(scan=F64(3.0, 2.0, 1.0), group_field=I64(0, 2)), "EINVAL", "strictly increasing"),
]
# grad_muf_run, :2900-2923
_NEG_DEN = np.full((4, 4), 1e11)
_NEG_DEN[2, 1] = -1.0
_GRAD_MUF = _grad_search(3) + [
    (dict(den=None), "EINVAL", "null array pointer"),                                            # :2900
    (dict(muf_target=None), "EINVAL", "null array pointer"),
    (dict(mode=7), "EINVAL", "Mode must be O or X"),                                             # :2905
    (dict(edge_order=3), "EINVAL", "edge_order is 1 or 2"),                                      # :2906
    (dict(edge_order=0), "EINVAL", "edge_order is 1 or 2"),
    (dict(n_bisect=0), "EINVAL", "n_bisect is 1 .. 64"),                                         # :2907
    (dict(n_bisect=65), "EINVAL", "n_bisect is 1 .. 64"),
    (dict(f_lo=0.0), "EINVAL", "the frequency bracket needs 0 < f_lo_hz < f_hi_hz, both finite"),          # :2908
    (dict(f_hi=1e6), "EINVAL", "the frequency bracket needs"),
    (dict(f_hi=INF), "EINVAL", "the frequency bracket needs"),
    (dict(n_links=0), "EINVAL", "the search needs at least one link"),                           # :2910
    (dict(n_links=BIG), "EINVAL", "more than 2^31 - 1 scan wavefronts: search in batches"),      # :2911
    (dict(n_links=(1 << 24) + 1), "EINVAL", "bad shape (the two axes hold at most"),             # :2914 (a field per link)
    (dict(n0=1, edge_order=1), "EINVAL", "axis 0 needs at least 2 values"),                      # :2914 (edge_order + 1, 2 at least)
    (dict(den=_NEG_DEN), "ENEGDEN", "Density must be non-negative"),                             # :2922
    (dict(elev_tol=-1.0, mode=7), "EINVAL", "elev_tol_deg"),
    (dict(mode=7, edge_order=3), "EINVAL", "Mode must be"),
    (dict(edge_order=3, n_bisect=0), "EINVAL", "edge_order is"),
    (dict(n_bisect=0, f_lo=0.0), "EINVAL", "n_bisect is"),
    (dict(f_lo=0.0, n_links=0), "EINVAL", "the frequency bracket needs"),
    (dict(n_links=0, axis0=None), "EINVAL", "the search needs"),
    (dict(scan=F64(3.0, 2.0, 1.0), den=_NEG_DEN), "EINVAL", "strictly increasing"),
    (dict(axis1=_DOWN, den=_NEG_DEN), "EINVAL", "axis 1 must be"),
]

def _retarget(cases, old, new):
    """The same table for a call that reads array ``new`` where the table names ``old``."""
    return [({(new if k == old else k): v for k, v in ch.items()}, rc, text) for ch, rc, text in cases]


GRADIENT = {
    "trace_gradient": (0, _trace_gradient, _GRAD_TRACE, "out"),
    # prhf_trace_gradient_spherical_f64: context and radius first (:2483-2484)
    "trace_gradient_spherical": (1, _trace_gradient_spherical, _RADIUS + _GRAD_TRACE + [
        (dict(r_e=0.0, records=None), "EINVAL", "earth_radius_km"),
        (dict(null_ctx=True, r_e=0.0), "EINVAL", "null context"),
    ], "out"),
    # prhf_trace_gradient_hops_f64: context, n_hops, geometry, radius, n_rays (:2501-2508)
    "trace_gradient_hops": (1, _trace_gradient_hops, _N_HOPS + _GRAD_GEOMETRY + _RADIUS + _GRAD_TRACE + [
        (dict(n_rays=(1 << 27)), "EINVAL", "more than 2^27 - 1 rays: trace in batches"),         # :2508
        (dict(n_hops=0, geometry=2), "EINVAL", "n_hops is"),
        (dict(geometry=2, r_e=0.0), "EINVAL", "geometry is 0"),
        (dict(r_e=0.0, n_rays=(1 << 27)), "EINVAL", "earth_radius_km"),
        (dict(n_rays=(1 << 27), records=None), "EINVAL", "more than 2^27 - 1 rays"),
    ], "hops_out"),
    "gradient_home": (0, _gradient_home, _GRAD_HOME, "home_out"),
    "gradient_hop_home": (1, _gradient_hop_home, _N_HOPS + _RADIUS + _GRAD_HOME + [
        (dict(n_hops=0, records=None), "EINVAL", "n_hops is"),
        (dict(geometry=2, r_e=0.0), "EINVAL", "geometry is 0"),
        (dict(r_e=0.0, flags=BAD_FLAG), "EINVAL", "earth_radius_km"),
        (dict(records=None, r_e=0.0), "EINVAL", "null array pointer"),
    ], "hop_home_out"),
    "gradient_skip": (1, _gradient_skip, _RADIUS + _GRAD_SKIP + [
        (dict(r_e=0.0, flags=BAD_FLAG), "EINVAL", "earth_radius_km"),
        (dict(scan=None, r_e=0.0), "EINVAL", "null array pointer"),
    ], "skip_out"),
    "gradient_hop_skip": (0, _gradient_hop_skip, _N_HOPS + _GRAD_SKIP + [
        (dict(n_hops=17, scan=None), "EINVAL", "n_hops is"),
        (dict(r_e=NAN), "OK", ""),                                                               # (Cartesian: the radius is not read)
    ], "hop_skip_out"),
    "gradient_muf": (0, _gradient_muf, _GRAD_MUF, "muf_out"),
    "gradient_hop_muf": (1, _gradient_hop_muf, _N_HOPS + _RADIUS + _retarget(_GRAD_MUF, "muf_target", "hop_muf_target") + [
        (dict(n_hops=0, den=None), "EINVAL", "n_hops is"),
        (dict(r_e=0.0, flags=BAD_FLAG), "EINVAL", "earth_radius_km"),
    ], "hop_muf_out"),
}


@pytest.fixture(scope="module")
def grad_bases():
    return {geo: _grad_base(geo) for geo in (0, 1)}


@pytest.mark.parametrize("name", sorted(GRADIENT))
def test_gradient_entry_point_rejections(name, ctx, null_ctx, grad_bases):
    n = _native()
    geo, call, cases, out_key = GRADIENT[name]
    base = dict(grad_bases[geo])
    _run(call, base, [(ch, getattr(n, rc), text) for ch, rc, text in cases], ctx, null_ctx, lambda a: a[out_key])


# ---------------------------------------------------------------------------------------------------------------------
# the derivatives: 2 profiles x 3 frequencies x a 16-point grid of g1_basic.npz
# ---------------------------------------------------------------------------------------------------------------------

def _deriv_base():
    from pyrayhf_amd import library
    n = _native()
    g = load_golden("g1_basic.npz")
    n_alt = g["alt"].size
    two = lambda k: np.ascontiguousarray(np.stack([g[k], g[k]]), dtype=np.float64)      # noqa: E731
    return dict(freq=np.ascontiguousarray(g["freq"], dtype=np.float64), n_freq=3, den=two("den"), bmag=two("bmag"), bpsi=two("bpsi"),
                alt=np.ascontiguousarray(g["alt"], dtype=np.float64), n_prof=2, n_alt=n_alt, prof_stride=n_alt, alt_stride=0,
                mult=np.ascontiguousarray(library._multiplier(16)), n_points=16, mode=n.MODE_O, flags=0,
                vh=np.zeros((2, 3)), jac=np.zeros((2, 3, n_alt)), grad_vh=np.ones((2, 3)), grad_den=np.zeros((2, n_alt)),
                tan=np.ones((2, n_alt)), n_tan=2, tan_stride=0, dvh=np.zeros((2, 3, 2)))


def _head(a):
    return (_ptr(a["freq"]), a["n_freq"], _ptr(a["den"]), _ptr(a["bmag"]), _ptr(a["bpsi"]), _ptr(a["alt"]), a["n_prof"], a["n_alt"],
            a["prof_stride"], a["alt_stride"], _ptr(a["mult"]), a["n_points"], a["mode"])


def _vfo_jacobian(c, a):
    return c.vfo_jacobian(*_head(a), _ptr(a["vh"]), _ptr(a["jac"]), a["flags"])


def _vfo_vjp(c, a):
    return c.vfo_vjp(*_head(a), _ptr(a["grad_vh"]), _ptr(a["vh"]), _ptr(a["grad_den"]), a["flags"])


def _vfo_jvp(c, a):
    return c.vfo_jvp(*_head(a), _ptr(a["tan"]), a["n_tan"], a["tan_stride"], _ptr(a["vh"]), _ptr(a["dvh"]), a["flags"])


def _down_mult():
    from pyrayhf_amd import library
    m = np.ascontiguousarray(library._multiplier(16)).copy()
    m[5] = m[3]
    if not m[5] < m[4]:
        m[5] = m[4] - 1.0
    return m


# derivative_check, :1172-1186
def _derivative_cases():
    n = _native()
    return [
        (dict(null_ctx=True), "EINVAL", "null context"),                                         # :1172
        (dict(freq=None), "EINVAL", "null array pointer"),                                       # :1173
        (dict(mult=None), "EINVAL", "null array pointer"),
        (dict(n_freq=0), "EINVAL", "bad shape"),                                                 # :1174
        (dict(n_prof=-1), "EINVAL", "bad shape"),
        (dict(n_alt=0), "EINVAL", "bad shape"),
        (dict(n_points=0), "EINVAL", "bad shape"),
        (dict(n_alt=1 << 40, prof_stride=1 << 40), "EINVAL", "exceeds the limit of"),            # :1175
        (dict(n_freq=(1 << 20) + 1), "EINVAL", "n_freq too large"),                              # :1176
        (dict(prof_stride=2), "EINVAL", "row stride shorter than a row"),                        # :1177
        (dict(alt_stride=2), "EINVAL", "row stride shorter than a row"),
        (dict(mode=7), "EINVAL", "mode must be 'O' or 'X'"),                                     # :1178
        (dict(flags=BAD_FLAG), "EINVAL", "unknown flag bits"),                                   # :1179
        (dict(flags=n.FLAG_ASYNC), "EINVAL", "PRHF_FLAG_ASYNC needs device pointers"),           # :1182
        (dict(mult=_down_mult()), "EINVAL", "multiplier[5] decreases"),                          # :1186
        (dict(null_ctx=True, freq=None), "EINVAL", "null context"),
        (dict(den=None, n_freq=0), "EINVAL", "null array pointer"),
        (dict(n_freq=0, mode=7), "EINVAL", "bad shape"),
        (dict(n_alt=1 << 40, n_freq=(1 << 20) + 1), "EINVAL", "exceeds the limit of"),
        (dict(n_freq=(1 << 20) + 1, prof_stride=2), "EINVAL", "n_freq too large"),
        (dict(prof_stride=2, mode=7), "EINVAL", "row stride"),
        (dict(mode=7, flags=BAD_FLAG), "EINVAL", "mode must be"),
        (dict(flags=BAD_FLAG | n.FLAG_ASYNC), "EINVAL", "unknown flag bits"),
        (dict(flags=n.FLAG_ASYNC, mult=_down_mult()), "EINVAL", "PRHF_FLAG_ASYNC"),
    ]


DERIVATIVES = {
    "vfo_jacobian": (_vfo_jacobian, lambda: [
        (dict(jac=None), "EINVAL", "null array pointer"),                                        # :1223
        (dict(jac=None, n_freq=0), "EINVAL", "null array pointer"),
    ], "jac"),
    "vfo_vjp": (_vfo_vjp, lambda: [
        (dict(grad_vh=None), "EINVAL", "null array pointer"),                                    # :1223
        (dict(grad_den=None), "EINVAL", "null array pointer"),
        (dict(grad_vh=None, mode=7), "EINVAL", "null array pointer"),
    ], "grad_den"),
    # jvp_run: derivative_check, then its own two (:1326-1327)
    "vfo_jvp": (_vfo_jvp, lambda: [
        (dict(tan=None), "EINVAL", "null array pointer"),                                        # :1324
        (dict(dvh=None), "EINVAL", "null array pointer"),
        (dict(n_tan=-1), "EINVAL", "bad number of tangents"),                                    # :1326
        (dict(n_tan=-1, tan=None, dvh=None), "EINVAL", "bad number of tangents"),                # (no tangents: no arrays asked for)
        (dict(n_tan=(1 << 20) + 1), "EINVAL", "bad number of tangents"),
        (dict(tan_stride=5), "EINVAL", "tangent stride shorter than a profile's tangents"),      # :1327
        (dict(n_tan=-1, mode=7), "EINVAL", "mode must be"),
        (dict(n_tan=(1 << 20) + 1, tan_stride=5), "EINVAL", "bad number of tangents"),
        (dict(tan_stride=5, mult=_down_mult()), "EINVAL", "multiplier[5] decreases"),
    ], "dvh"),
}


@pytest.mark.parametrize("name", sorted(DERIVATIVES))
def test_derivative_entry_point_rejections(name, ctx, null_ctx):
    n = _native()
    call, own, out_key = DERIVATIVES[name]
    base = _deriv_base()
    cases = _derivative_cases() + own()
    _run(call, base, [(ch, getattr(n, rc), text) for ch, rc, text in cases], ctx, null_ctx, lambda a: a[out_key])
