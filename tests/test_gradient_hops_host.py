"""Host-side checks of multi-hop gradient ray tracing and multi-hop homing: the two C symbols
and the six functions are exported, arguments are validated before any device call, and fixture G24
(tools/gen_golden_gradient_hops.py, reference-run) has the shape and the invariants the GPU tests of
tests/test_gpu_gradient_hops.py rest on, with the generator's two assertions restated on the stored arrays.

The apex: the reference's z_apex_km is the highest NODE of a ray, below the ray's highest point by up to
curvature x step^2 / 8, so between the step caps 0.25, 0.5 and 1 km of the truth, check and default runs the node values
alone give max |check - truth| / max |default - truth| near (0.5^2 - 0.25^2) / (1^2 - 0.25^2) = 0.2 (0.242 stored as
*_z_apex_node_km).  truth_z_apex_km and check_z_apex_km are therefore the highest point of their own rays (the generator's
`apex`: the maximum of the cubic Hermite interpolant between the nodes around it), the value the node maximum converges to;
default_z_apex_km is the reference's own number.
"""

import os
import re

import numpy as np
import pytest

from conftest import load_golden
import gradient_homing_rule as rule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km", "next_elevation_deg")
RUNS = ("default", "truth", "check")
FUNCTIONS = ("trace_hops_cartesian_gradient", "trace_hops_spherical_gradient", "trace_hop_fan_cartesian_gradient",
             "trace_hop_fan_spherical_gradient", "home_hops_cartesian_gradient", "home_hops_spherical_gradient")
SYMBOLS = ("prhf_trace_gradient_hops_f64", "prhf_gradient_hop_home_f64")


def test_symbols_and_functions_are_exported():
    import pyrayhf_amd
    from pyrayhf_amd import _native, gradient
    for name in FUNCTIONS:
        assert name in pyrayhf_amd.__all__ and name in gradient.__all__
        assert getattr(pyrayhf_amd, name) is getattr(gradient, name)
    lib = _native.load()
    text = open(os.path.join(REPO, "include", "prhf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    header = sorted(set(re.findall(r"\b(prhf_[a-z0-9_]+)\s*\(", code)))
    assert header == _native.exported_symbols()
    for name in SYMBOLS:
        assert name in header and hasattr(lib, name)
        # header <-> binding: as many arguments in the prototype as in the ctypes signature
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(proto.split(",")) == len(getattr(lib, name).argtypes), name
    assert lib.prhf_abi_version() == 4 == _native.ABI_VERSION


def _trace_args(n_hops, ctx=None):
    return (ctx, 0, None, 1, 3, 3, None, None, None, None, None, None, 0, 0.0, 4000.0, 1e-7, 1e-9, 1.0, 0.0, 600.0, -2000.0,
            2000.0, 50, np.nan, 0.0, np.nan, n_hops, None, None, None, None, None, None, 0, 0)


def _home_args(n_hops, ctx=None):
    return (ctx, 0, None, 1, 3, 3, None, None, None, None, None, 1, None, None, 0, None, 2, 0.0, 4000.0, 1e-7, 1e-9, 1.0, 0.0,
            600.0, -2000.0, 2000.0, 50, np.nan, 0.0, np.nan, 0.05, 64, 4, n_hops, None, None, 0)


def test_native_calls_reject_a_null_context_before_anything_else():
    from pyrayhf_amd import _native
    lib = _native.load()
    for n_hops in (3, 0, 17):
        for rc in (lib.prhf_trace_gradient_hops_f64(*_trace_args(n_hops)), lib.prhf_gradient_hop_home_f64(*_home_args(n_hops))):
            assert rc == _native.EINVAL and b"context" in lib.prhf_last_error()


@pytest.mark.parametrize("n_hops", [0, 17, -1])
def test_native_calls_reject_n_hops_outside_1_to_16_without_a_device(n_hops):
    """n_hops is checked right behind the context: every other argument here is null or empty, and no device is touched
    (a context handle is only dereferenced behind the argument checks)."""
    import ctypes
    from pyrayhf_amd import _native
    lib = _native.load()
    fake = ctypes.create_string_buffer(4096)                                  # never read: the call returns before it would be
    for rc in (lib.prhf_trace_gradient_hops_f64(*_trace_args(n_hops, ctypes.addressof(fake))),
               lib.prhf_gradient_hop_home_f64(*_home_args(n_hops, ctypes.addressof(fake)))):
        assert rc == _native.EINVAL and b"n_hops is 1 .. 16" in lib.prhf_last_error()


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
    two = gradient.RefractiveField(r_e + z, x / r_e, np.stack([mu, mu]), np.stack([mu, mu]), geometry="spherical", R_E=r_e) \
        if spherical else gradient.RefractiveField(z, x, np.stack([mu, mu]), np.stack([mu, mu]))
    geo = "spherical" if spherical else "cartesian"
    trace, fan, home = (getattr(gradient, f"{n}_{geo}_gradient") for n in ("trace_hops", "trace_hop_fan", "home_hops"))
    field, other = (sph, cart) if spherical else (cart, sph)
    e, t = np.array([20.0, 30.0]), np.array([300.0, 100.0])
    for call in (lambda f, h, **kw: trace(f, 0.0, 0.0, e, h, **kw), lambda f, h, **kw: fan(f, e, h, **kw),
                 lambda f, h, **kw: home(f, t, h, **kw)):
        with pytest.raises(TypeError):
            call(mu, 2)                                                   # not a field
        with pytest.raises(ValueError, match="needs a"):
            call(other, 2)                                                # a field of the other geometry
        for n_hops in (0, 17, -3, 2.5, True):
            with pytest.raises(ValueError, match="n_hops is an integer in 1 .. 16"):
                call(field, n_hops)
        with pytest.raises(ValueError, match="max_step"):
            call(field, 2, max_step_km=0.0)
        if spherical:
            with pytest.raises(ValueError, match="R_E"):
                call(field, 2, R_E=6400.0)
    with pytest.raises(ValueError, match="field_index is needed"):
        trace(two, 0.0, 0.0, e, 2)
    with pytest.raises(ValueError, match="field_index outside"):
        trace(two, 0.0, 0.0, e, 2, np.array([0, 2]))
    with pytest.raises(ValueError):
        trace(field, 0.0, np.zeros(3), e, 2)                              # shapes that do not broadcast
    with pytest.raises(ValueError, match="1-D"):
        fan(field, np.ones((2, 2)), 2)
    for kw in (dict(scan_elevation_deg=[10.0]), dict(scan_elevation_deg=[20.0, 10.0]), dict(max_roots=0), dict(max_roots=65),
               dict(max_iter=0), dict(max_iter=129), dict(range_tol_km=-1.0), dict(range_tol_km=np.nan)):
        with pytest.raises(ValueError):
            home(field, t, 2, **kw)
    with pytest.raises(ValueError, match="target_x_km"):
        home(field, t.reshape(2, 1), 2)


def test_fixture_shape_and_integrity():
    g = load_golden("g24_gradient_hops.npz")
    assert np.array_equal(g["elevation_deg"], np.linspace(10.0, 70.0, 13)) and g["n_hops"] == 3
    assert np.array_equal(g["freq_hz"], [6e6, 9e6]) and np.array_equal(g["mode_is_x"], [False, True])
    assert np.array_equal(g["launch_km"], [-1800.0, 0.0]) and np.array_equal(g["controls"], [4000.0, 600.0, 2000.0])
    for run in RUNS:
        st = g[run + "_status"]
        assert st.shape == (2, 13, 3) and np.isin(st, (-1, 0, 1, 2, 3)).all()
        assert np.all(st[..., 0] >= 0) and np.all(st[..., 1:][st[..., :-1] != 0] == -1)      # a chain ends where a hop does not land
        assert np.all(st[..., 1:][st[..., :-1] == 0] >= 0)
        used, landed = st >= 0, st == 0
        for k in ("launch_x_km", "launch_elevation_deg", "group_path_km", "group_delay_sec", "z_apex_km", "z_apex_node_km"):
            assert g[f"{run}_{k}"].shape == st.shape and np.array_equal(np.isfinite(g[f"{run}_{k}"]), used), (run, k)
        for k in ("ground_range_km", "next_elevation_deg"):
            assert np.array_equal(np.isfinite(g[f"{run}_{k}"]), landed), (run, k)
        # the chain: a hop launches where the hop before landed, with the reflected elevation, those bits
        assert np.all(g[run + "_launch_x_km"][..., 0] == -1800.0)
        assert np.array_equal(g[run + "_launch_elevation_deg"][..., 0], np.broadcast_to(g["elevation_deg"], (2, 13)))
        nxt = used[..., 1:]
        assert np.array_equal(g[run + "_launch_x_km"][..., 1:][nxt], g[run + "_ground_range_km"][..., :-1][nxt])
        assert np.array_equal(g[run + "_launch_elevation_deg"][..., 1:][nxt], g[run + "_next_elevation_deg"][..., :-1][nxt])
    st = g["default_status"]
    # 23 chains land hop 0, 22 land hops 1 and 2: the O rays at 60 - 70 degrees fail on hop 0, one X ray leaves on hop 1
    assert (st[..., 0] == 0).sum() == 23 and (st[..., 1] == 0).sum() == 22 and (st[..., 2] == 0).sum() == 22
    assert np.all(st[0, 10:, 0] == 3) and (st[1, :, 1] == 1).sum() == 1
    assert (g["default_next_elevation_deg"][st == 0] > 0).all()


def _agreement(g):
    return (g["default_status"] == g["truth_status"]) & (g["default_status"] == g["check_status"])


def test_fixture_status_agreement():
    """The generator's first assertion: the three runs agree in status on >= 90 % of the hop rows (stored: all 78)."""
    g = load_golden("g24_gradient_hops.npz")
    assert _agreement(g).mean() >= 0.9


@pytest.mark.parametrize("key", KEYS)
def test_fixture_truth_run_has_converged(key):
    """The generator's second assertion, per key: max |check - truth| <= 0.1 max |default - truth| over the landed hop
    rows on which the runs agree."""
    g = load_golden("g24_gradient_hops.npz")
    ok = _agreement(g) & (g["truth_status"] == 0)
    d = np.abs(g["default_" + key][ok] - g["truth_" + key][ok]).max()
    c = np.abs(g["check_" + key][ok] - g["truth_" + key][ok]).max()
    print(f"{key}: max|default - truth| = {d:.3e}, max|check - truth| = {c:.3e}, ratio {c / d:.3f}")
    assert c <= 0.1 * d, (key, c / d)


def test_fixture_apex():
    """The default run's apex is the reference's node maximum; the truth and check runs' apex is the highest point of the
    ray, at or above their highest node and above it by less than the default run's node is below the truth (the node
    spacing's error falls with the square of the cap, which is 4 and 2 times smaller)."""
    g = load_golden("g24_gradient_hops.npz")
    used = g["default_status"] >= 0
    assert np.array_equal(g["default_z_apex_km"][used], g["default_z_apex_node_km"][used])
    worst = np.abs(g["default_z_apex_node_km"] - g["truth_z_apex_km"])[used & (g["truth_status"] == g["default_status"])].max()
    for run in ("truth", "check"):
        lift = (g[run + "_z_apex_km"] - g[run + "_z_apex_node_km"])[g[run + "_status"] >= 0]
        print(f"{run}: the highest point lies up to {lift.max():.3e} km above the highest node (default run: {worst:.3e})")
        assert np.all(lift >= 0.0) and 0.0 < lift.max() <= worst


def test_fixture_homing_part():
    g = load_golden("g24_gradient_hops.npz")
    assert g["home_hops"] == 2 and g["range_tol_km"] == 0.05 and g["max_iter"] == 64
    t = g["target_km"]
    assert np.array_equal(t[:4], [-500.0, 0.0, -1100.0, 1900.0]) and np.isnan(t[4])
    st = g["default_status"][0, :, :2]
    d = np.where(np.all(st == 0, axis=1), g["default_ground_range_km"][0, :, 1], np.nan)
    assert np.array_equal(d, g["scan_ground_range_km"], equal_nan=True)
    assert np.array_equal(np.isfinite(d), np.isfinite(g["check_scan_ground_range_km"]))
    # D(e) of two hops is not monotonic: -500 km has three brackets, 0 and -1100 km one each, 1900 km and NaN none
    assert g["n_brackets"].tolist() == [3, 1, 1, 0, 0]
    want = [(ti, i) for ti, tt in enumerate(t) for i in rule.brackets(d, float(tt))]
    assert list(zip(g["bracket_target"].tolist(), g["bracket_scan_index"].tolist())) == want
    assert np.nanmin(np.abs(d[None, :] - t[:, None])) >= 1.0               # no scan node within 1 km of a target
    bst, miss = g["bracket_status"], g["bracket_miss_km"]
    assert np.all(((bst == 0) & (miss <= 0.05)) | (bst == 2) | ((bst == 1) & (miss >= 5.0)))
    conv = bst == 0
    assert conv.sum() >= 3
    scan = g["elevation_deg"]
    for name in ("bracket_elevation_deg", "e_truth"):
        e = g[name][conv]
        assert np.all((e >= scan[g["bracket_scan_index"][conv]]) & (e <= scan[g["bracket_scan_index"][conv] + 1]))
    for name in ("dD_de", "dP_de", "dT_de", "truth_total_group_path_km", "truth_total_group_delay_sec",
                 "default_total_ground_range_km"):
        assert np.all(np.isfinite(g[name][conv])), name
    assert np.all(g["dD_de"][conv] != 0.0)
    assert np.max(np.abs(g["truth_total_ground_range_km"][conv] - t[g["bracket_target"][conv]])) <= 1e-3 * 0.05
