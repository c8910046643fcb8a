"""GPU: the Cartesian gradient tracer against the reference's three runs per ray (fixture g18,
tools/gen_golden_gradient.py) and against itself.

Accuracy rule, per control set and per key among group_path_km, group_delay_sec, ground_range_km, z_apex_km:

    max over rays |GPU(default tolerances) - truth| <= 2 x max over rays |reference(default tolerances) - truth|

where "truth" is the reference at rtol 1e-10, atol 1e-12, max_step 0.25 km.  The bound comes from the reference alone;
the factor 2 is there because the same method at the same tolerances has truncation error of the same size but not of
the same sign.  x_apex_km - the x of whichever node is highest - moves by 0.1 .. 1 km with the step sequence in the
reference itself and is only tested as a node of the returned path.
"""

import functools

import numpy as np
import pytest

from conftest import load_golden, same_bits
from pyrayhf_amd import _native, gradient, synth, tracers

pytestmark = pytest.mark.gpu

SETS = (dict(s_max_km=4000.0, max_step_km=5.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0),   # reference test_core.py:818-828
        dict(max_step_km=None))                                                                     # the defaults
TILTS = (0.3, 0.0)
CASES = (("O", 6.0e6), ("X", 9.0e6))
RULE_KEYS = ("group_path_km", "group_delay_sec", "ground_range_km", "z_apex_km")


@functools.lru_cache(maxsize=None)
def _field(tilt):
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, tilt, 18)
    parts = [gradient.refractive_field([f], den, bmag, bpsi, z, x, mode) for mode, f in CASES]
    return gradient.RefractiveField(z, x, np.concatenate([p.mu for p in parts]), np.concatenate([p.mup for p in parts]))


@functools.lru_cache(maxsize=None)
def _fan(ti, si):
    g = load_golden("g18_gradient_rays.npz")
    return gradient.trace_fan_cartesian_gradient(_field(TILTS[ti]), g["elevation_deg"], return_paths=True, **SETS[si])


def _gpu(key, si):
    """(tilt, case, elevation) array of the GPU's values for control set si"""
    return np.stack([_fan(ti, si)[key] for ti in range(len(TILTS))])


@pytest.mark.parametrize("si", [0, 1])
def test_status_equals_the_references(si):
    g = load_golden("g18_gradient_rays.npz")
    agree = g["agree"][:, :, si]
    want = g["default_status"][:, :, si]
    got = _gpu("status", si)
    print("reference:", {gradient.STATUS_NAMES[s]: int((want == s).sum()) for s in range(4)},
          "GPU:", {gradient.STATUS_NAMES[s]: int((got == s).sum()) for s in range(4)}, "rays compared:", int(agree.sum()))
    assert agree.sum() >= 0.9 * agree.size
    assert np.array_equal(got[agree], want[agree]), np.argwhere(agree & (got != want))


@pytest.mark.parametrize("key", RULE_KEYS)
@pytest.mark.parametrize("si", [0, 1])
def test_accuracy_rule(si, key):
    g = load_golden("g18_gradient_rays.npz")
    agree = g["agree"][:, :, si]
    truth, ref = g["truth_" + key][:, :, si], g["default_" + key][:, :, si]
    got = _gpu(key, si)
    assert np.array_equal(np.isnan(got[agree]), np.isnan(ref[agree])), "NaN where the reference has a value (or the reverse)"
    m = agree & np.isfinite(truth) & np.isfinite(ref)
    assert m.sum() >= 8
    e_ref = np.abs(ref[m] - truth[m]).max()
    e_gpu = np.abs(got[m] - truth[m]).max()
    print(f"set {si} {key}: max|GPU - truth| = {e_gpu:.3e}, max|reference - truth| = {e_ref:.3e}, "
          f"ratio {e_gpu / e_ref:.3f} over {int(m.sum())} rays")
    assert e_gpu <= 2.0 * e_ref


@pytest.mark.parametrize("si", [0, 1])
def test_path_self_consistency_and_unit_tangent(si):
    for ti in range(len(TILTS)):
        r = _fan(ti, si)
        for idx in np.ndindex(r["status"].shape):
            n = int(r["n_nodes"][idx])
            t, x, z, vx, vz = (r[k][idx][:n] for k in ("t", "x", "z", "vx", "vz"))
            assert np.isfinite(x).all() and np.isfinite(z).all() and np.all(np.diff(t) > 0)
            for k in ("t", "x", "z", "vx", "vz"):
                assert np.isnan(r[k][idx][n:]).all()                            # NaN padding
            assert same_bits(r["x_midpoint"][idx], x[n // 2]) and same_bits(r["z_midpoint"][idx], z[n // 2])
            apex = int(np.nanargmax(z))
            assert same_bits(r["x_apex_km"][idx], x[apex]) and same_bits(r["z_apex_km"][idx], z[apex])
            chords = float(np.sum(np.hypot(np.diff(x), np.diff(z))))
            assert abs(r["group_path_km"][idx] - chords) <= 1e-12 * chords
            assert np.abs(np.hypot(vx, vz) - 1.0).max() <= 1e-5
            status = gradient.STATUS_NAMES[r["status"][idx]]
            if status == "ground":
                assert abs(z[-1] - (0.0 + 1e-3)) <= 1e-9
                assert same_bits(r["ground_range_km"][idx], x[-1])
            else:
                assert np.isnan(r["ground_range_km"][idx])
            if status == "length":
                assert t[-1] == SETS[si].get("s_max_km", 5000.0)
            assert r["n_rhs"][idx] == 2 + 6 * (n - 1 + r["n_rejected"][idx]) or status in ("ground", "domain")


def test_single_ray_equals_the_same_ray_in_a_batch():
    g = load_golden("g18_gradient_rays.npz")
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.3, 18)
    field = _field(0.3)
    n_and_grad = gradient.build_refractive_index_interpolator_cartesian(z, x, field.mu[0])
    mup_func = gradient.build_mup_function(field.mup[0], x, z)
    for ei in (3, 9, 14):
        one = gradient.trace_ray_cartesian_gradient(n_and_grad, mup_func, 0.0, 0.0, g["elevation_deg"][ei], **SETS[0])
        fan = _fan(0, 0)
        n = int(fan["n_nodes"][0, ei])
        assert set(one) == {"t", "x", "z", "vx", "vz", "status", "group_path_km", "group_delay_sec", "x_midpoint",
                            "z_midpoint", "ground_range_km", "x_apex_km", "z_apex_km"}
        assert one["status"] == gradient.STATUS_NAMES[fan["status"][0, ei]]
        for k in ("t", "x", "z", "vx", "vz"):
            assert one[k].shape == (n,) and same_bits(one[k], fan[k][0, ei, :n]), k
        for k in ("group_path_km", "group_delay_sec", "x_midpoint", "z_midpoint", "ground_range_km", "x_apex_km",
                  "z_apex_km"):
            assert isinstance(one[k], float) and same_bits(one[k], fan[k][0, ei]), k


def test_mirror_symmetry_of_the_uniform_twin():
    """A zero-tilt field is mirror-symmetric about the centre of the domain: elevations e and 180 - e from there land at
    mirrored ranges.  The fan is the fixture's; the rays that must land are the ones the reference lands in all three of
    its runs (the steeper ones go through the layer and end in the NaN cap, the shallowest leave the domain sideways).

    The rays run with max_step_km=0.5, where every step but the first few and the last is the capped one.  A mirrored ray
    is not the same arithmetic: 180 - e and its cosine are rounded, and SciPy's four-product sum adds the mirrored cell's
    corners in the other order.  Those last-bit differences stay last-bit differences along a fixed step sequence, but
    the error estimate of an embedded pair is a difference of nearly equal sums, so a free step-size controller turns them
    into a relative 1e-5 of every step size, or into another accept / reject decision, and the two rays then differ by a
    part, or by all, of their truncation error.  The reference does the same on this field (6 MHz O, the 8 landing rays):
    |range(e) + range(180 - e)| up to 8.4e-3 km with 153 against 170 nodes at max_step_km=5, at most 2.2e-12 km with equal
    node counts at max_step_km=0.5.  So the symmetry of the right-hand side, the sampler's cell choice and the events is
    tested here on the capped sequence; with the first control set's 5 km the figure is printed only."""
    g = load_golden("g18_gradient_rays.npz")
    e = g["elevation_deg"]
    lands = g["agree"][1, :, 0] & (g["default_status"][1, :, 0] == gradient.STATUS_NAMES.index("ground"))
    assert lands.sum() >= 8
    both = np.concatenate([e, 180.0 - e])
    free = gradient.trace_fan_cartesian_gradient(_field(0.0), both, **SETS[0])["ground_range_km"]
    print("mirror, max_step_km=5: max |range(e) + range(180 - e)| =", np.nanmax(np.abs(free[:, :e.size] + free[:, e.size:])))
    r = gradient.trace_fan_cartesian_gradient(_field(0.0), both, **dict(SETS[0], max_step_km=0.5))
    right, left = r["ground_range_km"][:, :e.size], r["ground_range_km"][:, e.size:]
    assert np.isfinite(right[lands]).all() and (right[lands] > 0).all() and (left[lands] < 0).all()
    assert np.array_equal(r["status"][:, :e.size], r["status"][:, e.size:])
    ok = np.isfinite(right)
    assert np.array_equal(ok, np.isfinite(left))
    print("mirror: max |range(e) + range(180 - e)| =", np.abs(right[ok] + left[ok]).max())
    assert np.abs(right[ok] + left[ok]).max() <= 1e-9
    assert np.abs(r["group_path_km"][:, :e.size] - r["group_path_km"][:, e.size:])[ok].max() <= 1e-9


def test_consistent_with_the_snell_tracer_on_the_uniform_twin():
    """The reference's own consistency check (test_core.py:831-834): 4 %."""
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.0, 18)
    fan = _fan(1, 0)
    g = load_golden("g18_gradient_rays.npz")
    checked = 0
    for ei in (6, 7, 8, 9):                                    # 37 .. 53 degrees
        if gradient.STATUS_NAMES[fan["status"][0, ei]] != "ground":
            continue
        snell = tracers.trace_ray_cartesian_snells(CASES[0][1], g["elevation_deg"][ei], z, den[:, 0], bmag[:, 0],
                                                   bpsi[:, 0], "O")
        for key in ("group_path_km", "group_delay_sec", "ground_range_km"):
            v1, v2 = snell[key], fan[key][0, ei]
            rel = abs(v1 - v2) / max(abs(v1), abs(v2))
            print(f"elevation {g['elevation_deg'][ei]:.1f} {key}: Snell {v1:.6g}, gradient {v2:.6g}, {100 * rel:.3f} %")
            assert rel < 0.04, key
        checked += 1
    assert checked >= 2


def test_sparse_rays_do_not_depend_on_their_wave_neighbours():
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(121, 201, 0.3, 18)
    field = gradient.refractive_field(np.linspace(5.0e6, 8.5e6, 8), den, bmag, bpsi, z, x, "O")
    elev = np.linspace(5.0, 85.0, 512)
    fan = gradient.trace_fan_cartesian_gradient(field, elev, **SETS[0])
    assert fan["status"].shape == (8, 512)
    assert fan["n_nodes"].sum() > 0 and len(set(fan["status"].ravel())) >= 2
    rng = np.random.default_rng(5)
    fi, ei = rng.integers(0, 8, 13), rng.integers(0, 512, 13)
    few = gradient.trace_rays_cartesian_gradient(field, 0.0, 0.0, elev[ei], fi, **SETS[0])
    for k in few:
        assert same_bits(few[k], fan[k][fi, ei]), k


def test_short_path_buffer_and_bad_field_index_are_einval():
    import torch
    field = _field(0.3)
    ctx = _native.host_context(None)
    rec = field.records()
    n = 3
    x0, z0, e = np.zeros(n), np.zeros(n), np.array([30.0, 45.0, 60.0])
    out = np.empty((n, 12))
    ctl = (4000.0, 1e-7, 1e-9, 5.0, 0.0, 600.0, -1000.0, 1000.0, 50)
    args = (rec.data_ptr(), field.n_fields, field.axis0.size, field.axis1.size, field.axis0.ctypes.data,
            field.axis1.ctypes.data)
    bufs = [np.empty((n, 4)) for _ in range(5)]
    rc = ctx.trace_gradient(*args, x0.ctypes.data, z0.ctypes.data, e.ctypes.data, None, n, ctl, field.fills,
                            out.ctypes.data, [b.ctypes.data for b in bufs], 4, 0)
    assert rc == _native.EINVAL and "path_stride" in _native.last_error()
    idx = np.array([0, 5, 1], dtype=np.int64)
    rc = ctx.trace_gradient(*args, x0.ctypes.data, z0.ctypes.data, e.ctypes.data, idx.ctypes.data, n, ctl, field.fills,
                            out.ctypes.data, None, 0, 0)
    assert rc == _native.EINVAL and "n_fields" in _native.last_error()
    # device-resident arrays: the kernel reports the index, gives that ray NaN and traces the others
    dev = f"cuda:{ctx.device}"
    tx0, tz0, te, tidx = (torch.as_tensor(v, device=dev) for v in (x0, z0, e, idx))
    tout = torch.zeros((n, 12), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    rc = ctx.trace_gradient(*args, tx0.data_ptr(), tz0.data_ptr(), te.data_ptr(), tidx.data_ptr(), n, ctl, field.fills,
                            tout.data_ptr(), None, 0, _native.FLAG_DEVICE_PTRS)
    assert rc == _native.EINVAL
    got = tout.cpu().numpy()
    assert np.isnan(got[1]).all() and np.isfinite(got[0, 0]) and np.isfinite(got[2, 0])
    ref = gradient.trace_rays_cartesian_gradient(field, x0[[0, 2]], z0[[0, 2]], e[[0, 2]], idx[[0, 2]], 4000.0,
                                                 max_step_km=5.0, z_max_km=600.0, x_min_km=-1000.0, x_max_km=1000.0)
    assert same_bits(got[[0, 2], 0], ref["group_path_km"])
