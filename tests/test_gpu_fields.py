"""GPU: node records and the point sampler against NumPy's np.gradient and SciPy's RegularGridInterpolator as the
reference's builders use them (fixture g17, tools/gen_golden_gradient.py)."""

import numpy as np
import pytest

from conftest import load_golden, same_bits
from pyrayhf_amd import gradient, library, synth

pytestmark = pytest.mark.gpu

GRIDS = (("nonuniform", False), ("uniform", True))
R_E = library.constants()[2]


def _axes(uniform):
    z, x, *_ = synth.tilted_ionosphere(41, 33, 0.3, 17, uniform=uniform)
    return z, x


@pytest.mark.parametrize("geometry", ["cartesian", "spherical"])
@pytest.mark.parametrize("edge_order", [1, 2])
@pytest.mark.parametrize("grid,uniform", GRIDS)
def test_pack_is_np_gradient_bit_for_bit(grid, uniform, edge_order, geometry):
    """Both of np.gradient's branches (the uniform grid takes the scalar one along z and x, the stretched grid and the
    spherical phi axis the three-point one), both edge orders, NaN cap included; mu and mu' copied bit for bit."""
    g = load_golden("g17_fields.npz")
    z, x = _axes(uniform)
    a0, a1 = (z, x) if geometry == "cartesian" else (R_E + z, x / R_E)
    mu = np.stack([g[f"{grid}_O_mu"], g[f"{grid}_X_mu"]])
    mup = np.stack([g[f"{grid}_O_mup"], g[f"{grid}_X_mup"]])
    field = gradient.RefractiveField(a0, a1, mu, mup, edge_order=edge_order)
    rec = field.records().cpu().numpy()
    assert rec.shape == (2, 41, 33, 4)
    for k, mode in enumerate("OX"):
        key = f"{grid}_{mode}_{geometry}_e{edge_order}"
        assert same_bits(rec[k, :, :, 0], mu[k]) and same_bits(rec[k, :, :, 3], mup[k])
        assert np.array_equal(rec[k, :, :, 0].view(np.uint64)[np.isfinite(mu[k])], mu[k].view(np.uint64)[np.isfinite(mu[k])])
        assert same_bits(rec[k, :, :, 1], g[key + "_d1"]), key + " d/da1"
        assert same_bits(rec[k, :, :, 2], g[key + "_d0"]), key + " d/da0"
        assert np.isnan(g[key + "_d0"]).any() and np.isfinite(g[key + "_d0"]).any()


def _corner_scale(planes, z, x, pts):
    """max |corner value| of the cell SciPy takes for each in-hull point, per plane."""
    c0 = np.clip(np.searchsorted(z, pts[:, 0], side="right") - 1, 0, z.size - 2)
    c1 = np.clip(np.searchsorted(x, pts[:, 1], side="right") - 1, 0, x.size - 2)
    out = []
    for p in planes:
        corners = np.stack([p[c0, c1], p[c0, c1 + 1], p[c0 + 1, c1], p[c0 + 1, c1 + 1]])
        out.append(np.abs(corners).max(axis=0))
    return np.stack(out)


@pytest.mark.parametrize("mode", ["O", "X"])
@pytest.mark.parametrize("grid,uniform", GRIDS)
def test_sampler_matches_regular_grid_interpolator(grid, uniform, mode):
    """NaN masks and filled points identical; finite values within 16 * 2^-52 * max|corner value| of SciPy: about ten
    roundings of at most half an ulp of the largest term.  (The kernel forms SciPy's four products and adds them in
    SciPy's order; the test prints how many values are bit-identical.)"""
    g = load_golden("g17_fields.npz")
    z, x = _axes(uniform)
    key = f"{grid}_{mode}"
    mu, mup, pts, want = g[key + "_mu"], g[key + "_mup"], g[key + "_points"], g[key + "_rgi"]
    n_and_grad = gradient.build_refractive_index_interpolator_cartesian(z, x, mu)
    mup_func = gradient.build_mup_function(mup, x, z)
    n, dndx, dndz = n_and_grad(pts[:, 1], pts[:, 0])
    got = np.stack([n, dndx, dndz, mup_func(pts[:, 1], pts[:, 0])])
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN masks differ"
    outside = (pts[:, 0] < z[0]) | (pts[:, 0] > z[-1]) | (pts[:, 1] < x[0]) | (pts[:, 1] > x[-1])
    assert outside.sum() >= 100
    assert same_bits(got[:, outside], want[:, outside]), "filled points differ"
    # a NaN coordinate gives NaN in every output even when the other coordinate is outside the hull, as in SciPy
    nan_pt = np.isnan(pts).any(axis=1)
    assert (outside & nan_pt).any() and np.isnan(got[:, nan_pt]).all()
    filled = outside & ~nan_pt
    assert np.isnan(got[0, filled]).all() and (got[1:3, filled] == 0.0).all()
    planes = [mu, g[key + "_cartesian_e2_d1"], g[key + "_cartesian_e2_d0"], mup]
    inside = ~outside & ~np.isnan(pts).any(axis=1)
    scale = np.zeros_like(want)
    scale[:, inside] = _corner_scale(planes, z, x, pts[inside])
    fin = np.isfinite(want)
    err = np.abs(got - want)
    bound = 16.0 * 2.0 ** -52 * scale
    print(f"{key}: {int(fin.sum())} finite values, {int((got[fin] == want[fin]).sum())} bit-identical, "
          f"worst error / bound {np.max(err[fin] / np.maximum(bound[fin], 1e-300)):.3f}")
    assert (err[fin] <= bound[fin]).all()
    # the spherical builder on the same field: (phi, r) -> (mu, dmu/dr, dmu/dphi)
    sph = gradient.build_refractive_index_interpolator_spherical(z, x, mu)
    got_s = np.stack(sph(pts[:, 1] / R_E, R_E + pts[:, 0]))
    want_s = g[key + "_rgi_spherical"]
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s))
    planes_s = [mu, g[key + "_spherical_e2_d0"], g[key + "_spherical_e2_d1"]]
    r_axis, phi_axis = R_E + z, x / R_E
    pts_s = np.column_stack([R_E + pts[:, 0], pts[:, 1] / R_E])
    outside_s = ((pts_s[:, 0] < r_axis[0]) | (pts_s[:, 0] > r_axis[-1]) | (pts_s[:, 1] < phi_axis[0]) |
                 (pts_s[:, 1] > phi_axis[-1]))
    inside_s = ~outside_s & ~np.isnan(pts_s).any(axis=1)
    assert same_bits(got_s[:, outside_s], want_s[:, outside_s])
    scale_s = np.zeros_like(want_s)
    scale_s[:, inside_s] = _corner_scale(planes_s, r_axis, phi_axis, pts_s[inside_s])
    fin_s = np.isfinite(want_s)
    assert (np.abs(got_s - want_s)[fin_s] <= (16.0 * 2.0 ** -52 * scale_s)[fin_s]).all()


def test_multi_field_sampling_and_field_index():
    g = load_golden("g17_fields.npz")
    z, x = _axes(False)
    mu = np.stack([g["nonuniform_O_mu"], g["nonuniform_X_mu"]])
    mup = np.stack([g["nonuniform_O_mup"], g["nonuniform_X_mup"]])
    field = gradient.RefractiveField(z, x, mu, mup)
    pts = g["nonuniform_O_points"][:500]
    idx = np.arange(500) % 2
    got = field.sample(pts[:, 0], pts[:, 1], idx)
    for k, mode in enumerate("OX"):
        one = gradient.RefractiveField(z, x, mu[k], mup[k]).sample(pts[idx == k, 0], pts[idx == k, 1])
        for a, b in zip(got, one):
            assert same_bits(a[idx == k], b)
    with pytest.raises(ValueError, match="field_index"):
        field.sample(pts[:, 0], pts[:, 1], np.full(500, 2))


def test_callables_return_the_references_shapes():
    g = load_golden("g17_fields.npz")
    z, x = _axes(True)
    mu, mup = g["uniform_O_mu"], g["uniform_O_mup"]
    n_and_grad = gradient.build_refractive_index_interpolator_cartesian(z, x, mu)
    mup_func = gradient.build_mup_function(mup, x, z)
    sph = gradient.build_refractive_index_interpolator_spherical(z, x, mu)
    mup_sph = gradient.build_mup_function(mup, x, z, geometry="spherical")
    for out in (n_and_grad(10.0, 100.0), sph(10.0 / R_E, R_E + 100.0)):          # scalars -> (1,), library.py:922-923
        assert len(out) == 3 and all(o.shape == (1,) for o in out)
    out = n_and_grad(np.array([0.0, 10.0, 20.0]), 100.0)                         # broadcast
    assert all(o.shape == (3,) for o in out)
    out = n_and_grad(np.zeros((4, 1)), np.full((1, 5), 50.0))
    assert all(o.shape == (4, 5) for o in out)
    assert np.shape(mup_func(10.0, 100.0)) == ()                                 # reshape(np.shape(x)), :1991
    assert mup_func(np.zeros(7), np.full(7, 90.0)).shape == (7,)
    assert mup_func(np.zeros((2, 3)), np.full((2, 3), 90.0)).shape == (2, 3)
    xs, zs = np.array([-300.0, 0.0, 250.0]), np.array([80.0, 120.0, 150.0])
    # spherical and Cartesian objects see the same field: mu agrees to the rounding of r = R_E + z, phi = x / R_E
    n_c = n_and_grad(xs, zs)[0]
    n_s = sph(xs / R_E, R_E + zs)[0]
    assert np.allclose(n_c, n_s, rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(mup_func(xs, zs), mup_sph(xs, zs), rtol=1e-9, atol=0, equal_nan=True)
    # fill values and NaN coordinates
    n, dx, dz = n_and_grad(np.array([5000.0, np.nan]), np.array([100.0, 100.0]))
    assert np.isnan(n).all() and dx[0] == 0.0 and dz[0] == 0.0 and np.isnan(dx[1]) and np.isnan(dz[1])
    filled = gradient.build_refractive_index_interpolator_cartesian(z, x, mu, fill_value_n=1.0, fill_value_grad=-2.0)
    n, dx, dz = filled(5000.0, 100.0)
    assert n[0] == 1.0 and dx[0] == -2.0 and dz[0] == -2.0
    assert gradient.build_mup_function(mup, x, z, fill_value=7.0)(5000.0, 100.0) == 7.0


def test_refractive_field_composes_find_mu_mup_and_the_pack_kernel():
    z, x, den, bmag, bpsi = synth.tilted_ionosphere(41, 33, 0.3, 17, uniform=False)
    freqs = np.array([6.0e6, 9.0e6])
    field = gradient.refractive_field(freqs, den, bmag, bpsi, z, x, "O")
    rec = field.records().cpu().numpy()
    for k, f in enumerate(freqs):
        mu, mup = library.find_mu_mup(library.find_X(den, f), library.find_Y(f, bmag), bpsi, "O")
        with np.errstate(all="ignore"):
            d0, d1 = np.gradient(mu, z, x, edge_order=2)
        assert same_bits(rec[k, :, :, 0], mu) and same_bits(rec[k, :, :, 3], mup)
        assert same_bits(rec[k, :, :, 1], d1) and same_bits(rec[k, :, :, 2], d0)
    sph = gradient.refractive_field(freqs[:1], den, bmag, bpsi, z, x, "X", geometry="spherical")
    assert np.array_equal(sph.axis0, R_E + z) and np.array_equal(sph.axis1, x / R_E)
