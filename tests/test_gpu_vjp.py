"""The VJP kernel (prhf_vfo_vjp_f64): it is the Jacobian kernel's rows times the upstream gradient up to
the order of the additions - |vjp - sum_f g J| <= n_freq 2^-52 sum_f |g J| elementwise, a reordering bound and not a
tolerance - and its bits depend on nothing but the profile and the launch's shape."""

import numpy as np
import pytest

from conftest import same_bits
from pyrayhf_amd import library, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    alt, den, bmag, bpsi = synth.chapman_profiles(24, 41)
    rows = [3, 11, 17]
    return alt[::8].copy(), den[rows, ::8].copy(), bmag[rows, ::8].copy(), bpsi[rows, ::8].copy()


def sweep(n_freq):
    return np.array([4.1]) if n_freq == 1 else np.linspace(1.3, 14.0, n_freq)


def upstream(shape, seed):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=shape)


@pytest.mark.parametrize("mode,n_points", [("O", 63), ("X", 64), ("O", 200), ("X", 65)])
@pytest.mark.parametrize("n_freq", [1, 4, 65])
def test_vjp_is_the_jacobian_times_the_gradient_up_to_reordering(batch, mode, n_points, n_freq):
    alt, den, bmag, bpsi = batch
    freq = sweep(n_freq)
    g = upstream((den.shape[0], n_freq), 7 + n_freq)
    vh, J = library.vertical_jacobian(freq, den, bmag, bpsi, alt, mode, n_points)
    got = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, n_points)
    assert got.shape == den.shape
    live = np.isfinite(vh)
    assert live.any()
    terms = np.where(live[:, :, None], g[:, :, None].astype(np.longdouble) * J.astype(np.longdouble), 0.0)
    want = terms.sum(axis=1)
    bound = n_freq * 2.0 ** -52 * np.abs(terms).sum(axis=1)
    excess = np.abs(got.astype(np.longdouble) - want) - bound
    print(f"vjp {mode} n={n_points} F={n_freq}: largest |vjp - sum| / bound "
          f"{float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1))):.3f}")
    assert (excess <= 0).all(), float(excess.max())
    assert got.any() and not got[:, np.argmax(den, axis=1).max():].any()


def test_two_calls_give_equal_bits(batch):
    alt, den, bmag, bpsi = batch
    freq, g = sweep(65), upstream((3, 65), 1)
    for mode in "OX":
        a = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, 200)
        b = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, 200)
        assert np.array_equal(a, b) and a.any()
        ja = library.vertical_jacobian(freq, den, bmag, bpsi, alt, mode, 200)[1]
        jb = library.vertical_jacobian(freq, den, bmag, bpsi, alt, mode, 200)[1]
        assert np.array_equal(ja, jb)


def test_a_profile_alone_and_among_three_gives_equal_bits(batch):
    alt, den, bmag, bpsi = batch
    freq, g = sweep(65), upstream((3, 65), 2)
    for mode in "OX":
        among = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, 64)
        jac = library.vertical_jacobian(freq, den, bmag, bpsi, alt, mode, 64)[1]
        for p in range(3):
            alone = library.vertical_vjp(freq, den[p], bmag[p], bpsi[p], alt, g[p], mode, 64)
            assert alone.shape == (alt.size,) and np.array_equal(alone, among[p]), (mode, p)
            assert np.array_equal(library.vertical_jacobian(freq, den[p], bmag[p], bpsi[p], alt, mode, 64)[1], jac[p])


def test_numpy_and_torch_resident_inputs_give_equal_bits(batch):
    import torch
    alt, den, bmag, bpsi = batch
    freq, g = sweep(4), upstream((3, 4), 3)
    t = lambda x: torch.as_tensor(x, device="cuda")     # noqa: E731
    for mode in "OX":
        host = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, 200)
        dev = library.vertical_vjp(t(freq), t(den), t(bmag), t(bpsi), t(alt), t(g), mode, 200)
        assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
        vh_h, j_h = library.vertical_jacobian(freq, den, bmag, bpsi, alt, mode, 200)
        vh_d, j_d = library.vertical_jacobian(t(freq), t(den), t(bmag), t(bpsi), t(alt), mode, 200)
        assert same_bits(vh_d.cpu().numpy(), vh_h) and np.array_equal(j_d.cpu().numpy(), j_h)
    # per-profile altitude rows
    alt2 = np.stack([alt, alt + 0.25, alt + 1.0])
    host = library.vertical_vjp(freq, den, bmag, bpsi, alt2, g, "X", 63)
    dev = library.vertical_vjp(t(freq), t(den), t(bmag), t(bpsi), t(alt2), t(g), "X", 63)
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(host[0], library.vertical_vjp(freq, den[0], bmag[0], bpsi[0], alt, g[0], "X", 63))


def test_shared_field_and_per_profile_fields_agree(batch):
    alt, den, bmag, bpsi = batch
    freq, g = sweep(65), upstream((3, 65), 4)
    for mode in "OX":
        shared = library.vertical_vjp(freq, den, bmag[0], bpsi[0], alt, g, mode, 65)
        tiled = library.vertical_vjp(freq, den, np.tile(bmag[0], (3, 1)), np.tile(bpsi[0], (3, 1)), alt, g, mode, 65)
        assert np.array_equal(shared, tiled) and shared.any()
        assert np.array_equal(library.vertical_jacobian(freq, den, bmag[0], bpsi[0], alt, mode, 65)[1],
                              library.vertical_jacobian(freq, den, np.tile(bmag[0], (3, 1)), np.tile(bpsi[0], (3, 1)), alt,
                                                        mode, 65)[1])


def test_a_tall_bottomside_is_refused_with_the_documented_error():
    n = 3000
    alt = 80.0 + 0.2 * np.arange(n)
    den = 1e11 * (1.0 + np.arange(n) / 100.0)
    den[2600:] = den[2599] * 0.5                       # the peak at level 2599: 2600 levels to stage
    bmag, bpsi = np.full(n, 4e-5), np.full(n, 50.0)
    freq = np.array([3.0, 5.0])
    with pytest.raises(ValueError, match="stages at most .* levels"):
        library.vertical_vjp(freq, den, bmag, bpsi, alt, np.ones(2), "O", 64)
    with pytest.raises(ValueError, match="stages at most .* levels"):
        library.vertical_jacobian(freq, den, bmag, bpsi, alt, "X", 64)
    # ... while a long column whose bottomside fits is taken (the peak pre-pass): peak at level 400
    den2 = den.copy()
    den2[401:] = den2[400] * 0.5
    out = library.vertical_vjp(freq, den2, bmag, bpsi, alt, np.ones(2), "O", 64)
    assert out.shape == (n,) and out[:400].any() and not out[400:].any()
