"""Forward-mode differentiation of pyrayhf_amd.autograd.differentiable_forward_operator: under torch.autograd.forward_ad a
dual density gives a dual trace whose tangent is library.vertical_jvp's, bit for bit; reverse mode on the same tensors
still gives library.vertical_vjp's bits."""

import numpy as np
import pytest

from conftest import same_bits
from pyrayhf_amd import library, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    alt, den, bmag, bpsi = synth.chapman_profiles(24, 41)
    rows = [3, 11, 17]
    alt, den, bmag, bpsi = alt[::8].copy(), den[rows, ::8].copy(), bmag[rows, ::8].copy(), bpsi[rows, ::8].copy()
    tangent = den * np.random.default_rng(13).uniform(-1.0, 1.0, size=den.shape)
    return np.linspace(1.3, 14.0, 6), alt, den, bmag, bpsi, tangent


@pytest.mark.parametrize("mode,n_points", [("O", 63), ("X", 64)])
def test_forward_mode_tangent_is_the_jvp_and_backward_is_still_the_vjp(batch, mode, n_points):
    import torch
    import torch.autograd.forward_ad as fwad
    from pyrayhf_amd.autograd import differentiable_forward_operator
    freq, alt, den, bmag, bpsi, tangent = batch
    t = lambda x: torch.as_tensor(x, device="cuda")     # noqa: E731
    d, b, p, tan = t(den), t(bmag), t(bpsi), t(tangent)
    want_vh, want = library.vertical_jvp(freq, den, bmag, bpsi, alt, tangent, mode, n_points)
    assert np.isnan(want_vh).any() and np.isfinite(want_vh).any() and want[np.isfinite(want_vh)].all()
    with fwad.dual_level():
        dual = fwad.make_dual(d, tan)
        out = differentiable_forward_operator(freq, dual, b, p, alt, mode, n_points)
        primal, got = fwad.unpack_dual(out)
        assert got is not None and got.shape == primal.shape == (3, freq.size)
        assert same_bits(primal.cpu().numpy(), want_vh) and same_bits(got.cpu().numpy(), want)
    # a single profile
    with fwad.dual_level():
        out = differentiable_forward_operator(freq, fwad.make_dual(d[1], tan[1]), b[1], p[1], alt, mode, n_points)
        assert same_bits(fwad.unpack_dual(out).tangent.cpu().numpy(), want[1])
    # reverse mode on the same tensors
    dr = d.clone().requires_grad_(True)
    vh = differentiable_forward_operator(freq, dr, b, p, alt, mode, n_points)
    g = np.random.default_rng(3).uniform(-2.0, 2.0, size=(3, freq.size))
    torch.nansum(vh * t(g)).backward()
    back = library.vertical_vjp(freq, den, bmag, bpsi, alt, g, mode, n_points)
    assert same_bits(dr.grad.cpu().numpy(), back) and back.any()
