"""pyrayhf_amd.autograd.differentiable_forward_operator: loss.backward() through the operator is one VJP launch."""

import numpy as np
import pytest

from conftest import same_bits
from pyrayhf_amd import library, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    import torch
    alt, den, bmag, bpsi = synth.chapman_profiles(24, 43)
    rows = [2, 9]
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")      # noqa: E731
    freq = np.linspace(1.5, 13.0, 24)
    return t(freq), t(den[rows, ::8]), t(bmag[rows, ::8]), t(bpsi[rows, ::8]), t(alt[::8])


@pytest.mark.parametrize("mode,n_points", [("O", 200), ("X", 64)])
def test_backward_is_the_vjp_call_bit_for_bit(setup, mode, n_points):
    import torch
    from pyrayhf_amd.autograd import differentiable_forward_operator
    freq, den, bmag, bpsi, alt = setup
    den = den.clone().requires_grad_(True)
    bmag = bmag.clone().requires_grad_(True)
    alt = alt.clone().requires_grad_(True)
    vh = differentiable_forward_operator(freq, den, bmag, bpsi, alt, mode, n_points)
    assert vh.requires_grad and vh.grad_fn is not None and vh.shape == (2, freq.numel())
    plain = library.vertical_forward_operator(freq, den.detach(), bmag.detach(), bpsi, alt.detach(), mode, n_points)
    assert same_bits(vh.detach().cpu().numpy(), plain.cpu().numpy())
    # a masked sum of squares against a synthetic trace
    mask = torch.isfinite(vh.detach())
    assert mask.any() and (~mask).any()
    trace = torch.where(mask, vh.detach() * 1.01 + 3.0, torch.zeros_like(vh))
    resid = torch.where(mask, vh - trace, torch.zeros_like(vh))
    loss = (resid * resid).sum()
    loss.backward()
    upstream = torch.where(mask, 2.0 * (vh.detach() - trace), torch.zeros_like(vh))
    want = library.vertical_vjp(freq, den.detach(), bmag.detach(), bpsi, alt.detach(), upstream, mode, n_points)
    assert den.grad is not None and den.grad.shape == den.shape
    assert torch.isfinite(den.grad).all() and den.grad.abs().sum() > 0
    assert np.array_equal(den.grad.cpu().numpy(), want.cpu().numpy())
    assert bmag.grad is None and alt.grad is None


def test_one_profile_and_the_plain_operator_without_a_graph(setup):
    import torch
    from pyrayhf_amd.autograd import differentiable_forward_operator
    freq, den, bmag, bpsi, alt = setup
    d = den[0].clone().requires_grad_(True)
    vh = differentiable_forward_operator(freq, d, bmag[0], bpsi[0], alt, "O", 63)
    assert vh.shape == (freq.numel(),)
    torch.nansum(vh).backward()
    g = torch.ones_like(vh)
    assert np.array_equal(d.grad.cpu().numpy(), library.vertical_vjp(freq, d.detach(), bmag[0], bpsi[0], alt, g, "O", 63).cpu().numpy())
    out = library.vertical_forward_operator(freq, d, bmag[0], bpsi[0], alt, "O", 63)
    assert torch.is_tensor(out) and not out.requires_grad and out.grad_fn is None
