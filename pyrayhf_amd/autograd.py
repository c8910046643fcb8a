"""The vertical forward operator as a differentiable torch function.

``differentiable_forward_operator`` evaluates ``library.vertical_forward_operator`` on GPU-resident tensors and records
one node in torch's graph whose backward pass is a single ``prhf_vfo_vjp_f64`` launch (``library.vertical_vjp``): the
analytic vector-Jacobian product of the discrete operator with respect to the density column, recomputed from the saved
inputs (nothing of the forward pass is kept but them).  Under ``torch.autograd.forward_ad`` the tangent of ``den`` goes
through a single ``prhf_vfo_jvp_f64`` call (``library.vertical_jvp``), the Jacobian-vector product, in the same way.
The gradient flows to ``den`` only; ``freq``, ``bmag``, ``bpsi`` and ``alt`` are treated as constants.  ``library.vertical_forward_operator`` itself stays outside autograd.
"""

from __future__ import annotations

import torch

from . import library

__all__ = ["differentiable_forward_operator"]


class _ForwardOperator(torch.autograd.Function):
    @staticmethod
    def forward(ctx, den, freq, bmag, bpsi, alt, mode, n_points):
        ctx.save_for_backward(den, freq, bmag, bpsi, alt)
        ctx.save_for_forward(den, freq, bmag, bpsi, alt)
        ctx.mode, ctx.n_points = mode, n_points
        return library.vertical_forward_operator(freq, den.detach(), bmag, bpsi, alt, mode, n_points)

    @staticmethod
    def backward(ctx, grad_vh):
        den, freq, bmag, bpsi, alt = ctx.saved_tensors
        grad_den = None
        if ctx.needs_input_grad[0]:
            # (entries of grad_vh at pairs without a virtual height - NaN in the forward pass - are not read)
            grad_den = library.vertical_vjp(freq, den.detach(), bmag, bpsi, alt, grad_vh, ctx.mode, ctx.n_points)
            grad_den = grad_den.to(den.dtype).reshape(den.shape)
        return grad_den, None, None, None, None, None, None

    @staticmethod
    def jvp(ctx, den_t, *rest):
        # (tangents of the other inputs are ignored, as their gradients are)
        if den_t is None:
            return None
        den, freq, bmag, bpsi, alt = ctx.saved_tensors
        dvh = library.vertical_jvp(freq, den.detach(), bmag, bpsi, alt, den_t.to(torch.float64), ctx.mode, ctx.n_points)[1]
        return dvh


def differentiable_forward_operator(freq, den, bmag, bpsi, alt, mode='O', n_points=200):
    """Virtual heights [km] like ``library.vertical_forward_operator`` - ``(F,)`` for a 1-D ``den``, ``(P, F)`` for a
    batch - as a tensor that carries a graph when ``den.requires_grad``: ``loss.backward()`` puts
    ``sum_f dloss/dvh_f * dvh_f/dden_k`` into ``den.grad``, and under ``torch.autograd.forward_ad`` a dual ``den`` gives
    a dual result whose tangent is ``sum_k dvh_f/dden_k * tangent_k`` (zero where the result is NaN).

    All of ``den``, ``bmag``, ``bpsi`` must be float64 tensors on one GPU; ``freq`` and ``alt`` may be tensors there or
    host arrays.  NaN outputs (frequencies that are not reflected) contribute nothing to the gradient: mask them out of
    the loss (``torch.where`` / ``nansum``), the backward pass ignores whatever upstream gradient they receive.
    The other inputs get no gradient.  Conventions of the derivative: ``library.vertical_jacobian``.
    """
    tensors = [x for x in (den, bmag, bpsi) if not (torch.is_tensor(x) and x.is_cuda)]
    if tensors:
        raise ValueError("den, bmag and bpsi must be torch tensors on the GPU")
    if den.dtype != torch.float64:
        raise ValueError("den must be float64")
    library._mode_code(mode)
    freq, alt = (x if torch.is_tensor(x) else torch.as_tensor(x, dtype=torch.float64, device=den.device) for x in (freq, alt))
    return _ForwardOperator.apply(den, freq, bmag, bpsi, alt, mode, int(n_points))
