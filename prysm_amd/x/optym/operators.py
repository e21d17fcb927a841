"""Differentiable operators on the device (prysm/x/optym/operators.py)."""
import numpy as np
import torch

from ... import _lib as L
from ...coordinates import _code

__all__ = ['SpatialGradient2D']

_FLOATS = (torch.float32, torch.float64)


def _apply(op, a):
    assert a.ndim == 2, 'This operator only works on 2D arrays.'
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    if t.is_complex():
        raise TypeError('SpatialGradient2D takes real arrays')
    t = L.as_device(t, t.dtype if t.dtype in _FLOATS else torch.float64)
    out = torch.empty_like(t)
    if t.numel():
        m, n = t.shape
        L.check(L.load().pm_optym_spatial_gradient(_code(t.dtype), op, m, n, L.ptr(t), L.ptr(out), L.stream_ptr()))
    return out


class SpatialGradient2D:
    """Forward differences over the interior of an axis, x[i + 1] - x[i] for 1 <= i <= end - 2 and zero elsewhere, and their adjoints
    (operators.py:5-48).  One sweep each; the adjoints gather (out[i] = xbar[i - 1] - xbar[i] with the same index ranges), so no
    atomics are involved."""

    def forward_x(self, x):
        return _apply(L.PM_GRAD_FORWARD_X, x)

    def adjoint_x(self, xbar):
        return _apply(L.PM_GRAD_ADJOINT_X, xbar)

    def forward_y(self, x):
        return _apply(L.PM_GRAD_FORWARD_Y, x)

    def adjoint_y(self, xbar):
        return _apply(L.PM_GRAD_ADJOINT_Y, xbar)
