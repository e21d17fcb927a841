"""Cost functions on the device (prysm/x/optym/cost.py): each returns (cost, d cost / d model).

mean_square_error, bias_and_gain_invariant_error and negative_loglikelihood, each `(M, D, mask=None)` with the reference's dtype check
(TypeError on a mismatch).  Inputs are numpy arrays or torch tensors of any shape; the cost comes back as a 0-d DEVICE tensor of the
data's dtype and the gradient as a device tensor of M's shape -- nothing is read on the host, so a cost can be captured in a graph
(prysm_amd.graph.capture).  A mask is a per-element predicate inside the kernels, not an index (`M[mask]` would need the selected
count on the host); the gradient is zero where it is false.

Differences from the reference, deliberate: an all-false mask gives a NaN cost and a zero gradient (the reference raises or divides
by zero); the sums are accumulated in float64 whatever the data's dtype.
"""
import numbers

import numpy as np
import torch

from ... import _lib as L
from ...coordinates import _code

__all__ = ['mean_square_error', 'bias_and_gain_invariant_error', 'negative_loglikelihood']

_FLOATS = (torch.float32, torch.float64)


def _dtype_check(name, M, D):
    if hasattr(M, 'dtype') and hasattr(D, 'dtype'):
        a = L.torch_dtype(M.dtype) if not isinstance(M.dtype, torch.dtype) else M.dtype
        b = L.torch_dtype(D.dtype) if not isinstance(D.dtype, torch.dtype) else D.dtype
        if a != b:
            raise TypeError(f'{name}: the dtypes of the two arrays differ ({M.dtype} and {D.dtype}); cast one of them first')


def _cost(name, kind, M, D, mask):
    _dtype_check(name, M, D)
    scalar = isinstance(D, numbers.Number)
    m = L.as_device(M)
    if m.dtype not in _FLOATS:
        raise TypeError(f'{name}: the data must be float32 or float64, got {m.dtype}')
    if scalar and kind != L.PM_COST_NLL:      # only the likelihood's kernel takes a scalar target
        D, scalar = torch.full_like(m, float(D)), False
    d = None
    if not scalar:
        d = L.as_device(D)
        if d.dtype != m.dtype:
            raise TypeError(f'{name}: the dtypes of the two arrays differ ({m.dtype} and {d.dtype}); cast one of them first')
        if d.shape != m.shape:
            raise ValueError(f'{name}: the shapes of the two arrays differ ({tuple(m.shape)} and {tuple(d.shape)})')
    k = None
    if mask is not None:
        k = L.as_device(mask)
        if k.shape != m.shape:
            raise ValueError(f'{name}: the mask must have the shape of the data')
        if k.dtype == torch.bool:
            k = k.view(torch.uint8)
        elif k.dtype != torch.uint8:
            k = (k != 0).view(torch.uint8)
    if m.numel() == 0:
        raise ValueError(f'{name}: empty arrays')
    cost = torch.empty((), dtype=m.dtype, device=m.device)
    grad = torch.empty_like(m)
    lib = L.load()
    ws = L.workspace(int(lib.pm_optym_cost_workspace()))
    L.check(lib.pm_optym_cost(_code(m.dtype), kind, m.numel(), L.ptr(m), L.ptr(d), float(D) if scalar else 0.0, L.ptr(k), L.ptr(cost),
                              L.ptr(grad), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return cost, grad


def mean_square_error(M, D, mask=None):
    """mean((M - D)^2) over the kept elements and its gradient 2 (M - D) / N (cost.py:73-96).  Three launches."""
    return _cost('mean_square_error', L.PM_COST_MSE, M, D, mask)


def bias_and_gain_invariant_error(I, D, mask=None):  # noqa: E741
    """The squared residual of D against the least-squares fit alpha I + beta over the kept elements, normalised by sum(D^2), and its
    gradient 2 R alpha (alpha I + beta - D) (cost.py:30-70).  Six launches: N, the two sums and sum D^2 in one read and the means on
    the device, the covariance and variance of the centred data in a second read and alpha, beta on the device, the gradient with
    the residual's sum of squares, the cost."""
    return _cost('bias_and_gain_invariant_error', L.PM_COST_BGI, I, D, mask)


def negative_loglikelihood(y, yhat, mask=None):
    """-mean(yhat log y + (1 - yhat) log(1 - y)) over the kept elements and its gradient (cost.py:99-125); yhat an array or a
    scalar.  Three launches."""
    return _cost('negative_loglikelihood', L.PM_COST_NLL, y, yhat, mask)
