"""Mode sums and their adjoint (prysm/polynomials/fitting.py) over a stored basis."""
import numpy as np
import torch

from .. import _lib as L
from .. import _ops

__all__ = ['sum_of_2d_modes', 'sum_of_2d_modes_adjoint']


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _is_complex(a):
    return a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a)


def _modes(modes):
    if isinstance(modes, (list, tuple)):
        modes = torch.stack([L.as_device(m) for m in modes])
    m = L.as_device(modes)
    if m.dim() < 2 or m.is_complex() or m.dtype not in (torch.float32, torch.float64):
        raise TypeError('modes must be a (K, ...) float32 or float64 array')
    return m


def sum_of_2d_modes(modes, weights):
    """sum_k weights[k] modes[k] over a (K, rows, cols) stack (fitting.py:7-37), in the modes' dtype (pm_sum_modes).

    The weights are read on the HOST when the call is made: a captured graph keeps the weights it was captured with.  To change the
    weights of a captured model, use zernike_sum, which reads its coefficients on the device."""
    shape = _shape(modes)
    if len(shape) != 3:
        raise ValueError('sum_of_2d_modes takes a (K, rows, cols) stack of modes')
    w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
    if w.ndim != 1 or len(w) != shape[0]:
        raise ValueError(f'{np.shape(w)} weights do not match {shape[0]} modes')
    m = _modes(modes)
    return _ops.sum_modes(m, [float(v) for v in w])


def sum_of_2d_modes_adjoint(modes, databar):
    """np.tensordot(modes, databar) of the reference (fitting.py:40-57): (K,) in the modes' dtype, sum_p modes[k][p] databar[p] over
    every point (pm_modes_dot).  Deterministic: two launches, no atomics."""
    shape, shape_g = _shape(modes), _shape(databar)
    if shape_g != tuple(shape[1:]):
        raise ValueError(f'databar of shape {shape_g} does not match modes of shape {shape}')
    if _is_complex(databar) or _is_complex(modes):
        raise TypeError('modes and databar must be real')
    m = _modes(modes)
    g = L.as_device(databar, m.dtype)
    K, npts = m.shape[0], g.numel()
    code = L.PM_F32 if m.dtype == torch.float32 else L.PM_F64
    out = torch.empty((K,), dtype=m.dtype, device=m.device)
    if K:
        lib = L.load()
        ws = L.workspace(lib.pm_modes_dot_workspace(code, K, npts))
        L.check(lib.pm_modes_dot(code, K, npts, L.ptr(m), m.stride(0), L.ptr(g), L.ptr(out), L.ptr(ws), ws.numel() if ws is not None else 0,
                                 L.stream_ptr()))
    return out
