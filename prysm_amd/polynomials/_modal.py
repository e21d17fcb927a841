"""The plumbing the polynomial families share (zernike.py, qpoly.py, _recur.py; segmented.py takes the projection call): the precision
rule, the bounded cache of device tables, the shape checks of coefficients and adjoint inputs, and the workspace-then-project call.
Each family words its own errors: the checks take the noun and the name that appear in the message.
"""
import numpy as np
import torch

from .. import _lib as L


def _dtype_of(a, what='Zernike coordinates'):
    """float32 for float32 input, float64 for any other real input; TypeError for complex"""
    if isinstance(a, torch.Tensor):
        if a.is_complex():
            raise TypeError(f'{what} must be real')
        return torch.float32 if a.dtype == torch.float32 else torch.float64
    dt = np.asarray(a).dtype
    if np.issubdtype(dt, np.complexfloating):
        raise TypeError(f'{what} must be real')
    return torch.float32 if dt == np.float32 else torch.float64


def _code(dt):
    return L.PM_F32 if dt == torch.float32 else L.PM_F64


def _cached(cache, limit, key, make):
    """cache[key], made on a miss; the oldest entry leaves a cache of `limit` entries first"""
    hit = cache.get(key)
    if hit is None:
        if len(cache) >= limit:
            cache.pop(next(iter(cache)))
        hit = cache[key] = make()
    return hit


def _device_table(cache, limit, key, dt, plan):
    """the step table plan(numpy dtype) of `key` on the current device: (uint8 device tensor, number of steps)"""
    def make():
        t = plan(np.float32 if dt == torch.float32 else np.float64)
        return torch.from_numpy(t.view(np.uint8).copy()).to(L.device()), len(t)
    return _cached(cache, limit, (*key, dt, L._cur_dev()), make)


def _check_coefs(coefs, K, what, noun, real=None):
    """(coefs as an array or tensor, its shape): (K,) or (B, K) and real (`real` names them in that TypeError), before any upload"""
    if not isinstance(coefs, torch.Tensor):
        coefs = np.asarray(coefs)
    shape = tuple(coefs.shape)
    if len(shape) not in (1, 2) or shape[-1] != K:
        raise ValueError(f'{what} of shape {shape} do not match the {K} {noun} given (want ({K},) or (B, {K}))')
    _dtype_of(coefs, real or what)
    return coefs, shape


def _check_bar(g, shape, what):
    """the shape of g: that of the coordinates or a (B, ...) stack of them, and real"""
    sg = tuple(g.shape) if isinstance(g, torch.Tensor) else tuple(np.shape(g))
    if sg != shape and sg[1:] != shape:
        raise ValueError(f'{what} of shape {sg} does not match coordinates of shape {shape} (or a (B, ...) stack of them)')
    _dtype_of(g, what)
    return sg


def _projector(unit, dt, *sizes):
    """run(*args) calls pm_<unit>_project(code of dt, *args, workspace, its bytes, stream) and checks the result; the workspace is what
    pm_<unit>_project_workspace(code of dt, *sizes) asks for"""
    lib = L.load()
    ws = L.workspace(getattr(lib, f'pm_{unit}_project_workspace')(_code(dt), *sizes))
    project = getattr(lib, f'pm_{unit}_project')
    tail = (L.ptr(ws), ws.numel() if ws is not None else 0)
    return lambda *args: L.check(project(_code(dt), *args, *tail, L.stream_ptr()))
