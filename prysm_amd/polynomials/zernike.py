"""Zernike polynomials (prysm/polynomials/zernike.py) on the device, without a stored basis where none is asked for.

zernike_nm_seq writes its K planes in one launch (pm_zernike_basis); zernike_sum evaluates sum_k c_k Z_k per point (pm_zernike_sum)
and zernike_sum_adjoint the projections sum_p g[p] Z_k[p] (pm_zernike_project), both walking the mode table in registers.  The table
(zernike_plan.plan) is built on the host once per (modes, norm, dtype) and kept on the device, so a call copies nothing to the device
but its numpy arguments.  Arguments are checked here, before any upload.
"""
import numpy as np
import torch

from .. import _lib as L
from ._modal import _dtype_of, _code, _device_table, _check_coefs, _check_bar, _projector
from .zernike_plan import (zernike_norm, noll_to_nm, fringe_to_nm, nm_to_fringe, nm_to_ansi_j, ansi_j_to_nm, check_nms,  # noqa: F401
                           plan)

__all__ = ['zernike_norm', 'noll_to_nm', 'fringe_to_nm', 'nm_to_fringe', 'nm_to_ansi_j', 'ansi_j_to_nm', 'zernike_nm', 'zernike_nm_seq',
           'zernike_sum', 'zernike_sum_adjoint']

_TABLES = {}
_TABLES_MAX = 64


def _table(nms, norm, dtype):
    """the step table of (nms, norm, dtype) on the current device: (uint8 device tensor, number of steps)"""
    return _device_table(_TABLES, _TABLES_MAX, (nms, bool(norm)), dtype, lambda npdt: plan(nms, norm, npdt))


def _coords(u, v):
    """(u, v, dtype, shape): checked for equal shapes and real dtypes before upload, then contiguous device arrays of one dtype
    (float32 when both are float32, float64 otherwise)"""
    su, sv = tuple(np.shape(u)), tuple(np.shape(v))
    if su != sv:
        raise ValueError(f'coordinate arrays differ in shape: {su} and {sv}')
    du, dv = _dtype_of(u), _dtype_of(v)
    dt = torch.float32 if du == dv == torch.float32 else torch.float64
    return L.as_device(u, dt), L.as_device(v, dt), dt, su


# _seq, _sum and _adjoint take either coordinate form: coords PM_ZERNIKE_POLAR reads (u, v) as (r, t), PM_ZERNIKE_CARTESIAN as (x, y)
def _seq(nms, u, v, norm, coords):
    nms = check_nms(nms)
    u, v, dt, shape = _coords(u, v)
    out = torch.empty((len(nms), *shape), dtype=dt, device=u.device)
    if len(nms) and u.numel():
        tab, nsteps = _table(nms, norm, dt)
        L.check(L.load().pm_zernike_basis(_code(dt), coords, u.numel(), L.ptr(u), L.ptr(v), L.ptr(tab), nsteps, len(nms), L.ptr(out),
                                          L.stream_ptr()))
    return out


def zernike_nm_seq(nms, r, t, norm=True):
    """Zernike polynomials (n, m) of `nms` at the polar points (r, t): (K, *r.shape) in r's precision, in one launch
    (zernike.py:72-163).  norm=True gives unit RMS, norm=False leaves out zernike_norm."""
    return _seq(nms, r, t, norm, L.PM_ZERNIKE_POLAR)


def zernike_nm(n, m, r, t, norm=True):
    """One Zernike polynomial at the polar points (r, t) (zernike.py:34-69): zernike_nm_seq with K = 1."""
    return zernike_nm_seq(((n, m),), r, t, norm=norm)[0]


def zernike_sum(coefs, nms, x, y, norm=True):
    """sum_k coefs[k] Z_k at the Cartesian points (x, y) (zernike.py:166-181), evaluated per point without forming the basis, in one
    launch.  coefs (K,) gives x.shape; (B, K) gives (B, *x.shape), the basis evaluated once per point for every 8 vectors.  The
    coefficients are read on the device when the kernel runs, so a captured graph uses their current values."""
    return _sum(coefs, nms, x, y, norm, L.PM_ZERNIKE_CARTESIAN)


def _sum(coefs, nms, x, y, norm, coords):
    nms = check_nms(nms)
    coefs, shape = _check_coefs(coefs, len(nms), 'coefs', 'modes', 'Zernike coefficients')
    x, y, dt, xshape = _coords(x, y)
    c = L.as_device(coefs, dt).reshape(-1, len(nms))
    single, B = len(shape) == 1, c.shape[0]
    out = torch.empty((B, *xshape), dtype=dt, device=x.device)
    if not len(nms):
        out.zero_()
    elif x.numel() and B:
        tab, nsteps = _table(nms, norm, dt)
        L.check(L.load().pm_zernike_sum(_code(dt), coords, x.numel(), L.ptr(x), L.ptr(y), L.ptr(tab), nsteps, len(nms), B,
                                        L.ptr(c), 0, L.ptr(out), L.stream_ptr()))
    return out[0] if single else out


def zernike_sum_adjoint(databar, nms, x, y, norm=True):
    """The adjoint of zernike_sum with respect to the coefficients: sum_p databar[p] Z_k[p], (K,) for a databar of x.shape and (B, K)
    for (B, *x.shape) -- sum_of_2d_modes_adjoint(zernike_nm_seq(...), databar) without the basis.  Deterministic: two launches, no
    atomics."""
    return _adjoint(databar, nms, x, y, norm, L.PM_ZERNIKE_CARTESIAN)


def _adjoint(databar, nms, x, y, norm, coords):
    nms = check_nms(nms)
    shape_x, shape_y = tuple(np.shape(x)), tuple(np.shape(y))
    if shape_x != shape_y:
        raise ValueError(f'coordinate arrays differ in shape: {shape_x} and {shape_y}')
    shape_g = _check_bar(databar, shape_x, 'databar')
    x, y, dt, xshape = _coords(x, y)
    single = shape_g == xshape
    g = L.as_device(databar, dt)
    B = 1 if single else shape_g[0]
    out = torch.empty((B, len(nms)), dtype=dt, device=x.device)
    if len(nms) and B:
        tab, nsteps = _table(nms, norm, dt)
        _projector('zernike', dt, x.numel(), len(nms), B)(coords, x.numel(), L.ptr(x), L.ptr(y), L.ptr(tab), nsteps, len(nms), B, L.ptr(g),
                                                          L.ptr(out))
    return out[0] if single else out
