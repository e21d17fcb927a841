"""Forbes Q polynomials (prysm/polynomials/qpoly.py) on the device: Qbfs, Qcon and Q2D bases, their matrix-free sums and the sums'
adjoints with respect to the coefficients.

The _seq functions write their K planes in one launch (pm_qpoly_basis); the sums evaluate sum_k c_k Q_k per point (pm_qpoly_sum) and
the adjoints sum_p g[p] Q_k[p] (pm_qpoly_project), walking the mode table in registers.  The table (qpoly_plan.plan) is built on the
host once per (modes, family, dtype) and kept on the device.  Inputs, outputs and precision follow zernike.py: float32 in gives
float32 out, any other real input float64; results are device tensors; arguments are checked before any upload.
"""
import numpy as np
import torch

from .. import _lib as L
from .qpoly_plan import (g_qbfs, h_qbfs, f_qbfs, abc_q2d, G_q2d, F_q2d, g_q2d, f_q2d, Q2d_nm_c_to_a_b,  # noqa: F401
                         check_ns, check_q2d_nms, plan, QBFS, QCON, Q2D)
from ._modal import _dtype_of, _code, _device_table, _check_coefs, _check_bar, _projector

__all__ = ['g_qbfs', 'h_qbfs', 'f_qbfs', 'abc_q2d', 'G_q2d', 'F_q2d', 'g_q2d', 'f_q2d', 'Q2d_nm_c_to_a_b', 'Qbfs', 'Qbfs_seq',
           'Qcon', 'Qcon_seq', 'Q2d', 'Q2d_seq', 'compute_z_Qbfs', 'compute_z_Q2d', 'Q2d_sum', 'Q2d_sum_adjoint', 'Qcon_sum',
           'Qcon_sum_adjoint']

_TABLES = {}
_TABLES_MAX = 64


def _table(modes, family, dtype):
    """the step table of (modes, family, dtype) on the current device: (uint8 device tensor, number of steps)"""
    return _device_table(_TABLES, _TABLES_MAX, (modes, family), dtype, lambda npdt: plan(modes, family, npdt))


def _modes(modes, family):
    return check_q2d_nms(modes) if family == Q2D else check_ns(modes)


def _points(u, v, what='Q polynomial coordinates'):
    """(u, v, dtype, shape), v None for radial points: shapes and dtypes checked before upload, then contiguous device arrays of one
    dtype (float32 when every coordinate is float32, float64 otherwise)"""
    su = tuple(np.shape(u))
    dts = [_dtype_of(u, what)]
    if v is not None:
        sv = tuple(np.shape(v))
        if su != sv:
            raise ValueError(f'coordinate arrays differ in shape: {su} and {sv}')
        dts.append(_dtype_of(v, what))
    dt = torch.float32 if all(d == torch.float32 for d in dts) else torch.float64
    return L.as_device(u, dt), (None if v is None else L.as_device(v, dt)), dt, su


def _seq(modes, family, u, v, coords):
    modes = _modes(modes, family)
    u, v, dt, shape = _points(u, v)
    out = torch.empty((len(modes), *shape), dtype=dt, device=u.device)
    if len(modes) and u.numel():
        tab, nsteps = _table(modes, family, dt)
        L.check(L.load().pm_qpoly_basis(_code(dt), coords, u.numel(), L.ptr(u), L.ptr(v), L.ptr(tab), nsteps, len(modes), L.ptr(out),
                                        L.stream_ptr()))
    return out


def _sum(coefs, modes, family, u, v, coords):
    modes = _modes(modes, family)
    coefs, shape = _check_coefs(coefs, len(modes), 'coefs', 'modes', 'Q polynomial coefficients')
    u, v, dt, ushape = _points(u, v)
    single = len(shape) == 1
    B = 1 if single else shape[0]
    c = L.as_device(coefs, dt).reshape(B, len(modes))
    out = torch.empty((B, *ushape), dtype=dt, device=u.device)
    if not len(modes):
        out.zero_()
    elif u.numel() and B:
        tab, nsteps = _table(modes, family, dt)
        L.check(L.load().pm_qpoly_sum(_code(dt), coords, u.numel(), L.ptr(u), L.ptr(v), L.ptr(tab), nsteps, len(modes), B, L.ptr(c), 0,
                                      L.ptr(out), L.stream_ptr()))
    return out[0] if single else out


def _adjoint(databar, modes, family, u, v, coords):
    modes = _modes(modes, family)
    shape_u = tuple(np.shape(u))
    if v is not None and tuple(np.shape(v)) != shape_u:
        raise ValueError(f'coordinate arrays differ in shape: {shape_u} and {tuple(np.shape(v))}')
    shape_g = _check_bar(databar, shape_u, 'databar')
    u, v, dt, ushape = _points(u, v)
    single = shape_g == ushape
    g = L.as_device(databar, dt)
    B = 1 if single else shape_g[0]
    out = torch.empty((B, len(modes)), dtype=dt, device=u.device)
    if len(modes) and B:
        tab, nsteps = _table(modes, family, dt)
        _projector('qpoly', dt, u.numel(), len(modes), B)(coords, u.numel(), L.ptr(u), L.ptr(v), L.ptr(tab), nsteps, len(modes), B, L.ptr(g),
                                                          L.ptr(out))
    return out[0] if single else out


# ---------------------------------------------------------------- the reference's functions
def Qbfs_seq(ns, x):
    """Qbfs polynomials of orders ns at the normalised radii x, prefix x^2 (1 - x^2) included: (len(ns), *x.shape), one launch
    (qpoly.py:408).  Any order of ns."""
    return _seq(ns, QBFS, x, None, L.PM_QPOLY_RADIAL)


def Qbfs(n, x):
    """Qbfs polynomial of order n at x (qpoly.py:65): Qbfs_seq with one order."""
    return Qbfs_seq((n,), x)[0]


def Qcon_seq(ns, x):
    """Qcon polynomials of orders ns at the normalised radii x, prefix x^4 included: (len(ns), *x.shape), one launch (qpoly.py:654)."""
    return _seq(ns, QCON, x, None, L.PM_QPOLY_RADIAL)


def Qcon(n, x):
    """Qcon polynomial of order n at x (qpoly.py:621): Qcon_seq with one order."""
    return Qcon_seq((n,), x)[0]


def Q2d_seq(nms, r, t):
    """2D-Q polynomials (n, m) of `nms` at the polar points (r, t), prefixes included: m > 0 the cosine, m < 0 the sine term, m = 0
    Qbfs.  (len(nms), *r.shape) in one launch (qpoly.py:1003)."""
    return _seq(nms, Q2D, r, t, L.PM_ZERNIKE_POLAR)


def Q2d(n, m, r, t):
    """One 2D-Q polynomial at the polar points (r, t) (qpoly.py:893): Q2d_seq with one mode."""
    return Q2d_seq(((n, m),), r, t)[0]


def _trim(c):
    c = list(np.asarray(c, dtype=np.float64).reshape(-1)) if c is not None else []
    while c and c[-1] == 0:
        c.pop()
    return c


def compute_z_Qbfs(coefs, u, usq=None):
    """sum_n coefs[n] Qbfs_n(u), n = 0 .. len(coefs) - 1: the sag u^2 (1 - u^2) S(u^2) of a Qbfs surface (qpoly.py:349), evaluated
    per point on the device in one launch (no Clenshaw).  `usq` is accepted for signature compatibility and not read: u^2 is
    computed from u in the kernel."""
    c = _trim(coefs)
    return _sum(np.asarray(c), range(len(c)), QBFS, u, None, L.PM_QPOLY_RADIAL)


def compute_z_Q2d(cm0, ams, bms, u, t):
    """The sag of a 2D-Q surface at the polar points (u, t) from the dense coefficients of Q2d_nm_c_to_a_b (qpoly.py:1888): cm0 the
    Qbfs (m = 0) terms by n, ams[m - 1] the cosine and bms[m - 1] the sine terms of order m.  Evaluated matrix-free in one launch:
    equal to sum c Q2d_seq(...) over the same modes."""
    nms, cs = [], []
    for n, c in enumerate(_trim(cm0)):
        nms.append((n, 0))
        cs.append(c)
    for sign, terms in ((1, ams), (-1, bms)):
        for i, row in enumerate(terms):
            for n, c in enumerate(_trim(row)):
                nms.append((n, sign * (i + 1)))
                cs.append(c)
    return _sum(np.asarray(cs, dtype=np.float64), nms, Q2D, u, t, L.PM_ZERNIKE_POLAR)


# ---------------------------------------------------------------- sums and adjoints (new)
def Q2d_sum(coefs, nms, x, y):
    """sum_k coefs[k] Q2d_k at the Cartesian points (x, y), evaluated per point without forming the basis, in one launch.  coefs
    (K,) gives x.shape; (B, K) gives (B, *x.shape), the basis evaluated once per point for every 8 vectors.  The coefficients are
    read on the device when the kernel runs, so a captured graph uses their current values."""
    return _sum(coefs, nms, Q2D, x, y, L.PM_ZERNIKE_CARTESIAN)


def Q2d_sum_adjoint(databar, nms, x, y):
    """The adjoint of Q2d_sum with respect to the coefficients: sum_p databar[p] Q2d_k[p], (K,) for a databar of x.shape and (B, K)
    for (B, *x.shape), without the basis.  Deterministic: two launches, no atomics."""
    return _adjoint(databar, nms, Q2D, x, y, L.PM_ZERNIKE_CARTESIAN)


def Qcon_sum(coefs, ns, x):
    """sum_k coefs[k] Qcon_{ns[k]}(x) at the normalised radii x; coefs (K,) or (B, K), as Q2d_sum."""
    return _sum(coefs, ns, QCON, x, None, L.PM_QPOLY_RADIAL)


def Qcon_sum_adjoint(databar, ns, x):
    """The adjoint of Qcon_sum with respect to the coefficients, as Q2d_sum_adjoint."""
    return _adjoint(databar, ns, QCON, x, None, L.PM_QPOLY_RADIAL)
