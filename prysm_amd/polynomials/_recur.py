"""The plumbing the recurrence families share (jacobi.py, cheby.py, legendre.py, hermite.py, laguerre.py, dickson.py, xy.py): argument
checks, the cache of device tables, and the calls into csrc/recur.hip.  The conventions are zernike.py's: torch tensors on the device in
and out, numpy accepted and uploaded, float32 stays float32 and any other real input becomes float64, complex input is a TypeError, and
every argument is checked before anything is uploaded.
"""
import numpy as np
import torch

from .. import _lib as L
from . import recur_plan as RP
from ._modal import _dtype_of, _code, _cached, _device_table, _check_coefs, _check_bar, _projector

_TABLES = {}
_TABLES_MAX = 128
_PAIRS = {}


def _table(family, params, ns, nmax, dt):
    """the table of (family, params, orders, dtype) on the current device: (uint8 device tensor, number of records)"""
    return _device_table(_TABLES, _TABLES_MAX, (family, params, ns, nmax), dt, lambda npdt: RP.plan(family, ns, *params, nmax=nmax, dtype=npdt))


def _params(family, params):
    if len(params) != RP.FAMILIES[family]:
        raise ValueError(f'{family} takes {RP.FAMILIES[family]} shape parameter(s), got {len(params)}')
    return tuple(float(p) for p in params)


# ----------------------------------------------------------------------------- 1-D: basis

def basis(family, params, ns, x, want):
    """P_k(x) ('p'), dP_k/dx ('d') or both ('pd') for the strictly ascending orders ns: (len(ns), *x.shape) each, one launch."""
    params = _params(family, params)
    ns = RP.check_ns(ns)
    dt = _dtype_of(x, 'polynomial coordinates')
    shape = tuple(np.shape(x))
    x = L.as_device(x, dt)
    outs = [torch.empty((len(ns), *shape), dtype=dt, device=x.device) if c in want else None for c in 'pd']
    if len(ns) and x.numel():
        tab, nsteps = _table(family, params, ns, None, dt)
        L.check(L.load().pm_recur_basis(_code(dt), L.PM_RECUR_X, x.numel(), L.ptr(x), None, 0.0, L.ptr(tab), nsteps, len(ns),
                                        L.ptr(outs[0]), L.ptr(outs[1]), L.stream_ptr()))
    got = tuple(o for o in outs if o is not None)
    return got if len(got) > 1 else got[0]


def _single(n):
    if int(n) != n or n < 0:
        raise ValueError(f'the polynomial order must be a non-negative integer, got {n!r}')
    return (int(n),)


def make_family(family, where):
    """(f, f_seq, f_der, f_der_seq) of a family, with the reference's signatures: the shape parameters between the order(s) and x."""
    npar = RP.FAMILIES[family]
    sig = ''.join(f', {p}' for p in ('alpha', 'beta')[:npar])

    def f(n, *args):
        return basis(family, args[:-1], _single(n), args[-1], 'p')[0]

    def f_seq(ns, *args):
        return basis(family, args[:-1], ns, args[-1], 'p')

    def f_der(n, *args):
        return basis(family, args[:-1], _single(n), args[-1], 'd')[0]

    def f_der_seq(ns, *args):
        return basis(family, args[:-1], ns, args[-1], 'd')

    f.__doc__ = f"""{family}(n{sig}, x): the polynomial of order n at the points x, in x's precision ({where}): {family}_seq with one order."""
    f_seq.__doc__ = f"""{family}_seq(ns{sig}, x): the polynomials of the orders ns at x, (len(ns), *x.shape), in one launch that walks the
    recurrence once per point ({where}).  ns must be strictly ascending (ValueError otherwise; the reference returns uninitialised planes
    for unsorted orders)."""
    f_der.__doc__ = f"""{family}_der(n{sig}, x): the first derivative with respect to x of the polynomial of order n ({where})."""
    f_der_seq.__doc__ = f"""{family}_der_seq(ns{sig}, x): the first derivatives of the orders ns, (len(ns), *x.shape), from the differentiated
    recurrence in one launch ({where}).  ns must be strictly ascending."""
    for fn, suffix in ((f, ''), (f_seq, '_seq'), (f_der, '_der'), (f_der_seq, '_der_seq')):
        fn.__name__ = fn.__qualname__ = family + suffix
    return f, f_seq, f_der, f_der_seq


# ----------------------------------------------------------------------------- 1-D: sums and their adjoint

def _coefs(coefs, K, what='coefficients'):
    """(coefs as given, single): checked for shape (K,) or (B, K) and a real dtype"""
    coefs, shape = _check_coefs(coefs, K, what, 'orders')
    return coefs, len(shape) == 1


def _points(x, y, radius):
    """(x, y or None, dtype, shape, form, radius) of the X or the R2 form, checked before upload"""
    if y is None:
        dt = _dtype_of(x, 'polynomial coordinates')
        return L.as_device(x, dt), None, dt, tuple(np.shape(x)), L.PM_RECUR_X, 0.0
    sx, sy = tuple(np.shape(x)), tuple(np.shape(y))
    if sx != sy:
        raise ValueError(f'coordinate arrays differ in shape: {sx} and {sy}')
    radius = float(radius)
    if not radius > 0:
        raise ValueError(f'the normalisation radius must be positive, got {radius}')
    dx, dy = _dtype_of(x, 'polynomial coordinates'), _dtype_of(y, 'polynomial coordinates')
    dt = torch.float32 if dx == dy == torch.float32 else torch.float64
    return L.as_device(x, dt), L.as_device(y, dt), dt, sx, L.PM_RECUR_R2, radius


def sum1d(family, params, coefs, ns, x, y=None, radius=None, want='z'):
    """sum_k coefs[k] P_{ns[k]} at x (y None), or at 2 (x^2 + y^2) / radius^2 - 1: a tuple of the outputs named in want -- 'z' the
    sum, 'x' its derivative (d/dx, with the chain factor of the radial form) and 'y' (radial form only).  coefs (K,) or (B, K)."""
    params = _params(family, params)
    ns = RP.check_ns(ns)
    coefs, single = _coefs(coefs, len(ns))
    x, y, dt, shape, form, radius = _points(x, y, radius)
    c = L.as_device(coefs, dt).reshape(-1, len(ns))
    B = c.shape[0]
    outs = [torch.empty((B, *shape), dtype=dt, device=x.device) if w in want else None for w in 'zxy']
    if not len(ns):
        for o in outs:
            if o is not None:
                o.zero_()
    elif x.numel() and B:
        tab, nsteps = _table(family, params, ns, None, dt)
        L.check(L.load().pm_recur_sum(_code(dt), form, x.numel(), L.ptr(x), L.ptr(y), radius, L.ptr(tab), nsteps, len(ns), B, L.ptr(c), 0,
                                      L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.stream_ptr()))
    return tuple((o[0] if single else o) for o in outs if o is not None)


def _bar(g, shape, what):
    """(g as given, is a single map): g of the coordinates' shape or a (B, ...) stack of them, real"""
    return g, _check_bar(g, shape, what) == shape


def project1d(family, params, ns, x, y=None, radius=None, databar=None, dx_bar=None, dy_bar=None):
    """The adjoint of sum1d with respect to the coefficients: sum_p databar P_k + (the derivative maps' adjoints) D_k, (K,) or (B, K).
    Deterministic: two launches per term, no atomics."""
    params = _params(family, params)
    ns = RP.check_ns(ns)
    shape = tuple(np.shape(x))
    if databar is None and dx_bar is None and dy_bar is None:
        raise ValueError('give at least one of databar, dx_bar, dy_bar')
    if dy_bar is not None and y is None:
        raise ValueError('dy_bar needs the radial form')
    singles = {_bar(g, shape, name)[1] for g, name in ((databar, 'databar'), (dx_bar, 'dx_bar'), (dy_bar, 'dy_bar')) if g is not None}
    if len(singles) != 1:
        raise ValueError('databar, dx_bar and dy_bar must have one shape')
    single = singles.pop()
    x, y, dt, shape, form, radius = _points(x, y, radius)
    g, gx, gy = (None if a is None else L.as_device(a, dt) for a in (databar, dx_bar, dy_bar))
    first = next(a for a in (g, gx, gy) if a is not None)
    B = 1 if single else first.shape[0]
    out = torch.zeros((B, len(ns)), dtype=dt, device=x.device)
    if len(ns) and B and x.numel():
        tab, nsteps = _table(family, params, ns, None, dt)
        project = _projector('recur', dt, x.numel(), len(ns), B)

        def run(der, a, b):
            project(form, x.numel(), L.ptr(x), L.ptr(y), radius, L.ptr(tab), nsteps, len(ns), B, der, L.ptr(a), L.ptr(b), 1, L.ptr(out))
        if g is not None:
            run(0, g, None)
        if form == L.PM_RECUR_X:
            if gx is not None:
                run(1, gx, None)
        elif gx is not None or gy is not None:
            if gx is None:          # the kernel's first map is dx_bar: a zero one stands in
                gx = torch.zeros_like(gy)
            run(1, gx, gy)
    return out[0] if single else out


# ----------------------------------------------------------------------------- 2-D: separable sums on a Cartesian grid

def _axes(x, y, cartesian_grid):
    """(x[cols], y[rows], dtype): 1-D axes as given, or row 0 of a 2-D x and column 0 of a 2-D y (coordinates.optimize_xy_separable)"""
    if not cartesian_grid:
        raise NotImplementedError('the 2-D polynomial sums are separable kernels: cartesian_grid=False is not supported')
    dx, dy = _dtype_of(x, 'grid coordinates'), _dtype_of(y, 'grid coordinates')
    dt = torch.float32 if dx == dy == torch.float32 else torch.float64
    sx, sy = tuple(np.shape(x)), tuple(np.shape(y))
    if len(sx) not in (1, 2) or len(sy) not in (1, 2):
        raise ValueError(f'x and y must be 1-D axes or 2-D meshgrids, got shapes {sx} and {sy}')
    if len(sx) == 2 and len(sy) == 2 and sx != sy:
        raise ValueError(f'coordinate arrays differ in shape: {sx} and {sy}')
    return (lambda: L.as_device(x[0] if len(sx) == 2 else x, dt), lambda: L.as_device(y[:, 0] if len(sy) == 2 else y, dt), dt,
            (sy[0], sx[-1]))


_MNS = {}


def _orders(mns):
    """(the pairs as a tuple of int pairs, nx, ny), checked; remembered per list of pairs, so a loop that calls with the same pairs
    pays for the checks once"""
    try:
        key = mns if isinstance(mns, tuple) else tuple(mns)
        hit = _MNS.get(key)
    except TypeError:                # rows that do not hash (lists, arrays)
        key = tuple(tuple(mn) for mn in mns)
        hit = _MNS.get(key)
    if hit is None:
        pairs = RP.check_mns(key)
        nx, ny = (max(m for m, _ in pairs) + 1, max(n for _, n in pairs) + 1) if pairs else (0, 0)
        if nx > RP.MAX_ORDERS_2D or ny > RP.MAX_ORDERS_2D:
            raise NotImplementedError(f'{ny} x {nx} orders: an axis of the separable kernels takes at most {RP.MAX_ORDERS_2D}')
        if len(_MNS) >= _TABLES_MAX:
            _MNS.pop(next(iter(_MNS)))
        hit = _MNS[key] = (pairs, nx, ny)
    return hit


def _flat_index(mns, nx):
    """(device int64 positions n * nx + m of the pairs in the dense matrix, whether any pair repeats)"""
    def make():
        idx = [n * nx + m for m, n in mns]
        return torch.tensor(idx, dtype=torch.int64, device=L.device()), len(set(idx)) != len(idx)
    return _cached(_PAIRS, _TABLES_MAX, ('flat', mns, nx, L._cur_dev()), make)


def sum2d(family, coefs, mns, x, y, want='z', x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """The tensor-product sum of `family` on a Cartesian grid and its gradient maps, a tuple of the outputs named in want ('z', 'x',
    'y'), each (rows, cols) or (B, rows, cols).  One launch; the dense coefficient matrix is gathered on the device from coefs."""
    if not hasattr(mns, '__len__'):
        mns = tuple(mns)
    coefs, single = _coefs(coefs, len(mns), 'coefficients')
    getx, gety, dt, (rows, cols) = _axes(x, y, cartesian_grid)
    mns, nx, ny = _orders(mns)
    if not mns:
        B = 1 if single else coefs.shape[0]
        z = torch.zeros((B, rows, cols), dtype=dt, device=L.device())
        return tuple((z[0] if single else z) for _ in want)
    x, y = getx(), gety()
    c = L.as_device(coefs, dt).reshape(-1, len(mns))
    B = c.shape[0]
    idx, dup = _flat_index(mns, nx)
    C = torch.zeros((B, ny * nx), dtype=dt, device=x.device)
    if dup:
        C.index_add_(1, idx, c)
    else:
        C.index_copy_(1, idx, c)
    buf = torch.empty((len(want), B, rows, cols), dtype=dt, device=x.device)         # one allocation for the maps asked for
    outs = [buf[want.index(w)] if w in want else None for w in 'zxy']
    what = sum(bit for w, bit in zip('zxy', (L.PM_RECUR2_Z, L.PM_RECUR2_ZX, L.PM_RECUR2_ZY)) if w in want)
    if rows and cols and B:
        xt, _ = _table(family, (), None, nx - 1, dt)
        yt, _ = _table(family, (), None, ny - 1, dt)
        L.check(L.load().pm_recur2_sum(_code(dt), rows, cols, L.ptr(x), L.ptr(y), L.ptr(xt), nx, L.ptr(yt), ny, B, L.ptr(C), what,
                                       1.0 / x_norm, 1.0 / y_norm, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), cols, rows * cols,
                                       L.stream_ptr()))
    return tuple((o[0] if single else o) for o in outs if o is not None)


def adjoint2d(family, mns, x, y, databar=None, dx_bar=None, dy_bar=None, x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """The gradient with respect to coefs of sum2d's maps, in the order of mns: (K,) or (B, K).  databar is the adjoint of z, dx_bar and
    dy_bar of the gradient maps; their projections add into one matrix.  Two launches per map given, deterministic, no atomics."""
    if databar is None and dx_bar is None and dy_bar is None:
        raise ValueError('give at least one of databar, dx_bar, dy_bar')
    getx, gety, dt, (rows, cols) = _axes(x, y, cartesian_grid)
    mns, nx, ny = _orders(mns)
    singles = {_bar(g, (rows, cols), name)[1] for g, name in ((databar, 'databar'), (dx_bar, 'dx_bar'), (dy_bar, 'dy_bar')) if g is not None}
    if len(singles) != 1:
        raise ValueError('databar, dx_bar and dy_bar must have one shape')
    single = singles.pop()
    first = next(a for a in (databar, dx_bar, dy_bar) if a is not None)
    B = 1 if single else first.shape[0]
    if not mns:
        out = torch.zeros((B, 0), dtype=dt, device=L.device())
        return out[0] if single else out
    x, y = getx(), gety()
    Cbar = torch.zeros((B, ny * nx), dtype=dt, device=x.device)
    if rows and cols and B:
        lib = L.load()
        xt, _ = _table(family, (), None, nx - 1, dt)
        yt, _ = _table(family, (), None, ny - 1, dt)
        ws = L.workspace(lib.pm_recur2_project_workspace(_code(dt), rows, cols, ny, B))
        for g, what in ((databar, L.PM_RECUR2_Z), (dx_bar, L.PM_RECUR2_ZX), (dy_bar, L.PM_RECUR2_ZY)):
            if g is None:
                continue
            g = L.as_device(g, dt)
            L.check(lib.pm_recur2_project(_code(dt), rows, cols, L.ptr(x), L.ptr(y), L.ptr(xt), nx, L.ptr(yt), ny, B, what, 1.0 / x_norm,
                                          1.0 / y_norm, L.ptr(g), cols, rows * cols, 1, L.ptr(Cbar), L.ptr(ws), ws.numel(), L.stream_ptr()))
    idx, _ = _flat_index(mns, nx)
    out = Cbar.index_select(1, idx)
    return out[0] if single else out


def outer_seq(mns, x, y, xder, yder, cartesian_grid=True):
    """out[k] = Fy_{n_k}(y) (x) Fx_{m_k}(x) of the monomials, F the powers or their derivatives: two small tables, one write-bound launch"""
    mns = RP.check_mns(mns)
    getx, gety, dt, (rows, cols) = _axes(x, y, cartesian_grid)
    out = torch.empty((len(mns), rows, cols), dtype=dt, device=L.device())
    if not (len(mns) and rows and cols):
        return out
    nx, ny = max(m for m, _ in mns) + 1, max(n for _, n in mns) + 1
    tx = basis('monomial', (), range(nx), getx(), 'd' if xder else 'p')
    ty = basis('monomial', (), range(ny), gety(), 'd' if yder else 'p')
    pairs = _cached(_PAIRS, _TABLES_MAX, ('pairs', mns, L._cur_dev()),
                    lambda: torch.tensor(mns, dtype=torch.int32, device=L.device()).contiguous())
    L.check(L.load().pm_recur2_outer(_code(dt), rows, cols, len(mns), L.ptr(ty), ny, L.ptr(tx), nx, L.ptr(pairs), L.ptr(out),
                                     L.stream_ptr()))
    return out
