"""Host side of the recurrence kernels (csrc/recur.hip), free of torch: the table every family is walked from, and the same walk in numpy.

Jacobi, the four Chebyshev kinds, Legendre, Hermite He / H, Laguerre, both Dickson kinds and the monomials all obey

    P_k = (a_k + b_k x) P_{k-1} - c_k P_{k-2},      D_k = b_k P_{k-1} + (a_k + b_k x) D_{k-1} - c_k D_{k-2}      (D = dP/dx)

so `plan` turns (family, parameters, orders) into one table of nmax + 1 records (a, b, c, slot), record k describing order k.  The walk
starts from P_{-1} = 1, P_{-2} = 0 and D = 0: record 0 is (P_0, 0, 0), and record 1 has c = 0 (the term it would multiply is P_{-1},
which the recurrences take as zero).  `slot` is the output plane of order k, or -1 for an order that is walked and not written.
`evaluate` is the walk in numpy, in the table's precision: the model the tests hold the kernels to.  `separable_sum` and
`separable_project` are the factored 2-D sum and its adjoint, Py(rows)^T . C . Px(cols), as pm_recur2_sum / pm_recur2_project form them.
"""
import numpy as np

__all__ = ['FAMILIES', 'MAX_ORDERS_2D', 'step_dtype', 'check_ns', 'plan', 'evaluate', 'separable_sum', 'separable_project', 'xy_j_to_mn',
           'recurrence_abc', 'weight', 'coefficient_matrix', 'check_mns']

# family -> number of shape parameters
FAMILIES = {'cheby1': 0, 'cheby2': 0, 'cheby3': 0, 'cheby4': 0, 'legendre': 0, 'hermite_He': 0, 'hermite_H': 0, 'laguerre': 1,
            'dickson1': 1, 'dickson2': 1, 'jacobi': 2, 'monomial': 0}
MAX_ORDERS_2D = 64      # orders per axis of the separable kernels (csrc/recur.hip kMaxOrder)


def weight(alpha, beta, x):
    """The weight function of the Jacobi polynomials, (1 - x)^alpha (1 + x)^beta (jacobi.py:10-12)."""
    return (1 - x) ** alpha * (1 + x) ** beta


def recurrence_abc(n, alpha, beta):
    """(A, B, C) of P_{n+1} = (A x + B) P_n - C P_{n-1} for the Jacobi polynomials (DLMF 18.9.1-2; jacobi.py:15-43), with the closed
    form at n = 0 where alpha + beta is 0 or -1 and the general expression divides by zero."""
    apb = alpha + beta
    if n == 0 and (apb == 0 or apb == -1):
        return apb / 2 + 1, (alpha - beta) / 2, 1
    s = 2 * n + apb
    A = (s + 1) * (s + 2) / (2 * (n + 1) * (n + apb + 1))
    B = (alpha ** 2 - beta ** 2) * (s + 1) / (2 * (n + 1) * (n + apb + 1) * s)
    C = (n + alpha) * (n + beta) * (s + 2) / ((n + 1) * (n + apb + 1) * s)
    return A, B, C


def xy_j_to_mn(j):
    """Mono-index j (from 1, piston) to the powers (m, n) of x^m y^n (xy.py:11-27): total order t holds j in
    (t (t + 1) / 2, (t + 1) (t + 2) / 2], the y power rising with j."""
    j = int(j)
    if j < 1:
        raise ValueError('j must be >= 1')
    t = 0
    while (t + 1) * (t + 2) // 2 < j:
        t += 1
    n = j - t * (t + 1) // 2 - 1
    return t - n, n


def step_dtype(dtype):
    """numpy layout of one record; the C struct pm::RStep<T> in csrc/recur.hip (16 bytes for float32, 32 with padding for float64)."""
    t = np.dtype(dtype)
    if t not in (np.dtype('float32'), np.dtype('float64')):
        raise TypeError(f'recurrence tables are float32 or float64, not {t}')
    return np.dtype({'names': ['a', 'b', 'c', 'slot'], 'formats': [t, t, t, '<i4'], 'offsets': [0, t.itemsize, 2 * t.itemsize, 3 * t.itemsize],
                     'itemsize': 4 * t.itemsize})


def check_ns(ns):
    """The orders as a tuple of ints; ValueError unless they are non-negative and strictly ascending."""
    out = []
    for n in ns:
        if int(n) != n:
            raise ValueError(f'polynomial orders must be integers, got {n!r}')
        n = int(n)
        if n < 0 or (out and n <= out[-1]):
            raise ValueError(f'polynomial orders must be non-negative and strictly ascending, got {tuple(ns)!r}')
        out.append(n)
    return tuple(out)


def _abc(family, k, params):
    """(a, b, c) of record k >= 1"""
    if family in ('cheby1', 'cheby2', 'cheby3', 'cheby4'):
        if k == 1:
            return {'cheby1': (0.0, 1.0), 'cheby2': (0.0, 2.0), 'cheby3': (-1.0, 2.0), 'cheby4': (1.0, 2.0)}[family] + (0.0,)
        return 0.0, 2.0, 1.0
    if family == 'legendre':
        return 0.0, (2 * k - 1) / k, (k - 1) / k
    if family == 'hermite_He':
        return 0.0, 1.0, k - 1.0
    if family == 'hermite_H':
        return 0.0, 2.0, 2.0 * (k - 1)
    if family == 'laguerre':
        alpha, = params
        return (alpha + 2 * k - 1) / k, -1.0 / k, (alpha + k - 1) / k
    if family in ('dickson1', 'dickson2'):
        alpha, = params
        if k == 1:          # P_1 = x for both kinds: half of x P_0 where P_0 = 2
            return 0.0, (0.5 if family == 'dickson1' else 1.0), 0.0
        return 0.0, 1.0, alpha
    if family == 'jacobi':
        alpha, beta = params
        if k == 1:
            return (alpha + 1) - (alpha + beta + 2) / 2, (alpha + beta + 2) / 2, 0.0
        A, B, C = recurrence_abc(k - 1, alpha, beta)
        return B, A, C
    return 0.0, 1.0, 0.0        # monomial: x^k = x x^(k-1)


def plan(family, ns=None, *params, nmax=None, dtype=np.float64):
    """The table of `family` as a structured array of step_dtype(dtype): records 0 .. max(ns), slot of order ns[i] = i (ns strictly
    ascending), or with nmax instead of ns every order 0 .. nmax written to its own plane.  params: alpha for 'laguerre' and the
    Dickson kinds, (alpha, beta) for 'jacobi'."""
    if family not in FAMILIES:
        raise ValueError(f'unknown family {family!r}; one of {sorted(FAMILIES)}')
    if len(params) != FAMILIES[family]:
        raise ValueError(f'{family} takes {FAMILIES[family]} shape parameter(s), got {len(params)}')
    params = tuple(float(p) for p in params)
    if (ns is None) == (nmax is None):
        raise ValueError('give either ns or nmax')
    ns = tuple(range(int(nmax) + 1)) if ns is None else check_ns(ns)
    table = np.zeros((max(ns) + 1) if ns else 0, dtype=step_dtype(dtype))
    if not ns:
        return table
    table['slot'] = -1
    for i, n in enumerate(ns):
        table['slot'][n] = i
    for k in range(len(table)):
        a, b, c = (2.0 if family == 'dickson1' else 1.0, 0.0, 0.0) if k == 0 else _abc(family, k, params)
        table[k]['a'], table[k]['b'], table[k]['c'] = a, b, (0.0 if k == 1 else c)
    return table


def evaluate(table, u):
    """Walk `table` over the points u in numpy, in the table's precision: (values, derivatives), each (nout, *u.shape) with
    nout = 1 + the largest slot.  The kernels' recurrences in the same order, one point per array element."""
    t = table['a'].dtype.type
    u = np.asarray(u, dtype=t)
    nout = int(table['slot'].max()) + 1 if len(table) else 0
    out = np.zeros((nout, *u.shape), dtype=t)
    der = np.zeros_like(out)
    p, pm, d, dm = np.ones_like(u), np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    for s in table:
        a, b, c = s['a'], s['b'], s['c']
        lin = a + b * u
        p, pm, d, dm = lin * p - c * pm, p, b * p + lin * d - c * dm, d
        if s['slot'] >= 0:
            out[int(s['slot'])], der[int(s['slot'])] = p, d
    return out, der


def check_mns(mns):
    """The (m, n) pairs as a tuple of int pairs; ValueError for a negative or fractional order."""
    out = []
    for mn in mns:
        m, n = mn
        if int(m) != m or int(n) != n or m < 0 or n < 0:
            raise ValueError(f'(m, n) orders must be non-negative integers, got {mn!r}')
        out.append((int(m), int(n)))
    return tuple(out)


def coefficient_matrix(coefs, mns, dtype=np.float64):
    """The dense matrix C[..., n, m] of the coefficients of the pairs (m, n): duplicates add into one entry, as the reference's
    _xy_coefficient_matrices does (xy.py:315-331).  coefs (K,) or (B, K)."""
    mns = check_mns(mns)
    coefs = np.asarray(coefs, dtype=dtype)
    ny, nx = max(n for _, n in mns) + 1, max(m for m, _ in mns) + 1
    C = np.zeros((*coefs.shape[:-1], ny, nx), dtype=dtype)
    for k, (m, n) in enumerate(mns):
        C[..., n, m] += coefs[..., k]
    return C


def _axes(xtable, ytable, x, y):
    t = xtable['a'].dtype.type
    (px, dx), (py, dy) = evaluate(xtable, np.asarray(x, dtype=t)), evaluate(ytable, np.asarray(y, dtype=t))
    return t, px, dx, py, dy


def separable_sum(xtable, ytable, C, x, y, inv_xnorm=1.0, inv_ynorm=1.0):
    """(z, dz/dx inv_xnorm, dz/dy inv_ynorm) on the grid y[rows] x x[cols] for the dense matrix C[ny, nx], as the factored products
    Py^T (C Px), Py^T (C Dx), Dy^T (C Px) in the tables' precision (dense tables: every order its own plane)."""
    t, px, dx, py, dy = _axes(xtable, ytable, x, y)
    C = np.asarray(C, dtype=t)
    tt, tx = C @ px, C @ dx
    return py.T @ tt, (py.T @ tx) * t(inv_xnorm), (dy.T @ tt) * t(inv_ynorm)


def separable_project(xtable, ytable, g, x, y, what='z', inv_xnorm=1.0, inv_ynorm=1.0):
    """The adjoint of one map of separable_sum with respect to C: Fy (g Fx^T), F the values or the derivatives chosen by what in
    'z', 'zx', 'zy'; (ny, nx)."""
    t, px, dx, py, dy = _axes(xtable, ytable, x, y)
    g = np.asarray(g, dtype=t)
    if what == 'z':
        return py @ g @ px.T
    if what == 'zx':
        return (py @ g @ dx.T) * t(inv_xnorm)
    if what == 'zy':
        return (dy @ g @ px.T) * t(inv_ynorm)
    raise ValueError(f"what must be 'z', 'zx' or 'zy', not {what!r}")
