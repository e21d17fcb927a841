"""Host side of the Forbes Q-polynomial kernels, free of torch: the recurrence coefficients, the mode checks, and the table the
kernels walk.

Every family is a three-term recurrence in x = u^2 for an auxiliary polynomial P, an orthogonalising step from P to Q, and a prefix:

    Qbfs   (Forbes, Opt. Express 18(19) 19700, 2010, App. A)   P_n = (2 - 4 x) P_{n-1} - P_{n-2},  P_0 = 2, P_1 = 6 - 8 x
           Q_n = (P_n - g_{n-1} Q_{n-1} - h_{n-2} Q_{n-2}) / f_n,  prefix x (1 - x)
    Qcon   (Forbes, Opt. Express 18(13) 13851, 2010)          P_n = Jacobi P_n^(0, 4)(2 x - 1),  Q_n = P_n,  prefix x^2
    Q2D    (Forbes, Opt. Express 20(3) 2483, 2012, App. A)    P_n = (A + B x) P_{n-1} - C P_{n-2},  Q_n = (P_n - g_{n-1} Q_{n-1}) / f_n
           prefix Re z^|m| (m > 0) or Im z^|m| (m < 0), z = u e^{i t}; m = 0 is Qbfs

With Q_0 = P_0 / f_0 (Qbfs: f_0 = 2, so Q_0 = 1) and Q_1 = (P_1 - g_0 Q_0) / f_1 (Qbfs: g_0 = -1/2, f_1 = sqrt(19) / 2, so
Q_1 = (13 - 16 x) / sqrt(19)), the seeds of Q come out of the same Q step.  The P seeds do not: a SEED step sets P to a cubic in x.
For |m| = 1 the three-term step starts at n = 4, so P_0 .. P_3 are all seeds (App. A of the Q2D paper).

`plan` turns a mode list into one table of steps, grouped by |m| (a Qcon table has one group), one step per order n in a group:

    op & RESET  start the group: z^|m| *= z `dm` times, P = Q = 0
    op & SEED   P_{n-1} = P;  P = a + b x + c x^2 + d x^3
    op & ADV    P_{n-1}, P = P, (a + b x) P - c P_{n-1}
    either      Q_{n-2}, Q_{n-1} = Q_{n-1}, (P - g Q_{n-1} - h Q_{n-2}) * rf      (rf = 1 / f)
    part        NONE, or the output written at this step: w Q_n times BFS x (1 - x), CON x^2, COS Re z^|m| or SIN Im z^|m|, into
                plane `slot`

An order no mode needs is still walked (part NONE); several outputs at one order share it (later steps have op 0).  `evaluate` is the
same walk in numpy: the model the CPU tests hold the table to.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from .zernike_plan import _abc as _jacobi_abc

__all__ = ['g_qbfs', 'h_qbfs', 'f_qbfs', 'abc_q2d', 'G_q2d', 'F_q2d', 'g_q2d', 'f_q2d', 'Q2d_nm_c_to_a_b', 'check_ns', 'check_q2d_nms',
           'plan', 'step_dtype', 'evaluate', 'QBFS', 'QCON', 'Q2D', 'RESET', 'SEED', 'ADV', 'NONE', 'BFS', 'CON', 'COS', 'SIN',
           'CARTESIAN', 'POLAR', 'RADIAL']

QBFS, QCON, Q2D = 'qbfs', 'qcon', 'q2d'
RESET, SEED, ADV = 1, 2, 4
NONE, BFS, CON, COS, SIN = 0, 1, 2, 3, 4
CARTESIAN, POLAR, RADIAL = 0, 1, 2          # PM_ZERNIKE_CARTESIAN, PM_ZERNIKE_POLAR, PM_QPOLY_RADIAL


# ---------------------------------------------------------------- Qbfs: f, g, h of eqs. A.14-A.16 (Opt. Express 18(19) 19700)
@functools.lru_cache(None)
def _bfs_fgh(n):
    """(f_n, g_n, h_n): f_0 = 2, g_0 = -1/2; f_n = sqrt(n (n + 1) + 3 - g_{n-1}^2 - h_{n-2}^2), g_n = -(1 + g_{n-1} h_{n-1}) / f_n,
    h_n = -(n + 1) (n + 2) / (2 f_n).  Built upwards so that deep orders recurse no further than one level per call."""
    if n == 0:
        f, g = 2.0, -0.5
    else:
        f1, g1, h1 = _bfs_fgh(n - 1)
        h2 = _bfs_fgh(n - 2)[2] if n >= 2 else 0.0
        f = math.sqrt(n * (n + 1) + 3 - g1 * g1 - h2 * h2)
        g = -(1 + g1 * h1) / f
    return f, g, -(n + 1) * (n + 2) / (2 * f)


def f_qbfs(n):
    """f_n of the Qbfs recurrence (eq. A.16)."""
    return _bfs_fgh(int(n))[0]


def g_qbfs(n_minus_1):
    """g_{n-1} of the Qbfs recurrence (eq. A.15), indexed by n - 1 as in the reference."""
    return _bfs_fgh(int(n_minus_1))[1]


def h_qbfs(n_minus_2):
    """h_{n-2} of the Qbfs recurrence (eq. A.14), indexed by n - 2 as in the reference."""
    return _bfs_fgh(int(n_minus_2))[2]


# ---------------------------------------------------------------- Q2D: eqs. A.3, A.13-A.18 (Opt. Express 20(3) 2483), exact rationals
def _dfact(k):
    """k!! for k >= -1 (1 for k <= 0)"""
    return math.prod(range(k, 0, -2)) if k > 0 else 1


@functools.lru_cache(None)
def _gamma_q2d(n, m):
    """Gamma_n^m of eq. A.14 (n >= 1, m >= 2): Gamma_1^2 = 3/8, Gamma_1^m = (2m - 1) / (2 (m - 2)) Gamma_1^{m-1},
    Gamma_n^m = n (2m + 2n - 3) / ((m + n - 3) (2n - 1)) Gamma_{n-1}^m."""
    v = Fraction(3, 8)
    for k in range(3, m + 1):
        v *= Fraction(2 * k - 1, 2 * (k - 2))
    for k in range(2, n + 1):
        v *= Fraction(k * (2 * m + 2 * k - 3), (m + k - 3) * (2 * k - 1))
    return v


@functools.lru_cache(None)
def _F_exact(n, m):
    if n == 0:
        return Fraction(1, 4) if m == 1 else Fraction(m * m * _dfact(2 * m - 3), 2 ** (m + 1) * math.factorial(m - 1))
    if m == 1:
        return Fraction(4 * (n - 1) ** 2 * n * n + 1, 8 * (2 * n - 1) ** 2) + (Fraction(11, 32) if n == 1 else 0)
    chi = m + n - 2
    num = 2 * n * chi * (3 - 5 * m + 4 * n * chi) + m * m * (3 - m + 4 * n * chi)
    den = (m + 2 * n - 3) * (m + 2 * n - 2) * (m + 2 * n - 1) * (2 * n - 1)
    return Fraction(num, den) * _gamma_q2d(n, m)


@functools.lru_cache(None)
def _G_exact(n, m):
    if n == 0:
        return Fraction(_dfact(2 * m - 1), 2 ** (m + 1) * math.factorial(m - 1))
    if m == 1:
        return -Fraction((2 * n * n - 1) * (n * n - 1), 8 * (4 * n * n - 1)) - (Fraction(1, 24) if n == 1 else 0)
    num = (2 * n * (m + n - 1) - m) * (n + 1) * (2 * m + 2 * n - 1)
    den = (m + 2 * n - 2) * (m + 2 * n - 1) * (m + 2 * n) * (2 * n + 1)
    return -Fraction(num, den) * _gamma_q2d(n, m)


def abc_q2d(n, m):
    """A, B, C of the Q2D auxiliary recurrence (eq. A.3); P_{n+1} = (A + B x) P_n - C P_{n-1} uses abc_q2d(n, m).  Undefined (a
    division by zero) where (4n^2 - 1)(m + n - 2)(m + 2n - 3) vanishes, e.g. (1, 1): |m| = 1 is seeded up to P_3 instead."""
    D = (4 * n * n - 1) * (m + n - 2) * (m + 2 * n - 3)
    A = (2 * n - 1) * (m + 2 * n - 2) * (4 * n * (m + n - 2) + (m - 3) * (2 * m - 1)) / D
    B = -2 * (2 * n - 1) * (m + 2 * n - 3) * (m + 2 * n - 2) * (m + 2 * n - 1) / D
    C = n * (2 * n - 3) * (m + 2 * n - 1) * (2 * m + 2 * n - 3) / D
    return A, B, C


def F_q2d(n, m):
    """F_n^m of the Q2D orthogonalisation (eq. A.13), m >= 1."""
    return float(_F_exact(int(n), int(m)))


def G_q2d(n, m):
    """G_n^m of the Q2D orthogonalisation (eq. A.15), m >= 1."""
    return float(_G_exact(int(n), int(m)))


@functools.lru_cache(None)
def f_q2d(n, m):
    """f_n^m (eq. A.18b): sqrt(F_0^m) for n = 0, sqrt(F_n^m - g_{n-1}^m ^2) otherwise."""
    if n == 0:
        return math.sqrt(F_q2d(0, m))
    g = g_q2d(n - 1, m)
    return math.sqrt(F_q2d(n, m) - g * g)


def g_q2d(n, m):
    """g_n^m = G_n^m / f_n^m (eq. A.18a)."""
    return G_q2d(n, m) / f_q2d(n, m)


def Q2d_nm_c_to_a_b(nms, coefs):
    """Q2D (n, m) / coefficient pairs to the dense form compute_z_Q2d takes: (cm0, ams, bms).  cm0 holds the m = 0 (Qbfs)
    coefficients by n, ams[|m| - 1] the cosine (m > 0) and bms[|m| - 1] the sine (m < 0) ones, for |m| = 1 .. the largest present
    (an empty list where an order has none).  Zero coefficients are dropped, so no list ends in a zero; a repeated (n, m) keeps its
    last coefficient.  (qpoly.py:1926)"""
    cm0, cos, sin = {}, {}, {}
    for (n, m), c in zip(nms, coefs):
        if c == 0:
            continue
        if m == 0:
            cm0[n] = c
        else:
            (cos if m > 0 else sin).setdefault(abs(m), {})[n] = c

    def dense(d):
        out = [0] * (max(d) + 1 if d else 0)
        for n, c in d.items():
            out[n] = c
        return out

    top = max([*cos, *sin], default=0)
    return dense(cm0), [dense(cos.get(m, {})) for m in range(1, top + 1)], [dense(sin.get(m, {})) for m in range(1, top + 1)]


# ---------------------------------------------------------------- modes
def _int(v, what):
    if isinstance(v, (bool, np.bool_)) or int(v) != v:
        raise ValueError(f'{what} must be an integer, got {v!r}')
    return int(v)


def check_ns(ns):
    """The orders of a Qbfs / Qcon call as a tuple of ints; ValueError for a non-integer or a negative order."""
    out = tuple(_int(n, 'Q polynomial order') for n in ns)
    for n in out:
        if n < 0:
            raise ValueError(f'Q polynomial order n={n} must be >= 0')
    return out


def check_q2d_nms(nms):
    """The (n, m) of a Q2D call as a tuple of int pairs; ValueError for non-integers or n < 0.  Any m: 0 is Qbfs, m < 0 the sine."""
    out = []
    for nm in nms:
        n, m = nm
        n, m = _int(n, 'Q2D order n'), _int(m, 'Q2D order m')
        if n < 0:
            raise ValueError(f'Q2D index (n={n}, m={m}) needs n >= 0')
        out.append((n, m))
    return tuple(out)


# ---------------------------------------------------------------- the table
def step_dtype(dtype):
    """numpy layout of one table step; the C struct pm::QStep<T> in csrc/qpoly.hip (48 bytes for float32, 80 for float64)."""
    t = np.dtype(dtype)
    if t not in (np.dtype('float32'), np.dtype('float64')):
        raise TypeError(f'Q polynomial tables are float32 or float64, not {t}')
    return np.dtype([('a', t), ('b', t), ('c', t), ('d', t), ('g', t), ('h', t), ('rf', t), ('w', t),
                     ('op', '<i4'), ('part', '<i4'), ('slot', '<i4'), ('dm', '<i4')])


def _bfs_step(n):
    """(op, a, b, c, d, g, h, rf) of order n of the Qbfs group"""
    f = f_qbfs(n)
    if n == 0:
        return SEED, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1 / f
    if n == 1:
        return SEED, 6.0, -8.0, 0.0, 0.0, g_qbfs(0), 0.0, 1 / f
    return ADV, 2.0, -4.0, 1.0, 0.0, g_qbfs(n - 1), h_qbfs(n - 2), 1 / f


def _con_step(n):
    """order n of the Qcon group: Jacobi P^(0, 4) in 2 x - 1, written in x"""
    if n == 0:
        return SEED, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0
    a, b, c = _jacobi_abc(n, 4)           # P_n = (a X + b) P_{n-1} - c P_{n-2},  X = 2 x - 1
    return (SEED if n == 1 else ADV), b - a, 2 * a, c, 0.0, 0.0, 0.0, 1.0


_SEEDS_M1 = {2: (0.5, -2.0, 4 / 3, 0.0), 3: (0.5, -6.0, 12.0, -6.4)}     # P_2 = (3 - 12x + 8x^2) / 6, P_3 = (5 - 60x + 120x^2 - 64x^3) / 10


def _q2d_step(n, m):
    """order n of the Q2D group |m| = m >= 1"""
    g, rf = (g_q2d(n - 1, m) if n else 0.0), 1 / f_q2d(n, m)
    if n == 0:
        return SEED, 0.5, 0.0, 0.0, 0.0, g, 0.0, rf
    if n == 1:
        a, b = (1.0, -0.5) if m == 1 else (m - 0.5, 1.0 - m)
        return SEED, a, b, 0.0, 0.0, g, 0.0, rf
    if m == 1 and n <= 3:
        return (SEED, *_SEEDS_M1[n], g, 0.0, rf)
    A, B, C = abc_q2d(n - 1, m)
    return ADV, A, B, C, 0.0, g, 0.0, rf


def plan(modes, family, dtype=np.float64):
    """The step table of `modes` -- orders n for QBFS / QCON (check_ns), (n, m) pairs for Q2D (check_q2d_nms) -- as a structured
    numpy array of step_dtype(dtype)."""
    if family == Q2D:
        nms = check_q2d_nms(modes)
    elif family in (QBFS, QCON):
        nms = tuple((n, 0) for n in check_ns(modes))
    else:
        raise ValueError(f'family must be {QBFS!r}, {QCON!r} or {Q2D!r}, not {family!r}')
    groups = {}
    for k, (n, m) in enumerate(nms):
        groups.setdefault(abs(m), {}).setdefault(n, []).append(k)
    rows = []
    cur = 0
    for am in sorted(groups):
        byn = groups[am]
        for n in range(max(byn) + 1):
            if family == QCON:
                op, *coef = _con_step(n)
            elif am == 0:
                op, *coef = _bfs_step(n)
            else:
                op, *coef = _q2d_step(n, am)
            dm = 0
            if n == 0:
                op, dm, cur = op | RESET, am - cur, am
            slots = byn.get(n, [])
            if not slots:
                rows.append((*coef, 0.0, op, NONE, -1, dm))
            for i, k in enumerate(slots):
                m = nms[k][1]
                part = (CON if family == QCON else BFS) if m == 0 else (COS if m > 0 else SIN)
                rows.append((*coef, 1.0, op, part, k, dm) if i == 0 else (0.0,) * 7 + (1.0, 0, part, k, 0))
    return np.array(rows, dtype=step_dtype(dtype))


def evaluate(table, u, v, nmodes, coords=CARTESIAN):
    """Walk `table` over the points in numpy, in the table's precision: (nmodes, *u.shape).  coords CARTESIAN reads (u, v) as (x, y),
    POLAR as (r, t), RADIAL reads u only (v may be None) as the radius at angle 0.  The kernels' arithmetic in the same order, one
    point per array element."""
    t = table['a'].dtype.type
    u = np.asarray(u, dtype=t)
    if coords == POLAR:
        v = np.asarray(v, dtype=t)
        zx, zy = u * np.cos(v), u * np.sin(v)
        X = u * u
    elif coords == CARTESIAN:
        v = np.asarray(v, dtype=t)
        zx, zy = u, v
        X = u * u + v * v
    else:
        zx, zy = u, np.zeros_like(u)
        X = u * u
    out = np.zeros((nmodes, *u.shape), dtype=t)
    pr, pi = np.ones_like(u), np.zeros_like(u)
    p, pm, q1, q2 = (np.zeros_like(u) for _ in range(4))
    for s in table:
        op = int(s['op'])
        if op & RESET:
            for _ in range(int(s['dm'])):
                pr, pi = pr * zx - pi * zy, pr * zy + pi * zx
            p, pm, q1, q2 = (np.zeros_like(u) for _ in range(4))
        if op & SEED:
            p, pm = s['a'] + X * (s['b'] + X * (s['c'] + X * s['d'])), p
        elif op & ADV:
            p, pm = (s['a'] + s['b'] * X) * p - s['c'] * pm, p
        if op & (SEED | ADV):
            q1, q2 = (p - s['g'] * q1 - s['h'] * q2) * s['rf'], q1
        part, k = int(s['part']), int(s['slot'])
        if part != NONE and 0 <= k < nmodes:
            wq = s['w'] * q1
            pre = {BFS: X * (t(1) - X), CON: X * X, COS: pr, SIN: pi}[part]
            out[k] = wq * pre
    return out
