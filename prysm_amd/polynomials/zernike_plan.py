"""Host side of the Zernike kernels, free of torch: index conventions, the norm, and the table the kernels walk.

The kernels (csrc/zernike.hip) evaluate Z_n^m at a point as

    norm(n, m) * P_j^(0, |m|)(2 r^2 - 1) * {1, Re z^|m|, Im z^|m|},   z = x + i y,  j = (n - |m|) // 2

(r^|m| cos(|m| t) = Re z^|m|, r^|m| sin(|m| t) = Im z^|m|, so the loop needs no trigonometry).  `plan` turns a mode list into one
table of steps, sorted by |m| and then by Jacobi order, so that a point walks it once with the Jacobi recurrence and z^|m| in
registers.  Each step:

    op & RESET  start the |m| group: z^|m| *= z `dm` times, P = 1, P_prev = 0 (Jacobi order 0)
    op & ADV    one recurrence step: P, P_prev = (a x + b) P - c P_prev, P
    part        NONE, or the output written at this step: RADIAL (m = 0), COS (m > 0) or SIN (m < 0), times `w`, into plane `slot`

A Jacobi order no mode needs is still walked (a step with part NONE); several modes at one order share it (later steps have op 0).
`evaluate` is the same walk in numpy: the model the CPU tests hold the table to.
"""
import math

import numpy as np

__all__ = ['zernike_norm', 'noll_to_nm', 'fringe_to_nm', 'nm_to_fringe', 'nm_to_ansi_j', 'ansi_j_to_nm', 'check_nms', 'plan',
           'step_dtype', 'evaluate', 'RESET', 'ADV', 'NONE', 'RADIAL', 'COS', 'SIN']

RESET, ADV = 1, 2
NONE, RADIAL, COS, SIN = 0, 1, 2, 3


def zernike_norm(n, m):
    """Norm of Z_n^m (unit RMS over the disk): sqrt(2 (n + 1) / (1 + delta_m0))."""
    return math.sqrt(2 * (n + 1) / (2 if m == 0 else 1))


def nm_to_ansi_j(n, m):
    """(n, m) to the ANSI / OSA single index j, counted from 0: j = (n (n + 2) + m) / 2."""
    return int((n * (n + 2) + m) / 2)


def ansi_j_to_nm(idx):
    """ANSI / OSA index j (from 0) to (n, m): order n holds j in [n (n + 1) / 2, (n + 1) (n + 2) / 2), m = 2 j - n (n + 2)."""
    idx = int(idx)
    n = 0
    while (n + 1) * (n + 2) // 2 <= idx:
        n += 1
    return n, 2 * idx - n * (n + 2)


def noll_to_nm(idx):
    """Noll index j (from 1) to (n, m).  Order n holds j in (n (n + 1) / 2, (n + 1) (n + 2) / 2]; inside it |m| rises in pairs from
    n mod 2 (a lone m = 0 first when n is even), and odd j take the sine (m < 0)."""
    idx = int(idx)
    n = 0
    while (n + 1) * (n + 2) // 2 < idx:
        n += 1
    pos = idx - n * (n + 1) // 2 - 1
    am = 2 * ((pos + 1) // 2) if n % 2 == 0 else 2 * (pos // 2) + 1
    return n, (-am if idx % 2 else am)


def fringe_to_nm(idx):
    """Fringe index j (from 1) to (n, m).  Group d = n / 2 + |m| / 2 holds j in [d^2 + 1, (d + 1)^2]; its s-th member (from 0) has
    n = d + s // 2, |m| = 2 d - n, cosine for even s and sine for odd s."""
    idx = int(idx)
    d = math.isqrt(idx - 1)
    s = idx - d * d - 1
    n = d + s // 2
    am = 2 * d - n
    return n, (-am if s % 2 else am)


def nm_to_fringe(n, m):
    """(n, m) to the Fringe index (from 1), the inverse of fringe_to_nm: (d + 1)^2 - 2 |m| + (1 if m < 0), d = (n + |m|) / 2."""
    d = (n + abs(m)) / 2
    return int((1 + d) ** 2 - 2 * abs(m) - (1 if m >= 0 else 0)) + 1


def check_nms(nms):
    """The mode list as a tuple of (int n, int m); ValueError for n < 0 or |m| > n."""
    out = []
    for nm in nms:
        n, m = nm
        if int(n) != n or int(m) != m:
            raise ValueError(f'Zernike indices must be integers, got {nm!r}')
        n, m = int(n), int(m)
        if n < 0 or abs(m) > n:
            raise ValueError(f'Zernike index (n={n}, m={m}) needs n >= 0 and |m| <= n')
        out.append((n, m))
    return tuple(out)


def step_dtype(dtype):
    """numpy layout of one table step; the C struct pm::ZStep<T> in csrc/zernike.hip (32 bytes for float32, 48 for float64)."""
    t = np.dtype(dtype)
    if t not in (np.dtype('float32'), np.dtype('float64')):
        raise TypeError(f'Zernike tables are float32 or float64, not {t}')
    return np.dtype([('a', t), ('b', t), ('c', t), ('w', t), ('op', '<i4'), ('part', '<i4'), ('slot', '<i4'), ('dm', '<i4')])


def _abc(j, beta):
    """Coefficients of P_j^(0, beta) = (a x + b) P_{j-1} - c P_{j-2} (DLMF 18.9.1-2 with alpha = 0); j = 1 is the explicit
    P_1 = 1 + (beta + 2) (x - 1) / 2."""
    if j == 1:
        return (beta + 2) / 2, -beta / 2, 0.0
    n = j - 1
    s = 2 * n + beta
    a = (s + 1) * (s + 2) / (2 * (n + 1) * (n + beta + 1))
    b = -(beta * beta) * (s + 1) / (2 * (n + 1) * (n + beta + 1) * s)
    c = n * (n + beta) * (s + 2) / ((n + 1) * (n + beta + 1) * s)
    return a, b, c


def plan(nms, norm=True, dtype=np.float64):
    """The step table for `nms` (validated by check_nms), as a structured numpy array of step_dtype(dtype)."""
    nms = check_nms(nms)
    groups = {}
    for k, (n, m) in enumerate(nms):
        am = abs(m)
        groups.setdefault(am, {}).setdefault((n - am) // 2, []).append(k)
    rows = []
    cur = 0
    for am in sorted(groups):
        byj = groups[am]
        for j in range(max(byj) + 1):
            if j == 0:
                op, (a, b, c), dm = RESET, (0.0, 0.0, 0.0), am - cur
                cur = am
            else:
                op, (a, b, c), dm = ADV, _abc(j, am), 0
            slots = byj.get(j, [])
            if not slots:
                rows.append((a, b, c, 0.0, op, NONE, -1, dm))
            for i, k in enumerate(slots):
                n, m = nms[k]
                part = RADIAL if m == 0 else (COS if m > 0 else SIN)
                w = zernike_norm(n, m) if norm else 1.0
                rows.append((a, b, c, w, op, part, k, dm) if i == 0 else (0.0, 0.0, 0.0, w, 0, part, k, 0))
    return np.array(rows, dtype=step_dtype(dtype))


def evaluate(table, u, v, nmodes, polar=False):
    """Walk `table` over the points (u, v) -- Cartesian (x, y), or polar (r, t) -- in numpy, in the table's precision:
    (nmodes, *u.shape).  The kernels' arithmetic in the same order, one point per array element."""
    t = table['a'].dtype.type
    u = np.asarray(u, dtype=t)
    v = np.asarray(v, dtype=t)
    if polar:
        zx, zy = u * np.cos(v), u * np.sin(v)
        X = t(2) * (u * u) - t(1)
    else:
        zx, zy = u, v
        X = t(2) * (u * u + v * v) - t(1)
    out = np.zeros((nmodes, *u.shape), dtype=t)
    pr, pi = np.ones_like(u), np.zeros_like(u)
    p, pm = np.ones_like(u), np.zeros_like(u)
    for s in table:
        if s['op'] & RESET:
            for _ in range(int(s['dm'])):
                pr, pi = pr * zx - pi * zy, pr * zy + pi * zx
            p, pm = np.ones_like(u), np.zeros_like(u)
        if s['op'] & ADV:
            p, pm = (s['a'] * X + s['b']) * p - s['c'] * pm, p
        part = int(s['part'])
        if part != NONE:
            wp = s['w'] * p
            out[int(s['slot'])] = wp if part == RADIAL else wp * (pr if part == COS else pi)
    return out
