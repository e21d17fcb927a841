"""The numpy model of csrc/modalfit.hip and the host-side checks of prysm_amd/polynomials/fitting.py.  Imports without a GPU.

Every function restates a kernel with the same predicate, the same drop rule and the same order of operations in the small algebra
(the unit is compiled with -ffp-contract=off, so each product and each sum is rounded by itself, as numpy rounds them).  Only the order
of the long sums over the points differs (the kernel adds 4 points per MFMA step, workgroup by workgroup): gram() and stats() agree
with the device to the bit on data whose sums are exact (small integers) and to a few eps otherwise.

The record (PM_MODES_REC_* in include/prysm_amd.h), in doubles:
    [COUNT | RANK | G (K x K) | L (K x K) | dropped (K) | T (K x K) | b (nrhs x K) | coef (nrhs x K)]
"""
import numpy as np

FIT_MAX = 128
REC_COUNT, REC_RANK, REC_G = 0, 1, 2
STAT_N, STAT_SUM, STAT_MIN, STAT_MAX, STAT_MEAN, STAT_M2, STAT_STD, STAT_RECORD = range(8)
EPS64 = float(np.finfo(np.float64).eps)
TILE = 1024            # points per workgroup of the Gram pass; pm_modes_gram_workspace grows by one workgroup per tile up to the cap


# ---------------------------------------------------------------- record layout
def record_doubles(K, nrhs):
    return REC_G + 3 * K * K + K + 2 * nrhs * K


def offsets(K, nrhs=0):
    """name -> (offset, shape) of the record's pieces"""
    g = REC_G
    return {'G': (g, (K, K)), 'L': (g + K * K, (K, K)), 'drop': (g + 2 * K * K, (K,)), 'T': (g + 2 * K * K + K, (K, K)),
            'b': (g + 3 * K * K + K, (nrhs, K)), 'coef': (g + 3 * K * K + K + nrhs * K, (nrhs, K))}


def piece(rec, name, K, nrhs=0):
    off, shape = offsets(K, nrhs)[name]
    return np.asarray(rec)[off:off + int(np.prod(shape))].reshape(shape)


# ---------------------------------------------------------------- host-side checks
def check_to(to):
    if to not in ('std', 'ptp'):
        raise ValueError(f"normalize_modes: to must be 'std' or 'ptp', not {to!r}")
    return to


def check_count(K):
    if K < 1:
        raise ValueError('at least one mode is needed')
    if K > FIT_MAX:
        raise NotImplementedError(f'{K} modes are more than the {FIT_MAX} a fit takes (PM_MODES_FIT_MAX)')


def check_shapes(mshape, dshape, what='data'):
    """modes (K, rows, cols) against data (rows, cols) or a (B, rows, cols) stack; returns B, or None for a single map"""
    if len(mshape) != 3:
        raise ValueError(f'modes must be a (K, rows, cols) stack, not of shape {tuple(mshape)}')
    if tuple(dshape) == tuple(mshape[1:]):
        return None
    if len(dshape) == 3 and tuple(dshape[1:]) == tuple(mshape[1:]):
        return dshape[0]
    raise ValueError(f'{what} of shape {tuple(dshape)} does not match modes of shape {tuple(mshape)}')


def check_mask(mshape, kshape):
    if tuple(kshape) != tuple(mshape[-2:]):
        raise ValueError(f'mask of shape {tuple(kshape)} does not match modes of shape {tuple(mshape)}')


# ---------------------------------------------------------------- the kernels
def valid(npts, mask=None, data0=None):
    """the predicate: (mask is None or mask != 0) and (data0 is None or isfinite(data0))"""
    ok = np.ones(npts, dtype=bool)
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1) != 0
    if data0 is not None:
        ok &= np.isfinite(np.asarray(data0).reshape(-1))
    return ok


def gram(modes, data=None, mask=None, finite_from_data=False):
    """(count, G, b) in double over the valid points: a select, so nothing at an invalid point is read into a sum"""
    m = np.asarray(modes)
    K = m.shape[0]
    m = m.reshape(K, -1)
    d = None if data is None else np.asarray(data).reshape(-1, m.shape[1])
    ok = valid(m.shape[1], mask, d[0] if finite_from_data else None)
    mv = m[:, ok].astype(np.float64)
    G = mv @ mv.T
    b = np.zeros((0, K)) if d is None else d[:, ok].astype(np.float64) @ mv.T
    return float(ok.sum()), G, b


def factor(G):
    """(L, dropped, rank): the unpivoted Cholesky in mode order; a pivot not above K eps (largest pivot so far) drops its mode"""
    G = np.asarray(G, dtype=np.float64)
    K = G.shape[0]
    L = np.zeros((K, K))
    drop = np.zeros(K)
    largest, rank = 0.0, 0
    for j in range(K):
        d = G[j, j]
        for t in range(j):
            d = d - L[j, t] * L[j, t]
        if d > 0.0 and d > K * EPS64 * largest:
            ljj = np.sqrt(d)
            largest = max(largest, d)
            rank += 1
            s = G[j + 1:, j].copy()
            for t in range(j):
                s = s - L[j + 1:, t] * L[j, t]
            L[j + 1:, j] = s / ljj
            L[j, j] = ljj
        else:
            L[:, j] = 0.0
            L[j, :] = 0.0
            drop[j] = 1.0
    return L, drop, rank


def solve(L, drop, b):
    """coef (nrhs, K) = G^-1 b by the two substitutions, column by column as the kernel does; dropped modes 0"""
    x = np.array(b, dtype=np.float64, copy=True).reshape(-1, L.shape[0])
    K = L.shape[0]
    for j in range(K):
        if drop[j]:
            continue
        x[:, j] = x[:, j] / L[j, j]
        x[:, j + 1:] = x[:, j + 1:] - L[j + 1:, j][None, :] * x[:, j][:, None]
    for j in range(K - 1, -1, -1):
        if drop[j]:
            x[:, j] = 0.0
            continue
        x[:, j] = x[:, j] / L[j, j]
        x[:, :j] = x[:, :j] - L[j, :j][None, :] * x[:, j][:, None]
    return x


def invert(L, drop):
    """T = L^-1, lower triangular, by forward substitution per column; dropped rows and columns 0"""
    K = L.shape[0]
    T = np.zeros((K, K))
    for c in range(K):
        if drop[c]:
            continue
        for i in range(c, K):
            if drop[i]:
                continue
            s = 1.0 if i == c else 0.0
            for t in range(c, i):
                s = s - L[i, t] * T[t, c]
            T[i, c] = s / L[i, i]
    return T


def stats(modes, mask=None):
    """(K, STAT_RECORD): count, sum, min, max, mean, sum (m - mean)^2, population std of each mode over the mask"""
    m = np.asarray(modes)
    K = m.shape[0]
    m = m.reshape(K, -1)
    ok = valid(m.shape[1], mask)
    mv = m[:, ok].astype(np.float64)
    out = np.full((K, STAT_RECORD), np.nan)
    out[:, STAT_N] = mv.shape[1]
    out[:, STAT_SUM] = mv.sum(axis=1)
    if mv.shape[1]:
        out[:, STAT_MIN], out[:, STAT_MAX] = mv.min(axis=1), mv.max(axis=1)
        out[:, STAT_MEAN] = out[:, STAT_SUM] / out[:, STAT_N]
        out[:, STAT_M2] = ((mv - out[:, STAT_MEAN][:, None]) ** 2).sum(axis=1)
        out[:, STAT_STD] = np.sqrt(out[:, STAT_M2] / out[:, STAT_N])
    return out


def norms(st, to):
    """T = diag(1 / norm) with the reference's loophole norm < 1e-9 -> 1"""
    st = np.asarray(st).reshape(-1, STAT_RECORD)
    norm = st[:, STAT_STD].copy() if to == 'std' else st[:, STAT_MAX] - st[:, STAT_MIN]
    norm[norm < 1e-9] = 1.0
    return np.diag(1.0 / norm)


def transform(T, modes, mask=None, diagonal=False, zero_outside=False):
    """out[k] = sum_{j <= k} T[k][j] modes[j] (or T[k][k] modes[k]) in double, j ascending from 0.0, rounded once to the modes' dtype"""
    m = np.asarray(modes)
    K = m.shape[0]
    md = m.reshape(K, -1).astype(np.float64)
    out = np.zeros_like(md)
    for k in range(K):
        if diagonal:
            out[k] = T[k, k] * md[k]
        else:
            s = np.zeros(md.shape[1])
            for j in range(k + 1):
                s = s + T[k, j] * md[j]
            out[k] = s
    if zero_outside:
        out[:, ~valid(md.shape[1], mask)] = 0.0
    return out.astype(m.dtype).reshape(m.shape)


# ---------------------------------------------------------------- the public functions, as compositions of the kernels
def lstsq(modes, data):
    m = np.asarray(modes)
    _, G, b = gram(m, np.asarray(data)[None], None, True)
    L, drop, _ = factor(G)
    return solve(L, drop, b)[0].astype(m.dtype)


def normalize_modes(modes, mask, to='std'):
    m = np.asarray(modes)
    stack = m if m.ndim == 3 else m[None]
    out = transform(norms(stats(stack, mask), check_to(to)), stack, diagonal=True)
    return out if m.ndim == 3 else out[0]


def orthogonalize_modes(modes, mask):
    m = np.asarray(modes)
    _, G, _ = gram(m, None, mask)
    L, drop, _ = factor(G)
    return transform(invert(L, drop), m, mask, zero_outside=True)


def hopkins(a, b, c, r, t, H):
    c1 = np.sin(abs(a) * t) if a < 0 else np.cos(a * t)
    return c1 * r ** b * H ** c


def rmax_square_array(shape):
    """the index _rmax_square_array reads: (rows - 1, cols // 2)"""
    return shape[0] - 1, shape[1] // 2
