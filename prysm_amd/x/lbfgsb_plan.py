"""L-BFGS-B in numpy: the model of csrc/lbfgsb.hip and the one implementation of everything that is not a pass over the variables.

No torch and no device here.  Three layers:

- the strong-Wolfe search of the reference (_prysm_lbfgsb.py:31-203) as plain Python scalar logic: `strong_wolfe`, `_zoom`, `quadmin`,
  `cubicmin`.  It touches the problem only through phi(alpha) -> (phi, phi'), so the numpy model and the device class run THIS search.
- `History` and the small algebra, everything of size 2k x 2k, in double (on the device this is pm_lbfgsb_small, one single-workgroup
  launch per use, with the Gram matrices resident there; History is its model and the tests hold the two against each other): the Gram matrices S S^T, S Y^T, Y Y^T in LOGICAL order
  (oldest pair first), updated incrementally from the 4k + 3 products the update pass leaves (the reference's S @ Y.T and S @ S.T over
  all of n, _WM lines 394-395, do not come back); M and N = -M + W^T W / theta of the compact form B = theta I - W M^-1 W^T,
  W = [Y, theta S]; the chunked sweep over the positive breakpoints (lines 611-741); the curvature test.
- `Stepper.step`: one iteration (lines 1009-1108) written ONCE against a set of passes.  `NumpyPasses` below does the passes in numpy
  with the arithmetic of the kernels (element arithmetic in the data's type, sums and combinations in double); the device class
  (prysm_amd/x/optym/lbfgsb.py) does them with the kernels.

What differs from the reference's formulation, the same in both sets of passes:
- variables with t_i = 0 (on a bound, the gradient pushing outward) are taken out of the path at once: d0 = -g where t_i > 0 and 0
  elsewhere, df = -d0.d0, p = W^T d0.  The reference walks them through the sorted sweep with segments of zero length, which move
  neither c nor the break test.  They still count in cauchy_breaks and leave the free set.
- the unbounded direction is the compact form through N (_Hg, lines 424-437), not the two-loop recursion.
- the history ring has memory + 1 physical rows: the new pair is formed in the update pass and stored into the one row that is not
  live, so a pair refused by the curvature test overwrites nothing.
- under bounds every trial point of the search is clipped into the box, not only the accepted one (the reference's _wolfe_eval,
  line 25, evaluates the unclipped x + alpha p and clips x_new afterwards, lines 1088-1093): inside [0, alpha_max] the two differ by
  roundoff, and here g_new belongs to the very point that becomes x.
- an unbounded step reads W^T g and g.g first (also with an empty history) and stops with 'no descent direction' on g.g = 0
  before it evaluates a trial point; g.p and the count of p != 0 then travel with the first evaluation's record.
- theta, s.y and y.y come from double sums; theta is rounded to the data's type as the reference stores it.
"""
import math

import numpy as np

MAX_MEMORY = 32      # PM_LBFGSB_MAX_MEMORY
TILE = 8             # PM_LBFGSB_TILE
FIRST_CHUNK = 64     # the sweep's first chunk of positive breakpoints; it grows by 8x (lines 289-292, 733)


class OptimizerStop:
    """StopIteration payload consumed by run_until."""
    __slots__ = ('success', 'message')

    def __init__(self, success, message):
        self.success = bool(success)
        self.message = message


# ---------------------------------------------------------------------------------------------------------------- line search

def quadmin(a, fa, fpa, b, fb):
    """_wolfe_quadmin, lines 31-41"""
    try:
        db = b - a
        B = (fb - fa - fpa * db) / (db * db)
        xmin = a - fpa / (2.0 * B)
    except ArithmeticError:
        return None
    if not math.isfinite(xmin):
        return None
    return xmin


def cubicmin(a, fa, fpa, b, fb, c, fc):
    """_wolfe_cubicmin, lines 44-60"""
    try:
        db = b - a
        dc = c - a
        denom = (db * dc) ** 2 * (db - dc)
        rhs0 = fb - fa - fpa * db
        rhs1 = fc - fa - fpa * dc
        A = (dc * dc * rhs0 - db * db * rhs1) / denom
        B = (-dc ** 3 * rhs0 + db ** 3 * rhs1) / denom
        radical = B * B - 3.0 * A * fpa
        xmin = a + (-B + math.sqrt(radical)) / (3.0 * A)
    except (ArithmeticError, ValueError):
        return None
    if not math.isfinite(xmin):
        return None
    return xmin


def _zoom(phi, a_lo, a_hi, phi_lo, phi_hi, derphi_lo, phi0, derphi0, c1, c2, branches):
    """_strong_wolfe_zoom, lines 63-125"""
    maxiter = 10
    delta1 = 0.2
    delta2 = 0.1
    phi_rec = phi0
    a_rec = 0.0
    for i in range(maxiter + 1):
        dalpha = a_hi - a_lo
        if dalpha < 0:
            a, b = a_hi, a_lo
        else:
            a, b = a_lo, a_hi
        a_j = None
        kind = 'cubic'
        if i > 0:
            cchk = delta1 * dalpha
            a_j = cubicmin(a_lo, phi_lo, derphi_lo, a_hi, phi_hi, a_rec, phi_rec)
            if a_j is not None and (a_j > b - cchk or a_j < a + cchk):
                a_j = None
        if a_j is None:
            kind = 'quadratic'
            qchk = delta2 * dalpha
            a_j = quadmin(a_lo, phi_lo, derphi_lo, a_hi, phi_hi)
            if a_j is None or a_j > b - qchk or a_j < a + qchk:
                kind = 'bisection'
                a_j = a_lo + 0.5 * dalpha
        branches.append(kind)
        phi_aj, derphi_aj = phi(a_j)
        if (phi_aj > phi0 + c1 * a_j * derphi0) or (phi_aj >= phi_lo):
            phi_rec = phi_hi
            a_rec = a_hi
            a_hi = a_j
            phi_hi = phi_aj
            continue
        if abs(derphi_aj) <= -c2 * derphi0:
            branches.append('accepted in zoom')
            return a_j, phi_aj, derphi_aj
        if derphi_aj * (a_hi - a_lo) >= 0:
            phi_rec = phi_hi
            a_rec = a_hi
            a_hi = a_lo
            phi_hi = phi_lo
        else:
            phi_rec = phi_lo
            a_rec = a_lo
        a_lo = a_j
        phi_lo = phi_aj
        derphi_lo = derphi_aj
    branches.append('zoom exhausted')
    return None, None, None


def strong_wolfe(phi, phi0, derphi0, maxalpha=None, c1=1e-4, c2=0.9, maxiter=10, branches=None):
    """_strong_wolfe_lean, lines 128-203.  phi(alpha) -> (phi, phi') as Python floats; the accepted alpha is always the LAST one phi was
    called with, so the caller owns the gradient that goes with it.  Returns (alpha, phi, phi') or (None, None, None).  `branches`, a
    list, receives the branch taken at every turn (the tests compare it with the reference's)."""
    if branches is None:
        branches = []
    phi0 = float(phi0)
    derphi0 = float(derphi0)
    alpha0 = 0.0
    alpha1 = 1.0
    if maxalpha is not None:
        alpha1 = min(alpha1, maxalpha)
    phi_a0 = phi0
    derphi_a0 = derphi0
    phi_a1, derphi_a1 = phi(alpha1)
    for i in range(maxiter):
        if alpha1 == 0:
            branches.append('alpha1 == 0')
            break
        if (phi_a1 > phi0 + c1 * alpha1 * derphi0) or (i > 0 and phi_a1 >= phi_a0):
            branches.append('bracket by increase')
            return _zoom(phi, alpha0, alpha1, phi_a0, phi_a1, derphi_a0, phi0, derphi0, c1, c2, branches)
        if abs(derphi_a1) <= -c2 * derphi0:
            branches.append('accepted')
            return alpha1, phi_a1, derphi_a1
        if derphi_a1 >= 0:
            branches.append('bracket by slope')
            return _zoom(phi, alpha1, alpha0, phi_a1, phi_a0, derphi_a1, phi0, derphi0, c1, c2, branches)
        alpha2 = 2.0 * alpha1
        if maxalpha is not None:
            alpha2 = min(alpha2, maxalpha)
            if alpha2 == alpha1:
                # pinned at maxalpha: sufficient decrease holds and the slope is still descent; accept the cap (lines 188-195)
                branches.append('pinned')
                return alpha1, phi_a1, derphi_a1
        branches.append('doubling')
        alpha0 = alpha1
        alpha1 = alpha2
        phi_a0 = phi_a1
        derphi_a0 = derphi_a1
        phi_a1, derphi_a1 = phi(alpha1)
    branches.append('bracket exhausted')
    return None, None, None


# ---------------------------------------------------------------------------------------------------------------- records

def tiles_of(k):
    return max(1, (2 * k + TILE - 1) // TILE)


def unpack_dots(raw, k, nv, nx):
    """The record of a dots pass (tiles x (8 nv + nx) doubles) -> (products, shape (2k, nv), row q of W's order; the nx extra sums)"""
    ns = TILE * nv + nx
    raw = np.asarray(raw, dtype=np.float64)[:tiles_of(k) * ns].reshape(-1, ns)
    prod = raw[:, :TILE * nv].reshape(-1, nv)[:2 * k]
    return prod, raw[0, TILE * nv:]


def unpack_gram(raw, k):
    """The record of the Gram pass (64 doubles per tile pair ti <= tj) -> the symmetric (2k, 2k) matrix of raw row products"""
    nt = (2 * k + TILE - 1) // TILE
    raw = np.asarray(raw, dtype=np.float64)
    G = np.zeros((nt * TILE, nt * TILE))
    pair = 0
    for ti in range(nt):
        for tj in range(ti, nt):
            blk = raw[pair * 64:(pair + 1) * 64].reshape(TILE, TILE)
            G[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = blk
            if tj != ti:
                G[tj * TILE:(tj + 1) * TILE, ti * TILE:(ti + 1) * TILE] = blk.T
            pair += 1
    return G[:2 * k, :2 * k]


def gram_record_doubles(k):
    nt = (2 * k + TILE - 1) // TILE
    return 64 * nt * (nt + 1) // 2


# ---------------------------------------------------------------------------------------------------------------- small algebra

def _solve(A, b):
    """np.linalg.solve; a matrix LAPACK calls singular (a NaN gradient is data, not an error) gives NaN, which the search then refuses"""
    try:
        return np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return np.full(np.shape(b), np.nan)


class History:
    """The ring's bookkeeping and the three Gram matrices, in logical order, in double."""

    def __init__(self, memory, dtype):
        if memory < 1:
            raise ValueError('memory must be at least 1')
        if memory > MAX_MEMORY:
            raise NotImplementedError(f'memory {memory} is above the cap of {MAX_MEMORY} pairs (PM_LBFGSB_MAX_MEMORY)')
        self.m = int(memory)
        self.ring = self.m + 1
        self.dtype = np.dtype(dtype)
        self.eps = float(np.finfo(self.dtype).eps)
        self.clear()

    def clear(self):
        m = self.m
        self.k = 0
        self.start = 0
        self.SS = np.zeros((m, m))
        self.SY = np.zeros((m, m))      # [i, j] = s_i . y_j
        self.YY = np.zeros((m, m))
        self.theta = 1.0

    @property
    def slot(self):
        """the physical row that is not live: where the update pass stores the new pair"""
        return (self.start + self.k) % self.ring

    def rows(self):
        """physical rows of the live pairs, oldest first"""
        return [(self.start + j) % self.ring for j in range(self.k)]

    def curvature_ok(self, sy, yy):
        """s.y > eps max(y.y, 1) (_update_history, line 989)"""
        return not (sy <= self.eps * max(yy, 1.0))

    def accept(self, Ys, Ss, Yy, Sy, ss, sy, yy):
        """The new pair becomes the newest live one.  Ys[i] = y_i . s, Ss[i] = s_i . s, Yy[i] = y_i . y, Sy[i] = s_i . y over the k
        live pairs.  A full ring drops its oldest pair: the Gram matrices move up and left by one."""
        Ys, Ss, Yy, Sy = (np.asarray(a, dtype=np.float64) for a in (Ys, Ss, Yy, Sy))
        if self.k == self.m:
            for G in (self.SS, self.SY, self.YY):
                G[:-1, :-1] = G[1:, 1:].copy()
            Ys, Ss, Yy, Sy = Ys[1:], Ss[1:], Yy[1:], Sy[1:]
            self.start = (self.start + 1) % self.ring
            self.k -= 1
        j = self.k
        self.SS[j, :j], self.SS[:j, j], self.SS[j, j] = Ss, Ss, ss
        self.SY[j, :j], self.SY[:j, j], self.SY[j, j] = Ys, Sy, sy
        self.YY[j, :j], self.YY[:j, j], self.YY[j, j] = Yy, Yy, yy
        self.k = j + 1
        self.theta = float(self.dtype.type(yy / sy))

    def advance(self, theta):
        """the ring's bookkeeping of an accepted pair alone (the device class, whose Gram matrices live on the device)"""
        if self.k == self.m:
            self.start = (self.start + 1) % self.ring
            self.k -= 1
        self.k += 1
        self.theta = float(theta)

    def rebuild(self, S, Y, theta=None):
        """From k stored pairs in logical order (a state handed in, not one a run arrived at): the Gram matrices by full products"""
        S = np.asarray(S, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        k = S.shape[0]
        if k > self.m:
            raise ValueError('more pairs than the memory')
        self.clear()
        self.k = k
        self.SS[:k, :k], self.SY[:k, :k], self.YY[:k, :k] = S @ S.T, S @ Y.T, Y @ Y.T
        if theta is None:
            theta = self.YY[k - 1, k - 1] / self.SY[k - 1, k - 1] if k else 1.0
        self.theta = float(self.dtype.type(theta))

    # everything below is in W's order: k rows of Y, then k rows of theta S
    def scale(self):
        return np.concatenate([np.ones(self.k), np.full(self.k, self.theta)])

    def M(self):
        """[[-D, L^T], [L, theta S S^T]] (_WM, lines 400-406)"""
        k = self.k
        SY = self.SY[:k, :k]
        M = np.zeros((2 * k, 2 * k))
        M[:k, :k] = -np.diag(np.diag(SY))
        L = np.tril(SY, -1)
        M[k:, :k] = L
        M[:k, k:] = L.T
        M[k:, k:] = self.theta * self.SS[:k, :k]
        return M

    def raw_gram(self):
        """the products of W's rows without theta, over all variables"""
        k = self.k
        return np.block([[self.YY[:k, :k], self.SY[:k, :k].T], [self.SY[:k, :k], self.SS[:k, :k]]])

    def solve_N(self, raw_gram, raw_rhs):
        """N^-1 W_F^T v with N = -M + W_F^T W_F / theta, from the raw products; returns the coefficients of the RAW rows in
        (1 / theta^2) W N^-1 W^T v"""
        d = self.scale()
        N = (d[:, None] * raw_gram * d[None, :]) / self.theta - self.M()
        z = _solve(N, d * raw_rhs)
        return d * z / (self.theta * self.theta)


def next_dt_min(df, ddf):
    """_next_dt_min, lines 509-520"""
    if df >= 0:
        return 0.0
    if ddf <= 0:
        return np.inf
    return -df / ddf


def cauchy_sweep(k, theta, M, raw_p0, d0d0, npos, chunk_fn):
    """Algorithm CP over the finite positive breakpoints in chunks (lines 586-741).  raw_p0: rows . d0 without theta; chunk_fn(lo, hi)
    -> (t, g, raw W columns (2k, hi - lo)) of the sorted positive breakpoints lo .. hi - 1, one host read each.  Returns (K, the number
    visited; t_old, the time of the last one visited or 0; t_old + dt_min; c = W^T (xc - x); the chunks read)."""
    df = -float(d0d0)
    ddf = theta * float(d0d0)
    if k:
        d = np.concatenate([np.ones(k), np.full(k, theta)])
        p = d * np.asarray(raw_p0, dtype=np.float64)
        ddf = ddf - float(p @ _solve(M, p))
        c = np.zeros(2 * k)
    K = None
    dt_min_final = None
    t_prev = 0.0
    lo = 0
    chunk = FIRST_CHUNK
    chunks = 0
    with np.errstate(all='ignore'):
        while lo < npos:
            hi = min(lo + chunk, npos)
            m_c = hi - lo
            t_c, g_c, Wc = chunk_fn(lo, hi)
            chunks += 1
            t_c = np.asarray(t_c, dtype=np.float64)
            g_c = np.asarray(g_c, dtype=np.float64)
            dt_c = np.diff(t_c, prepend=t_prev)
            gg = g_c * g_c
            ddf_step = -theta * gg
            df_alpha = gg - theta * gg * t_c
            if k:
                W = d[:, None] * np.asarray(Wc, dtype=np.float64)
                wMw = np.einsum('ib,ib->b', W, _solve(M, W))
                dP = W * g_c
                P = p[:, None] + np.concatenate([np.zeros((2 * k, 1)), np.cumsum(dP[:, :-1], axis=1)], axis=1)
                dC = P * dt_c
                C = c[:, None] + np.concatenate([np.zeros((2 * k, 1)), np.cumsum(dC[:, :-1], axis=1)], axis=1)
                wb_Mp = np.einsum('ib,ib->b', W, _solve(M, P))
                wb_Mc = np.einsum('ib,ib->b', W, _solve(M, C))
                ddf_step = ddf_step - 2.0 * g_c * wb_Mp - gg * wMw
                df_alpha = df_alpha - g_c * wb_Mc
            ddf_at = ddf + np.concatenate([[0.0], np.cumsum(ddf_step)])
            df_at = df + np.concatenate([[0.0], np.cumsum(dt_c * ddf_at[:-1] + df_alpha)])
            dt_min_at = np.where(df_at >= 0, 0.0, np.where(ddf_at <= 0, np.inf, -df_at / np.where(ddf_at <= 0, 1.0, ddf_at)))
            pred = dt_min_at[:m_c] < dt_c
            if pred.any():
                j = int(np.argmax(pred))
                K = lo + j
                dt_min_final = float(dt_min_at[j])
                t_old = t_prev if j == 0 else float(t_c[j - 1])
                if k:
                    p, c = P[:, j], C[:, j].copy()
                break
            df = float(df_at[m_c])
            ddf = float(ddf_at[m_c])
            t_prev = float(t_c[-1])
            if k:
                p = P[:, -1] + dP[:, -1]
                c = C[:, -1] + dC[:, -1]
            lo = hi
            chunk *= 8
    if K is None:
        K = npos
        dt_min_final = next_dt_min(df, ddf)
        t_old = t_prev
    dt_min = max(dt_min_final, 0.0) if np.isfinite(dt_min_final) else 0.0
    if k:
        c = c + p * dt_min
    else:
        c = np.zeros(0)
    return K, t_old, t_old + dt_min, c, chunks


# ---------------------------------------------------------------------------------------------------------------- one step

class Stepper:
    """One L-BFGS-B iteration over a set of passes `P`.  The passes own the n-long arrays (x, g, the ring, the direction, the trial
    point) and return the small records as numpy doubles; every method of P that returns something is one host read:

      begin()                        fg at x
      dots_g()                       -> raw W^T g, (2k,), and g.g
      direction(a, coef)             p = a g + sum coef row           (nothing read)
      breakpoints()                  -> raw W^T d0, d0.d0, the count of t <= 0, the count of finite t > 0
      sort_breakpoints()             (nothing read)
      chunk(lo, hi)                  -> t, g, raw W columns of the sorted positive breakpoints lo .. hi - 1
      cauchy_point(t_last, t_stop)   xc and the free mask             (nothing read)
      residual(theta, coef)          r = g + theta (xc - x) + sum coef row     (nothing read)
      free_products(with_gram)       -> raw W_F^T r, raw W_F^T W_F or None
      subspace(a, coef)              dx, x_hat, x_bar, p, p_hat       (nothing read)
      direction_info()               -> g.p, count p != 0, g.p_hat, count p_hat != 0, min bound_alpha(p_hat)
      use_truncated()                p = p_hat                        (nothing read)
      evaluate(alpha)                the trial point, fg there -> phi, phi'; the first call of an unbounded step also brings
                                     g.p and the count of p != 0, read through direction_info() afterwards without another read
      f0()                           f at x as a float (read with the first record that follows begin())
      update(alpha)                  the new pair into the ring's free row -> (products (2k, 2) with s and y; s.s, s.y, y.y)
      commit()                       x_prev = x, x = the trial point  (nothing read)
    """

    def __init__(self, passes, memory, dtype, has_bounds, c1=1e-4, c2=0.9, maxls=30):
        self.P = passes
        self.H = History(memory, dtype)
        self.has_bounds = bool(has_bounds)
        self.c1, self.c2, self.maxls = c1, c2, maxls
        self.iter = 0
        self.nfev = 0
        self.last_step_metadata = {}
        self.last_branches = []
        self.last_cauchy = None
        self.last_pair_accepted = False

    def _stop(self, reason, message):
        self.last_step_metadata = {'reason': reason}
        raise StopIteration(OptimizerStop(False, message))

    def step(self):
        P, H = self.P, self.H
        k, theta = H.k, H.theta
        P.begin()
        self.nfev += 1
        cache = {}
        if not self.has_bounds:
            gg = P.direction_unbounded()
            if gg == 0.0:       # -H g is zero exactly when g is: the stop comes before any trial point is evaluated, as in the reference
                self._stop('no_descent', 'no descent direction')
            alpha_max = None
            n_free = P.n
            cauchy_breaks = 0
            mode = 'unbounded'
            cache[1.0] = P.evaluate(1.0)
            gp, nnz = P.direction_info()[:2]
        else:
            raw_p0, d0d0, nzero, npos, M = P.breakpoints()
            nzero, npos = int(nzero), int(npos)
            if npos:
                P.sort_breakpoints()
            K, t_last, t_stop, c, chunks = cauchy_sweep(k, theta, M, raw_p0, d0d0, npos, P.chunk)
            cauchy_breaks = nzero + K
            n_free = P.n - cauchy_breaks
            P.cauchy_point(t_last, t_stop)
            self.last_cauchy = dict(t_last=t_last, t_stop=t_stop, c=c, chunks=chunks)
            P.residual_from(c)
            P.subspace_step(n_free)
            gp, nnz, gph, nnzh, amin = P.direction_info()
            if gp < 0.0:
                alpha_max = 1.0
                mode = 'projected'
            else:
                P.use_truncated()
                gp, nnz = gph, nnzh
                alpha_max = 1.0 if amin > 1.0 else 0.0 if amin < 0.0 else float(amin)
                mode = 'truncated'
        if (alpha_max is not None and alpha_max <= 0.0) or not nnz:
            self._stop('no_descent', 'no descent direction')
        f0 = P.f0()

        def phi(alpha):
            if alpha in cache:
                return cache.pop(alpha)
            return P.evaluate(alpha)

        self.last_branches = []
        alpha, _, _ = strong_wolfe(phi, f0, gp, maxalpha=alpha_max, c1=self.c1, c2=self.c2, maxiter=self.maxls, branches=self.last_branches)
        if alpha is None:
            self._stop('linesearch_fail', 'line search failed')
        self.last_pair_accepted = bool(P.update_history(alpha))
        P.commit()
        self.iter += 1
        self.last_step_metadata = {'alpha': float(alpha), 'free_vars': n_free, 'cauchy_breaks': cauchy_breaks, 'subspace_solved': True,
                                   'subspace_mode': mode}
        return f0


# ---------------------------------------------------------------------------------------------------------------- the passes in numpy

class NumpyPasses:
    """The passes of csrc/lbfgsb.hip in numpy: element arithmetic in the data's type, sums and combinations in double."""

    def __init__(self, fg, x0, memory, lower, upper):
        self.fg = fg
        self.x = np.array(x0).ravel().copy()
        self.dtype = self.x.dtype
        self.n = self.x.size
        self.lo, self.hi = lower, upper
        self.bounded = lower is not None
        self.S = np.zeros((memory + 1, self.n), dtype=self.dtype)
        self.Y = np.zeros((memory + 1, self.n), dtype=self.dtype)
        self.x_prev = self.x.copy()
        self.xt = self.x.copy()
        self.p = np.zeros_like(self.x)
        self.H = None      # set by the owner: the passes read k, start and ring from it
        self.host_reads = 0

    def _W(self):
        rows = self.H.rows()
        return np.concatenate([self.Y[rows], self.S[rows]]).astype(np.float64)

    def begin(self):
        f, g = self.fg(self.x)
        self._f0 = float(f)
        self.g = np.asarray(g, dtype=self.dtype).ravel()
        self.evals = 0

    def f0(self):
        return self._f0

    def dots_g(self):
        g64 = self.g.astype(np.float64)
        return self._W() @ g64, float(g64 @ g64)

    def _combine(self, a, v, b, u1, u2, coef):
        acc = a * v.astype(np.float64)
        if u1 is not None:
            acc = acc + b * (u1.astype(np.float64) - u2.astype(np.float64))
        if coef is not None and len(coef):
            W = self._W()
            for q in range(W.shape[0]):
                acc = acc + coef[q] * W[q]
        return acc

    def direction(self, a, coef):
        with np.errstate(all='ignore'):
            self.p = self._combine(a, self.g, 0.0, None, None, coef).astype(self.dtype)
        self._info = None

    def breakpoints(self):
        x, g, lo, hi = self.x, self.g, self.lo, self.hi
        with np.errstate(all='ignore'):
            t = np.full(self.n, np.inf, dtype=self.dtype)
            hit = (g > 0) & np.isfinite(lo)
            t[hit] = ((x - lo) / g)[hit]
            hit = (g < 0) & np.isfinite(hi)
            t[hit] = ((x - hi) / g)[hit]
            d0 = np.where(t > 0, -g, 0).astype(self.dtype)
        self.t, self.d0 = t, d0
        d64 = d0.astype(np.float64)
        return self._W() @ d64, float(d64 @ d64), int(np.sum(t <= 0)), int(np.sum((t > 0) & np.isfinite(t))), self.H.M()

    def sort_breakpoints(self):
        self.order = np.argsort(self.t, kind='stable')
        self.nzero = int(np.sum(self.t <= 0))

    def chunk(self, lo, hi):
        idx = self.order[self.nzero + lo:self.nzero + hi]
        return self.t[idx], self.g[idx], self._W()[:, idx]

    def cauchy_point(self, t_last, t_stop):
        T = self.dtype.type
        with np.errstate(all='ignore'):
            visited = self.t <= T(t_last)
            self.xc = np.where(visited, self.x - self.t * self.g, (-self.g) * T(t_stop) + self.x).astype(self.dtype)
        self.free = ~visited

    def residual(self, theta, coef):
        with np.errstate(all='ignore'):
            self.r = self._combine(1.0, self.g, theta, self.xc, self.x, coef).astype(self.dtype)

    def free_products(self, with_gram):
        W = self._W()[:, self.free]
        rhs = W @ self.r[self.free].astype(np.float64)
        return rhs, (W @ W.T if with_gram else None)

    def subspace(self, a, coef):
        with np.errstate(all='ignore'):
            dx = np.where(self.free, self._combine(a, self.r, 0.0, None, None, coef).astype(self.dtype), 0).astype(self.dtype)
            xhat = self.xc + dx
            xbar = np.minimum(np.maximum(xhat, self.lo), self.hi)
            self.p = xbar - self.x
            self.p_hat = ph = xhat - self.x
            ba = np.full(self.n, np.inf, dtype=self.dtype)
            pos, neg = ph > 0, ph < 0
            ba[pos] = ((self.hi - self.x) / ph)[pos]
            ba[neg] = ((self.lo - self.x) / ph)[neg]
        g64 = self.g.astype(np.float64)
        self._info = (float(g64 @ self.p.astype(np.float64)), int(np.sum(self.p != 0)), float(g64 @ ph.astype(np.float64)), int(np.sum(ph != 0)),
                      float(np.min(ba.astype(np.float64))))

    # ---- a pass with the small algebra that follows it (csrc/lbfgsb.hip small_kernel on the device)
    def direction_unbounded(self):
        H = self.H
        raw_g, gg = self.dots_g()
        if H.k:
            self.direction(-1.0 / H.theta, H.solve_N(H.raw_gram(), raw_g))
        else:
            self.direction(-1.0, None)
        return gg

    def residual_from(self, c):
        H = self.H
        self.residual(H.theta, -H.scale() * _solve(H.M(), c) if H.k else None)

    def subspace_step(self, n_free):
        H = self.H
        coef = None
        if H.k and n_free > 0:
            raw_rhs, raw_gram = self.free_products(with_gram=n_free < self.n)
            coef = H.solve_N(H.raw_gram() if raw_gram is None else raw_gram, raw_rhs)
        self.subspace(-1.0 / H.theta, coef)

    def update_history(self, alpha):
        H = self.H
        k = H.k
        prod, (ss, sy, yy) = self.update(alpha)
        ok = H.curvature_ok(sy, yy)
        if ok:
            H.accept(prod[:k, 0], prod[k:, 0], prod[:k, 1], prod[k:, 1], ss, sy, yy)
        return ok

    def direction_info(self):
        if self._info is None:
            self._info = (float(self.g.astype(np.float64) @ self.p.astype(np.float64)), int(np.sum(self.p != 0)), 0.0, 0, np.inf)
        return self._info

    def use_truncated(self):
        self.p = self.p_hat

    def trial(self, alpha):
        with np.errstate(all='ignore'):
            xt = self.x + self.dtype.type(alpha) * self.p
            if self.bounded:
                ok = xt == xt
                xt = np.where(ok, np.minimum(np.maximum(xt, self.lo), self.hi), xt)
        self.xt = xt.astype(self.dtype)

    def evaluate(self, alpha):
        self.evals += 1
        self.trial(alpha)
        f, g = self.fg(self.xt)
        self.g_new = np.asarray(g, dtype=self.dtype).ravel()
        return float(f), float(self.g_new.astype(np.float64) @ self.p.astype(np.float64))

    def update(self, alpha):
        with np.errstate(all='ignore'):
            s = (self.xt - self.x) if self.bounded else self.p * self.dtype.type(alpha)
            y = self.g_new - self.g
        W = self._W()
        slot = self.H.slot
        self.S[slot], self.Y[slot] = s, y
        s64, y64 = s.astype(np.float64), y.astype(np.float64)
        return np.stack([W @ s64, W @ y64], axis=1), (float(s64 @ s64), float(s64 @ y64), float(y64 @ y64))

    def commit(self):
        self.x_prev = self.x
        self.x = self.xt.copy()

    def set_history(self, S, Y):
        k = len(S)
        self.S[:] = 0
        self.Y[:] = 0
        self.S[:k], self.Y[:k] = S, Y


class LBFGSBModel:
    """PrysmLBFGSB on the host in numpy, with the formulation of the kernels: what the device class is held against."""

    def __init__(self, fg, x0, memory=10, lower_bounds=None, upper_bounds=None, c1=1e-4, c2=0.9, maxls=30):
        x0 = np.asarray(x0)
        dtype = x0.dtype
        n = x0.size
        lo = np.full(n, -np.inf, dtype=dtype) if lower_bounds is None else np.broadcast_to(np.asarray(lower_bounds, dtype=dtype), (n,)).copy()
        hi = np.full(n, np.inf, dtype=dtype) if upper_bounds is None else np.broadcast_to(np.asarray(upper_bounds, dtype=dtype), (n,)).copy()
        has_bounds = bool(np.any(np.isfinite(lo)) or np.any(np.isfinite(hi)))
        self.l, self.u = lo, hi  # noqa: E741
        self.passes = NumpyPasses(fg if callable(fg) else fg.fg, x0, memory, lo if has_bounds else None, hi if has_bounds else None)
        self.core = Stepper(self.passes, memory, dtype, has_bounds, c1, c2, maxls)
        self.passes.H = self.core.H

    x = property(lambda self: self.passes.x)
    iter = property(lambda self: self.core.iter)
    nfev = property(lambda self: self.core.nfev)
    theta = property(lambda self: self.core.H.theta)
    last_step_metadata = property(lambda self: self.core.last_step_metadata)

    def _set_state(self, x, S, Y, theta=None):
        """x and k pairs in logical order (oldest first)"""
        self.passes.x = np.asarray(x, dtype=self.passes.dtype).copy()
        self.core.H.rebuild(S, Y, theta)
        self.passes.set_history(np.asarray(S, dtype=self.passes.dtype), np.asarray(Y, dtype=self.passes.dtype))

    def _history(self):
        """the live pairs in logical order"""
        rows = self.core.H.rows()
        return self.passes.S[rows], self.passes.Y[rows]

    def step(self):
        f = self.core.step()
        return self.passes.x_prev, f, self.passes.g
