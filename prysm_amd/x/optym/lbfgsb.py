"""PrysmLBFGSB on the device (prysm/x/optym/_prysm_lbfgsb.py:206-1108): limited-memory BFGS with box constraints -- BLNZ 1995 with the
compact form B = theta I - W M^-1 W^T, the generalized Cauchy point, subspace minimisation through Sherman-Morrison-Woodbury, the
Morales-Nocedal projection with BLNZ truncation as fallback, and a strong-Wolfe bracket and zoom.

The constructor, step() -> (x_prev, f, g), x, iter, nfev, theta, last_step_metadata and the StopIteration stops are the reference's,
so runN, run_until and every governor work unchanged.  Where things live:

- every pass over the n variables is a kernel of csrc/lbfgsb.hip (history products, the free-set Gram, the combinations with their
  fused tails, the breakpoints, the Cauchy point, the trial point, the history update); each reads every history row it needs once.
  Sorting the breakpoint times and gathering one chunk of sorted breakpoints are torch calls.
- everything of size 2k x 2k is pm_lbfgsb_small, ONE single-workgroup launch per use, in double: it adds the first-stage partials
  of the pass before it, assembles M and N = -M + W^T W / theta from the three Gram matrices, which LIVE ON THE DEVICE and are updated
  incrementally, solves with partial pivoting, takes the curvature decision and theta, and leaves the coefficients of the next
  combination on the device and a small record for the host.
- the iteration's control flow, the strong-Wolfe search and the chunked sweep over the sorted positive breakpoints (with M from
  the breakpoint record, its result c the only 2k doubles that go up to the device) are prysm_amd/x/lbfgsb_plan.py on the host:
  the same code the numpy model runs, whose History is the model of pm_lbfgsb_small.
- x, x_prev, the history ring (memory + 1 rows: the new pair is formed in the update pass and stored into the row that is not
  live), the direction and the trial point are device tensors that keep their ADDRESS for the optimizer's life.  `fg` is called with
  x and with the trial tensor; f may come back as a Python float or a 0-d tensor (it is then copied into the record on the device).
  The tensor step() returns as x_prev is overwritten by the next step.

Host reads, counted in `host_reads`: a small record of doubles each, except a chunk of the breakpoint sweep, which is
(2k + 2) x chunk doubles (t, g and W's columns at the chunk's breakpoints; the chunk grows 8 x each time, so a minimiser deep in
the path makes the last read O(2k n)) with its prefix sums taken in numpy.  With E the evaluations of the line search
(E = 1 when the first trial is accepted) and C the chunks of the breakpoint sweep (64 positive breakpoints, then 8 x as many each
time; C = 0 without a finite positive breakpoint), a step that completes reads

    unbounded:  1 + E + 1                                (g.g; phi and phi' per evaluation; the update's decision)
    bounded:    1 + C + 1 + E + 1
                (the breakpoint sums with M; one per chunk; the direction decision; the evaluations; the update's decision)

so an unbounded step whose first trial is accepted reads 3 records.  f at x and g.p travel with the first
record read after them.  A step's control flow depends on what it reads, so a step is NOT capturable in a graph.
"""
import ctypes

import numpy as np
import torch

from ... import _lib as L
from ...coordinates import _code
from .. import lbfgsb_plan as plan
from .optimizers import _FLOATS, _bound, _host_tensor, as_problem

__all__ = ['PrysmLBFGSB']

# the record, in doubles: [0, 5) the direction's sums, 8 f at x, 9 f at the trial point, [16, 25) the record of phi', from 32 on what
# pm_lbfgsb_small leaves (at most 2k + 4 + 4k^2 = 4164 doubles, the breakpoint record with M)
_R_DIR, _R_F, _R_EVAL, _R_HEAD, _R_DOTS, _R_SIZE = 0, 8, 16, 32, 32, 4352


class _DevicePasses:
    """The passes lbfgsb_plan.Stepper asks for, on the kernels."""

    def __init__(self, problem, x0, memory, lo, hi):
        dev = L.device()
        self.problem = problem
        self.x = x0
        self.dtype = x0.dtype
        self.code = _code(x0.dtype)
        self.n = x0.numel()
        self.lo, self.hi = lo, hi
        self.bounded = lo is not None
        self.x_prev = x0.clone()
        self.xt = x0.clone()
        self.p = torch.zeros_like(x0)
        self.S = torch.zeros((memory + 1, self.n), dtype=self.dtype, device=dev)
        self.Y = torch.zeros_like(self.S)
        if self.bounded:
            self.p_hat, self.t, self.d0, self.xc, self.r = (torch.zeros_like(x0) for _ in range(5))
            self.free = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.coef = torch.zeros(2 * plan.MAX_MEMORY, dtype=torch.float64, device=dev)
        self.c_in = torch.zeros(2 * plan.MAX_MEMORY, dtype=torch.float64, device=dev)
        self.rec = torch.zeros(_R_SIZE, dtype=torch.float64, device=dev)
        self.lib = L.load()
        self.ws_bytes = self.lib.pm_lbfgsb_workspace()
        self.ws = torch.empty(2 * (self.ws_bytes // 8), dtype=torch.float64, device=dev)      # the passes' partials | the Gram pass's
        self.state = torch.zeros(self.lib.pm_lbfgsb_state_doubles(memory), dtype=torch.float64, device=dev)
        self.state[3 * memory * memory] = 1.0
        self.nparts = min(L.PM_LBFGSB_WGS, -(-self.n // L.PM_LBFGSB_THREADS))
        self.gparts = min(L.PM_LBFGSB_GRAM_WGS, -(-self.n // L.PM_LBFGSB_THREADS))
        self.H = None
        self.g = self.g_new = None
        self.host_reads = 0

    # ---- plumbing
    def _hist(self, k=None):
        H = self.H
        return (self.code, self.n, L.ptr(self.S), L.ptr(self.Y), self.n, H.ring, H.start, H.k if k is None else k)

    def _rec(self, at):
        return ctypes.c_void_p(self.rec.data_ptr() + 8 * at)

    def _tail(self):
        return (L.ptr(self.ws), self.ws_bytes, L.stream_ptr())

    def _read(self, lo, hi):
        self.host_reads += 1
        return self.rec[lo:hi].cpu().numpy()

    def _head(self):
        """the head of the record: the direction's sums, f at x and at the trial point, phi'"""
        head = self._read(0, _R_HEAD)
        if self._f0_on_device:
            self._f0 = float(head[_R_F])
        self._info = head[_R_DIR:_R_DIR + 5]
        return head

    def _upload_state(self, H):
        """the device's Gram matrices and theta from a History (the start, reset(), and the tests' hook)"""
        m = H.m
        host = np.concatenate([H.SS.ravel(), H.SY.ravel(), H.YY.ravel(), [H.theta], np.zeros(self.state.numel() - 3 * m * m - 1)])
        self.state.copy_(torch.from_numpy(host))

    def gram_matrices(self):
        """(S S^T, S Y^T, Y Y^T, theta) as the device holds them: a host read, for the tests"""
        m = self.H.m
        host = self.state.cpu().numpy()
        return host[:m * m].reshape(m, m), host[m * m:2 * m * m].reshape(m, m), host[2 * m * m:3 * m * m].reshape(m, m), host[3 * m * m]

    def _gradient(self, g):
        g = L.as_device(g, self.dtype)
        if g.numel() != self.n:
            raise ValueError(f'the gradient has {g.numel()} elements, x has {self.n}')
        return g

    def _combine(self, mode, a, v, b, u1, u2, out, out2=None):
        bounded = mode == L.PM_LBFGSB_SUBSPACE
        L.check(self.lib.pm_lbfgsb_combine(self.code, mode, self.n, *self._hist()[2:], a, L.ptr(v), b, L.ptr(u1), L.ptr(u2), L.ptr(self.coef if self.H.k else None),
                                           L.ptr(self.free if bounded else None), L.ptr(self.xc if bounded else None), L.ptr(self.x),
                                           L.ptr(self.lo), L.ptr(self.hi), L.ptr(self.g), L.ptr(out), L.ptr(out2), self._rec(_R_DIR), *self._tail()))

    # ---- the passes
    def begin(self):
        f, g = self.problem.fg(self.x)
        self.g = self._gradient(g)
        self._f0_on_device = isinstance(f, torch.Tensor)
        if self._f0_on_device:
            self.rec[_R_F].copy_(f.reshape(()))
            self._f0 = None
        else:
            self._f0 = float(f)
        self._info = None
        self.evals = 0

    def f0(self):
        return self._f0

    def _small(self, op, c_in=None, gram=False):
        """the single-workgroup small algebra on the partials the pass before it left (pm_lbfgsb_small); coef and the Gram matrices
        stay on the device"""
        L.check(self.lib.pm_lbfgsb_small(self.code, op, self.H.m, self.H.k, self.nparts, self.gparts if gram else 0, L.ptr(self.state),
                                         L.ptr(c_in), L.ptr(self.coef), self._rec(_R_DOTS), L.ptr(self.ws), self._gram_ws(), L.stream_ptr()))

    def _gram_ws(self):
        return ctypes.c_void_p(self.ws.data_ptr() + self.ws_bytes)

    def _no_record(self):
        return (None, L.ptr(self.ws), self.ws_bytes, L.stream_ptr())

    def direction_unbounded(self):
        k = self.H.k
        L.check(self.lib.pm_lbfgsb_dots(*self._hist(), L.ptr(self.g), None, None, *self._no_record()))
        self._small(L.PM_LBFGSB_SMALL_DIRECTION)
        self._combine(L.PM_LBFGSB_DIRECTION, -1.0 / self.H.theta if k else -1.0, self.g, 0.0, None, None, self.p)
        return float(self._read(_R_DOTS, _R_DOTS + 1)[0])

    def breakpoints(self):
        n2 = 2 * self.H.k
        L.check(self.lib.pm_lbfgsb_breakpoints(*self._hist(), L.ptr(self.x), L.ptr(self.g), L.ptr(self.lo), L.ptr(self.hi), L.ptr(self.t),
                                               L.ptr(self.d0), *self._no_record()))
        self._small(L.PM_LBFGSB_SMALL_BREAK)
        raw = self._read(_R_DOTS, _R_DOTS + n2 + 4 + n2 * n2)
        self.nzero = int(raw[n2 + 1])
        return raw[:n2], raw[n2], raw[n2 + 1], raw[n2 + 2], raw[n2 + 4:].reshape(n2, n2)

    def sort_breakpoints(self):
        self.order = torch.sort(self.t.reshape(-1), stable=True)[1]

    def chunk(self, lo, hi):
        idx = self.order[self.nzero + lo:self.nzero + hi]
        rows = self.H.rows()
        parts = [self.t.reshape(-1)[idx][None], self.g.reshape(-1)[idx][None]]
        if rows:
            parts += [self.Y[:, idx][rows], self.S[:, idx][rows]]
        self.host_reads += 1
        pack = torch.cat(parts).to(torch.float64).cpu().numpy()
        return pack[0], pack[1], pack[2:]

    def cauchy_point(self, t_last, t_stop):
        L.check(self.lib.pm_lbfgsb_cauchy_point(self.code, self.n, L.ptr(self.x), L.ptr(self.g), L.ptr(self.t), float(t_last), float(t_stop),
                                                L.ptr(self.xc), L.ptr(self.free), L.stream_ptr()))

    def residual_from(self, c):
        k = self.H.k
        if k:      # c, 2k doubles from the host's sweep, is the one thing that goes up; the solve against M stays on the device
            self.c_in[:2 * k].copy_(torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)))
            self._small(L.PM_LBFGSB_SMALL_RESIDUAL, self.c_in)
        self._combine(L.PM_LBFGSB_RESIDUAL, 1.0, self.g, float(self.H.theta), self.xc, self.x, self.r)

    def subspace_step(self, n_free):
        if self.H.k and n_free > 0:
            L.check(self.lib.pm_lbfgsb_dots(*self._hist(), L.ptr(self.r), None, L.ptr(self.free), *self._no_record()))
            gram = n_free < self.n      # with no variable active the free-set Gram IS the maintained one
            if gram:
                L.check(self.lib.pm_lbfgsb_gram(*self._hist(), L.ptr(self.free), None, self._gram_ws(), self.ws_bytes, L.stream_ptr()))
            self._small(L.PM_LBFGSB_SMALL_SUBSPACE, gram=gram)
        self._combine(L.PM_LBFGSB_SUBSPACE, -1.0 / self.H.theta, self.r, 0.0, None, None, self.p, self.p_hat)

    def direction_info(self):
        if self._info is None:
            self._head()
        return self._info

    def use_truncated(self):
        self.p.copy_(self.p_hat)

    def evaluate(self, alpha):
        self.evals += 1
        L.check(self.lib.pm_lbfgsb_trial(self.code, self.n, L.ptr(self.x), L.ptr(self.p), float(alpha), L.ptr(self.lo), L.ptr(self.hi),
                                         L.ptr(self.xt), L.stream_ptr()))
        f, g = self.problem.fg(self.xt)
        self.g_new = self._gradient(g)
        on_device = isinstance(f, torch.Tensor)
        if on_device:
            self.rec[_R_F + 1].copy_(f.reshape(()))
        L.check(self.lib.pm_lbfgsb_dots(*self._hist(0), L.ptr(self.g_new), L.ptr(self.p), None, self._rec(_R_EVAL), *self._tail()))
        head = self._head()
        return (float(head[_R_F + 1]) if on_device else float(f)), float(head[_R_EVAL + plan.TILE])

    def update_history(self, alpha):
        xt, x = (self.xt, self.x) if self.bounded else (None, None)
        L.check(self.lib.pm_lbfgsb_update(*self._hist(), self.H.slot, L.ptr(xt), L.ptr(x), L.ptr(self.p), float(alpha), L.ptr(self.g_new),
                                          L.ptr(self.g), *self._no_record()))
        self._small(L.PM_LBFGSB_SMALL_UPDATE)
        accepted, _, _, _, theta = self._read(_R_DOTS, _R_DOTS + 5)
        if accepted:
            self.H.advance(theta)
        return bool(accepted)

    def commit(self):
        self.x_prev.copy_(self.x)
        self.x.copy_(self.xt)


class PrysmLBFGSB:
    """L-BFGS-B (BLNZ 1995, Morales-Nocedal 2011) on the device.

    fg: a callable x -> (f, g) or an object with .fg; x0: float32 or float64, its dtype is the dtype of every array; memory: the
    history length, at most 32; lower_bounds / upper_bounds: None or per-variable bounds (infinite where there is none); c1, c2: the
    Wolfe constants; maxls: the bracket phase's iteration cap."""

    def __init__(self, fg, x0, memory=10, lower_bounds=None, upper_bounds=None, c1=1e-4, c2=0.9, maxls=30):
        self.problem = as_problem(fg)
        x0t = _host_tensor(x0)
        if x0t.dtype not in _FLOATS:
            raise TypeError(f'x0 must be float32 or float64, got {x0t.dtype}')
        npdtype = np.float32 if x0t.dtype == torch.float32 else np.float64
        plan.History(memory, npdtype)      # refuses a memory above the cap before anything touches the device
        lo, hi = _bound(lower_bounds, x0t, -np.inf), _bound(upper_bounds, x0t, np.inf)
        if bool(torch.any(lo > hi)):
            raise ValueError('lower_bounds must be <= upper_bounds')
        self._has_bounds = bool(torch.any(torch.isfinite(lo)) or torch.any(torch.isfinite(hi)))
        dev = L.device()
        self.x0 = x0
        self.m = int(memory)
        self.l = lo.to(dev).contiguous()  # noqa: E741 -- the reference's name
        self.u = hi.to(dev).contiguous()
        self._x0 = self._project(L.as_device(x0t).clone())
        self._passes = _DevicePasses(self.problem, self._x0.clone(), self.m, self.l if self._has_bounds else None,
                                     self.u if self._has_bounds else None)
        self._core = plan.Stepper(self._passes, self.m, npdtype, self._has_bounds, c1, c2, maxls)
        self._passes.H = self._core.H
        self.c1, self.c2, self.maxls = c1, c2, maxls

    def _project(self, x):
        if not self._has_bounds:
            return x
        return torch.minimum(torch.maximum(x, self.l), self.u)

    x = property(lambda self: self._passes.x)
    x_prev = property(lambda self: self._passes.x_prev)
    n = property(lambda self: self._passes.n)
    iter = property(lambda self: self._core.iter)
    nfev = property(lambda self: self._core.nfev)
    theta = property(lambda self: self._core.H.theta)
    host_reads = property(lambda self: self._passes.host_reads)
    last_step_metadata = property(lambda self: self._core.last_step_metadata)

    def reset(self, x0=None):
        """Back to the start (or to a new x0 of the same size) IN PLACE: x, x_prev, the history, iter and nfev."""
        if x0 is not None:
            new = L.as_device(_host_tensor(x0), self.x.dtype)
            if new.numel() != self.x.numel():
                raise ValueError('x0 must have the size of the variables')
            self._x0 = self._project(new.reshape(self.x.shape).clone())
            self.x0 = x0
        P = self._passes
        P.x.copy_(self._x0)
        P.x_prev.copy_(self._x0)
        P.S.zero_()
        P.Y.zero_()
        self._core.H.clear()
        P._upload_state(self._core.H)
        self._core.iter = self._core.nfev = 0
        self._core.last_step_metadata = {}
        return self

    def _set_state(self, x, S, Y, theta=None):
        """A hook of the tests, not part of the reference's interface (x is taken as it is, not projected).  Continue from x and k stored pairs, S and Y of shape (k, n) in logical order (oldest first), IN PLACE.  The Gram matrices are
        formed on the host from the arrays handed in."""
        P = self._passes
        S = np.asarray(S, dtype=np.float64).reshape(-1, P.n)
        Y = np.asarray(Y, dtype=np.float64).reshape(-1, P.n)
        self._core.H.rebuild(S, Y, theta)
        P._upload_state(self._core.H)
        P.x.copy_(L.as_device(_host_tensor(x), P.dtype).reshape(P.x.shape))
        P.S.zero_()
        P.Y.zero_()
        if len(S):
            P.S[:len(S)].copy_(L.as_device(S, P.dtype))
            P.Y[:len(Y)].copy_(L.as_device(Y, P.dtype))
        return self

    def _history(self):
        """a hook of the tests: the live pairs (S, Y), each (k, n), in logical order (copies)"""
        rows = self._core.H.rows()
        return self._passes.S[rows], self._passes.Y[rows]

    def step(self):
        """One iteration: (x_prev, f, g).  Raises StopIteration carrying .success / .message ('no descent direction', 'line search
        failed'); x is then unchanged.  x_prev is the optimizer's own buffer, overwritten by the next step."""
        f = self._core.step()
        return self._passes.x_prev, f, self._passes.g
