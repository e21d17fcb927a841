"""First-order optimizers on the device (prysm/x/optym/optimizers.py): GradientDescent, AdaGrad, RMSProp, Adam, RAdam, AdaMomentum,
Yogi, and the runners runN and run_until.

Constructors and step() are the reference's: `fg` (a callable x -> (f, g) or an object with .fg), `x0`, `alpha`, the betas or gamma,
`lower_bounds` / `upper_bounds`; step() returns (x_prev, f, g).  What is different is where things live:

- `x`, the state (`m` / `v` or `accumulator`) and `x_prev` are device tensors that keep their ADDRESS for the optimizer's life: a
  step updates x and the state in place and stores the pre-step iterate in x_prev, so the tensor step() returns as `x_prev` is
  OVERWRITTEN BY THE NEXT STEP (clone it to keep it).  A model captured in a graph reads `self.x` at a fixed address.
- A step is two launches whatever the optimizer: pm_optym_advance (one thread: the step counter, a device int64, and the
  coefficients that depend on it -- 1 - beta1^k, 1 - beta2^k, RAdam's rho, r and branch -- in double) and pm_optym_step (one kernel:
  projected gradient, moments, step, clamp).  Nothing is read on the host, so `fg` + step() can be captured and replayed.
- `iter` counts on the host as in the reference; `counter` is the device's copy, the one the kernels use.
- Under bounds the step kernel also stores the projected gradient and the active-bound bytes; `last_step_metadata` carries those
  tensors, and its 'bounded_variables' is counted (a host read) only when it is looked up.
- reset(x0=None) restores x, the state and the counter IN PLACE: graph.capture runs its function a few times to warm up, and a
  captured iteration starts from a defined state after reset().
- RAdam keeps x in its own dtype (the reference's Python-float r promotes a float32 x to float64).

PrysmLBFGSB is in lbfgsb.py.  The finite-difference Problem, the scipy-driver classes LBFGSB / F77LBFGSB / CLBFGSB and
DampedLeastSquares of the reference are not part of this package.
"""
import numpy as np
import torch

from ... import _lib as L
from ...coordinates import _code
from .governors import GovernorDecision, OptimizationResult, StepRecord

__all__ = ['runN', 'run_until', 'as_problem', 'GradientDescent', 'AdaGrad', 'RMSProp', 'Adam', 'RAdam', 'AdaMomentum', 'Yogi']

_FLOATS = (torch.float32, torch.float64)


class _CallableProblem:
    """fg(x) -> (f, g) from a plain callable"""

    def __init__(self, fg):
        self._fg = fg

    def fg(self, x):
        return self._fg(x)


def as_problem(obj):
    """obj itself when it has .fg, a wrapper when it is callable, else TypeError"""
    if hasattr(obj, 'fg'):
        return obj
    if callable(obj):
        return _CallableProblem(obj)
    raise TypeError(f'expected an object with fg(x) or a callable; got {type(obj).__name__}')


def runN(optimizer, N):
    """A generator over N steps of the optimizer, yielding what step() returns."""
    for _ in range(N):
        yield optimizer.step()


def _decision_of_stop(exc):
    value = exc.value
    message = getattr(value, 'message', None) or 'optimizer stopped'
    return GovernorDecision(True, bool(getattr(value, 'success', True)), message)


def run_until(optimizer, governor, *, maxiter=None):
    """Step the optimizer until the governor stops it, the optimizer raises StopIteration, or `maxiter` steps have been taken (a cap
    of the runner's own, apart from any MaxIterations governor).  Returns an OptimizationResult with optimizer.x, the terminal
    decision and the records.  With the device optimizers the arrays of a record alias buffers that later steps overwrite."""
    records = []
    exhausted = GovernorDecision(True, False, 'maximum iterations reached')
    if maxiter is not None:
        maxiter = int(maxiter)
        if maxiter <= 0:
            return OptimizationResult(getattr(optimizer, 'x', None), exhausted, records, optimizer)
    done = 0
    while maxiter is None or done < maxiter:
        done += 1
        try:
            x, f, g = optimizer.step()
        except StopIteration as exc:
            return OptimizationResult(getattr(optimizer, 'x', None), _decision_of_stop(exc), records, optimizer)
        metadata = getattr(optimizer, 'last_step_metadata', None)
        record = StepRecord(optimizer=optimizer, iteration=done, x=x, f=f, g=g, x_next=optimizer.x, metadata=metadata or {})
        records.append(record)
        decision = governor.observe(record)
        if decision.stop:
            return OptimizationResult(optimizer.x, decision, records, optimizer)
    return OptimizationResult(optimizer.x, exhausted, records, optimizer)


class _BoundedMetadata(dict):
    """projected_gradient and active_bounds are the device tensors the step kernel stored; bounded_variables is their count, summed
    (and read on the host) when it is asked for"""

    def __missing__(self, key):
        if key == 'bounded_variables' and 'active_bounds' in self:
            return int(self['active_bounds'].sum().item())
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or (key == 'bounded_variables' and dict.__contains__(self, 'active_bounds'))

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        return list(dict.keys(self)) + (['bounded_variables'] if dict.__contains__(self, 'active_bounds') else [])

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def items(self):
        return [(k, self[k]) for k in self.keys()]


def _host_tensor(a, dtype=None):
    """numpy array / tensor -> tensor where it lies (no device needed for the argument checks)"""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or t.dtype == dtype else t.to(dtype)


def _bound(bound, x0, default):
    if bound is None:
        return torch.full(x0.shape, default, dtype=x0.dtype, device=x0.device)
    if isinstance(bound, torch.Tensor):
        b = bound.to(device=x0.device, dtype=x0.dtype)
    else:
        b = torch.from_numpy(np.ascontiguousarray(np.asarray(bound, dtype=np.float64))).to(device=x0.device, dtype=x0.dtype)
    if b.shape == x0.shape:
        return b
    if b.numel() == x0.numel():
        return b.reshape(x0.shape)
    raise ValueError('bounds must have the same shape or size as x0')


class _Optimizer:
    """What the seven optimizers share: the device buffers, the bounds, the two launches of a step."""
    _kind = None
    _nstate = 0      # state arrays: 0 GradientDescent, 1 the accumulator, 2 m and v

    def _setup(self, fg, x0, alpha, beta1, beta2, lower_bounds, upper_bounds):
        self.problem = as_problem(fg)
        x0t = _host_tensor(x0)
        if x0t.dtype not in _FLOATS:
            raise TypeError(f'x0 must be float32 or float64, got {x0t.dtype}')
        lo, hi = _bound(lower_bounds, x0t, -np.inf), _bound(upper_bounds, x0t, np.inf)
        if bool(torch.any(lo > hi)):
            raise ValueError('lower_bounds must be <= upper_bounds')
        self._has_bounds = bool(torch.any(torch.isfinite(lo)) or torch.any(torch.isfinite(hi)))
        self.x0 = x0
        self.alpha = alpha
        self._beta1, self._beta2 = float(beta1), float(beta2)
        dev = L.device()
        self.l = lo.to(dev).contiguous()  # noqa: E741 -- the reference's name
        self.u = hi.to(dev).contiguous()
        self._x0 = self._project(L.as_device(x0t).clone())
        self.x = self._x0.clone()
        self.x_prev = self.x.clone()
        self.eps = float(np.finfo(np.float32 if self.x.dtype == torch.float32 else np.float64).eps)
        self._state = [torch.zeros_like(self.x) for _ in range(self._nstate)]
        self.counter = torch.zeros((), dtype=torch.int64, device=dev)
        self._coef = torch.zeros(8, dtype=torch.float64, device=dev)
        self._g_step = torch.zeros_like(self.x) if self._has_bounds else None
        self._active = torch.zeros(self.x.shape, dtype=torch.bool, device=dev) if self._has_bounds else None
        self.iter = 0
        self.last_step_metadata = {}

    def _project(self, x):
        if not self._has_bounds:
            return x
        return torch.minimum(torch.maximum(x, self.l), self.u)

    def reset(self, x0=None):
        """Back to the start (or to a new x0 of the same shape), IN PLACE: x, x_prev, the state, the device counter and `iter`."""
        if x0 is not None:
            new = L.as_device(_host_tensor(x0), self.x.dtype)
            if new.numel() != self.x.numel():
                raise ValueError('x0 must have the size of the variables')
            self._x0 = self._project(new.reshape(self.x.shape).clone())
            self.x0 = x0
        self.x.copy_(self._x0)
        self.x_prev.copy_(self._x0)
        for s in self._state:
            s.zero_()
        self.counter.zero_()
        self._coef.zero_()
        self.iter = 0
        self.last_step_metadata = {}
        return self

    def _gradient(self, g):
        g = L.as_device(g, self.x.dtype)
        if g.numel() != self.x.numel():
            raise ValueError(f'the gradient has {g.numel()} elements, x has {self.x.numel()}')
        return g

    def step(self):
        """One iteration: (x_prev, f, g).  x_prev is the optimizer's own buffer, overwritten by the next step."""
        f, g = self.problem.fg(self.x)
        gd = self._gradient(g)
        lib = L.load()
        st = L.stream_ptr()
        L.check(lib.pm_optym_advance(self._kind, self._beta1, self._beta2, L.ptr(self.counter), L.ptr(self._coef), st))
        s1 = self._state[0] if self._nstate >= 1 else None
        s2 = self._state[1] if self._nstate >= 2 else None
        bounded = self._has_bounds
        L.check(lib.pm_optym_step(_code(self.x.dtype), self._kind, self.x.numel(), L.ptr(self.x), L.ptr(gd), L.ptr(s1), L.ptr(s2),
                                  L.ptr(self.l if bounded else None), L.ptr(self.u if bounded else None), float(self.alpha), self._beta1,
                                  self._beta2, self.eps, L.ptr(self._coef), L.ptr(self.x_prev), L.ptr(self._g_step), L.ptr(self._active), st))
        self.iter += 1
        if bounded:
            self.last_step_metadata = _BoundedMetadata(projected_gradient=self._g_step, active_bounds=self._active)
        else:
            self.last_step_metadata = {}
        return self.x_prev, f, g


class GradientDescent(_Optimizer):
    """x <- x - alpha g (optimizers.py:205-244)."""
    _kind, _nstate = L.PM_OPT_GD, 0

    def __init__(self, fg, x0, alpha, lower_bounds=None, upper_bounds=None):
        self._setup(fg, x0, alpha, 0.0, 0.0, lower_bounds, upper_bounds)


class _Accumulator(_Optimizer):
    _nstate = 1

    @property
    def accumulator(self):
        return self._state[0]


class AdaGrad(_Accumulator):
    """s += g^2; x <- x - alpha g / (sqrt(s) + eps) (optimizers.py:247-276)."""
    _kind = L.PM_OPT_ADAGRAD

    def __init__(self, fg, x0, alpha, lower_bounds=None, upper_bounds=None):
        self._setup(fg, x0, alpha, 0.0, 0.0, lower_bounds, upper_bounds)


class RMSProp(_Accumulator):
    """s <- gamma s + (1 - gamma) g^2; x <- x - alpha g / (sqrt(s) + eps) (optimizers.py:279-313)."""
    _kind = L.PM_OPT_RMSPROP

    def __init__(self, fg, x0, alpha, gamma=0.9, lower_bounds=None, upper_bounds=None):
        self._setup(fg, x0, alpha, gamma, 0.0, lower_bounds, upper_bounds)

    @property
    def gamma(self):
        return self._beta1

    @gamma.setter
    def gamma(self, value):
        self._beta1 = float(value)


class _MomentBased(_Optimizer):
    _nstate = 2

    def __init__(self, fg, x0, alpha, beta1=0.9, beta2=0.999, lower_bounds=None, upper_bounds=None):
        self._setup(fg, x0, alpha, beta1, beta2, lower_bounds, upper_bounds)

    @property
    def m(self):
        return self._state[0]

    @property
    def v(self):
        return self._state[1]

    @property
    def beta1(self):
        return self._beta1

    @beta1.setter
    def beta1(self, value):
        self._beta1 = float(value)

    @property
    def beta2(self):
        return self._beta2

    @beta2.setter
    def beta2(self, value):
        self._beta2 = float(value)


class Adam(_MomentBased):
    """m, v moving averages of g and g^2, bias-corrected; x <- x - alpha mhat / (sqrt(vhat) + eps) (optimizers.py:316-355)."""
    _kind = L.PM_OPT_ADAM


class RAdam(_MomentBased):
    """Adam with the rectified step: from rho >= 5 x <- x - alpha r mhat sqrt(1 - beta2^k) / (sqrt(v) + eps), before that plain
    gradient descent (optimizers.py:358-418).  x keeps its dtype."""
    _kind = L.PM_OPT_RADAM

    @property
    def rhoinf(self):
        return 2 / (1 - self._beta2) - 1


class AdaMomentum(_MomentBased):
    """Adam with v built from m^2, eps added INTO v at every step, and no eps in the denominator (optimizers.py:421-459)."""
    _kind = L.PM_OPT_ADAMOMENTUM


class Yogi(_MomentBased):
    """Adam with the additive update v <- v - (1 - beta2) sign(v - g^2) g^2 and, as the reference has it, a second square root:
    x <- x - alpha m / (sqrt(sqrt(v + eps)) + eps) (optimizers.py:462-500)."""
    _kind = L.PM_OPT_YOGI
