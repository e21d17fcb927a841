"""Stop conditions for run_until (prysm/x/optym/governors.py): host logic around the device optimizers.

A governor sees a StepRecord after every completed step and answers with a GovernorDecision.  The arrays of a record are whatever the
optimizer works on -- device tensors for the optimizers of this package, numpy arrays or lists for anything else -- and each
observation may read a scalar from the device (the norm of a gradient, the cost).  The device optimizers update `x` IN PLACE and
overwrite `x_prev` at the next step, so a record's `x` / `x_next` are only meaningful until then; a governor that wants history
copies what it needs when it observes.
"""
import numpy as np

__all__ = ['StepRecord', 'GovernorDecision', 'OptimizationResult', 'Governor', 'AnyGovernor', 'AllGovernor', 'MaxIterations',
           'MaxEvaluations', 'FunctionTolerance', 'GradientTolerance', 'StepTolerance', 'ConstraintTolerance']


def _host(a):
    """a numpy array of whatever a record holds (a device tensor is copied to the host)"""
    if hasattr(a, 'detach') and hasattr(a, 'cpu'):
        return a.detach().cpu().numpy()
    return np.asarray(a)


class StepRecord:
    """One completed step: the optimizer, the one-based iteration, the iterate `x` at which `f` and `g` were evaluated, the iterate
    after the step `x_next`, and the optimizer's metadata (copied into a dict)."""
    __slots__ = ('optimizer', 'iteration', 'x', 'f', 'g', 'x_next', 'metadata')

    def __init__(self, optimizer, iteration, x, f, g, x_next, metadata=None):
        self.optimizer = optimizer
        self.iteration = int(iteration)
        self.x = x
        self.f = float(f)       # a 0-d device tensor is read here
        self.g = g
        self.x_next = x_next
        self.metadata = dict(metadata) if metadata is not None else {}


class GovernorDecision:
    """stop: end the run; success: the stop is a convergence; message: why."""
    __slots__ = ('stop', 'success', 'message')

    def __init__(self, stop=False, success=False, message=''):
        self.stop = bool(stop)
        self.success = bool(success)
        self.message = message

    def __bool__(self):
        return self.stop


def _go_on():
    return GovernorDecision(False, False, '')


class OptimizationResult:
    """What run_until returns: the final iterate, the decision that ended the run, the records, the optimizer and its counters."""
    __slots__ = ('x', 'success', 'message', 'nit', 'nfev', 'njev', 'decision', 'records', 'optimizer')

    def __init__(self, x, decision, records, optimizer=None):
        self.x = x
        self.decision = decision
        self.success = bool(decision.success)
        self.message = decision.message
        self.records = records
        self.nit = len(records)
        self.optimizer = optimizer
        self.nfev = getattr(optimizer, 'nfev', None)
        self.njev = getattr(optimizer, 'njev', None)

    def __repr__(self):
        return f'OptimizationResult(success={self.success}, message={self.message!r}, nit={self.nit})'


class Governor:
    """Base class: never stops."""

    def observe(self, record):
        return _go_on()


class AnyGovernor(Governor):
    """Stops with the first child (in the order given) that stops.  Every child observes every record."""

    def __init__(self, governors):
        self.governors = tuple(governors)

    def observe(self, record):
        seen = [gov.observe(record) for gov in self.governors]
        for dec in seen:
            if dec.stop:
                return dec
        return _go_on()


class AllGovernor(Governor):
    """Stops once every child has stopped at least once (not necessarily on the same record); a success if all of those were."""

    def __init__(self, governors):
        self.governors = tuple(governors)
        self._decisions = [None] * len(self.governors)

    def observe(self, record):
        for i, gov in enumerate(self.governors):
            dec = gov.observe(record)
            if dec.stop:
                self._decisions[i] = dec
        held = self._decisions
        if not held or any(d is None for d in held):
            return _go_on()
        return GovernorDecision(True, all(d.success for d in held), '; '.join(d.message for d in held if d.message))


def _nonnegative(value, name):
    if value < 0:
        raise ValueError(f'{name} must be nonnegative')


def _vector_norm(x, norm):
    """the norm of an array (host or device) as a Python float; an empty array has norm 0"""
    x = _host(x)
    if x.size == 0:
        return 0.0
    if isinstance(norm, str) and norm == 'inf' or (not isinstance(norm, str) and norm == np.inf):
        return float(np.abs(x).max())
    return float(np.linalg.norm(x.ravel(), ord=norm))


class MaxIterations(Governor):
    """Stops (without success) when the record's iteration reaches n."""

    def __init__(self, n):
        n = int(n)
        _nonnegative(n, 'n')
        self.n = n

    def observe(self, record):
        if record.iteration >= self.n:
            return GovernorDecision(True, False, 'maximum iterations reached')
        return _go_on()


class MaxEvaluations(Governor):
    """Stops (without success) when the optimizer reports nfev >= n; an optimizer without nfev never trips it."""

    def __init__(self, n):
        n = int(n)
        _nonnegative(n, 'n')
        self.n = n

    def observe(self, record):
        nfev = getattr(record.optimizer, 'nfev', None)
        if nfev is not None and nfev >= self.n:
            return GovernorDecision(True, False, 'maximum function evaluations reached')
        return _go_on()


class FunctionTolerance(Governor):
    """Stops when two consecutive objective values differ by at most ftol (times max(1, |f_prev|, |f|) when relative).  The current
    value is metadata['f_next'] where the optimizer reports it, else the record's f; with f_next the first record already compares
    (f against f_next), without it the first record only primes."""

    def __init__(self, ftol, relative=True):
        ftol = float(ftol)
        _nonnegative(ftol, 'ftol')
        self.ftol = ftol
        self.relative = bool(relative)
        self._previous_f = None

    def observe(self, record):
        reported = 'f_next' in record.metadata
        now = float(record.metadata['f_next']) if reported else float(record.f)
        before = self._previous_f
        self._previous_f = now
        if before is None:
            if not reported:
                return _go_on()
            before = record.f
        scale = max(1.0, abs(before), abs(now)) if self.relative else 1.0
        if abs(before - now) <= self.ftol * scale:
            return GovernorDecision(True, True, 'function tolerance reached')
        return _go_on()


class GradientTolerance(Governor):
    """Stops when the norm of the gradient is at most gtol."""

    def __init__(self, gtol, norm=np.inf):
        gtol = float(gtol)
        _nonnegative(gtol, 'gtol')
        self.gtol = gtol
        self.norm = norm

    def observe(self, record):
        if _vector_norm(record.g, self.norm) <= self.gtol:
            return GovernorDecision(True, True, 'gradient tolerance reached')
        return _go_on()


class StepTolerance(Governor):
    """Stops when the norm of x_next - x is at most xtol (times max(1, |x|) when relative)."""

    def __init__(self, xtol, relative=True, norm=np.inf):
        xtol = float(xtol)
        _nonnegative(xtol, 'xtol')
        self.xtol = xtol
        self.relative = bool(relative)
        self.norm = norm

    def observe(self, record):
        x = _host(record.x)
        moved = _vector_norm(_host(record.x_next) - x, self.norm)
        scale = max(1.0, _vector_norm(x, self.norm)) if self.relative else 1.0
        if moved <= self.xtol * scale:
            return GovernorDecision(True, True, 'step tolerance reached')
        return _go_on()


class ConstraintTolerance(Governor):
    """Stops when the reported constraint violation (metadata['constraint_violation'], else the optimizer's attribute of that name)
    is at most tol; never without a report."""

    def __init__(self, tol):
        tol = float(tol)
        _nonnegative(tol, 'tol')
        self.tol = tol

    def observe(self, record):
        violation = record.metadata.get('constraint_violation')
        if violation is None:
            violation = getattr(record.optimizer, 'constraint_violation', None)
        if violation is not None and float(violation) <= self.tol:
            return GovernorDecision(True, True, 'constraint tolerance reached')
        return _go_on()
