"""Activation functions and related nodes on the device (prysm/x/optym/activation.py).

Tanh, Arctan, Softplus and Sigmoid are one sweep per forward / backprop (pm_optym_activation) with the reference's expressions.
Softmax and GumbelSoftmax run over the last axis in one launch each way (pm_optym_softmax, pm_optym_softmax_backprop): a row of K
logits is spread over the lanes of a wavefront, and the Gumbel noise, the add and the division by tau are formed in the load.
DiscreteEncoder composes an estimator with torch for the contraction over the levels.

Inputs are numpy arrays or torch tensors (float32 / float64; anything else real becomes float64); results are device tensors.

One addition to the reference's signatures: GumbelSoftmax.forward(x, u=None) takes the uniform variates, so that the node can be
tested; by default they are drawn on the device with torch.rand.
"""
import numpy as np
import torch

from ... import _lib as L
from ...conf import config
from ...coordinates import _code

__all__ = ['Softmax', 'GumbelSoftmax', 'DiscreteEncoder', 'Tanh', 'Arctan', 'Softplus', 'Sigmoid']

_FLOATS = (torch.float32, torch.float64)


def _real(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))
    if t.is_complex():
        raise TypeError('activations take real arrays')
    if dtype is None:
        dtype = t.dtype if t.dtype in _FLOATS else torch.float64
    return L.as_device(t, dtype)


class Softmax:
    """Softmax over the final axis; the leading axes are independent variables."""

    def __init__(self):
        self.out = None
        self.in_shape = None
        self.work_shape = None

    def _forward(self, x, u, tau, eps):
        assert x.ndim > 1, "prysm's softmax is meant for use with multiple independent variables at once"
        x = _real(x)
        self.in_shape = tuple(x.shape)
        K = x.shape[-1]
        rows = x.numel() // K if K else 0
        self.work_shape = (rows, K)
        out = torch.empty((rows, K), dtype=x.dtype, device=x.device)
        if out.numel():
            L.check(L.load().pm_optym_softmax(_code(x.dtype), rows, K, L.ptr(x), L.ptr(u), float(tau), float(eps), L.ptr(out), L.stream_ptr()))
        self.out = out
        return out.reshape(self.in_shape)

    def forward(self, x):
        """exp(x - max) / sum over the last axis (activation.py:27-52); x of shape (..., K), at least 2-D."""
        return self._forward(x, None, 1.0, 0.0)

    def _backprop(self, grad, tau):
        assert self.out is not None, 'must run forward() before running reverse()'
        y = self.out
        g = _real(grad, y.dtype)
        if g.numel() != y.numel():
            raise ValueError('grad must have the shape of the input to forward()')
        gin = torch.empty_like(y)
        if gin.numel():
            rows, K = self.work_shape
            L.check(L.load().pm_optym_softmax_backprop(_code(y.dtype), rows, K, L.ptr(y), L.ptr(g), float(tau), L.ptr(gin), L.stream_ptr()))
        return gin.reshape(self.in_shape)

    def backprop(self, grad):
        """out (grad - sum_k grad out) (activation.py:54-83), evaluated as out_k (grad_k sum_j out_j - sum_j grad_j out_j) with the
        sums in double, which keeps its digits on a saturated row."""
        return self._backprop(grad, 1.0)


class GumbelSoftmax:
    """Softmax of (x + Gumbel noise) / tau (activation.py:86-127)."""

    def __init__(self, tau=1, eps=None):
        self.tau = tau
        self.eps = eps or np.finfo(config.precision).eps
        self.smax = Softmax()

    def forward(self, x, u=None):
        """u: uniform variates in [0, 1) of x's shape (drawn on the device when None); the noise is -log(-log(u + eps) + eps)."""
        assert x.ndim > 1, "prysm's softmax is meant for use with multiple independent variables at once"
        x = _real(x)
        if u is None:
            u = torch.rand(x.shape, dtype=x.dtype, device=x.device)
        else:
            u = _real(u, x.dtype)
            if u.shape != x.shape:
                raise ValueError('u must have the shape of x')
        return self.smax._forward(x, u, self.tau, self.eps)

    def backprop(self, protograd):
        """the softmax's backprop divided by tau (the noise does not depend on x)"""
        return self.smax._backprop(protograd, self.tau)


class DiscreteEncoder:
    """Continuous proxy for discrete-valued variables (activation.py:130-183): the expectation of `levels` under an estimator's
    probabilities."""

    def __init__(self, estimator, levels):
        if isinstance(levels, int):
            levels = np.arange(levels)
        self.est = estimator
        self.levels = levels
        self.tmpshape = None

    def _levels(self, like):
        lv = self.levels
        t = lv if isinstance(lv, torch.Tensor) else torch.from_numpy(np.asarray(lv))
        return t.to(like.device)

    def forward(self, x):
        samples = self.est.forward(x)
        lv = self._levels(samples).to(samples.dtype)
        tmp = samples * lv[None, :]
        self.tmpshape = tuple(tmp.shape)
        return tmp.sum(dim=-1)

    def backprop(self, grad):
        g = _real(grad)
        lv = self._levels(g).to(g.dtype)
        tmpbar = torch.broadcast_to(g[:, None], self.tmpshape) * lv[None, :]
        return self.est.backprop(tmpbar)

    def discretize(self, x):
        """the level with the largest probability"""
        encoded = self.est.forward(x)
        return torch.take(self._levels(encoded), torch.argmax(encoded, dim=-1))


class _AffineActivation:
    """y = f(a (x - x0)) + y0, elementwise"""
    _kind = None

    def __init__(self, a=1, x0=0, y0=0):
        self.a = a
        self.x0 = x0
        self.y0 = y0

    def _run(self, x, back):
        x = _real(x)
        out = torch.empty_like(x)
        if x.numel():
            L.check(L.load().pm_optym_activation(_code(x.dtype), self._kind, back, x.numel(), L.ptr(x), float(self.a), float(self.x0),
                                                 float(self.y0), L.ptr(out), L.stream_ptr()))
        return out

    def forward(self, x):
        return self._run(x, 0)

    def backprop(self, x):
        """d forward / d x at x"""
        return self._run(x, 1)


class Tanh(_AffineActivation):
    """2 / (1 + exp(-2 a (x - x0))) - 1 + y0 (activation.py:207-216)."""
    _kind = L.PM_ACT_TANH


class Arctan(_AffineActivation):
    """arctan(a (x - x0)) + y0 (activation.py:219-228)."""
    _kind = L.PM_ACT_ARCTAN


class Softplus(_AffineActivation):
    """log(1 + exp(a (x - x0))) + y0 (activation.py:231-240)."""
    _kind = L.PM_ACT_SOFTPLUS


class Sigmoid(_AffineActivation):
    """1 / (1 + exp(-a (x - x0))) + y0 (activation.py:243-252)."""
    _kind = L.PM_ACT_SIGMOID
