"""Jacobi polynomials (prysm/polynomials/jacobi.py) on the device: the recurrence of DLMF 18.9 as one table of csrc/recur.hip, the sums
evaluated per point without a stored basis, and the adjoint of the radial sum (the reference has none).
"""
from . import _recur as R
from .recur_plan import weight, recurrence_abc  # noqa: F401

__all__ = ['weight', 'recurrence_abc', 'jacobi', 'jacobi_with_der', 'jacobi_seq', 'jacobi_seq_with_der', 'jacobi_der', 'jacobi_der_seq',
           'jacobi_sum_clenshaw', 'jacobi_radial_sum', 'jacobi_radial_sum_der_xy', 'jacobi_radial_sum_adjoint']

jacobi, jacobi_seq, jacobi_der, jacobi_der_seq = R.make_family('jacobi', 'jacobi.py:46-276')


def jacobi_seq_with_der(ns, alpha, beta, x):
    """(P_n, dP_n/dx) for the orders ns, each (len(ns), *x.shape), both from one launch (jacobi.py:178-201).  ns must be strictly
    ascending."""
    return R.basis('jacobi', (alpha, beta), ns, x, 'pd')


def jacobi_with_der(n, alpha, beta, x):
    """(P_n, dP_n/dx) of one order (jacobi.py:88-134)."""
    p, d = R.basis('jacobi', (alpha, beta), R._single(n), x, 'pd')
    return p[0], d[0]


def jacobi_sum_clenshaw(s, alpha, beta, x, alphas=None, der=False):
    """sum_k s[k] P_k(x) for the dense weights s of P_0, P_1, ... (jacobi.py:279-316), by the forward recurrence in one launch; s (K,)
    or (B, K) for a stack.  der=True returns (sum, d sum / dx).  Departures: the reference's alphas= work array is not provided
    (NotImplementedError when given), nor is jacobi_sum_clenshaw_der -- use der=True or jacobi_radial_sum_der_xy."""
    if alphas is not None:
        raise NotImplementedError('jacobi_sum_clenshaw: the alphas= work array of the reference is not provided; use der=True for the '
                                  'derivative sum')
    K = s.shape[-1] if hasattr(s, 'shape') else len(s)
    out = R.sum1d('jacobi', (alpha, beta), s, range(K), x, want='zx' if der else 'z')
    return out if der else out[0]


def jacobi_radial_sum(coefs, ns, alpha, beta, x, y, normalization_radius):
    """sum_k coefs[k] P_{ns[k]}(2 (x^2 + y^2) / R^2 - 1) at the Cartesian points (x, y) (jacobi.py:376-389), one launch, no stored
    basis.  ns must be strictly ascending; coefs (K,) or (B, K)."""
    return R.sum1d('jacobi', (alpha, beta), coefs, ns, x, y, normalization_radius, 'z')[0]


def jacobi_radial_sum_der_xy(coefs, ns, alpha, beta, x, y, normalization_radius):
    """(z, dz/dx, dz/dy) of jacobi_radial_sum with dz/dx = dz/du 4 x / R^2 and dz/dy = dz/du 4 y / R^2 (jacobi.py:392-413), all three
    from one launch."""
    return R.sum1d('jacobi', (alpha, beta), coefs, ns, x, y, normalization_radius, 'zxy')


def jacobi_radial_sum_adjoint(databar, ns, alpha, beta, x, y, normalization_radius, dx_bar=None, dy_bar=None):
    """The gradient with respect to coefs of jacobi_radial_sum_der_xy's outputs: databar is the adjoint of z, dx_bar and dy_bar
    (optional) of the gradient maps, databar may be None when one of those is given; (K,) or (B, K).  Deterministic, no atomics."""
    return R.project1d('jacobi', (alpha, beta), ns, x, y, normalization_radius, databar, dx_bar, dy_bar)
