"""Legendre polynomials (prysm/polynomials/legendre.py) on the device: k P_k = (2k - 1) x P_{k-1} - (k - 1) P_{k-2} as one table of
csrc/recur.hip.  legendre_2d_sum[_der_xy] and legendre_2d_sum_adjoint are the separable kernels with the Legendre table: the
rectangular-aperture counterpart of zernike_sum and its adjoint (the reference has neither).
"""
from . import _recur as R

__all__ = ['legendre', 'legendre_seq', 'legendre_der', 'legendre_der_seq', 'legendre_2d_sum', 'legendre_2d_sum_der_xy',
           'legendre_2d_sum_adjoint']

legendre, legendre_seq, legendre_der, legendre_der_seq = R.make_family('legendre', 'legendre.py:7-110')


def legendre_2d_sum(coefs, mns, x, y, cartesian_grid=True):
    """sum_k coefs[k] P_m(x) P_n(y) over the pairs (m, n) of mns on a Cartesian grid, in one launch without a stored basis.  x and y
    are 1-D axes or 2-D meshgrids (row 0 of x and column 0 of y are used); cartesian_grid=False raises NotImplementedError; duplicate
    pairs add; at most 64 orders per axis.  coefs (K,) gives (rows, cols), (B, K) a stack; they are read on the device at launch."""
    return R.sum2d('legendre', coefs, mns, x, y, 'z', cartesian_grid=cartesian_grid)[0]


def legendre_2d_sum_der_xy(coefs, mns, x, y, x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """(z, dz/dx / x_norm, dz/dy / y_norm) of legendre_2d_sum from one launch."""
    return R.sum2d('legendre', coefs, mns, x, y, 'zxy', x_norm, y_norm, cartesian_grid)


def legendre_2d_sum_adjoint(databar, mns, x, y, dx_bar=None, dy_bar=None, x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """The gradient with respect to coefs, in the order of mns, of legendre_2d_sum_der_xy's outputs (databar for z, dx_bar / dy_bar for
    the gradient maps, each optional).  Deterministic: two launches per map, no atomics."""
    return R.adjoint2d('legendre', mns, x, y, databar, dx_bar, dy_bar, x_norm, y_norm, cartesian_grid)
