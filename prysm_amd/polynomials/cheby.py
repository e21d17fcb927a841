"""Chebyshev polynomials of the four kinds (prysm/polynomials/cheby.py) on the device: T, U, V, W share the recurrence
P_k = 2 x P_{k-1} - P_{k-2} and differ in P_1 (x, 2x, 2x - 1, 2x + 1), so each is one table of csrc/recur.hip.  The tensor-product sum
cheby1_2d_sum[_der_xy] is the separable kernel pm_recur2_sum, and cheby1_2d_sum_adjoint its adjoint (the reference has none).
"""
from . import _recur as R

__all__ = [f'cheby{k}{s}' for k in (1, 2, 3, 4) for s in ('', '_seq', '_der', '_der_seq')] + ['cheby1_2d_sum', 'cheby1_2d_sum_der_xy',
                                                                                               'cheby1_2d_sum_adjoint']

cheby1, cheby1_seq, cheby1_der, cheby1_der_seq = R.make_family('cheby1', 'cheby.py:60-123')
cheby2, cheby2_seq, cheby2_der, cheby2_der_seq = R.make_family('cheby2', 'cheby.py:126-189')
cheby3, cheby3_seq, cheby3_der, cheby3_der_seq = R.make_family('cheby3', 'cheby.py:192-255')
cheby4, cheby4_seq, cheby4_der, cheby4_der_seq = R.make_family('cheby4', 'cheby.py:258-321')


def cheby1_2d_sum(coefs, mns, x, y, cartesian_grid=True):
    """sum_k coefs[k] T_m(x) T_n(y) over the pairs (m, n) of mns (cheby.py:324-338), in one launch without a stored basis.  Departures
    from the reference: x and y are 1-D axes or 2-D meshgrids of a Cartesian grid (row 0 of x and column 0 of y are used, as
    coordinates.optimize_xy_separable does) and cartesian_grid=False raises NotImplementedError; duplicate pairs add; at most 64 orders
    per axis.  coefs (K,) gives (rows, cols), (B, K) a stack; they are read on the device when the kernel runs."""
    return R.sum2d('cheby1', coefs, mns, x, y, 'z', cartesian_grid=cartesian_grid)[0]


def cheby1_2d_sum_der_xy(coefs, mns, x, y, x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """(z, dz/dx / x_norm, dz/dy / y_norm) of cheby1_2d_sum (cheby.py:341-362), all three from one launch.  Departures as
    cheby1_2d_sum."""
    return R.sum2d('cheby1', coefs, mns, x, y, 'zxy', x_norm, y_norm, cartesian_grid)


def cheby1_2d_sum_adjoint(databar, mns, x, y, dx_bar=None, dy_bar=None, x_norm=1.0, y_norm=1.0, cartesian_grid=True):
    """The gradient with respect to coefs, in the order of mns, of cheby1_2d_sum_der_xy's outputs: databar is the adjoint of z, dx_bar and
    dy_bar (optional) of the two gradient maps; databar may be None when one of those is given.  A duplicate pair receives its matrix
    entry once per duplicate.  Deterministic: two launches per map, no atomics."""
    return R.adjoint2d('cheby1', mns, x, y, databar, dx_bar, dy_bar, x_norm, y_norm, cartesian_grid)
