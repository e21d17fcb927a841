"""XY monomials x^m y^n (prysm/polynomials/xy.py) on the device.  On a Cartesian grid every function is separable: the sequences are
outer products of two small power tables (pm_recur2_outer), the sums the separable kernel pm_recur2_sum with the monomial table, whose
derivative track gives m x^(m-1).  Departures from the reference, common to all: x and y are 1-D axes or 2-D meshgrids (row 0 of x
and column 0 of y are used, as coordinates.optimize_xy_separable does) and cartesian_grid=False raises NotImplementedError.
"""
from . import _recur as R
from .recur_plan import xy_j_to_mn  # noqa: F401

__all__ = ['xy_j_to_mn', 'xy', 'xy_seq', 'xy_der_x', 'xy_der_x_seq', 'xy_der_y', 'xy_der_y_seq', 'xy_der_xy', 'xy_der_xy_seq', 'xy_sum',
           'xy_sum_der_xy', 'xy_sum_adjoint']


def xy_seq(mns, x, y, cartesian_grid=True):
    """x^m y^n for the pairs of mns, (len(mns), rows, cols) in their order (xy.py:218-243)."""
    return R.outer_seq(mns, x, y, False, False, cartesian_grid)


def xy_der_x_seq(mns, x, y, cartesian_grid=True):
    """m x^(m-1) y^n for the pairs of mns (xy.py:246-262)."""
    return R.outer_seq(mns, x, y, True, False, cartesian_grid)


def xy_der_y_seq(mns, x, y, cartesian_grid=True):
    """n x^m y^(n-1) for the pairs of mns (xy.py:265-281)."""
    return R.outer_seq(mns, x, y, False, True, cartesian_grid)


def xy_der_xy_seq(mns, x, y, cartesian_grid=True):
    """m n x^(m-1) y^(n-1) for the pairs of mns (xy.py:284-300)."""
    return R.outer_seq(mns, x, y, True, True, cartesian_grid)


def xy(m, n, x, y, cartesian_grid=True):
    """x^m y^n on the grid (xy.py:30-57)."""
    return xy_seq(((m, n),), x, y, cartesian_grid)[0]


def xy_der_x(m, n, x, y, cartesian_grid=True):
    """d/dx of x^m y^n (xy.py:60-93)."""
    return xy_der_x_seq(((m, n),), x, y, cartesian_grid)[0]


def xy_der_y(m, n, x, y, cartesian_grid=True):
    """d/dy of x^m y^n (xy.py:96-128)."""
    return xy_der_y_seq(((m, n),), x, y, cartesian_grid)[0]


def xy_der_xy(m, n, x, y, cartesian_grid=True):
    """d^2/dxdy of x^m y^n (xy.py:131-163)."""
    return xy_der_xy_seq(((m, n),), x, y, cartesian_grid)[0]


def xy_sum(coefs, mns, x, y, cartesian_grid=True):
    """sum_k coefs[k] x^m y^n over the pairs of mns (xy.py:355-363), in one launch without power tables.  Duplicate pairs add into one
    matrix entry, as the reference's _xy_coefficient_matrices does; at most 64 orders per axis.  coefs (K,) or (B, K)."""
    return R.sum2d('monomial', coefs, mns, x, y, 'z', cartesian_grid=cartesian_grid)[0]


def xy_sum_der_xy(coefs, mns, x, y, cartesian_grid=True):
    """(z, dz/dx, dz/dy) of xy_sum (xy.py:366-383): the reference's three matrix products as one launch."""
    return R.sum2d('monomial', coefs, mns, x, y, 'zxy', cartesian_grid=cartesian_grid)


def xy_sum_adjoint(databar, mns, x, y, dx_bar=None, dy_bar=None, cartesian_grid=True):
    """The gradient with respect to coefs, in the order of mns, of xy_sum_der_xy's outputs (databar for z, dx_bar / dy_bar for the
    gradient maps, each optional; the reference has no adjoint).  A duplicate pair receives its matrix entry once per duplicate.
    Deterministic: two launches per map, no atomics."""
    return R.adjoint2d('monomial', mns, x, y, databar, dx_bar, dy_bar, cartesian_grid=cartesian_grid)
