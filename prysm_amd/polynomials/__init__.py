"""Polynomials (prysm/polynomials) on the device: the Zernike basis, its matrix-free sum and adjoint, and mode sums over a stored basis.

    from prysm_amd.polynomials import zernike_sum, zernike_sum_adjoint, noll_to_nm
    nms = [noll_to_nm(j) for j in range(1, 37)]
    opd = zernike_sum(coefs, nms, x, y)                 # (rows, cols); coefs may live on the device and change between calls
    coefs_bar = zernike_sum_adjoint(opd_bar, nms, x, y)  # (K,)

The Forbes Q polynomials (Qbfs, Qcon, Q2D) follow the same pattern: Q2d_seq / Q2d_sum / Q2d_sum_adjoint and their radial siblings.

The families defined by a three-term recurrence -- Jacobi, Chebyshev (four kinds), Legendre, Hermite (He, H), Laguerre, Dickson (two
kinds) and the XY monomials -- carry the reference's names (cheby1_seq, legendre_der_seq, jacobi_radial_sum_der_xy, xy_sum_der_xy, ...);
on a Cartesian grid their tensor-product sums and adjoints are one fused kernel each:

    z, zx, zy = legendre_2d_sum_der_xy(coefs, mns, x, y)        # mns: (m, n) pairs, x / y: axes or meshgrids
    coefs_bar = legendre_2d_sum_adjoint(z_bar, mns, x, y, dx_bar=zx_bar, dy_bar=zy_bar)
"""
from .zernike import (zernike_norm, noll_to_nm, fringe_to_nm, nm_to_fringe, nm_to_ansi_j, ansi_j_to_nm, zernike_nm,  # noqa: F401
                      zernike_nm_seq, zernike_sum, zernike_sum_adjoint)
from .qpoly import (g_qbfs, h_qbfs, f_qbfs, abc_q2d, G_q2d, F_q2d, g_q2d, f_q2d, Q2d_nm_c_to_a_b, Qbfs, Qbfs_seq, Qcon,  # noqa: F401
                    Qcon_seq, Q2d, Q2d_seq, compute_z_Qbfs, compute_z_Q2d, Q2d_sum, Q2d_sum_adjoint, Qcon_sum, Qcon_sum_adjoint)
from .fitting import (sum_of_2d_modes, sum_of_2d_modes_adjoint, lstsq, normalize_modes, orthogonalize_modes, hopkins,  # noqa: F401
                      prepare_lstsq, ModalFit)
from . import cheby as _cheby, dickson as _dickson, hermite as _hermite, jacobi as _jacobi, laguerre as _laguerre, legendre as _legendre, xy as _xy
from .cheby import *  # noqa: F401,F403
from .dickson import *  # noqa: F401,F403
from .hermite import *  # noqa: F401,F403
from .jacobi import *  # noqa: F401,F403
from .laguerre import *  # noqa: F401,F403
from .legendre import *  # noqa: F401,F403
from .xy import *  # noqa: F401,F403

__all__ = ['zernike_norm', 'noll_to_nm', 'fringe_to_nm', 'nm_to_fringe', 'nm_to_ansi_j', 'ansi_j_to_nm', 'zernike_nm', 'zernike_nm_seq',
           'zernike_sum', 'zernike_sum_adjoint', 'sum_of_2d_modes', 'sum_of_2d_modes_adjoint', 'lstsq', 'normalize_modes', 'orthogonalize_modes',
           'hopkins', 'prepare_lstsq', 'ModalFit',
           'g_qbfs', 'h_qbfs', 'f_qbfs', 'abc_q2d', 'G_q2d', 'F_q2d', 'g_q2d', 'f_q2d', 'Q2d_nm_c_to_a_b', 'Qbfs', 'Qbfs_seq', 'Qcon',
           'Qcon_seq', 'Q2d', 'Q2d_seq', 'compute_z_Qbfs', 'compute_z_Q2d', 'Q2d_sum', 'Q2d_sum_adjoint', 'Qcon_sum', 'Qcon_sum_adjoint']
# the recurrence families (csrc/recur.hip): Jacobi, Chebyshev, Legendre, Hermite, Laguerre, Dickson, XY -- every name their modules export
for _m in (_cheby, _dickson, _hermite, _jacobi, _laguerre, _legendre, _xy):
    __all__ += [_n for _n in _m.__all__ if _n not in ('weight', 'recurrence_abc')]
