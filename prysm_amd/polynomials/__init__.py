"""Polynomials (prysm/polynomials) on the device: the Zernike basis, its matrix-free sum and adjoint, and mode sums over a stored basis.

    from prysm_amd.polynomials import zernike_sum, zernike_sum_adjoint, noll_to_nm
    nms = [noll_to_nm(j) for j in range(1, 37)]
    opd = zernike_sum(coefs, nms, x, y)                 # (rows, cols); coefs may live on the device and change between calls
    coefs_bar = zernike_sum_adjoint(opd_bar, nms, x, y)  # (K,)

The Forbes Q polynomials (Qbfs, Qcon, Q2D) follow the same pattern: Q2d_seq / Q2d_sum / Q2d_sum_adjoint and their radial siblings.
"""
from .zernike import (zernike_norm, noll_to_nm, fringe_to_nm, nm_to_fringe, nm_to_ansi_j, ansi_j_to_nm, zernike_nm,  # noqa: F401
                      zernike_nm_seq, zernike_sum, zernike_sum_adjoint)
from .qpoly import (g_qbfs, h_qbfs, f_qbfs, abc_q2d, G_q2d, F_q2d, g_q2d, f_q2d, Q2d_nm_c_to_a_b, Qbfs, Qbfs_seq, Qcon,  # noqa: F401
                    Qcon_seq, Q2d, Q2d_seq, compute_z_Qbfs, compute_z_Q2d, Q2d_sum, Q2d_sum_adjoint, Qcon_sum, Qcon_sum_adjoint)
from .fitting import sum_of_2d_modes, sum_of_2d_modes_adjoint  # noqa: F401

__all__ = ['zernike_norm', 'noll_to_nm', 'fringe_to_nm', 'nm_to_fringe', 'nm_to_ansi_j', 'ansi_j_to_nm', 'zernike_nm', 'zernike_nm_seq',
           'zernike_sum', 'zernike_sum_adjoint', 'sum_of_2d_modes', 'sum_of_2d_modes_adjoint',
           'g_qbfs', 'h_qbfs', 'f_qbfs', 'abc_q2d', 'G_q2d', 'F_q2d', 'g_q2d', 'f_q2d', 'Q2d_nm_c_to_a_b', 'Qbfs', 'Qbfs_seq', 'Qcon',
           'Qcon_seq', 'Q2d', 'Q2d_seq', 'compute_z_Qbfs', 'compute_z_Q2d', 'Q2d_sum', 'Q2d_sum_adjoint', 'Qcon_sum', 'Qcon_sum_adjoint']
