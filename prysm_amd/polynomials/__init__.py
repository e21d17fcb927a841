"""Polynomials (prysm/polynomials) on the device: the Zernike basis, its matrix-free sum and adjoint, and mode sums over a stored basis.

    from prysm_amd.polynomials import zernike_sum, zernike_sum_adjoint, noll_to_nm
    nms = [noll_to_nm(j) for j in range(1, 37)]
    opd = zernike_sum(coefs, nms, x, y)                 # (rows, cols); coefs may live on the device and change between calls
    coefs_bar = zernike_sum_adjoint(opd_bar, nms, x, y)  # (K,)
"""
from .zernike import (zernike_norm, noll_to_nm, fringe_to_nm, nm_to_fringe, nm_to_ansi_j, ansi_j_to_nm, zernike_nm,  # noqa: F401
                      zernike_nm_seq, zernike_sum, zernike_sum_adjoint)
from .fitting import sum_of_2d_modes, sum_of_2d_modes_adjoint  # noqa: F401

__all__ = ['zernike_norm', 'noll_to_nm', 'fringe_to_nm', 'nm_to_fringe', 'nm_to_ansi_j', 'ansi_j_to_nm', 'zernike_nm', 'zernike_nm_seq',
           'zernike_sum', 'zernike_sum_adjoint', 'sum_of_2d_modes', 'sum_of_2d_modes_adjoint']
