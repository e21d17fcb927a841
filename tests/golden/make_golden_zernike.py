"""Generate the Zernike fixture (tests/golden/zernike.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_zernike.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores, all in fp64:
- the index conventions for j = 1 .. 120 (noll_to_nm, fringe_to_nm, ansi_j_to_nm) and, for every (n, m) with n <= 12, zernike_norm,
  nm_to_fringe and nm_to_ansi_j;
- zernike_nm_seq of all 91 modes with n <= 12 on a 17 x 17 grid over [-1.2, 1.2] (the origin, the axes and the corners outside the
  unit disk among its points), with the grid's (x, y) and the (r, t) of cart_to_polar;
- zernike_nm_seq of the 21 modes with n = 20 on a 15 x 15 grid over [-0.7, 0.7] (inside the disk, where they stay O(1));
- zernike_nm of (5, 2) (odd n - |m|: Jacobi order 1) and zernike_nm_seq(norm=False) of four modes on the first grid;
- zernike_sum of two seeded coefficient vectors over the 45 modes with n <= 8, and sum_of_2d_modes_adjoint of their basis with a
  seeded databar, on the first grid.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm.coordinates import cart_to_polar  # noqa: E402
from prysm.polynomials import zernike as Z  # noqa: E402
from prysm.polynomials.fitting import sum_of_2d_modes_adjoint  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def nms_upto(nmax, nmin=0):
    return [(n, m) for n in range(nmin, nmax + 1) for m in range(-n, n + 1, 2)]


def main():
    out = {}
    js = np.arange(1, 121)
    out['j'] = js
    out['noll'] = np.array([Z.noll_to_nm(int(j)) for j in js])
    out['fringe'] = np.array([Z.fringe_to_nm(int(j)) for j in js])
    out['ansi'] = np.array([Z.ansi_j_to_nm(int(j)) for j in js])
    nms12 = nms_upto(12)
    out['nms12'] = np.array(nms12)
    out['norm12'] = np.array([Z.zernike_norm(n, m) for n, m in nms12])
    out['nm_to_fringe12'] = np.array([Z.nm_to_fringe(n, m) for n, m in nms12])
    out['nm_to_ansi12'] = np.array([Z.nm_to_ansi_j(n, m) for n, m in nms12])

    g = np.arange(-8, 9) * 0.15
    x, y = np.meshgrid(g, g)
    r, t = cart_to_polar(x, y)
    out.update(x=x, y=y, r=r, t=t)
    out['seq12'] = Z.zernike_nm_seq(nms12, r, t)

    g20 = np.arange(-7, 8) * 0.1
    x20, y20 = np.meshgrid(g20, g20)
    r20, t20 = cart_to_polar(x20, y20)
    nms20 = nms_upto(20, 20)
    out.update(x20=x20, y20=y20, r20=r20, t20=t20, nms20=np.array(nms20))
    out['seq20'] = Z.zernike_nm_seq(nms20, r20, t20)

    out['odd_nm'] = np.array((5, 2))
    out['odd'] = Z.zernike_nm(5, 2, r, t)
    nms_raw = [(2, 0), (3, 1), (4, -2), (6, 6)]
    out['nms_raw'] = np.array(nms_raw)
    out['seq_raw'] = Z.zernike_nm_seq(nms_raw, r, t, norm=False)

    nms8 = nms_upto(8)
    out['nms8'] = np.array(nms8)
    coefs = np.random.default_rng(11).standard_normal((2, len(nms8)))
    out['coefs'] = coefs
    out['sums'] = np.stack([Z.zernike_sum(c, nms8, x, y) for c in coefs])
    databar = np.random.default_rng(12).standard_normal(x.shape)
    out['databar'] = databar
    out['modes_adj'] = sum_of_2d_modes_adjoint(Z.zernike_nm_seq(nms8, r, t), databar)

    path = os.path.join(HERE, 'zernike.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
