"""Generate the Forbes Q-polynomial fixture (tests/golden/qpoly.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_qpoly.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores, all in fp64:
- Qbfs_seq and Qcon_seq of n = 0 .. 20 on 41 radii u in [0, 1] (0 and 1 included);
- Q2d_seq of every (n, m) with n <= 8, |m| <= 8 on an 11 x 11 grid over [-0.7, 0.7] (inside the unit disk, the origin and the
  axes among its points), with the grid's (x, y) and the (r, t) of cart_to_polar;
- Q2d_seq of the sparse high-order set n = 20, m in {0, +-1, +-2, +-7, +-20} on the same points;
- Q2d(n, +-1) for n = 0 .. 5 one at a time (the |m| = 1 seeds P_0 .. P_3 and the first recurrence steps);
- the scalar helpers g_qbfs, h_qbfs, f_qbfs for n <= 20, and abc_q2d, G_q2d, F_q2d, g_q2d, f_q2d for n <= 20, 1 <= m <= 20 (abc_q2d
  only where its denominator is not zero);
- compute_z_Qbfs of 12 seeded coefficients on the radii, and compute_z_Q2d of seeded coefficients over the n <= 8 modes on the
  points, with the coefficients;
- Q2d_nm_c_to_a_b of two small mode lists (zeros, gaps, sines without cosines), flattened with their lengths.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm.coordinates import cart_to_polar  # noqa: E402
from prysm.polynomials import qpoly as Q  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _flat(lists):
    """a list of lists as (concatenated values, lengths)"""
    return np.array([v for row in lists for v in row], dtype=np.float64), np.array([len(row) for row in lists], dtype=np.int64)


def main():
    out = {}
    ns = list(range(21))
    u = np.linspace(0, 1, 41)
    out['u'] = u
    out['qbfs_seq'] = Q.Qbfs_seq(ns, u)
    out['qcon_seq'] = Q.Qcon_seq(ns, u)

    g = np.arange(-5, 6) * 0.14
    x, y = np.meshgrid(g, g)
    r, t = cart_to_polar(x, y)
    out.update(x=x, y=y, r=r, t=t)
    nms8 = [(n, m) for n in range(9) for m in range(-8, 9)]
    out['nms8'] = np.array(nms8)
    out['q2d_seq8'] = Q.Q2d_seq(nms8, r, t)
    nms20 = [(20, m) for m in (0, 1, -1, 2, -2, 7, -7, 20, -20)]
    out['nms20'] = np.array(nms20)
    out['q2d_seq20'] = Q.Q2d_seq(nms20, r, t)
    singles = [(n, m) for m in (1, -1) for n in range(6)]
    out['nms_single'] = np.array(singles)
    out['q2d_single'] = np.stack([Q.Q2d(n, m, r, t) for n, m in singles])

    out['bfs_fgh'] = np.array([[Q.f_qbfs(n), Q.g_qbfs(n), Q.h_qbfs(n)] for n in ns])
    hm = [(n, m) for n in range(21) for m in range(1, 21)]
    out['helper_nm'] = np.array(hm)
    out['q2d_FGfg'] = np.array([[Q.F_q2d(n, m), Q.G_q2d(n, m), Q.f_q2d(n, m), Q.g_q2d(n, m)] for n, m in hm])
    abc_nm = [(n, m) for n, m in hm if (4 * n * n - 1) * (m + n - 2) * (m + 2 * n - 3) != 0]
    out['abc_nm'] = np.array(abc_nm)
    out['abc'] = np.array([Q.abc_q2d(n, m) for n, m in abc_nm])

    rng = np.random.default_rng(21)
    cbfs = rng.standard_normal(12)
    out['zbfs_coefs'] = cbfs
    out['zbfs'] = Q.compute_z_Qbfs(cbfs, u, u * u)
    c8 = rng.standard_normal(len(nms8))
    out['z2d_coefs'] = c8
    cm0, ams, bms = Q.Q2d_nm_c_to_a_b(nms8, c8)
    out['z2d'] = Q.compute_z_Q2d(cm0, ams, bms, r, t)

    examples = [([(0, 0), (3, 0), (2, 2), (1, -3), (4, 2), (0, -1)], [1.0, 2.0, 3.0, 4.0, 0.0, 5.0]),
                ([(2, -2), (0, 1), (1, 0), (5, 1), (2, -2)], [0.5, 0.0, -1.5, 2.5, 7.0])]
    for i, (nms, cs) in enumerate(examples):
        cm0, ams, bms = Q.Q2d_nm_c_to_a_b(nms, cs)
        out[f'ab{i}_nms'] = np.array(nms)
        out[f'ab{i}_coefs'] = np.array(cs)
        out[f'ab{i}_cm0'] = np.array(cm0, dtype=np.float64)
        out[f'ab{i}_a'], out[f'ab{i}_alen'] = _flat(ams)
        out[f'ab{i}_b'], out[f'ab{i}_blen'] = _flat(bms)

    path = os.path.join(HERE, 'qpoly.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
