"""Generate the fixture of the recurrence families (tests/golden/recur.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_recur.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores, all in fp64:
- the 1-D families: *_seq and *_der_seq of the orders 0 .. 30 and of the sparse orders [2, 5, 30] on 65 points --
  linspace(-1, 1) for cheby1 .. cheby4, legendre, dickson1 / dickson2 (alpha = 0.75) and jacobi (0, 2), (1/2, -1/2), (0, 0);
  linspace(-3, 3) for hermite_He / hermite_H; linspace(0, 12) for laguerre (alpha = 1.5) -- under '<case>_seq', '<case>_der_seq',
  '<case>_sparse_seq', '<case>_sparse_der_seq'; jacobi_sum_clenshaw of 12 seeded weights for jacobi (0, 2); recurrence_abc of
  n = 0 .. 10 for the three Jacobi cases;
- the radial sums: jacobi_radial_sum_der_xy for (alpha, beta) = (0, 2), orders 0 .. 10, R = 1.3 on an 11 x 11 grid over
  [-0.9, 0.9] (the origin among its points), with seeded coefficients;
- the 2-D sums: cheby1_2d_sum_der_xy (x_norm = 2, y_norm = 0.5) and xy_sum_der_xy for mns = [(m, n) for m < 9 for n < 7]
  with seeded coefficients on a grid of 33 rows x 29 columns over [-1, 1]; xy_j_to_mn of 1 .. 40;
- XY: xy_seq, xy_der_x_seq, xy_der_y_seq and xy_der_xy_seq of xy_j_to_mn(j), j = 1 .. 21 ('xy_mns'), on that grid.
About 1.1 MB raw, 0.4 MB compressed.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm import polynomials as P  # noqa: E402
from prysm.polynomials.jacobi import recurrence_abc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

# case -> (the reference's family name, shape parameters, the interval's key)
CASES = {
    'cheby1': ('cheby1', (), 'x_unit'), 'cheby2': ('cheby2', (), 'x_unit'), 'cheby3': ('cheby3', (), 'x_unit'),
    'cheby4': ('cheby4', (), 'x_unit'), 'legendre': ('legendre', (), 'x_unit'),
    'hermite_He': ('hermite_He', (), 'x_hermite'), 'hermite_H': ('hermite_H', (), 'x_hermite'),
    'laguerre': ('laguerre', (1.5,), 'x_laguerre'),
    'dickson1': ('dickson1', (0.75,), 'x_unit'), 'dickson2': ('dickson2', (0.75,), 'x_unit'),
    'jacobi_0_2': ('jacobi', (0.0, 2.0), 'x_unit'), 'jacobi_h_mh': ('jacobi', (0.5, -0.5), 'x_unit'),
    'jacobi_0_0': ('jacobi', (0.0, 0.0), 'x_unit'),
}
SPARSE = [2, 5, 30]


def main():
    out = {'x_unit': np.linspace(-1, 1, 65), 'x_hermite': np.linspace(-3, 3, 65), 'x_laguerre': np.linspace(0, 12, 65)}
    ns = list(range(31))
    for case, (fam, params, xk) in CASES.items():
        seq, der = getattr(P, fam + '_seq'), getattr(P, fam + '_der_seq')
        x = out[xk]
        out[case + '_seq'] = np.asarray(seq(ns, *params, x))
        out[case + '_der_seq'] = np.asarray(der(ns, *params, x))
        out[case + '_sparse_seq'] = np.asarray(seq(SPARSE, *params, x))
        out[case + '_sparse_der_seq'] = np.asarray(der(SPARSE, *params, x))
    rng = np.random.default_rng(31)
    s = rng.standard_normal(12)
    out['clenshaw_s'] = s
    out['clenshaw'] = P.jacobi_sum_clenshaw(s, 0.0, 2.0, out['x_unit'])
    abc_args = [(n, a, b) for (a, b) in ((0.0, 2.0), (0.5, -0.5), (0.0, 0.0)) for n in range(11)]
    out['abc_args'] = np.array(abc_args)
    out['abc'] = np.array([recurrence_abc(int(n), a, b) for n, a, b in abc_args], dtype=np.float64)

    g = np.arange(-5, 6) * 0.18
    rx, ry = np.meshgrid(g, g)
    rc = rng.standard_normal(11)
    z, zx, zy = P.jacobi_radial_sum_der_xy(rc, range(11), 0.0, 2.0, rx, ry, 1.3)
    out.update(rad_x=rx, rad_y=ry, rad_coefs=rc, rad_z=z, rad_zx=zx, rad_zy=zy)

    gx, gy = np.linspace(-1, 1, 29), np.linspace(-1, 1, 33)
    X, Y = np.meshgrid(gx, gy)
    mns = [(m, n) for m in range(9) for n in range(7)]
    c2 = rng.standard_normal(len(mns))
    out.update(grid_x=gx, grid_y=gy, mns=np.array(mns), c2d=c2)
    out['cheby_z'], out['cheby_zx'], out['cheby_zy'] = P.cheby1_2d_sum_der_xy(c2, mns, X, Y, x_norm=2.0, y_norm=0.5)
    out['xy_z'], out['xy_zx'], out['xy_zy'] = P.xy_sum_der_xy(c2, mns, X, Y)
    out['j_to_mn'] = np.array([P.xy_j_to_mn(j) for j in range(1, 41)])

    xy_mns = [P.xy_j_to_mn(j) for j in range(1, 22)]
    out['xy_mns'] = np.array(xy_mns)
    for name in ('xy_seq', 'xy_der_x_seq', 'xy_der_y_seq', 'xy_der_xy_seq'):
        out[name] = np.asarray(getattr(P, name)(xy_mns, X, Y))
        assert out[name].shape == (21, 33, 29)
    path = os.path.join(HERE, 'recur.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
