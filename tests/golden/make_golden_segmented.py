"""Generate the segmented-aperture fixture (tests/golden/segmented.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_segmented.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores, for four CompositeHexagonalAperture cases (prefix c1_ .. c4_), in fp64:
- the case: grid size N, diameter, rings, segment diameter / separation / angle, exclude, the Noll indices or monomial orders, the
  normalisation radius (0: the default), and the 1-D x / y sample vectors (the grid is their meshgrid);
- the constructor's attributes: vtov, all_centers, windows (y0, y1, x0, x1), segment_ids, the local-coordinate corners
  (local_x[0, 0], local_y[0, 0]), the local masks' sums and [::3, ::3] samples (concatenated), amp[::3, ::3];
- the grid-sharing groups of prepare_opd_bases as the grid source of each segment (the first segment whose basis is the same object);
- compose_opd of two seeded coefficient sets, the second added into out = default_rng(seed_out).standard_normal(shape), sampled
  every `sub` rows and columns;
- the adjoint sum_p mask * basis * g over each window, from the reference's own opd_bases, g = default_rng(seed_g).standard_normal.

Cases: 1 JWST-like (rings 2, exclude 0, angle 90, Noll 1-6, 256^2); 2 rings 1, angle 0, centre included; 3 an aperture wider than
the grid (clamped windows); 4 the stored route: x / y monomials through a lambda, separate x and y normalisation radii.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm.coordinates import make_xy_grid  # noqa: E402
from prysm.polynomials import zernike_nm_seq, noll_to_nm  # noqa: E402
from prysm.segmented import CompositeHexagonalAperture  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

MONO = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 1)]


monomials = lambda orders, x, y: [x ** a * y ** b for a, b in orders]  # noqa: E731  (numpy and torch alike)


CASES = [
    dict(N=256, D=6.628, rings=2, sd=1.32, sep=0.007, angle=90, exclude=(0,), noll=6, nr=0.0, sub=3, seed=1),
    dict(N=192, D=4.5, rings=1, sd=1.32, sep=0.05, angle=0, exclude=(), noll=8, nr=0.0, sub=3, seed=2),
    dict(N=128, D=3.2, rings=1, sd=1.32, sep=0.05, angle=90, exclude=(), noll=4, nr=0.0, sub=2, seed=3),
    dict(N=160, D=5.0, rings=1, sd=1.32, sep=0.02, angle=90, exclude=(2,), noll=0, nr=(0.7, 0.9), sub=2, seed=4),
]


def main():
    out = {}
    for i, c in enumerate(CASES, 1):
        p = f'c{i}_'
        x, y = make_xy_grid(c['N'], diameter=c['D'])
        ap = CompositeHexagonalAperture(x, y, c['rings'], c['sd'], c['sep'], segment_angle=c['angle'], exclude=c['exclude'])
        S = len(ap.segment_ids)
        out.update({p + 'N': c['N'], p + 'D': c['D'], p + 'rings': c['rings'], p + 'sd': c['sd'], p + 'sep': c['sep'],
                    p + 'angle': c['angle'], p + 'exclude': np.array(c['exclude'], dtype=int), p + 'sub': c['sub'],
                    p + 'xv': x[0].copy(), p + 'yv': y[:, 0].copy()})
        out[p + 'vtov'] = ap.vtov
        out[p + 'centers'] = np.array(ap.all_centers, dtype=float).reshape(-1, 2)
        out[p + 'windows'] = np.array([(w[0].start, w[0].stop, w[1].start, w[1].stop) for w in ap.windows])
        out[p + 'ids'] = np.array(ap.segment_ids, dtype=int)
        out[p + 'corners'] = np.array([(lx[0, 0], ly[0, 0]) for lx, ly in ap.local_coords])
        out[p + 'mask_sum'] = np.array([m.sum() for m in ap.local_masks])
        out[p + 'mask_sub'] = np.concatenate([m[::3, ::3].ravel() for m in ap.local_masks])
        out[p + 'amp_sub'] = ap.amp[::3, ::3]
        if c['noll']:
            orders = [noll_to_nm(j) for j in range(1, c['noll'] + 1)]
            grids, bases = ap.prepare_opd_bases(zernike_nm_seq, orders)
            out[p + 'nms'] = np.array(orders)
        else:
            orders = MONO
            grids, bases = ap.prepare_opd_bases(monomials, orders, normalization_radius=c['nr'])
            out[p + 'orders'] = np.array(orders)
            out[p + 'nr'] = np.array(c['nr'])
        out[p + 'src'] = np.array([next(j for j in range(S) if bases[j] is bases[s]) for s in range(S)])
        K = len(orders)
        rng = np.random.default_rng(c['seed'])
        coefs = rng.standard_normal((2, S, K))
        out[p + 'coefs'] = coefs
        sub = c['sub']
        out[p + 'opd1'] = ap.compose_opd(coefs[0])[::sub, ::sub]
        seed_out, seed_g = 100 + c['seed'], 200 + c['seed']
        base = np.random.default_rng(seed_out).standard_normal(x.shape)
        out[p + 'seed_out'], out[p + 'seed_g'] = seed_out, seed_g
        out[p + 'opd2'] = ap.compose_opd(coefs[1], out=base.copy())[::sub, ::sub]
        g = np.random.default_rng(seed_g).standard_normal(x.shape)
        out[p + 'adj'] = np.array([(np.asarray(b) * m * g[w]).reshape(K, -1).sum(axis=1)
                                   for b, m, w in zip(bases, ap.local_masks, ap.windows)])
    path = os.path.join(HERE, 'segmented.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
