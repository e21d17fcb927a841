"""What tests/test_fibers_host.py, tests/test_gpu_fibers.py and tests/golden/make_golden_fibers.py share: the grids, the cases, the
incident fields, access to tests/golden/fibers.npz and the bounds.

Bounds (eps is that of the precision under test, V the fibre's V-number):
  mode values   |got - ref| <= 16 (1 + V) eps max|mode_k|, per mode.  |J'| and the cladding's logarithmic slope are <= 1, so two roundings
                of an argument x <= V move a value by <= 2 V eps; the division by the normaliser spreads its relative error over the mode,
                hence max|mode_k|.  The reference's own functions with every intermediate rounded to float32 sit at 0.91 (1 + V) eps.
  J_l           absolute 8 eps max(1, x), plus what scipy itself misses against 40-digit arithmetic at that point (stored)
  e^x K_l       relative 8 (1 + l) eps, plus the same (scipy's e^x K_0 is 13 to 16 eps off around x = 2)
  roots         |U - U_ref| <= 2e-12 / |df_ref| + 16 eps V: both solvers stop at |f| < 1e-12
  coupling      |eta - eta_ref| <= 4 npts eps + 2 * 16 (1 + V) eps: eta <= 1, a sum of npts terms is off by at most npts eps
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fibers.npz')
A = 4.0                                    # core radius
VS = (1.5, 2.0, 2.41, 3.9, 5.5, 12.0, 30.0)
COUNTS = (1, 1, 3, 6, 8, 38, 228)
# case -> (V, the l kept, None for all)
CASES = {'V2.41': (2.41, None), 'V3.9': (3.9, None), 'V5.5': (5.5, None), 'V12': (12.0, None), 'V30s': (30.0, (0, 22, -22, 25, -25))}
GRIDS = ('g33', 'g48')
TAB_L = (0, 1, 2, 5, 8, 25)
SMF_V = 2.0
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def vtag(V):
    return ('%g' % V).replace('.', 'p')


def grid_xy(name):
    """(x, y) in float64.  g33: 33 x 31 over a diameter of 30 (pitch 0.9375 x 1); g48: 48 x 40 (pitch 0.625 x 0.8, 30 x 32 across -- a
    pitch of 0.75 has no sample at r == a).  Both hold r = 0 and (x, y) = (+-4, 0) with r == a to the bit."""
    if name == 'g33':
        yv, xv = np.linspace(-15, 15, 33), np.linspace(-15, 15, 31)
    else:
        yv, xv = (np.arange(48) - 24) * 5 / 8, (np.arange(40) - 20) * 4 / 5
    x, y = np.meshgrid(xv, yv)
    return x, y


def grid(name, dtype=np.float64):
    """(r, t) of the grid in `dtype`: the float32 grid is the float64 grid rounded, so that input rounding is not charged to anybody"""
    x, y = grid_xy(name)
    r, t = np.sqrt(x * x + y * y), np.arctan2(y, x)
    assert (r == 0).any() and (r == A).any()
    return r.astype(dtype), t.astype(dtype)


def incident(name, dtype=np.float64):
    """a tilted Gaussian at the fibre face, complex, in the complex type of `dtype` (rounded from float64)"""
    x, y = grid_xy(name)
    E = np.exp(-(x * x + y * y) / 3.5 ** 2) * np.exp(2j * np.pi * (0.021 * x - 0.013 * y))
    return E.astype(np.complex64 if np.dtype(dtype) == np.float32 else np.complex128)


def second_field(name, dtype=np.float64):
    """the other complex field of the overlap case: an offset, elliptical, defocused Gaussian"""
    x, y = grid_xy(name)
    E = np.exp(-((x - 0.7) ** 2 / 9 + (y + 0.4) ** 2 / 5)) * np.exp(1j * (0.05 * (x * x + y * y) + 0.3))
    return E.astype(np.complex64 if np.dtype(dtype) == np.float32 else np.complex128)


def mode_dict(case):
    """the mode dictionary of a case with the REFERENCE's b, in the reference's key order"""
    g = golden()
    keys, counts, b = g[case + '_keys'], g[case + '_counts'], g[case + '_b']
    out, k = {}, 0
    for l, n in zip(keys, counts):
        out[int(l)] = b[k:k + n].copy()
        k += n
    return out


def suffix(dtype):
    return '32' if np.dtype(dtype) == np.float32 else '64'


def stack(case, gname, dtype):
    """(idx, ref): the reference's modes of a case on a grid, float64, at the flat point indices idx.  The float32 reference is stored as
    its float32 difference from the float64 one (it is tiny, so nothing is lost)."""
    g = golden()
    ref = g[f'{case}_{gname}_stack']
    if np.dtype(dtype) == np.float32:
        ref = ref + g[f'{case}_{gname}_delta32']
    return g[f'{case}_{gname}_idx'], ref


def eps(dtype):
    return float(np.finfo(dtype).eps)


def mode_bound(V, dtype, ref):
    """per mode (rows of ref)"""
    return 16 * (1 + V) * eps(dtype) * np.max(np.abs(ref), axis=-1)


def coupling_bound(V, dtype, npts):
    return 4 * npts * eps(dtype) + 2 * 16 * (1 + V) * eps(dtype)


def check_modes(case, gname, dtype, got, label=''):
    """got: (nmodes, npts) of the whole grid against the fixture; prints the worst ratio to the bound before asserting"""
    V = CASES[case][0]
    idx, ref = stack(case, gname, dtype)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape[0], -1)[:, idx]
    dev = np.max(np.abs(got - ref), axis=-1)
    bound = mode_bound(V, dtype, ref)
    worst = int(np.argmax(dev / bound))
    print(f'{label}{case} {gname} {np.dtype(dtype).name}: worst mode {worst}, deviation {dev[worst]:.3e}, bound {bound[worst]:.3e} '
          f'({dev[worst] / bound[worst]:.3f})')
    assert np.all(np.isfinite(got)) and np.all(dev <= bound), (case, gname, worst, dev[worst], bound[worst])
