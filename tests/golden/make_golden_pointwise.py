"""Generate the map-sampling fixture (tests/golden/pointwise.npz) with scipy on the CPU.

    python tests/golden/make_golden_pointwise.py

For a 9 x 11 and a 32 x 32 complex map it stores scipy.ndimage.map_coordinates(order 0 .. 5, mode='nearest') of the real and the
imaginary part at a separable set of sample points:
- `<name>_map`: the map, complex64 (so that the complex64 and the complex128 kernels read the same values);
- `<name>_row`, `<name>_col`: the row coordinate of every output row and the column coordinate of every output column, in map samples;
- `<name>_o<order>`: the (len(row), len(col)) complex128 result.

The coordinates are multiples of 2^-10 and the tests use dx = 0.5 and dyadic centres, so the kernel's (xf - cx) / dx + n / 2 is exact
in float32 and in float64 and both precisions sample at exactly these points.  They hold 0 and n - 1 exactly, points 2^-10 inside
and 2^-10 outside either end, points far outside, and odd multiples of 1/16 in between (never a half-integer, where the nearest
sample of order 0 would hang on the last bit).
"""
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = 2.0 ** -10


def axis_points(rng, n, count):
    edge = [-TINY, 0.0, TINY, n - 1 - TINY, float(n - 1), n - 1 + TINY, -3.0625, n + 1.5625]
    inner = (2 * rng.integers(0, 8 * (n - 1), size=count - len(edge)) + 1) / 16.0
    pts = np.array(edge + list(inner))
    rng.shuffle(pts)
    return pts


def main():
    rng = np.random.default_rng(20261017)
    out = {}
    for name, (ny, nx) in (('small', (9, 11)), ('square', (32, 32))):
        m = (rng.standard_normal((ny, nx)) + 1j * rng.standard_normal((ny, nx))).astype(np.complex64)
        row, col = axis_points(rng, ny, 11), axis_points(rng, nx, 13)
        rr, cc = np.meshgrid(row, col, indexing='ij')
        out[f'{name}_map'], out[f'{name}_row'], out[f'{name}_col'] = m, row, col
        m64 = m.astype(np.complex128)
        for order in range(6):
            re = ndimage.map_coordinates(m64.real, [rr, cc], order=order, mode='nearest')
            im = ndimage.map_coordinates(m64.imag, [rr, cc], order=order, mode='nearest')
            out[f'{name}_o{order}'] = re + 1j * im
    path = os.path.join(HERE, 'pointwise.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
