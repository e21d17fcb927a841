"""Generate the geometry / coordinates fixture (tests/golden/geometry.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_geometry.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores, all in fp64:
- make_xy_grid for even, odd and rectangular shapes with dx and with diameter, as grids (`grid_<i>_x/y`) and vectors, with the
  arguments in `grids` (JSON);
- cart_to_polar / polar_to_cart on the 48 x 64 grid and on a warped copy of it;
- the coordinate sets the cases use: `A` a 30 x 40 grid (dx 0.1731), `B` the 48 x 64 grid (dx 0.1084), `C` a 65 x 65 grid (dx 0.1084),
  each as vectors `<set>_xv`, `<set>_yv` (the meshgrid is their outer broadcast), and `AW`, a WARPED, non-separable copy of A;
- `cases` (JSON): a list of {name, fn, kw, coords, form} -- the reference function, its keyword arguments, the coordinate set and
  the form the coordinates are passed in ('grid' meshgrids, 'vec' 1-D vectors, 'warp' the warped arrays, 'r' the radial coordinate of
  the set) -- and per case `d_<name>`, the reference's signed distance (for gaussian: its value; for offset_circle, which returns a
  mask only: hypot(x - x0, y - y0) - radius).  Masks are `d <= 0` and coverage is antialias(d, dx) = clip(0.5 - d / dx, 0, 1) by the
  reference's own definitions (asserted here for every case), so only the composites store them too (`mask_<name>`, `aa_<name>`);
- two composites built with the reference's union / intersect / subtract: `four` (circle & hexagon - obscuration - spider) and
  `ring` (six hexagons), on B and C.

Asserted for every stored case, so that the reference alone stays inside the mask rule's cap (tests/test_gpu_geometry.py): no pixel
has |d| <= 1e-12 max|d|; at most 0.5 % of the pixels have |d| <= 5e-5 max|d|; the reference run on float32-rounded coordinates
stays within 5e-5 max|d64| of the float64 run.  (rotated_ellipse_sdf is -1e15 at the origin by construction: max|d| leaves the origin
out and the origin is compared relatively.)  If an assertion fails, change the parameters, not the tolerance.
"""
import json
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm import geometry as RG  # noqa: E402
from prysm.coordinates import make_xy_grid, cart_to_polar, polar_to_cart  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

PENTAGON = [(-2.0137, -1.5113), (2.2171, -1.7319), (2.5113, 1.9171), (0.2137, 0.3113), (-1.8171, 2.1137)]      # concave at vertex 3
SETS = {'A': ((30, 40), 0.1731), 'B': ((48, 64), 0.1084), 'C': ((65, 65), 0.1084)}

CASES = [
    ('circle', 'circle_sdf', dict(radius=3.0137), 'B', 'r'),
    ('circle_warp', 'circle_sdf', dict(radius=2.0137), 'AW', 'r'),
    ('annulus', 'annulus_sdf', dict(rin=0.7113, rout=3.0137), 'A', 'r'),
    ('rect0', 'rectangle_sdf', dict(width=1.2345, height=0.6789), 'A', 'grid'),
    ('rect0_vec', 'rectangle_sdf', dict(width=1.2345), 'A', 'vec'),
    ('rect90', 'rectangle_sdf', dict(width=1.2345, height=0.6789, angle=90), 'AW', 'warp'),
    ('rect31', 'rectangle_sdf', dict(width=1.2345, height=0.6789, angle=31.7), 'A', 'grid'),
    ('rect31_vec', 'rectangle_sdf', dict(width=1.2345, height=0.6789, angle=31.7), 'A', 'vec'),
    ('rect31_warp', 'rectangle_sdf', dict(width=1.2345, height=0.6789, angle=-58.3), 'AW', 'warp'),
    ('ellipse', 'rotated_ellipse_sdf', dict(width_major=2.3171, width_minor=1.1193, major_axis_angle=17.3), 'A', 'grid'),
    ('ellipse_warp', 'rotated_ellipse_sdf', dict(width_major=2.3171, width_minor=1.1193, major_axis_angle=-40.1), 'AW', 'warp'),
    ('hexagon', 'regular_polygon_sdf', dict(sides=6, radius=2.7319, center=(0.1013, -0.2027), rotation=11.3), 'B', 'grid'),
    ('hexagon_vec', 'regular_polygon_sdf', dict(sides=7, radius=2.3319, center=(-0.1513, 0.0727), rotation=-3.3), 'A', 'vec'),
    ('pentagon_ccw', 'polygon_sdf', dict(vertices=PENTAGON), 'A', 'grid'),
    ('pentagon_cw', 'polygon_sdf', dict(vertices=PENTAGON[::-1]), 'A', 'grid'),
    ('spider', 'spider_sdf', dict(vanes=3, width=0.1371, rotation=13.7, center=(0.0513, 0.0271)), 'A', 'grid'),
    ('spider_rad', 'spider_sdf', dict(vanes=4, width=0.2371, rotation=0.4137, center=(-0.0513, 0.1271), rotation_is_rad=True), 'AW', 'warp'),
    ('fillet0', 'rectangle_with_corner_fillets_sdf', dict(width=2.1173, height=1.4139, cradius=0.5171, center=(0.2113, -0.1327)), 'A', 'grid'),
    ('fillet0_vec', 'rectangle_with_corner_fillets_sdf', dict(width=2.1173, height=1.4139, cradius=0.5171), 'A', 'vec'),
    ('fillet24', 'rectangle_with_corner_fillets_sdf', dict(width=2.1173, height=1.4139, cradius=0.5171, center=(0.2113, -0.1327), rotation=23.9),
     'A', 'grid'),
    ('fillet24_warp', 'rectangle_with_corner_fillets_sdf', dict(width=2.1173, height=1.4139, cradius=0.5171, rotation=23.9), 'AW', 'warp'),
    ('offset_circle', 'offset_circle', dict(radius=1.7137, center=(0.5113, -0.3171)), 'A', 'grid'),
    ('gaussian', 'gaussian', dict(sigma=1.3171, center=(0.2113, -0.4171)), 'A', 'grid'),
    ('gaussian_vec', 'gaussian', dict(sigma=0.9171), 'A', 'vec'),
]

FOUR = dict(r_outer=3.0137, hex_radius=2.7319, hex_rotation=11.3, r_inner=0.7113, vanes=3, vane_width=0.1371, vane_rotation=13.7)
RING = dict(sides=6, radius=0.9137, ring_radius=1.9171, rotation=7.3)


def coords_of(out, cset, form):
    base = cset.rstrip('W')
    xv, yv = out[f'{base}_xv'], out[f'{base}_yv']
    if cset.endswith('W'):
        x, y = out[f'{cset}_x'], out[f'{cset}_y']
    else:
        x, y = np.meshgrid(xv, yv)
    if form == 'vec':
        return xv, yv
    if form == 'r':
        return (np.hypot(x, y),)
    return x, y


def run_case(fn, kw, coords, cast=None):
    c = [a.astype(cast) if cast else a for a in coords]
    names = ('r',) if len(c) == 1 else ('x', 'y')
    if fn == 'offset_circle':       # the reference has no distance form of it
        x, y = c if c[0].ndim == 2 else np.meshgrid(*c)
        return np.hypot(x - kw['center'][0], y - kw['center'][1]) - kw['radius']
    return getattr(RG, fn)(**kw, **dict(zip(names, c)))


def four(x, y, P=FOUR):
    r = np.hypot(x, y)
    d = RG.intersect(RG.circle_sdf(P['r_outer'], r), RG.regular_polygon_sdf(6, P['hex_radius'], x, y, rotation=P['hex_rotation']))
    d = RG.subtract(d, RG.circle_sdf(P['r_inner'], r))
    return RG.subtract(d, RG.spider_sdf(P['vanes'], P['vane_width'], x, y, rotation=P['vane_rotation']))


def ring_centers(P=RING):
    return [(P['ring_radius'] * np.cos(k * np.pi / 3 + 0.2137), P['ring_radius'] * np.sin(k * np.pi / 3 + 0.2137)) for k in range(6)]


def ring(x, y, P=RING):
    return RG.union(*[RG.regular_polygon_sdf(P['sides'], P['radius'], x, y, center=c, rotation=P['rotation']) for c in ring_centers(P)])


def check(name, d64, d32, origin=None):
    keep = np.ones(d64.shape, bool)
    if origin is not None:
        keep[origin] = False
    top = np.max(np.abs(d64[keep]))
    share64 = np.mean(np.abs(d64) <= 1e-12 * top)
    share32 = np.mean(np.abs(d64) <= 5e-5 * top)
    err32 = np.max(np.abs(d32.astype(np.float64) - d64)[keep]) / top
    print(f'{name:16s} max|d| {top:9.4f}  share(1e-12) {share64:.4%}  share(5e-5) {share32:.4%}  f32 inputs {err32:.2e}')
    assert share64 == 0, name
    assert share32 <= 0.005, name
    assert err32 < 5e-5, name


def main():
    out = {}
    grids = [dict(shape=16, dx=0.0271), dict(shape=17, dx=0.0271), dict(shape=(12, 16), dx=0.1084), dict(shape=(12, 17), diameter=6.0137),
             dict(shape=(33, 16), diameter=2.5), dict(shape=(48, 64), dx=0.1084, grid=False), dict(shape=7, diameter=1.0137, grid=False)]
    out['grids'] = np.array(json.dumps(grids))
    for i, g in enumerate(grids):
        g = dict(g)
        shape = g.pop('shape')
        shape = tuple(shape) if isinstance(shape, list) else shape
        out[f'grid_{i}_x'], out[f'grid_{i}_y'] = make_xy_grid(shape, **g)
    for k, (shape, dx) in SETS.items():
        out[f'{k}_xv'], out[f'{k}_yv'] = make_xy_grid(shape, dx=dx, grid=False)
        out[f'{k}_dx'] = np.array(dx)
    x, y = np.meshgrid(out['A_xv'], out['A_yv'])
    out['AW_x'] = x + 0.0313 * np.sin(1.3 * y) + 0.0071
    out['AW_y'] = y + 0.0213 * np.cos(0.7 * x) + 0.0113 * x + 0.0037
    out['AW_dx'] = out['A_dx']

    xb, yb = np.meshgrid(out['B_xv'], out['B_yv'])
    out['polar_rho'], out['polar_phi'] = cart_to_polar(xb, yb)
    out['polar_rho_w'], out['polar_phi_w'] = cart_to_polar(out['AW_x'], out['AW_y'])
    out['cart_x_w'], out['cart_y_w'] = polar_to_cart(out['polar_rho_w'], out['polar_phi_w'])

    cases = []
    for name, fn, kw, cset, form in CASES:
        coords = coords_of(out, cset, form)
        d64 = np.asarray(run_case(fn, kw, coords), dtype=np.float64)
        if fn.startswith('gaussian'):
            d32 = np.asarray(run_case(fn, kw, coords, np.float32), dtype=np.float64)
            assert np.max(np.abs(d32 - d64)) < 5e-5, name
        else:
            origin = None
            if fn == 'rotated_ellipse_sdf':
                hit = np.argwhere((coords[0] == 0) & (coords[1] == 0))
                origin = tuple(hit[0]) if len(hit) else None
            check(name, d64, run_case(fn, kw, coords, np.float32), origin)
            if fn == 'polygon_sdf':
                pass                    # the reference has no mask form of it
            elif fn != 'offset_circle':
                mask_fn = fn[:-4]
                assert np.array_equal(run_case(mask_fn, kw, coords), d64 <= 0), name
            else:
                assert np.array_equal(RG.offset_circle(kw['radius'], *coords, kw['center']), d64 <= 0), name
        out[f'd_{name}'] = d64
        cases.append(dict(name=name, fn=fn, kw=kw, coords=cset, form=form))
    out['cases'] = np.array(json.dumps(cases))
    out['pentagon'] = np.array(PENTAGON)

    out['four'] = np.array(json.dumps(FOUR))
    out['ring'] = np.array(json.dumps(dict(RING, centers=ring_centers())))
    for cset in ('B', 'C'):
        x, y = np.meshgrid(out[f'{cset}_xv'], out[f'{cset}_yv'])
        dx = float(out[f'{cset}_dx'])
        for nm, f in (('four', four), ('ring', ring)):
            d64 = f(x, y)
            check(f'{nm}_{cset}', d64, f(x.astype(np.float32), y.astype(np.float32)))
            out[f'd_{nm}_{cset}'] = d64
            out[f'mask_{nm}_{cset}'] = d64 <= 0
            out[f'aa_{nm}_{cset}'] = RG.antialias(d64, dx)
            assert np.array_equal(out[f'aa_{nm}_{cset}'], np.clip(0.5 - d64 / dx, 0, 1))

    path = os.path.join(HERE, 'geometry.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
