"""Shared by tests/test_geometry_host.py and tests/test_gpu_geometry.py: the geometry fixture, its cases as shape nodes, and the
comparison rules.

Distances: max|got - ref| / max|ref| < TOL (1e-12 float64, 5e-5 float32 inputs against the float64 fixture: the pair of
tests/test_gpu_qpoly.py).  Coverage: that absolute distance error divided by dx.  rotated_ellipse_sdf is -1e15 at the origin by
construction: max|ref| leaves the origin out and the origin is compared relatively.  Masks: with band = TOL max|d_ref|, every pixel
with |d_ref| > band must equal the reference mask; the share of pixels left out is capped at 0.5 % (float32) and 0 (float64).
"""
import json
import os

import numpy as np

from prysm_amd import geometry_plan as GP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'geometry.npz')
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 5e-5}
CAP = {np.dtype(np.float64): 0.0, np.dtype(np.float32): 0.005}


def fixture():
    f = np.load(GOLDEN)
    return f, json.loads(str(f['cases']))


def coords_of(f, case, dtype=np.float64):
    """(names, arrays) of a case's coordinates in the form the case passes them"""
    cset, form = case['coords'], case['form']
    base = cset.rstrip('W')
    xv, yv = f[f'{base}_xv'], f[f'{base}_yv']
    if cset.endswith('W'):
        x, y = f[f'{cset}_x'], f[f'{cset}_y']
    else:
        x, y = np.meshgrid(xv, yv)
    if form == 'vec':
        arrs = (xv, yv)
    elif form == 'r':
        arrs = (np.hypot(x, y),)
    else:
        arrs = (x, y)
    names = ('r',) if form == 'r' else ('x', 'y')
    return names, tuple(np.ascontiguousarray(a.astype(dtype)) for a in arrs)


def points_of(f, case, dtype=np.float64):
    """broadcastable (x, y) for geometry_plan.evaluate: vectors become a row and a column, r is passed as x"""
    names, arrs = coords_of(f, case, dtype)
    if names == ('r',):
        return arrs[0], arrs[0]
    if case['form'] == 'vec':
        return arrs[0][None, :], arrs[1][:, None]
    return arrs


def node_of(case, vertex_dtype=np.float64):
    fn, kw = case['fn'], dict(case['kw'])
    if fn == 'circle_sdf':
        return GP.radial_circle(kw['radius'])
    if fn == 'annulus_sdf':
        return GP.radial_annulus(kw['rin'], kw['rout'])
    if fn == 'rectangle_sdf':
        return GP.rectangle(kw['width'], kw.get('height'), kw.get('angle', 0))
    if fn == 'rotated_ellipse_sdf':
        return GP.rotated_ellipse(kw['width_major'], kw['width_minor'], kw.get('major_axis_angle', 0))
    if fn == 'regular_polygon_sdf':
        return GP.regular_polygon(kw['sides'], kw['radius'], kw.get('center', (0, 0)), kw.get('rotation', 0), dtype=vertex_dtype)
    if fn == 'polygon_sdf':
        return GP.polygon(kw['vertices'])
    if fn == 'spider_sdf':
        return GP.spider(kw['vanes'], kw['width'], kw.get('rotation', 0), kw.get('center', (0, 0)), kw.get('rotation_is_rad', False))
    if fn == 'rectangle_with_corner_fillets_sdf':
        return GP.rectangle_with_corner_fillets(kw['width'], kw['height'], kw['cradius'], kw.get('center', (0, 0)), kw.get('rotation', 0))
    if fn == 'offset_circle':
        return GP.circle(kw['radius'], kw['center'])
    if fn == 'gaussian':
        return GP.gaussian(kw['sigma'], kw.get('center', (0, 0)))
    raise KeyError(fn)


def four_node(P, S=GP):
    """the four-shape aperture of the fixture: circle & hexagon, minus the central obscuration, minus a spider"""
    return S.circle(P['r_outer']).intersect(S.regular_polygon(6, P['hex_radius'], rotation=P['hex_rotation'])) \
        .subtract(S.circle(P['r_inner'])).subtract(S.spider(P['vanes'], P['vane_width'], rotation=P['vane_rotation']))


def ring_node(P, S=GP):
    return S.union(*[S.regular_polygon(P['sides'], P['radius'], center=tuple(c), rotation=P['rotation']) for c in P['centers']])


def hex18_node(S=GP, pitch=1.0137, radius=0.5713):
    """a union of 18 hexagons: the two inner rings of a hexagonal tiling without its centre"""
    cs = []
    for q in range(-2, 3):
        for r in range(-2, 3):
            if (q or r) and abs(q + r) <= 2:
                cs.append((pitch * (q + r / 2) + 0.0113, pitch * r * np.sqrt(3) / 2 - 0.0071))
    assert len(cs) == 18
    return S.union(*[S.regular_polygon(6, radius, center=c, rotation=3.7) for c in cs])


def origin_of(case, x, y):
    """index of the point (0, 0) for the ellipse (None elsewhere, or when the coordinates do not hold it)"""
    if case is None or case['fn'] != 'rotated_ellipse_sdf':
        return None
    hit = np.argwhere((np.broadcast_to(x, np.broadcast_shapes(x.shape, y.shape)) == 0) & (np.broadcast_to(y, np.broadcast_shapes(x.shape, y.shape)) == 0))
    return tuple(hit[0]) if len(hit) else None


def distance_error(got, ref, origin=None):
    """(max|got - ref| / max|ref|, max|ref|), the origin left out of both and compared relatively"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    keep = np.ones(ref.shape, bool)
    err0 = 0.0
    if origin is not None:
        keep[origin] = False
        err0 = abs(got[origin] / ref[origin] - 1)
    top = np.max(np.abs(ref[keep]))
    return max(np.max(np.abs(got - ref)[keep]) / top, err0), top


def mask_check(got, ref_d, dtype, origin=None):
    """the mask rule; returns the share of pixels left out"""
    dtype = np.dtype(dtype)
    got, ref_d = np.asarray(got), np.asarray(ref_d, dtype=np.float64)
    assert got.dtype == np.bool_ and got.shape == ref_d.shape, (got.dtype, got.shape, ref_d.shape)
    keep = np.ones(ref_d.shape, bool)
    if origin is not None:
        keep[origin] = False
    band = TOL[dtype] * np.max(np.abs(ref_d[keep]))
    judged = np.abs(ref_d) > band
    assert np.array_equal(got[judged], (ref_d <= 0)[judged]), f'{np.sum(got[judged] != (ref_d <= 0)[judged])} mask pixels differ outside the band'
    share = 1.0 - np.mean(judged)
    assert share <= CAP[dtype], f'{share:.4%} of the pixels are inside the band (cap {CAP[dtype]:.2%})'
    return share


def coverage_error(got, ref_d, dx, origin=None):
    """(max|got - antialias(ref_d, dx)|, the allowance per unit tolerance = max|ref_d| / dx)"""
    ref_d = np.asarray(ref_d, dtype=np.float64)
    keep = np.ones(ref_d.shape, bool)
    if origin is not None:
        keep[origin] = False
    want = np.clip(0.5 - ref_d / dx, 0, 1)
    return np.max(np.abs(np.asarray(got, dtype=np.float64) - want)), np.max(np.abs(ref_d[keep])) / dx
