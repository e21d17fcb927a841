"""CPU: the host side of prysm_amd.geometry / prysm_amd.coordinates -- the numpy walk of the step table (geometry_plan.evaluate)
against the reference fixture for every case and both composites, make_xy_grid's host arithmetic, plan-time errors raised before any
device call, table layout and caching keys, and the C-ABI argument errors of the new entry points (no GPU here)."""
import ctypes
import json
import os

import numpy as np
import pytest

import geometry_common as C
from prysm_amd import geometry_plan as GP

F, CASES = C.fixture()
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------- the walk against the reference
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_walk_of_every_fixture_case(case, dtype):
    x, y = C.points_of(F, case, dtype)
    table = GP.plan(C.node_of(case, vertex_dtype=dtype), dtype)
    assert table.shape[0] == 1
    d = GP.evaluate(table[0], x, y)
    ref = F['d_' + case['name']]
    origin = C.origin_of(case, x, y)
    assert d.dtype == np.dtype(dtype) and d.shape == ref.shape
    err, top = C.distance_error(d, ref, origin)
    assert err < C.TOL[np.dtype(dtype)], err
    if case['fn'] == 'gaussian':
        return
    C.mask_check(d <= 0, ref, dtype, origin)
    dx = float(F[case['coords'] + '_dx'])
    keep = np.ones(ref.shape, bool)
    if origin is not None:
        keep[origin] = False
    cerr, scale = C.coverage_error(GP.coverage(d, dx), ref, dx, origin)
    assert cerr <= C.TOL[np.dtype(dtype)] * scale


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('cset', ['B', 'C'])
@pytest.mark.parametrize('name', ['four', 'ring'])
def test_walk_of_the_composites(name, cset, dtype):
    P = json.loads(str(F[name]))
    node = C.four_node(P) if name == 'four' else C.ring_node(P)
    dx = float(F[f'{cset}_dx'])
    xv, yv = F[f'{cset}_xv'].astype(dtype), F[f'{cset}_yv'].astype(dtype)
    d = GP.evaluate(GP.plan(node, dtype)[0], xv[None, :], yv[:, None])
    ref = F[f'd_{name}_{cset}']
    err, top = C.distance_error(d, ref)
    tol = C.TOL[np.dtype(dtype)]
    assert err < tol
    C.mask_check(d <= 0, ref, dtype)
    assert np.max(np.abs(GP.coverage(d, dx) - F[f'aa_{name}_{cset}'])) <= tol * top / dx
    if dtype == np.float64:
        assert np.array_equal(d <= 0, F[f'mask_{name}_{cset}'])


def test_the_fixture_keeps_the_reference_inside_the_mask_cap():
    """what tests/golden/make_golden_geometry.py asserts when it writes the file, checked again on the stored arrays"""
    for k in F.files:
        if not k.startswith('d_') or 'gaussian' in k:
            continue
        d = F[k]
        top = np.max(np.abs(d[np.abs(d) < 1e14]))
        assert np.mean(np.abs(d) <= 1e-12 * top) == 0, k
        assert np.mean(np.abs(d) <= 5e-5 * top) <= 0.005, k


# ---------------------------------------------------------------- make_xy_grid on the host
def test_grid_axis_reproduces_make_xy_grid():
    for i, g in enumerate(json.loads(str(F['grids']))):
        shape = g['shape']
        shape = tuple(shape) if isinstance(shape, list) else shape
        (ny, nx), dx = GP.grid_spacing(shape, g.get('dx', 0), g.get('diameter', 0))
        ax, ay = GP.grid_axis(nx, dx, np.float64), GP.grid_axis(ny, dx, np.float64)
        if g.get('grid', True):
            ax, ay = np.meshgrid(ax, ay)
        assert np.array_equal(ax, F[f'grid_{i}_x']) and np.array_equal(ay, F[f'grid_{i}_y'])
    assert GP.grid_spacing(5, diameter=2.0) == ((5, 5), 0.4)
    assert GP.grid_spacing((4, 10), dx=1.0, diameter=5.0) == ((4, 10), 0.5)       # the diameter overrides dx
    assert GP.grid_axis(4, 0.1, np.float32).dtype == np.float32
    assert np.array_equal(GP.grid_axis(5, 1, np.float64), [-2, -1, 0, 1, 2]) and np.array_equal(GP.grid_axis(4, 1, np.float64), [-2, -1, 0, 1])
    with pytest.raises(ValueError):
        GP.grid_spacing((1, 2, 3))


def test_generate_vertices_follows_the_reference():
    v = GP.generate_vertices(6, 2.7319, (0.1013, -0.2027), 11.3)
    k = np.arange(6)
    a = k * (2 * np.pi / 6) + np.radians(11.3)
    assert np.allclose(v[:, 0], 2.7319 * np.sin(a) + 0.1013, rtol=0, atol=1e-15)
    assert np.allclose(v[:, 1], 2.7319 * np.cos(a) - 0.2027, rtol=0, atol=1e-15)


# ---------------------------------------------------------------- the table
def test_step_layout_and_flattening():
    assert GP.step_dtype(np.float32).itemsize == 48 and GP.step_dtype(np.float64).itemsize == 80
    t = GP.plan(C.four_node(json.loads(str(F['four']))), np.float64)[0]
    # circle, six hexagon edges, the obscuration, three vanes: all into accumulator 0
    assert [int(s['op']) for s in t] == [GP.OP_CIRCLE] + [GP.OP_EDGE] * 6 + [GP.OP_CIRCLE] + [GP.OP_VANE] * 3
    assert set(int(s['slot']) for s in t) == {0}
    ends = [int(s['comb']) for s in t if s['flags'] & GP.FL_END]
    assert ends == [GP.CB_SET, GP.CB_MAX, GP.CB_MAXNEG, GP.CB_MAXNEG]
    assert t[1]['flags'] & GP.FL_BEGIN and not t[2]['flags'] & GP.FL_BEGIN and t[6]['flags'] & GP.FL_END
    # a composite child of a composite goes through the next accumulator and a MERGE
    S = GP
    n = S.intersect(S.circle(2.0), S.union(S.circle(1.0, (1, 0)), S.circle(1.0, (-1, 0))))
    t = GP.plan(n, np.float32)[0]
    assert [(int(s['op']), int(s['comb']), int(s['slot'])) for s in t] == [
        (GP.OP_CIRCLE, GP.CB_SET, 0), (GP.OP_CIRCLE, GP.CB_SET, 1), (GP.OP_CIRCLE, GP.CB_MIN, 1), (GP.OP_MERGE, GP.CB_MAX, 0)]
    assert GP.depth(n) == 2
    # a stack pads the shorter programs with NOPs
    st = GP.plan([n, S.circle(1.0)], np.float64)
    assert st.shape == (2, 4) and [int(s['op']) for s in st[1]] == [GP.OP_CIRCLE, 0, 0, 0]
    x = np.linspace(-2, 2, 9)
    assert np.array_equal(GP.evaluate(st[1], x[None, :], x[:, None]), np.sqrt(x[None, :] ** 2 + x[:, None] ** 2) - 1.0)
    # scalars are rounded once to the table's precision
    assert GP.plan(S.circle(3.0137), np.float32)[0]['f'][0][2] == np.float32(3.0137)


def test_union_of_one_and_the_deepest_tree():
    S = GP
    leaf = [S.circle(0.5 + 0.37 * i, center=(0.1 * i, -0.05 * i)) for i in range(6)]
    x, y = np.linspace(-3, 3, 41)[None, :], np.linspace(-2, 2, 31)[:, None]
    d = [GP.evaluate(GP.plan(n, np.float64)[0], x, y) for n in leaf]
    assert np.array_equal(GP.evaluate(GP.plan(S.union(leaf[2]), np.float64)[0], x, y), d[2])
    deep = S.union(leaf[0], S.intersect(leaf[1], S.subtract(leaf[2], S.union(leaf[3], leaf[4]))))
    assert GP.depth(deep) == GP.MAX_SLOTS
    want = np.minimum(d[0], np.maximum(d[1], np.maximum(d[2], -np.minimum(d[3], d[4]))))
    assert np.array_equal(GP.evaluate(GP.plan(deep, np.float64)[0], x, y), want)
    # a composite FIRST child costs no slot
    left = S.subtract(S.subtract(S.subtract(S.subtract(S.union(leaf[5], leaf[4]), leaf[3]), leaf[2]), leaf[1]), leaf[0])
    assert GP.depth(left) == 1
    want = np.minimum(d[5], d[4])
    for k in (3, 2, 1, 0):
        want = np.maximum(want, -d[k])
    assert np.array_equal(GP.evaluate(GP.plan(left, np.float64)[0], x, y), want)


# ---------------------------------------------------------------- errors before any device call
def test_plan_time_errors():
    S = GP
    c = S.circle(1.0)
    too_deep = S.union(c, S.union(c, S.union(c, S.union(c, S.union(c, c)))))
    assert GP.depth(too_deep) == 5
    with pytest.raises(ValueError):
        GP.plan(too_deep, np.float64)
    with pytest.raises(ValueError):
        S.rotated_ellipse(1.0, 2.0)
    with pytest.raises(ValueError):
        S.polygon([(0, 0), (1, 1)])
    with pytest.raises(ValueError):
        S.polygon([(0, 0, 0), (1, 1, 1), (2, 2, 2)])
    with pytest.raises(ValueError):
        S.regular_polygon(2, 1.0)
    with pytest.raises(TypeError):
        S.circle(1 + 2j)
    with pytest.raises(TypeError):
        S.polygon(np.ones((3, 2), complex))
    with pytest.raises(TypeError):
        S.union(c, 3.0)
    with pytest.raises(ValueError):
        S.union(c, S.gaussian(1.0))
    with pytest.raises(TypeError):
        GP.plan(c, np.float16)
    with pytest.raises(TypeError):
        GP.plan([], np.float64)


def test_public_functions_refuse_bad_arguments_before_upload():
    # no GPU here: every one of these must be refused by the Python checks, not by a failed upload
    from prysm_amd import geometry as G, coordinates as K
    a, b = np.zeros((4, 5)), np.zeros((4, 6))
    S = G.shape
    c = S.circle(1.0)
    with pytest.raises(ValueError):
        G.rotated_ellipse_sdf(1.0, 2.0, a, a)
    with pytest.raises(ValueError):
        G.rotated_ellipse(1.0, 2.0, a, a)
    with pytest.raises(ValueError):
        G.polygon_sdf([(0, 0), (1, 0)], a, a)
    with pytest.raises(ValueError):
        G.regular_polygon_sdf(6, 1.0, a, b)               # meshgrids differ in shape
    with pytest.raises(ValueError):
        G.spider_sdf(3, 0.1, a, b)                        # do not broadcast
    with pytest.raises(ValueError):
        G.rectangle_sdf(1.0, a, b)
    with pytest.raises(TypeError):
        G.circle_sdf(1.0, a.astype(complex))
    with pytest.raises(TypeError):
        G.gaussian(1.0, a, a.astype(np.complex64))
    with pytest.raises(TypeError):
        K.cart_to_polar(a.astype(complex), a)
    with pytest.raises(TypeError):
        K.polar_to_cart(a, a.astype(complex))
    with pytest.raises(ValueError):
        K.cart_to_polar(a, b, vec_to_grid=False)
    too_deep = S.union(c, S.union(c, S.union(c, S.union(c, S.union(c, c)))))
    with pytest.raises(ValueError):
        G.render(too_deep, shape=(8, 8), dx=0.1)
    with pytest.raises(ValueError):
        G.render(c, shape=(8, 8), dx=0.1, x=a, y=a)       # a grid or coordinates, not both
    with pytest.raises(ValueError):
        G.render(c)
    with pytest.raises(ValueError):
        G.render(c, x=a, y=b)
    with pytest.raises(ValueError):
        G.render(c, x=a, y=a, antialias=True)             # no grid to take the spacing from
    with pytest.raises(ValueError):
        G.render(c, shape=(8, 8), dx=0.1, output='distance')
    with pytest.raises(ValueError):
        G.render(c, shape=(8, 8), dx=0.0, antialias=True)
    with pytest.raises(ValueError):
        G.render(S.gaussian(1.0), shape=(8, 8), dx=0.1)   # a gaussian has no mask
    with pytest.raises(TypeError):
        G.render(c, x=a.astype(complex), y=a)
    with pytest.raises(TypeError):
        G.render([c, 1.0], shape=(8, 8), dx=0.1)
    with pytest.raises(TypeError):
        G.render(c, shape=(8, 8), dx=0.1, dtype=np.float16)
    assert not hasattr(G, 'multisample')


def test_table_cache_keys(monkeypatch):
    """one device table per (programs, dtype, device): equal trees share it, any parameter, the precision or the device separates"""
    import torch
    from prysm_amd import geometry as G, _lib as L
    made = []
    monkeypatch.setattr(L, 'device', lambda: torch.device('cpu'))
    monkeypatch.setattr(L, '_cur_dev', lambda: 0)
    monkeypatch.setattr(G, '_TABLES', {})
    real = GP.plan
    monkeypatch.setattr(GP, 'plan', lambda *a: made.append(a) or real(*a))
    S = G.shape
    a = (S.circle(1.0).subtract(S.spider(3, 0.1)),)
    t0, n0 = G._table(a, torch.float64)
    assert n0 == 4 and t0.dtype == torch.uint8 and t0.numel() == 4 * 80
    assert G._table((S.circle(1.0).subtract(S.spider(3, 0.1)),), torch.float64)[0] is t0 and len(made) == 1
    assert G._table(a, torch.float32)[0].numel() == 4 * 48 and len(made) == 2
    G._table((S.circle(1.0).subtract(S.spider(3, 0.1, rotation=1e-9)),), torch.float64)
    G._table(a + a, torch.float64)
    assert len(made) == 4
    monkeypatch.setattr(L, '_cur_dev', lambda: 1)
    G._table(a, torch.float64)
    assert len(made) == 5 and len(G._TABLES) == 5
    assert S.circle(1.0) == S.circle(1.0) and S.circle(1.0) != S.circle(1.0, (0, 1e-12)) and hash(S.circle(2)) == hash(S.circle(2.0))


# ---------------------------------------------------------------- the C ABI without a GPU
SYMS = ['pm_xy_grid', 'pm_cart_to_polar', 'pm_polar_to_cart', 'pm_sdf_render']
BAD = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation before a launch


def test_symbols_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'prysm_amd.h')).read()
    for s in SYMS:
        assert s + '(' in hdr and hasattr(lib, s) and s in L.SIGNATURES
    assert 'PM_COORDS_GRID = 0, PM_COORDS_SEPARABLE = 1, PM_COORDS_POINTWISE = 2' in hdr
    assert 'PM_SDF_MASK = 0, PM_SDF_DISTANCE = 1, PM_SDF_COVERAGE = 2' in hdr
    assert (L.PM_COORDS_GRID, L.PM_COORDS_SEPARABLE, L.PM_COORDS_POINTWISE) == (0, 1, 2)
    assert (L.PM_SDF_MASK, L.PM_SDF_DISTANCE, L.PM_SDF_COVERAGE) == (0, 1, 2)
    assert lib.pm_version() == 107


@pytest.mark.parametrize('kw', [
    dict(dtype=0), dict(dtype=7), dict(coords=3), dict(coords=-1), dict(ny=-1), dict(nx=-2), dict(table=None), dict(out=None),
    dict(nsteps=-1), dict(batch=-1), dict(batch=70000), dict(out_kind=3), dict(out_kind=-1), dict(out_ld=15), dict(x=None), dict(y=None),
    dict(out_kind=2, aa_dx=0.0), dict(out_kind=2, aa_dx=float('nan')), dict(coords=0, dx=float('inf')), dict(batch=2, out_bstride=100),
    dict(ny=1 << 40),
])
def test_render_argument_errors(lib, kw):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, coords=L.PM_COORDS_SEPARABLE, ny=16, nx=16, x=BAD, y=BAD, ox=8, oy=8, dx=0.1, dy=0.1, table=BAD, nsteps=3, batch=1,
             out_kind=L.PM_SDF_DISTANCE, aa_dx=0.1, out=BAD, out_ld=16, out_bstride=256)
    a.update(kw)
    rc = lib.pm_sdf_render(a['dtype'], a['coords'], a['ny'], a['nx'], a['x'], a['y'], a['ox'], a['oy'], a['dx'], a['dy'], a['table'],
                           a['nsteps'], a['batch'], a['out_kind'], a['aa_dx'], a['out'], a['out_ld'], a['out_bstride'], None)
    assert rc == L.PM_ERR_ARG and b'pm_sdf_render' in lib.pm_last_error()
    with pytest.raises(ValueError):
        L.check(rc)


def test_render_of_nothing_launches_nothing(lib):
    from prysm_amd import _lib as L
    # grid mode reads no coordinates: NULL passes; an empty output means no launch, so no device is needed
    for ny, nx, batch in ((0, 16, 1), (16, 0, 1), (16, 16, 0)):
        assert lib.pm_sdf_render(L.PM_F32, L.PM_COORDS_GRID, ny, nx, None, None, 8, 8, 0.1, 0.1, BAD, 3, batch, L.PM_SDF_MASK, 0.0, BAD, 16, 256,
                                 None) == 0


def test_coordinate_entry_points_argument_errors(lib):
    from prysm_amd import _lib as L
    E = L.PM_ERR_ARG
    assert lib.pm_xy_grid(L.PM_C64, 4, 4, 0.1, 1, BAD, BAD, None) == E and b'pm_xy_grid' in lib.pm_last_error()
    assert lib.pm_xy_grid(L.PM_F64, -1, 4, 0.1, 1, BAD, BAD, None) == E
    assert lib.pm_xy_grid(L.PM_F64, 4, 4, 0.1, 1, None, BAD, None) == E
    assert lib.pm_xy_grid(L.PM_F64, 4, 4, 0.1, 0, BAD, None, None) == E
    assert lib.pm_xy_grid(L.PM_F32, 0, 0, 0.1, 1, BAD, BAD, None) == 0
    assert lib.pm_cart_to_polar(L.PM_BOOL, 4, 4, 0, BAD, BAD, BAD, BAD, None) == E and b'pm_cart_to_polar' in lib.pm_last_error()
    assert lib.pm_cart_to_polar(L.PM_F32, 4, -4, 0, BAD, BAD, BAD, BAD, None) == E
    for i in range(4):
        p = [BAD] * 4
        p[i] = None
        assert lib.pm_cart_to_polar(L.PM_F32, 4, 4, 1, *p, None) == E
        assert lib.pm_polar_to_cart(L.PM_F64, 16, *p, None) == E
    assert lib.pm_cart_to_polar(L.PM_F32, 0, 4, 1, BAD, BAD, BAD, BAD, None) == 0
    assert lib.pm_polar_to_cart(L.PM_C128, 16, BAD, BAD, BAD, BAD, None) == E and b'pm_polar_to_cart' in lib.pm_last_error()
    assert lib.pm_polar_to_cart(L.PM_F64, -1, BAD, BAD, BAD, BAD, None) == E
    assert lib.pm_polar_to_cart(L.PM_F64, 0, BAD, BAD, BAD, BAD, None) == 0
