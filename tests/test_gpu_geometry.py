"""GPU: prysm_amd.coordinates and prysm_amd.geometry -- every fixture case through the reference-named functions in both precisions
(distances, coverage, masks by the rules of tests/geometry_common.py), the coordinate functions, the fused composites through render
in its three coordinate modes, render against the numpy walk of its own table at 1024^2 and 1000 x 1536, odd sizes, strided outputs
and unaligned inputs, stacks, the deepest legal tree, graph replay, and an aperture rendered straight into a propagation."""
import json

import numpy as np
import pytest
import torch

import geometry_common as C
from prysm_amd import geometry_plan as GP

pytestmark = pytest.mark.gpu

F, CASES = C.fixture()
DTYPES = [np.float64, np.float32]
TDT = {np.float64: torch.float64, np.float32: torch.float32}


def tonp(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def G(pa):
    from prysm_amd import geometry
    return geometry


@pytest.fixture
def precision():
    from prysm_amd.conf import config

    def set_(dt):
        config.precision = 32 if np.dtype(dt) == np.float32 else 64
    yield set_
    config.precision = 64


def four(G):
    return C.four_node(json.loads(str(F['four'])), G.shape)


def ring(G):
    return C.ring_node(json.loads(str(F['ring'])), G.shape)


# ---------------------------------------------------------------- 1. the reference's functions
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_fixture_case_through_the_public_function(G, precision, case, dtype):
    precision(dtype)
    names, arrs = C.coords_of(F, case, dtype)
    kw = dict(case['kw'])
    kw.update({n: dev(a) for n, a in zip(names, arrs)})
    ref = F['d_' + case['name']]
    dx = float(F[case['coords'] + '_dx'])
    tol = C.TOL[np.dtype(dtype)]
    x, y = C.points_of(F, case, dtype)
    origin = C.origin_of(case, x, y)
    fn = case['fn']
    if fn == 'offset_circle':
        m = G.offset_circle(**kw)
        assert m.dtype == torch.bool and tuple(m.shape) == ref.shape
        print(case['name'], 'left out', C.mask_check(tonp(m), ref, dtype))
        return
    d = getattr(G, fn)(**kw)
    assert d.dtype == TDT[dtype] and tuple(d.shape) == ref.shape
    err, top = C.distance_error(tonp(d), ref, origin)
    print(case['name'], np.dtype(dtype).name, 'distance error %.3e' % err)
    assert err < tol
    if fn == 'gaussian':
        return
    cov = G.antialias(d, dx)
    cerr, scale = C.coverage_error(tonp(cov), ref, dx, origin)
    print(case['name'], 'coverage error %.3e (allowed %.3e)' % (cerr, tol * scale))
    assert cov.dtype == d.dtype and cerr <= tol * scale
    if fn != 'polygon_sdf':
        m = getattr(G, fn[:-4])(**kw)
        assert m.dtype == torch.bool and tuple(m.shape) == ref.shape
        print(case['name'], 'left out', C.mask_check(tonp(m), ref, dtype, origin))
    # the function is the one-node render: the same bits
    node = C.node_of(case, vertex_dtype=dtype)
    if case['form'] == 'vec' or (case['form'] == 'grid' and fn not in ('rotated_ellipse_sdf', 'spider_sdf')):
        xv, yv = F[case['coords'] + '_xv'].astype(dtype), F[case['coords'] + '_yv'].astype(dtype)
        one = G.render(node, x=dev(xv), y=dev(yv), output='sdf')
    else:
        xx, yy = np.broadcast_arrays(x, y)
        one = G.render(node, x=dev(xx), y=dev(yy), output='sdf')
    assert torch.equal(one, d)


def test_float32_stays_float32_where_the_reference_promotes(G):
    x, y = (dev(a) for a in C.coords_of(F, CASES[0] | dict(form='grid'), np.float32)[1])
    assert G.rotated_ellipse_sdf(2.0, 1.0, x, y, 17.0).dtype == torch.float32
    assert G.spider_sdf(3, 0.1, x, y, rotation=5.0).dtype == torch.float32
    assert G.spider_sdf(3, 0.1, x, y.double()).dtype == torch.float64
    assert G.square(x, y).dtype == torch.float32 and bool(G.square(x, y).all())
    with pytest.raises(TypeError):
        G.circle(1.0, x.to(torch.complex64))


def test_tensor_combinators_match_the_fused_form(G):
    xv, yv = dev(F['B_xv']), dev(F['B_yv'])
    x, y = torch.meshgrid(xv, yv, indexing='xy')
    r = torch.hypot(x, y)
    P = json.loads(str(F['four']))
    d = G.intersect(G.circle_sdf(P['r_outer'], r), G.regular_polygon_sdf(6, P['hex_radius'], x, y, rotation=P['hex_rotation']))
    d = G.subtract(d, G.circle_sdf(P['r_inner'], r))
    d = G.subtract(d, G.spider_sdf(P['vanes'], P['vane_width'], x, y, rotation=P['vane_rotation']))
    err, _ = C.distance_error(tonp(d), F['d_four_B'])
    assert err < 1e-12
    u = G.union(G.circle_sdf(1.0, r), G.circle_sdf(2.0, r))
    assert torch.equal(u, G.circle_sdf(2.0, r))
    assert isinstance(G.union(G.shape.circle(1.0), G.shape.circle(2.0)), G.Node)


# ---------------------------------------------------------------- 2. coordinates
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_make_xy_grid_is_bit_equal(pa, precision, dtype):
    from prysm_amd import coordinates as K
    precision(dtype)
    for i, g in enumerate(json.loads(str(F['grids']))):
        g = dict(g)
        shape = g.pop('shape')
        shape = tuple(shape) if isinstance(shape, list) else shape
        x, y = K.make_xy_grid(shape, **g)
        wx, wy = F[f'grid_{i}_x'], F[f'grid_{i}_y']
        assert x.dtype == TDT[dtype] and tuple(x.shape) == wx.shape and tuple(y.shape) == wy.shape
        if dtype == np.float64:
            assert np.array_equal(tonp(x), wx) and np.array_equal(tonp(y), wy)
        else:       # the reference's arithmetic in float32: the index in float32 times dx rounded once
            (ny, nx), dx = GP.grid_spacing(shape, g.get('dx', 0), g.get('diameter', 0))
            ax, ay = GP.grid_axis(nx, dx, np.float32), GP.grid_axis(ny, dx, np.float32)
            if g.get('grid', True):
                ax, ay = np.meshgrid(ax, ay)
            assert np.array_equal(tonp(x), ax) and np.array_equal(tonp(y), ay)
            assert np.max(np.abs(tonp(x) - wx)) <= 5e-5 * max(np.max(np.abs(wx)), 1e-30)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_polar_conversions(pa, dtype):
    from prysm_amd import coordinates as K
    tol = C.TOL[np.dtype(dtype)]
    xv, yv = F['B_xv'].astype(dtype), F['B_yv'].astype(dtype)
    rho, phi = K.cart_to_polar(dev(xv), dev(yv))          # vectors to a grid
    assert tuple(rho.shape) == F['polar_rho'].shape and rho.dtype == TDT[dtype]
    assert np.max(np.abs(tonp(rho) - F['polar_rho'])) / np.max(F['polar_rho']) < tol
    # the angle is discontinuous across the negative x axis, where a float32 y of -0.0 / tiny sign cannot flip: the grid holds y = 0 exactly
    assert np.max(np.abs(tonp(phi) - F['polar_phi'])) / np.pi < tol
    xw, yw = F['AW_x'].astype(dtype), F['AW_y'].astype(dtype)
    rho, phi = K.cart_to_polar(dev(xw), dev(yw))
    assert np.max(np.abs(tonp(rho) - F['polar_rho_w'])) / np.max(F['polar_rho_w']) < tol
    assert np.max(np.abs(tonp(phi) - F['polar_phi_w'])) / np.pi < tol
    x, y = K.polar_to_cart(dev(F['polar_rho_w'].astype(dtype)), dev(F['polar_phi_w'].astype(dtype)))
    top = np.max(np.abs(F['cart_x_w']))
    assert np.max(np.abs(tonp(x) - F['cart_x_w'])) / top < tol and np.max(np.abs(tonp(y) - F['cart_y_w'])) / top < tol
    a, b = K.optimize_xy_separable(*torch.meshgrid(dev(xv), dev(yv), indexing='xy'))
    assert tuple(a.shape) == (1, 64) and tuple(b.shape) == (48, 1)
    a, b = K.broadcast_1d_to_2d(dev(xv), dev(yv))
    assert tuple(a.shape) == (48, 64) and torch.equal(a[5], dev(xv)) and torch.equal(b[:, 7], dev(yv))


# ---------------------------------------------------------------- 3. the fused composites, three coordinate modes
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('cset', ['B', 'C'])
@pytest.mark.parametrize('name', ['four', 'ring'])
def test_composites_in_every_coordinate_mode(G, precision, name, cset, dtype):
    precision(dtype)
    ap = four(G) if name == 'four' else ring(G)
    ref, dx = F[f'd_{name}_{cset}'], float(F[f'{cset}_dx'])
    tol = C.TOL[np.dtype(dtype)]
    # the coordinates as arrays are make_xy_grid's (in float64 the fixture's own, bit for bit; in float32 the float32 products)
    from prysm_amd import coordinates as K
    xv, yv = K.make_xy_grid(ref.shape, dx=dx, grid=False)
    x, y = K.make_xy_grid(ref.shape, dx=dx)
    if dtype == np.float64:
        assert np.array_equal(tonp(xv), F[f'{cset}_xv']) and np.array_equal(tonp(yv), F[f'{cset}_yv'])
    got = {'grid': {}, 'separable': {}, 'pointwise': {}}
    for out, extra in (('sdf', {}), ('mask', {}), ('coverage', dict(antialias=dx))):
        got['grid'][out] = G.render(ap, shape=ref.shape, dx=dx, output=out, **({'antialias': True} if out == 'coverage' else {}))
        got['separable'][out] = G.render(ap, x=xv, y=yv, output=out, **extra)
        got['pointwise'][out] = G.render(ap, x=x, y=y, output=out, **extra)
    for mode, r in got.items():
        err, top = C.distance_error(tonp(r['sdf']), ref)
        cerr, scale = C.coverage_error(tonp(r['coverage']), ref, dx)
        share = C.mask_check(tonp(r['mask']), ref, dtype)
        print(name, cset, mode, np.dtype(dtype).name, 'distance %.3e coverage %.3e left out %.4f' % (err, cerr, share))
        assert err < tol and cerr <= tol * scale
        assert r['sdf'].dtype == TDT[dtype] and r['coverage'].dtype == TDT[dtype] and r['mask'].dtype == torch.bool
        if dtype == np.float64:
            assert np.max(np.abs(tonp(r['coverage']) - F[f'aa_{name}_{cset}'])) <= tol * scale
            assert np.array_equal(tonp(r['mask']), F[f'mask_{name}_{cset}'])
        for out in r:       # the grid's coordinates are make_xy_grid's: the same bits in every mode
            assert torch.equal(r[out], got['grid'][out]), (mode, out)


# ---------------------------------------------------------------- 4. against the numpy walk at size
@pytest.mark.parametrize('shape', [(1024, 1024), (1000, 1536)], ids=['1024', '1000x1536'])
@pytest.mark.parametrize('which', ['four', 'hex18'])
def test_render_against_the_numpy_walk_at_size(G, which, shape):
    ap = four(G) if which == 'four' else C.hex18_node(G.shape)
    dx = 6.5137 / max(shape)
    d = tonp(G.render(ap, shape=shape, dx=dx, output='sdf', dtype=torch.float64))
    cov = tonp(G.render(ap, shape=shape, dx=dx, antialias=True, dtype=torch.float64))
    m = tonp(G.render(ap, shape=shape, dx=dx, dtype=torch.float64))
    rows = np.arange(0, shape[0], 37)
    xv, yv = GP.grid_axis(shape[1], dx, np.float64), GP.grid_axis(shape[0], dx, np.float64)
    want = GP.evaluate(GP.plan(ap, np.float64)[0], xv[None, :], yv[rows][:, None])
    err, top = C.distance_error(d[rows], want)
    print(which, shape, 'distance error against the walk %.3e' % err)
    assert err < 1e-12
    assert np.max(np.abs(cov[rows] - GP.coverage(want, dx))) <= 1e-12 * top / dx
    band = np.abs(want) > 1e-12 * top
    assert np.array_equal(m[rows][band], (want <= 0)[band]) and np.mean(~band) == 0
    assert 0.05 < m.mean() < 0.95


# ---------------------------------------------------------------- 5. odd sizes, strides, alignment
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (7, 255), (5, 257), (33, 1023), (2, 1030)])
def test_odd_shapes_in_every_mode(G, shape, dtype):
    ap = four(G)
    dx = 6.3 / max(shape[1], 8)
    td = TDT[dtype]
    xv, yv = dev(GP.grid_axis(shape[1], dx, dtype)), dev(GP.grid_axis(shape[0], dx, dtype))
    want = GP.evaluate(GP.plan(ap, dtype)[0], tonp(xv)[None, :], tonp(yv)[:, None])
    x, y = (t.contiguous() for t in torch.meshgrid(xv, yv, indexing='xy'))
    for out in ('sdf', 'mask', 'coverage'):
        aa = dict(antialias=dx) if out == 'coverage' else {}
        g = G.render(ap, shape=shape, dx=dx, output=out, dtype=td, **({'antialias': True} if aa else {}))
        assert torch.equal(G.render(ap, x=xv, y=yv, output=out, **aa), g)
        assert torch.equal(G.render(ap, x=x, y=y, output=out, **aa), g)
        if out == 'sdf':
            err, _ = C.distance_error(tonp(g), want)
            assert err < C.TOL[np.dtype(dtype)]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_strided_outputs_and_unaligned_inputs(G, dtype):
    ap, td = ring(G), TDT[dtype]
    ny, nx, dx = 37, 301, 0.0213
    for out, odt in (('sdf', td), ('mask', torch.bool), ('coverage', td)):
        aa = dict(antialias=True) if out == 'coverage' else {}
        want = G.render(ap, shape=(ny, nx), dx=dx, output=out, dtype=td, **aa)
        big = torch.full((ny + 4, nx + 11), 7, dtype=odt, device='cuda') if odt != torch.bool else torch.ones((ny + 4, nx + 11), dtype=odt, device='cuda')
        keep = big.clone()
        view = big[2:2 + ny, 3:3 + nx]          # a row stride, and a start off any 16-byte boundary
        assert G.render(ap, shape=(ny, nx), dx=dx, output=out, dtype=td, out=view, **aa) is view
        assert torch.equal(view, want)
        keep[2:2 + ny, 3:3 + nx] = want
        assert torch.equal(big, keep)           # nothing outside the view was written
    # inputs that start off a 16-byte boundary
    xv, yv = GP.grid_axis(nx, dx, dtype), GP.grid_axis(ny, dx, dtype)
    want = G.render(ap, shape=(ny, nx), dx=dx, output='sdf', dtype=td)
    bx, by = torch.zeros(nx + 1, dtype=td, device='cuda'), torch.zeros(ny + 1, dtype=td, device='cuda')
    bx[1:], by[1:] = dev(xv), dev(yv)
    assert bx[1:].data_ptr() % 16 != 0
    assert torch.equal(G.render(ap, x=bx[1:], y=by[1:], output='sdf'), want)
    X, Y = np.meshgrid(xv, yv)
    fx, fy = torch.zeros(ny * nx + 1, dtype=td, device='cuda'), torch.zeros(ny * nx + 1, dtype=td, device='cuda')
    fx[1:], fy[1:] = dev(X).reshape(-1), dev(Y).reshape(-1)
    px, py = fx[1:].view(ny, nx), fy[1:].view(ny, nx)
    assert px.is_contiguous() and px.data_ptr() % 16 != 0
    assert torch.equal(G.render(ap, x=px, y=py, output='sdf'), want)
    # points of any dimensionality
    p3 = G.render(ap, x=px.reshape(1, ny, nx), y=py.reshape(1, ny, nx), output='sdf')
    assert tuple(p3.shape) == (1, ny, nx) and torch.equal(p3[0], want)


# ---------------------------------------------------------------- 6. stacks, depth
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_stack_equals_single_renders(G, dtype):
    S, td = G.shape, TDT[dtype]
    aps = [four(G), ring(G), S.circle(1.3137), S.union(S.rectangle(1.1, 0.7, 31.7)), C.hex18_node(S),
           S.rotated_ellipse(2.1, 0.9, 33.0).subtract(S.annulus(0.3, 0.6, center=(0.2, 0.1)))]
    shape, dx = (130, 517), 0.0131
    for out in ('sdf', 'mask', 'coverage'):
        aa = dict(antialias=True) if out == 'coverage' else {}
        st = G.render(aps, shape=shape, dx=dx, output=out, dtype=td, **aa)
        assert tuple(st.shape) == (len(aps), *shape)
        for b, ap in enumerate(aps):
            assert torch.equal(st[b], G.render(ap, shape=shape, dx=dx, output=out, dtype=td, **aa)), (out, b)
    buf = torch.zeros((len(aps), shape[0] + 1, shape[1] + 3), dtype=td, device='cuda')
    G.render(aps, shape=shape, dx=dx, output='sdf', dtype=td, out=buf[:, 1:, 3:])
    assert torch.equal(buf[:, 1:, 3:], G.render(aps, shape=shape, dx=dx, output='sdf', dtype=td))


def test_deepest_legal_tree_and_union_of_one(G):
    S = G.shape
    leaf = [S.circle(0.5 + 0.37 * i, center=(0.1 * i, -0.05 * i)) for i in range(8)]
    deep = S.union(leaf[0], S.intersect(leaf[1], S.subtract(leaf[2], S.union(leaf[3], leaf[4]))))      # slots 0 .. 3
    assert GP.depth(deep) == GP.MAX_SLOTS
    xv, yv = GP.grid_axis(200, 0.031, np.float64), GP.grid_axis(90, 0.031, np.float64)
    d = [GP.evaluate(GP.plan(n, np.float64)[0], xv[None, :], yv[:, None]) for n in leaf]
    want = np.minimum(d[0], np.maximum(d[1], np.maximum(d[2], -np.minimum(d[3], d[4]))))
    got = tonp(G.render(deep, shape=(90, 200), dx=0.031, output='sdf', dtype=torch.float64))
    assert C.distance_error(got, want)[0] < 1e-12
    with pytest.raises(ValueError):
        G.render(S.union(leaf[0], S.union(leaf[1], deep.children[1])), shape=(8, 8), dx=0.1)
    one = G.render(S.union(leaf[2]), shape=(90, 200), dx=0.031, output='sdf', dtype=torch.float64)
    assert torch.equal(one, G.render(leaf[2], shape=(90, 200), dx=0.031, output='sdf', dtype=torch.float64))


# ---------------------------------------------------------------- 7. graph capture
def test_graph_replay_is_bit_equal(G):
    from prysm_amd import graph
    ap = four(G)
    shape, dx = (300, 420), 0.0157
    xv, yv = dev(GP.grid_axis(shape[1], dx, np.float32)), dev(GP.grid_axis(shape[0], dx, np.float32))

    def run(x, y):
        return (G.render(ap, shape=shape, dx=dx, antialias=True, dtype=torch.float32), G.render(ap, x=x, y=y, output='sdf'),
                G.render([ap, ring(G)], shape=shape, dx=dx))
    eager = [t.clone() for t in run(xv, yv)]
    model = graph.capture(run, xv, yv)
    for _ in range(2):
        for e, r in zip(eager, model(xv, yv)):
            assert torch.equal(e, r)
    moved = model(xv + 0.25, yv)[1].clone()
    assert torch.equal(moved, G.render(ap, x=xv + 0.25, y=yv, output='sdf')) and not torch.equal(moved, eager[1])


# ---------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_rendered_amplitude_through_a_propagation(pa, G, precision, dtype):
    """the aperture rendered on the device, straight into a Wavefront, against the same model with the amplitude uploaded from the
    fixture's reference-built coverage: TOL64 = 1e-10 / TOL32 = 5e-6 of tests/test_gpu_parity.py"""
    from prysm_amd import propagation as P, coordinates as K
    from prysm_amd.polynomials import zernike_sum
    precision(dtype)
    dx, ref = float(F['C_dx']), F['aa_four_C']
    amp = G.render(four(G), shape=ref.shape, dx=dx, antialias=True)
    assert amp.dtype == TDT[dtype]
    x, y = K.make_xy_grid(ref.shape, dx=dx)
    nms, coefs = [(2, 0), (2, 2), (3, 1), (4, 0)], np.array([120.0, -75.0, 40.0, 33.0], dtype=dtype)
    opd = zernike_sum(coefs, nms, x / 3.1, y / 3.1)
    got = tonp(P.Wavefront.from_amp_and_phase(amp, opd, 0.6328, dx).focus(100.0, Q=2).data)
    want = tonp(P.Wavefront.from_amp_and_phase(dev(ref.astype(dtype)), opd, 0.6328, dx).focus(100.0, Q=2).data)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print('end to end', np.dtype(dtype).name, '%.3e' % err)
    assert err < (1e-10 if dtype == np.float64 else 5e-6)
