"""GPU: the recurrence families of prysm_amd.polynomials -- every family's basis and derivative basis against the reference fixture in
both precisions, tails and unaligned views against the numpy walk, the 1-D sums and their adjoint, the separable 2-D sum and adjoint
against the fixture and the factored numpy model (tile edges, a strided output, stacks, 64 orders), the XY sequences, and the gradient
of a PSF loss back to Legendre-2D coefficients against finite differences and under graph replay."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_common import tonp
from recur_common import CASES, TOL, mns_of, rel as _rel, rel_per_mode as _rel_per_mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'recur.npz'))


def _fns(fam):
    from prysm_amd import polynomials as P
    return tuple(getattr(P, fam + s) for s in ('', '_seq', '_der', '_der_seq'))


# ----------------------------------------------------------------------------- the 1-D families

@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('case', sorted(CASES))
def test_basis_matches_the_reference(fx, case, dt):
    fam, params, xk = CASES[case]
    f, f_seq, f_der, f_der_seq = _fns(fam)
    x = fx[xk].astype(dt)
    val, der = tonp(f_seq(range(31), *params, x)), tonp(f_der_seq(range(31), *params, x))
    assert val.dtype == dt and val.shape == (31, 65) and der.dtype == dt and der.shape == (31, 65)
    ev, ed = _rel_per_mode(val.astype(np.float64), fx[case + '_seq']), _rel_per_mode(der.astype(np.float64), fx[case + '_der_seq'])
    print(f'recur figure: {case} {np.dtype(dt).name} values {ev:.2e} derivatives {ed:.2e}')
    assert ev < TOL[dt] and ed < TOL[dt]
    sv, sd = tonp(f_seq([2, 5, 30], *params, x)), tonp(f_der_seq([2, 5, 30], *params, x))
    assert sv.shape == (3, 65)
    assert _rel_per_mode(sv.astype(np.float64), fx[case + '_sparse_seq']) < TOL[dt]
    assert _rel_per_mode(sd.astype(np.float64), fx[case + '_sparse_der_seq']) < TOL[dt]
    for n in (0, 1, 7):
        one, done = tonp(f(n, *params, x)), tonp(f_der(n, *params, x))
        assert one.shape == (65,) and one.dtype == dt
        assert _rel(one.astype(np.float64), fx[case + '_seq'][n]) < TOL[dt]
        if n:
            assert _rel(done.astype(np.float64), fx[case + '_der_seq'][n]) < TOL[dt]
        else:
            assert not done.any()


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_jacobi_with_der_equals_the_separate_calls_bitwise(fx, dt):
    from prysm_amd import polynomials as P
    x = torch.from_numpy(fx['x_unit'].astype(dt)).cuda()
    for ns in (range(31), [2, 5, 30]):
        p, d = P.jacobi_seq_with_der(ns, 0.5, -0.5, x)
        assert torch.equal(p, P.jacobi_seq(ns, 0.5, -0.5, x)) and torch.equal(d, P.jacobi_der_seq(ns, 0.5, -0.5, x))
    p, d = P.jacobi_with_der(7, 0.0, 2.0, x)
    assert torch.equal(p, P.jacobi(7, 0.0, 2.0, x)) and torch.equal(d, P.jacobi_der(7, 0.0, 2.0, x))


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_tails_and_unaligned_views(dt):
    """1024 points take the 16-byte path, 1027 leave a tail, views 1 and 3 elements off a 16-byte boundary go element-wise"""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.recur_plan import evaluate, plan
    full = torch.from_numpy(np.linspace(-1, 1, 1031).astype(dt)).cuda()
    tab = plan('legendre', nmax=12, dtype=dt)
    for lo, hi in ((0, 1024), (0, 1027), (1, 1025), (3, 1030)):
        xs = full[lo:hi]
        wv, wd = evaluate(tab, tonp(xs))
        p, d = tonp(P.legendre_seq(range(13), xs)), tonp(P.legendre_der_seq(range(13), xs))
        assert p.shape == (13, hi - lo)
        assert _rel_per_mode(p, wv) < TOL[dt] and _rel_per_mode(d, wd) < TOL[dt]
        c = np.linspace(-1, 1, 13).astype(dt)
        z, dz = (tonp(a) for a in P.jacobi_sum_clenshaw(c, 0.0, 0.0, xs, der=True))      # Jacobi (0, 0) is Legendre
        assert _rel(z, c.astype(np.float64) @ wv.astype(np.float64)) < TOL[dt]
        assert _rel(dz, c.astype(np.float64) @ wd.astype(np.float64)) < TOL[dt]


# ----------------------------------------------------------------------------- 1-D sums and their adjoint

@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_1d_sums_match_the_reference(fx, dt):
    from prysm_amd import polynomials as P
    x = fx['x_unit'].astype(dt)
    got = tonp(P.jacobi_sum_clenshaw(fx['clenshaw_s'].astype(dt), 0.0, 2.0, x))
    assert got.dtype == dt and _rel(got.astype(np.float64), fx['clenshaw']) < TOL[dt]
    rx, ry, c = fx['rad_x'].astype(dt), fx['rad_y'].astype(dt), fx['rad_coefs'].astype(dt)
    z, zx, zy = (tonp(a).astype(np.float64) for a in P.jacobi_radial_sum_der_xy(c, range(11), 0.0, 2.0, rx, ry, 1.3))
    assert z.shape == (11, 11)
    assert _rel(z, fx['rad_z']) < TOL[dt] and _rel(zx, fx['rad_zx']) < TOL[dt] and _rel(zy, fx['rad_zy']) < TOL[dt]
    assert _rel(tonp(P.jacobi_radial_sum(c, range(11), 0.0, 2.0, rx, ry, 1.3)).astype(np.float64), fx['rad_z']) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_a_stack_of_11_equals_single_calls(dt):
    """11 = 8 + 2 + 1 vectors per walk"""
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(51)
    x, y = (rng.uniform(-0.7, 0.7, (30, 35)).astype(dt) for _ in range(2))
    ns = [0, 1, 2, 4, 7, 9]
    C = rng.standard_normal((11, len(ns))).astype(dt)
    S = [tonp(a) for a in P.jacobi_radial_sum_der_xy(C, ns, 0.0, 2.0, x, y, 1.1)]
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(11):
        one = [tonp(a) for a in P.jacobi_radial_sum_der_xy(C[b], ns, 0.0, 2.0, x, y, 1.1)]
        for s, o in zip(S, one):
            assert s.shape == (11, 30, 35) and _rel(s[b], o) < tol
    G = rng.standard_normal((11, 30, 35)).astype(dt)
    A = tonp(P.jacobi_radial_sum_adjoint(G, ns, 0.0, 2.0, x, y, 1.1, dx_bar=G[::-1].copy()))
    assert A.shape == (11, len(ns))
    for b in range(11):
        assert _rel(A[b], tonp(P.jacobi_radial_sum_adjoint(G[b], ns, 0.0, 2.0, x, y, 1.1, dx_bar=G[10 - b]))) < tol


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('npts', [1024, 1027])
def test_a_stack_of_15_equals_single_calls(dt, npts):
    """15 = 8 + 4 + 2 + 1 vectors per walk (the stack of 11 never takes the pieces of 4), each piece at its own offset into the
    coefficients, the outputs, the three adjoint inputs and the partials; 1024 points take the 16-byte path, 1027 the element-wise one"""
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(15)
    x, y = (rng.uniform(-0.7, 0.7, npts).astype(dt) for _ in range(2))
    ns = [0, 1, 2, 4, 7, 9]
    C = rng.standard_normal((15, len(ns))).astype(dt)
    S = [tonp(a) for a in P.jacobi_radial_sum_der_xy(C, ns, 0.0, 2.0, x, y, 1.1)]
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(15):
        one = [tonp(a) for a in P.jacobi_radial_sum_der_xy(C[b], ns, 0.0, 2.0, x, y, 1.1)]
        for s, o in zip(S, one):
            assert s.shape == (15, npts) and s.dtype == dt and _rel(s[b], o) < tol
    G, GX, GY = (rng.standard_normal((15, npts)).astype(dt) for _ in range(3))
    A = tonp(P.jacobi_radial_sum_adjoint(G, ns, 0.0, 2.0, x, y, 1.1, dx_bar=GX, dy_bar=GY))
    assert A.shape == (15, len(ns)) and A.dtype == dt
    for b in range(15):
        assert _rel(A[b], tonp(P.jacobi_radial_sum_adjoint(G[b], ns, 0.0, 2.0, x, y, 1.1, dx_bar=GX[b], dy_bar=GY[b]))) < tol


def test_1d_project_against_the_numpy_walk_and_the_dot_product_identity():
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials import _recur as R
    from prysm_amd.polynomials.recur_plan import evaluate, plan
    rng = np.random.default_rng(52)
    x = rng.uniform(-1, 1, 5003)
    ns = list(range(0, 21, 2))
    wv, wd = evaluate(plan('cheby2', ns), x)
    g = rng.standard_normal(5003)
    assert _rel(tonp(R.project1d('cheby2', (), ns, x, databar=g)), wv @ g) < 1e-12
    assert _rel(tonp(R.project1d('cheby2', (), ns, x, dx_bar=g)), wd @ g) < 1e-12
    # <sum(c), g> = <c, project(g)> for the radial form and its two gradient maps
    xx, yy = rng.uniform(-0.8, 0.8, (2, 70, 61))
    c = rng.standard_normal(len(ns))
    gs = rng.standard_normal((3, 70, 61))
    outs = [tonp(a) for a in P.jacobi_radial_sum_der_xy(c, ns, 0.0, 2.0, xx, yy, 1.2)]
    for k, name in enumerate(('databar', 'dx_bar', 'dy_bar')):
        lhs = float(np.vdot(outs[k], gs[k]))
        rhs = float(np.vdot(c, tonp(P.jacobi_radial_sum_adjoint(gs[0] if k == 0 else None, ns, 0.0, 2.0, xx, yy, 1.2,
                                                                  **({name: gs[k]} if k else {})))))
        assert abs(lhs - rhs) / abs(lhs) < 1e-12, name
    lhs = sum(float(np.vdot(o, g)) for o, g in zip(outs, gs))
    both = P.jacobi_radial_sum_adjoint(gs[0], ns, 0.0, 2.0, xx, yy, 1.2, dx_bar=gs[1], dy_bar=gs[2])
    assert abs(lhs - float(np.vdot(c, tonp(both)))) / abs(lhs) < 1e-12
    again = P.jacobi_radial_sum_adjoint(gs[0], ns, 0.0, 2.0, xx, yy, 1.2, dx_bar=gs[1], dy_bar=gs[2])
    assert torch.equal(both, again)


# ----------------------------------------------------------------------------- the separable sum

FAMILY_2D = {'cheby': ('cheby1', 2.0, 0.5), 'xy': ('monomial', 1.0, 1.0)}


def _sum_der(key, coefs, mns, x, y):
    from prysm_amd import polynomials as P
    if key == 'cheby':
        return P.cheby1_2d_sum_der_xy(coefs, mns, x, y, x_norm=2.0, y_norm=0.5)
    return P.xy_sum_der_xy(coefs, mns, x, y)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('key', ['cheby', 'xy'])
def test_separable_sum_matches_the_reference(fx, key, dt):
    """33 x 29: less than one tile of 64 columns, odd sizes, three row chunks"""
    from prysm_amd import polynomials as P
    mns = mns_of(fx['mns'])
    x, y, c = fx['grid_x'].astype(dt), fx['grid_y'].astype(dt), fx['c2d'].astype(dt)
    got = [tonp(a) for a in _sum_der(key, c, mns, x, y)]
    for g, name in zip(got, ('_z', '_zx', '_zy')):
        assert g.dtype == dt and g.shape == (33, 29)
        assert _rel(g.astype(np.float64), fx[key + name]) < TOL[dt], name
    # meshgrids give the same bits as their axes, and the plain sum the same as the first output
    X, Y = np.meshgrid(x, y)
    again = [tonp(a) for a in _sum_der(key, c, mns, X, Y)]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    plain = P.cheby1_2d_sum(c, mns, x, y) if key == 'cheby' else P.xy_sum(c, mns, x, y)
    assert np.array_equal(tonp(plain), got[0])


def _model_2d(fam, C, x, y, ixn=1.0, iyn=1.0, dt=np.float64):
    from prysm_amd.polynomials.recur_plan import plan, separable_sum
    ny, nx = C.shape
    return separable_sum(plan(fam, nmax=nx - 1, dtype=dt), plan(fam, nmax=ny - 1, dtype=dt), C, x, y, ixn, iyn)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_separable_sum_across_a_tile_edge(dt):
    """70 x 130: two whole tiles of columns and a partial one, rows that do not fill the last chunk; duplicate pairs add"""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.recur_plan import coefficient_matrix
    rng = np.random.default_rng(53)
    x, y = np.linspace(-1, 1, 130).astype(dt), np.linspace(-0.9, 1, 70).astype(dt)
    mns = [(m, n) for m in range(6) for n in range(5)] + [(2, 3), (0, 0)]
    c = rng.standard_normal(len(mns)).astype(dt)
    want = _model_2d('legendre', coefficient_matrix(c, mns, dt), x, y, 1 / 1.5, 1 / 0.75, dt)
    got = [tonp(a) for a in P.legendre_2d_sum_der_xy(c, mns, x, y, x_norm=1.5, y_norm=0.75)]
    for g, w in zip(got, want):
        assert g.shape == (70, 130) and _rel(g.astype(np.float64), w.astype(np.float64)) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_separable_sum_1024(dt):
    """1024 x 1024 with 16 x 16 modes: every 37th row against the numpy model"""
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(54)
    x = np.linspace(-1, 1, 1024).astype(dt)
    mns = [(m, n) for m in range(16) for n in range(16)]
    c = rng.standard_normal(256).astype(dt)
    C = np.zeros((16, 16), dtype=dt)
    for k, (m, n) in enumerate(mns):
        C[n, m] = c[k]
    want = _model_2d('cheby1', C, x, x[::37], dt=np.float64)
    got = [tonp(a)[::37] for a in P.cheby1_2d_sum_der_xy(c, mns, x, x)]
    for g, w in zip(got, want):
        assert g.shape == w.shape and _rel(g.astype(np.float64), w) < TOL[dt]


def test_separable_sum_into_a_strided_output_and_a_stack_of_3(fx):
    from prysm_amd import _lib as L, polynomials as P
    from prysm_amd.polynomials import _recur as R
    from prysm_amd.polynomials.recur_plan import coefficient_matrix
    mns = mns_of(fx['mns'])
    rng = np.random.default_rng(55)
    C3 = rng.standard_normal((3, len(mns)))
    x, y = fx['grid_x'], fx['grid_y']
    S = [tonp(a) for a in P.cheby1_2d_sum_der_xy(C3, mns, x, y, x_norm=2.0, y_norm=0.5)]
    for b in range(3):
        one = [tonp(a) for a in P.cheby1_2d_sum_der_xy(C3[b], mns, x, y, x_norm=2.0, y_norm=0.5)]
        for s, o in zip(S, one):
            assert s.shape == (3, 33, 29) and np.array_equal(s[b], o)
    # rows 40 elements apart: the 11 elements between the rows stay untouched
    rows, cols, ld = 33, 29, 40
    dt = torch.float64
    xd, yd = L.as_device(x, dt), L.as_device(y, dt)
    Cd = L.as_device(coefficient_matrix(C3[0], mns), dt)
    xt, yt = R._table('cheby1', (), None, 8, dt)[0], R._table('cheby1', (), None, 6, dt)[0]
    out = torch.full((3, rows, ld), float('nan'), dtype=dt, device='cuda')
    L.check(L.load().pm_recur2_sum(L.PM_F64, rows, cols, L.ptr(xd), L.ptr(yd), L.ptr(xt), 9, L.ptr(yt), 7, 1, L.ptr(Cd),
                                   L.PM_RECUR2_Z | L.PM_RECUR2_ZX | L.PM_RECUR2_ZY, 0.5, 2.0, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                                   ld, rows * ld, L.stream_ptr()))
    o = tonp(out)
    assert np.isnan(o[:, :, cols:]).all()
    for k in range(3):
        assert np.array_equal(o[k, :, :cols], S[k][0])


def test_64_orders_on_an_axis():
    """the largest axis the kernels take: 64 x 64 orders in fp64 use the whole 64 KiB of LDS"""
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(56)
    x, y = np.linspace(-1, 1, 130), np.linspace(-1, 1, 70)
    mns = [(m, n) for m in range(64) for n in range(64)]
    C = rng.standard_normal((64, 64))
    c = np.array([C[n, m] for m, n in mns])
    want = _model_2d('legendre', C, x, y)
    got = [tonp(a) for a in P.legendre_2d_sum_der_xy(c, mns, x, y)]
    for g, w in zip(got, want):
        assert _rel(g, w) < 1e-12
    g = rng.standard_normal((70, 130))
    lhs = float(np.vdot(got[0], g))
    rhs = float(np.vdot(c, tonp(P.legendre_2d_sum_adjoint(g, mns, x, y))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12


# ----------------------------------------------------------------------------- the separable adjoint

@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(33, 29), (70, 130)])
def test_separable_adjoint_against_the_numpy_model(shape, dt):
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.recur_plan import plan, separable_project
    rng = np.random.default_rng(57)
    rows, cols = shape
    x, y = np.linspace(-1, 1, cols).astype(dt), np.linspace(-1, 0.8, rows).astype(dt)
    mns = [(m, n) for m in range(9) for n in range(7)]
    xt, yt = plan('cheby1', nmax=8, dtype=dt), plan('cheby1', nmax=6, dtype=dt)
    gs = rng.standard_normal((3, rows, cols)).astype(dt)
    want = [separable_project(xt, yt, gs[k].astype(np.float64), x.astype(np.float64), y.astype(np.float64), w, 0.5, 2.0)
            for k, w in enumerate(('z', 'zx', 'zy'))]
    args = [dict(databar=gs[0]), dict(databar=None, dx_bar=gs[1]), dict(databar=None, dy_bar=gs[2])]
    for kw, w in zip(args, want):
        got = tonp(P.cheby1_2d_sum_adjoint(kw.pop('databar'), mns, x, y, x_norm=2.0, y_norm=0.5, **kw))
        assert got.dtype == dt and got.shape == (63,)
        assert _rel(got.astype(np.float64), np.array([w[n, m] for m, n in mns])) < TOL[dt]
    # the three together add into one matrix
    tot = tonp(P.cheby1_2d_sum_adjoint(gs[0], mns, x, y, dx_bar=gs[1], dy_bar=gs[2], x_norm=2.0, y_norm=0.5))
    assert _rel(tot.astype(np.float64), np.array([sum(w[n, m] for w in want) for m, n in mns])) < TOL[dt]


def test_separable_adjoint_dot_product_identities():
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(58)
    x, y = np.linspace(-1, 1, 130), np.linspace(-1, 1, 70)
    mns = [(m, n) for m in range(7) for n in range(6)] + [(3, 3)]        # a duplicate receives its entry twice
    c = rng.standard_normal((2, len(mns)))
    gs = rng.standard_normal((3, 2, 70, 130))
    for name, fwd, adj in (('xy', P.xy_sum_der_xy, P.xy_sum_adjoint), ('legendre', P.legendre_2d_sum_der_xy, P.legendre_2d_sum_adjoint)):
        outs = [tonp(a) for a in fwd(c, mns, x, y)]
        singles = [adj(gs[0], mns, x, y), adj(None, mns, x, y, dx_bar=gs[1]), adj(None, mns, x, y, dy_bar=gs[2])]
        for o, g, a in zip(outs, gs, singles):
            lhs, rhs = float(np.vdot(o, g)), float(np.vdot(c, tonp(a)))
            assert tuple(a.shape) == c.shape and abs(lhs - rhs) / abs(lhs) < 1e-12, name
        lhs = sum(float(np.vdot(o, g)) for o, g in zip(outs, gs))
        rhs = float(np.vdot(c, tonp(adj(gs[0], mns, x, y, dx_bar=gs[1], dy_bar=gs[2]))))
        assert abs(lhs - rhs) / abs(lhs) < 1e-12, name


def test_separable_adjoint_is_bitwise_reproducible():
    from prysm_amd import polynomials as P
    x = np.linspace(-1, 1, 512)
    mns = [(m, n) for m in range(12) for n in range(10)]
    g = torch.from_numpy(np.random.default_rng(59).standard_normal((3, 512, 512))).cuda()
    a = P.cheby1_2d_sum_adjoint(g[0], mns, x, x, dx_bar=g[1], dy_bar=g[2]).clone()
    b = P.cheby1_2d_sum_adjoint(g[0], mns, x, x, dx_bar=g[1], dy_bar=g[2]).clone()
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- XY sequences

@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_xy_sequences_match_the_reference(fx, dt):
    from prysm_amd import polynomials as P
    mns = mns_of(fx['xy_mns'])
    assert mns == [P.xy_j_to_mn(j) for j in range(1, 22)]
    x, y = fx['grid_x'].astype(dt), fx['grid_y'].astype(dt)
    for name in ('xy_seq', 'xy_der_x_seq', 'xy_der_y_seq', 'xy_der_xy_seq'):
        got = tonp(getattr(P, name)(mns, x, y))
        assert got.dtype == dt and got.shape == (21, 33, 29)
        assert _rel_per_mode(got.astype(np.float64), fx[name]) < TOL[dt], name
        one = tonp(getattr(P, name[:-4])(2, 1, x, y))
        assert np.array_equal(one, got[mns.index((2, 1))])


# ----------------------------------------------------------------------------- the chain the feature exists for

EFL, WVL, DX, Q = 100.0, 0.6328, 10.0 / 128, 2
MNS4 = [(m, n) for m in range(4) for n in range(4)]


def _model(amp, x, y, target):
    """loss and its gradient with respect to the Legendre-2D coefficients of a square pupil's OPD, all on the device"""
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront

    def run(c):
        opd = P.legendre_2d_sum(c, MNS4, x, y)
        wf = Wavefront.from_amp_and_phase(amp, opd, WVL, DX)
        psf = wf.focus(EFL, Q=Q)
        diff = psf.intensity.data - target
        loss = (diff * diff).sum()
        wbar = psf.intensity_adjoint(2 * diff).focus_adjoint(EFL, Q=Q)
        obar = wf.from_amp_and_phase_adjoint_phase(wbar).imag    # the reference's quirk: the gradient times 1j
        return loss, P.legendre_2d_sum_adjoint(obar, MNS4, x, y)
    return run


def _setup():
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront
    g = (np.arange(128) - 64) / 64
    x = torch.from_numpy(g).cuda()
    amp = torch.ones((128, 128), dtype=torch.float64, device='cuda')
    rng = np.random.default_rng(60)
    c_true = torch.from_numpy(30 * rng.standard_normal(len(MNS4))).cuda()
    c0 = torch.from_numpy(30 * rng.standard_normal(len(MNS4))).cuda()
    target = Wavefront.from_amp_and_phase(amp, P.legendre_2d_sum(c_true, MNS4, x, x), WVL, DX).focus(EFL, Q=Q).intensity.data.clone()
    return amp, x, x, target, c0


def test_psf_loss_gradient_matches_finite_differences():
    amp, x, y, target, c0 = _setup()
    run = _model(amp, x, y, target)
    loss, grad = run(c0)
    grad = tonp(grad)
    h = 1e-2
    for k in (1, 6, 11):
        e = torch.zeros_like(c0)
        e[k] = h
        lp, _ = run(c0 + e)
        lm, _ = run(c0 - e)
        fd = (float(lp) - float(lm)) / (2 * h)
        print(f'recur figure: psf gradient coefficient {k}: {grad[k]:.9e} finite difference {fd:.9e}')
        assert abs(grad[k] - fd) / abs(fd) < 1e-6, (k, grad[k], fd)


def test_graph_replay_of_the_gradient_chain_is_bit_equal():
    from prysm_amd import graph
    amp, x, y, target, c0 = _setup()
    run = _model(amp, x, y, target)
    eager_loss, eager_grad = (t.clone() for t in run(c0))
    model = graph.capture(run, c0)
    loss, grad = model(c0)
    assert torch.equal(loss, eager_loss) and torch.equal(grad, eager_grad)
    # the coefficients are read on the device: a replay with new ones gives the eager answer for them
    c1 = c0 * 0.5
    eager1 = run(c1)[1].clone()
    assert torch.equal(model(c1)[1], eager1)
    assert not torch.equal(eager1, eager_grad)
