"""CPU: the host side of the recurrence families without a GPU -- the table layout, a numpy walk of every family's table against the
reference fixture in both precisions, the factored separable models and their adjoint identity, the plain host functions, the Python
argument checks, and the C entry points' symbols, argument errors and workspace queries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from prysm_amd.polynomials import recur_plan as RP
from recur_common import CASES, TOL, mns_of as _mns, rel as _rel, rel_per_mode as _rel_per_mode

SYMS = ('pm_recur_basis', 'pm_recur_sum', 'pm_recur_project', 'pm_recur_project_workspace', 'pm_recur2_sum', 'pm_recur2_project',
        'pm_recur2_project_workspace', 'pm_recur2_outer')


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'recur.npz'))


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_table_layout():
    assert RP.step_dtype(np.float32).itemsize == 16 and RP.step_dtype(np.float64).itemsize == 32
    assert RP.step_dtype(np.float64).fields['slot'][1] == 24 and RP.step_dtype(np.float32).fields['slot'][1] == 12
    with pytest.raises(TypeError):
        RP.step_dtype(np.complex64)
    t = RP.plan('legendre', nmax=30)
    assert len(t) == 31 and list(t['slot']) == list(range(31))
    t = RP.plan('jacobi', [2, 5, 30], 0.0, 2.0, dtype=np.float32)
    assert len(t) == 31 and t.dtype.itemsize == 16
    assert [int(t['slot'][n]) for n in (2, 5, 30)] == [0, 1, 2] and int(np.sum(t['slot'] == -1)) == 28
    assert len(RP.plan('cheby1', [])) == 0
    # the seeds: record 0 is (P_0, 0, 0), record 1 has c = 0
    assert tuple(RP.plan('dickson1', None, 0.75, nmax=3)[0])[:3] == (2.0, 0.0, 0.0)
    for fam, params in (('cheby3', ()), ('laguerre', (1.5,)), ('dickson2', (0.75,)), ('jacobi', (0.5, -0.5))):
        t = RP.plan(fam, None, *params, nmax=4)
        assert tuple(t[0])[:3] == (1.0, 0.0, 0.0) and t[1]['c'] == 0
    assert tuple(RP.plan('cheby4', nmax=2)[1])[:2] == (1.0, 2.0) and tuple(RP.plan('cheby2', nmax=2)[2])[:3] == (0.0, 2.0, 1.0)
    t = RP.plan('laguerre', None, 1.5, nmax=3)
    assert tuple(t[2])[:3] == pytest.approx(((1.5 + 3) / 2, -0.5, (1.5 + 1) / 2))
    with pytest.raises(ValueError):
        RP.plan('legendre', [3, 2])
    with pytest.raises(ValueError):
        RP.plan('laguerre', [1, 2])        # alpha missing
    with pytest.raises(ValueError):
        RP.plan('nonesuch', [1])


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('case', sorted(CASES))
def test_numpy_walk_matches_the_reference(fx, case, dt):
    fam, params, xk = CASES[case]
    x = fx[xk]
    val, der = RP.evaluate(RP.plan(fam, None, *params, nmax=30, dtype=dt), x)
    assert val.dtype == dt and val.shape == (31, 65)
    assert _rel_per_mode(val.astype(np.float64), fx[case + '_seq']) < TOL[dt]
    assert _rel_per_mode(der.astype(np.float64), fx[case + '_der_seq']) < TOL[dt]
    val, der = RP.evaluate(RP.plan(fam, [2, 5, 30], *params, dtype=dt), x)
    assert val.shape == (3, 65)
    assert _rel_per_mode(val.astype(np.float64), fx[case + '_sparse_seq']) < TOL[dt]
    assert _rel_per_mode(der.astype(np.float64), fx[case + '_sparse_der_seq']) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_walk_sums_match_the_reference(fx, dt):
    val, _ = RP.evaluate(RP.plan('jacobi', None, 0.0, 2.0, nmax=11, dtype=dt), fx['x_unit'])
    assert _rel(fx['clenshaw_s'] @ val.astype(np.float64), fx['clenshaw']) < TOL[dt]
    R = 1.3
    u = 2 * (fx['rad_x'] ** 2 + fx['rad_y'] ** 2) / R ** 2 - 1
    val, der = (a.astype(np.float64) for a in RP.evaluate(RP.plan('jacobi', None, 0.0, 2.0, nmax=10, dtype=dt), u))
    c = fx['rad_coefs']
    assert _rel(np.tensordot(c, val, 1), fx['rad_z']) < TOL[dt]
    assert _rel(np.tensordot(c, der, 1) * 4 * fx['rad_x'] / R ** 2, fx['rad_zx']) < TOL[dt]
    assert _rel(np.tensordot(c, der, 1) * 4 * fx['rad_y'] / R ** 2, fx['rad_zy']) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_separable_models_match_the_reference(fx, dt):
    mns = _mns(fx['mns'])
    C = RP.coefficient_matrix(fx['c2d'], mns)
    assert C.shape == (7, 9)
    for fam, key, xn, yn in (('cheby1', 'cheby', 2.0, 0.5), ('monomial', 'xy', 1.0, 1.0)):
        xt, yt = RP.plan(fam, nmax=8, dtype=dt), RP.plan(fam, nmax=6, dtype=dt)
        got = RP.separable_sum(xt, yt, C, fx['grid_x'], fx['grid_y'], 1 / xn, 1 / yn)
        for g, name in zip(got, ('_z', '_zx', '_zy')):
            assert g.dtype == dt and g.shape == (33, 29)
            assert _rel(g.astype(np.float64), fx[key + name]) < TOL[dt], (fam, name)
    # duplicates add into one entry
    C2 = RP.coefficient_matrix([1.0, 2.0, 4.0], [(1, 0), (0, 2), (1, 0)])
    assert C2.shape == (3, 2) and C2[0, 1] == 5.0 and C2[2, 0] == 2.0


def test_separable_project_is_the_adjoint_of_the_sum(fx):
    rng = np.random.default_rng(41)
    x, y = fx['grid_x'], fx['grid_y']
    xt, yt = RP.plan('legendre', nmax=8), RP.plan('legendre', nmax=6)
    C = rng.standard_normal((7, 9))
    outs = RP.separable_sum(xt, yt, C, x, y, 0.5, 2.0)
    for out, what in zip(outs, ('z', 'zx', 'zy')):
        g = rng.standard_normal((33, 29))
        lhs = float(np.vdot(out, g))
        rhs = float(np.vdot(C, RP.separable_project(xt, yt, g, x, y, what, 0.5, 2.0)))
        assert abs(lhs - rhs) / abs(lhs) < 1e-12, what
    with pytest.raises(ValueError):
        RP.separable_project(xt, yt, outs[0], x, y, 'zz')


def test_host_functions_match_the_reference(fx):
    from prysm_amd import polynomials as P
    for j, want in zip(range(1, 41), fx['j_to_mn']):
        assert RP.xy_j_to_mn(j) == tuple(want)
    with pytest.raises(ValueError):
        RP.xy_j_to_mn(0)
    for (n, a, b), want in zip(fx['abc_args'], fx['abc']):
        assert RP.recurrence_abc(int(n), a, b) == pytest.approx(tuple(want), rel=1e-15)
    assert P.xy_j_to_mn is RP.xy_j_to_mn and P.jacobi.__name__ == 'jacobi'
    x = np.linspace(-0.9, 0.9, 7)
    assert np.allclose(RP.weight(0.5, 2.0, x), (1 - x) ** 0.5 * (1 + x) ** 2.0)
    ref_names = ['jacobi', 'jacobi_with_der', 'jacobi_seq', 'jacobi_seq_with_der', 'jacobi_der', 'jacobi_der_seq', 'jacobi_sum_clenshaw',
                 'jacobi_radial_sum', 'jacobi_radial_sum_der_xy', 'cheby1_2d_sum', 'cheby1_2d_sum_der_xy', 'xy_j_to_mn', 'xy', 'xy_seq',
                 'xy_der_x', 'xy_der_x_seq', 'xy_der_y', 'xy_der_y_seq', 'xy_der_xy', 'xy_der_xy_seq', 'xy_sum', 'xy_sum_der_xy',
                 'jacobi_radial_sum_adjoint', 'cheby1_2d_sum_adjoint', 'xy_sum_adjoint', 'legendre_2d_sum', 'legendre_2d_sum_der_xy',
                 'legendre_2d_sum_adjoint']
    ref_names += [f + s for f in ('cheby1', 'cheby2', 'cheby3', 'cheby4', 'legendre', 'hermite_He', 'hermite_H', 'laguerre', 'dickson1',
                                  'dickson2') for s in ('', '_seq', '_der', '_der_seq')]
    for name in ref_names:
        assert callable(getattr(P, name)) and name in P.__all__, name


def test_python_argument_checks_fire_before_any_upload():
    from prysm_amd import polynomials as P
    x = np.linspace(-1, 1, 9)
    X, Y = np.meshgrid(x, x)
    with pytest.raises(ValueError, match='ascending'):
        P.legendre_seq([0, 2, 2], x)
    with pytest.raises(ValueError, match='ascending'):
        P.jacobi_der_seq([3, 1], 0.0, 2.0, x)
    with pytest.raises(ValueError):
        P.cheby1(-1, x)
    with pytest.raises(TypeError):
        P.cheby2_seq([0, 1], x.astype(np.complex128))
    with pytest.raises(TypeError):
        P.xy_sum(np.ones(2, dtype=np.complex64), [(0, 0), (1, 0)], X, Y)
    with pytest.raises(ValueError, match='do not match'):
        P.cheby1_2d_sum(np.ones(3), [(0, 0), (1, 0)], X, Y)
    with pytest.raises(ValueError, match='do not match'):
        P.jacobi_radial_sum(np.ones(3), [0, 1], 0.0, 2.0, X, Y, 1.0)
    with pytest.raises(NotImplementedError, match='64'):
        P.legendre_2d_sum(np.ones(2), [(0, 0), (64, 0)], X, Y)
    with pytest.raises(NotImplementedError, match='64'):
        P.xy_sum_adjoint(X, [(0, 0), (0, 64)], X, Y)
    with pytest.raises(NotImplementedError, match='cartesian_grid'):
        P.xy_sum(np.ones(1), [(0, 0)], X, Y, cartesian_grid=False)
    with pytest.raises(NotImplementedError, match='cartesian_grid'):
        P.cheby1_2d_sum_der_xy(np.ones(1), [(0, 0)], X, Y, cartesian_grid=False)
    with pytest.raises(NotImplementedError, match='cartesian_grid'):
        P.xy_seq([(0, 0)], X, Y, cartesian_grid=False)
    with pytest.raises(NotImplementedError, match='alphas'):
        P.jacobi_sum_clenshaw(np.ones(3), 0.0, 0.0, x, alphas=np.zeros((3, 9)))
    with pytest.raises(ValueError):
        P.xy_sum(np.ones(1), [(0, -1)], X, Y)
    with pytest.raises(ValueError, match='does not match'):
        P.cheby1_2d_sum_adjoint(np.ones((4, 4)), [(0, 0)], X, Y)
    with pytest.raises(ValueError, match='radius'):
        P.jacobi_radial_sum(np.ones(2), [0, 1], 0.0, 2.0, X, Y, 0.0)


def test_symbols_are_exported(lib):
    from prysm_amd import _lib
    for s in SYMS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.pm_version() == 107


def test_argument_errors_are_reported_without_a_gpu(lib):
    from prysm_amd import _lib as L
    p = ctypes.c_void_p(16)
    # empty shapes are not an error and launch nothing
    assert lib.pm_recur_basis(L.PM_F64, L.PM_RECUR_X, 0, p, None, 0.0, p, 4, 4, p, None, None) == 0
    assert lib.pm_recur_sum(L.PM_F32, L.PM_RECUR_X, 100, p, None, 0.0, p, 4, 4, 0, p, 0, p, None, None, None) == 0
    assert lib.pm_recur_project(L.PM_F32, L.PM_RECUR_X, 100, p, None, 0.0, p, 4, 0, 1, 0, p, None, 0, p, None, 0, None) == 0
    assert lib.pm_recur2_sum(L.PM_F64, 0, 8, p, p, p, 3, p, 3, 1, p, L.PM_RECUR2_Z, 1.0, 1.0, p, None, None, 8, 0, None) == 0
    assert lib.pm_recur2_project(L.PM_F64, 8, 8, p, p, p, 3, p, 3, 0, L.PM_RECUR2_Z, 1.0, 1.0, p, 8, 64, 0, p, None, 0, None) == 0
    assert lib.pm_recur2_outer(L.PM_F64, 8, 8, 0, p, 3, p, 3, p, p, None) == 0
    # dtypes
    assert lib.pm_recur_basis(L.PM_C64, L.PM_RECUR_X, 8, p, None, 0.0, p, 4, 4, p, None, None) == L.PM_ERR_ARG
    assert b'dtype' in lib.pm_last_error()
    assert lib.pm_recur2_sum(L.PM_C128, 8, 8, p, p, p, 3, p, 3, 1, p, L.PM_RECUR2_Z, 1.0, 1.0, p, None, None, 8, 64, None) == L.PM_ERR_ARG
    assert b'dtype' in lib.pm_last_error()
    assert lib.pm_recur2_outer(L.PM_U8, 8, 8, 1, p, 3, p, 3, p, p, None) == L.PM_ERR_ARG
    # forms, null pointers, the radius
    assert lib.pm_recur_basis(L.PM_F64, 7, 8, p, None, 0.0, p, 4, 4, p, None, None) == L.PM_ERR_ARG
    assert b'form' in lib.pm_last_error()
    assert lib.pm_recur_basis(L.PM_F64, L.PM_RECUR_R2, 8, p, None, 1.0, p, 4, 4, p, None, None) == L.PM_ERR_ARG
    assert b'null' in lib.pm_last_error()
    assert lib.pm_recur_basis(L.PM_F64, L.PM_RECUR_R2, 8, p, p, 0.0, p, 4, 4, p, None, None) == L.PM_ERR_ARG
    assert b'radius' in lib.pm_last_error()
    assert lib.pm_recur_basis(L.PM_F64, L.PM_RECUR_X, 8, p, None, 0.0, p, 4, 4, None, None, None) == L.PM_ERR_ARG
    assert lib.pm_recur_sum(L.PM_F32, L.PM_RECUR_X, 100, p, None, 0.0, p, 4, 4, 1, p, 0, p, None, p, None) == L.PM_ERR_ARG
    assert b'out_dy' in lib.pm_last_error()
    assert lib.pm_recur_sum(L.PM_F32, L.PM_RECUR_X, 100, p, None, 0.0, p, 4, 4, 1, None, 0, p, None, None, None) == L.PM_ERR_ARG
    # a short workspace
    need = lib.pm_recur_project_workspace(L.PM_F64, 5000, 11, 3)
    assert lib.pm_recur_project(L.PM_F64, L.PM_RECUR_X, 5000, p, None, 0.0, p, 11, 11, 3, 0, p, None, 0, p, p, need - 1, None) == L.PM_ERR_WORKSPACE
    assert b'workspace' in lib.pm_last_error()
    with pytest.raises(ValueError):
        L.check(L.PM_ERR_WORKSPACE)
    need = lib.pm_recur2_project_workspace(L.PM_F32, 100, 100, 7, 1)
    assert lib.pm_recur2_project(L.PM_F32, 100, 100, p, p, p, 9, p, 7, 1, L.PM_RECUR2_ZX, 1.0, 1.0, p, 100, 0, 0, p, p, need - 1,
                                 None) == L.PM_ERR_WORKSPACE
    assert lib.pm_recur2_project(L.PM_F32, 100, 100, p, p, p, 9, p, 7, 1, 3, 1.0, 1.0, p, 100, 0, 0, p, p, need, None) == L.PM_ERR_ARG
    assert b'what' in lib.pm_last_error()
    # leading dimension and batch stride
    assert lib.pm_recur2_sum(L.PM_F64, 8, 8, p, p, p, 3, p, 3, 1, p, L.PM_RECUR2_Z, 1.0, 1.0, p, None, None, 7, 64, None) == L.PM_ERR_ARG
    assert b'leading dimension' in lib.pm_last_error()
    assert lib.pm_recur2_sum(L.PM_F64, 8, 8, p, p, p, 3, p, 3, 2, p, L.PM_RECUR2_Z, 1.0, 1.0, p, None, None, 8, 63, None) == L.PM_ERR_ARG
    assert b'batch stride' in lib.pm_last_error()
    assert lib.pm_recur2_sum(L.PM_F64, 8, 8, p, p, p, 3, p, 3, 1, p, L.PM_RECUR2_ZX, 1.0, 1.0, p, None, None, 8, 64, None) == L.PM_ERR_ARG
    assert lib.pm_recur2_sum(L.PM_F64, 8, 8, p, p, p, 3, p, 3, 1, p, 0, 1.0, 1.0, p, None, None, 8, 64, None) == L.PM_ERR_ARG
    # more than 64 orders on an axis
    rc = lib.pm_recur2_sum(L.PM_F64, 8, 8, p, p, p, 65, p, 3, 1, p, L.PM_RECUR2_Z, 1.0, 1.0, p, None, None, 8, 64, None)
    assert rc == L.PM_ERR_UNSUPPORTED and b'64' in lib.pm_last_error()
    with pytest.raises(NotImplementedError):
        L.check(rc)
    assert lib.pm_recur2_project(L.PM_F64, 8, 8, p, p, p, 3, p, 65, 1, L.PM_RECUR2_Z, 1.0, 1.0, p, 8, 64, 0, p, p, 1 << 20,
                                 None) == L.PM_ERR_UNSUPPORTED


def test_workspace_queries_are_host_arithmetic(lib):
    from prysm_amd import _lib as L
    # 1-D projection: one partial per (workgroup of 1024 points, at most 1024 of them, vector, order)
    assert lib.pm_recur_project_workspace(L.PM_F64, 5000, 11, 3) == 5 * 3 * 11 * 8
    assert lib.pm_recur_project_workspace(L.PM_F32, 1 << 22, 31, 1) == 1024 * 31 * 4
    assert lib.pm_recur_project_workspace(L.PM_F32, 0, 31, 1) == 1 * 31 * 4
    assert lib.pm_recur_project_workspace(L.PM_C64, 100, 3, 1) == 0
    # separable adjoint: (stack, chunks of 64 rows, ny, columns padded to whole tiles of 64)
    assert lib.pm_recur2_project_workspace(L.PM_F32, 100, 100, 7, 1) == 2 * 7 * 128 * 4
    assert lib.pm_recur2_project_workspace(L.PM_F64, 33, 29, 7, 3) == 3 * 1 * 7 * 64 * 8
    assert lib.pm_recur2_project_workspace(L.PM_F32, 4096, 4096, 16, 1) == 64 * 16 * 4096 * 4
    assert lib.pm_recur2_project_workspace(L.PM_F64, 70, 130, 64, 2) == 2 * 2 * 64 * 192 * 8
    assert lib.pm_recur2_project_workspace(L.PM_F32, 0, 100, 7, 1) == 0
    assert lib.pm_recur2_project_workspace(L.PM_BOOL, 8, 8, 3, 1) == 0
