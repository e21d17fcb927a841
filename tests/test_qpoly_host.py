"""CPU: the Forbes Q-polynomial host side without a GPU -- the recurrence helpers against the reference fixture, the step table the
kernels walk (a numpy walk of it against the fixture, its layout, seeds and slot guard), the Python argument checks, and the C entry
points' symbols, argument errors and workspace queries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from prysm_amd.polynomials import qpoly_plan as QP

SYMS = ('pm_qpoly_basis', 'pm_qpoly_sum', 'pm_qpoly_project', 'pm_qpoly_project_workspace')


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'qpoly.npz'))


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _nms(a):
    return [tuple(int(v) for v in row) for row in a]


def _rel_per_mode(got, ref):
    ax = tuple(range(1, ref.ndim))
    return np.max(np.max(np.abs(got - ref), axis=ax) / np.max(np.abs(ref), axis=ax))


def _rel(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def test_helpers_match_the_reference(fx):
    for n, (f, g, h) in enumerate(fx['bfs_fgh']):
        assert QP.f_qbfs(n) == pytest.approx(f, rel=1e-14)
        assert QP.g_qbfs(n) == pytest.approx(g, rel=1e-14)
        assert QP.h_qbfs(n) == pytest.approx(h, rel=1e-14)
    for (n, m), (F, G, f, g) in zip(_nms(fx['helper_nm']), fx['q2d_FGfg']):
        assert QP.F_q2d(n, m) == pytest.approx(F, rel=1e-14, abs=1e-300)
        assert QP.G_q2d(n, m) == pytest.approx(G, rel=1e-14, abs=1e-300)
        assert QP.f_q2d(n, m) == pytest.approx(f, rel=1e-14)
        assert QP.g_q2d(n, m) == pytest.approx(g, rel=1e-14, abs=1e-300)
    for (n, m), abc in zip(_nms(fx['abc_nm']), fx['abc']):
        assert np.allclose(QP.abc_q2d(n, m), abc, rtol=1e-14, atol=0)
    with pytest.raises(ZeroDivisionError):
        QP.abc_q2d(1, 1)                        # why |m| = 1 is seeded up to P_3


def test_public_helpers_are_the_plan_module_ones():
    from prysm_amd import polynomials as P
    assert P.f_qbfs is QP.f_qbfs and P.abc_q2d is QP.abc_q2d and P.Q2d_nm_c_to_a_b is QP.Q2d_nm_c_to_a_b


def test_nm_c_to_a_b_matches_the_reference(fx):
    def split(flat, lens):
        out, i = [], 0
        for n in lens:
            out.append(list(flat[i:i + n]))
            i += n
        return out
    for k in (0, 1):
        cm0, ams, bms = QP.Q2d_nm_c_to_a_b(_nms(fx[f'ab{k}_nms']), list(fx[f'ab{k}_coefs']))
        assert list(cm0) == list(fx[f'ab{k}_cm0'])
        assert ams == split(fx[f'ab{k}_a'], fx[f'ab{k}_alen'])
        assert bms == split(fx[f'ab{k}_b'], fx[f'ab{k}_blen'])
    assert QP.Q2d_nm_c_to_a_b([], []) == ([], [], [])


def test_numpy_walk_of_the_radial_tables_matches_the_reference(fx):
    ns = list(range(21))
    assert _rel_per_mode(QP.evaluate(QP.plan(ns, QP.QBFS), fx['u'], None, 21, QP.RADIAL), fx['qbfs_seq']) < 1e-12
    assert _rel_per_mode(QP.evaluate(QP.plan(ns, QP.QCON), fx['u'], None, 21, QP.RADIAL), fx['qcon_seq']) < 1e-12
    # any order of the orders, repeats included
    perm = [7, 0, 20, 3, 3, 1]
    got = QP.evaluate(QP.plan(perm, QP.QBFS), fx['u'], None, len(perm), QP.RADIAL)
    assert _rel_per_mode(got, fx['qbfs_seq'][perm]) < 1e-12


@pytest.mark.parametrize('coords', [QP.CARTESIAN, QP.POLAR])
def test_numpy_walk_of_the_q2d_table_matches_the_reference(fx, coords):
    u, v = (fx['r'], fx['t']) if coords == QP.POLAR else (fx['x'], fx['y'])
    for key, seq in (('nms8', 'q2d_seq8'), ('nms20', 'q2d_seq20'), ('nms_single', 'q2d_single')):
        nms = _nms(fx[key])
        got = QP.evaluate(QP.plan(nms, QP.Q2D), u, v, len(nms), coords)
        assert _rel_per_mode(got, fx[seq]) < 1e-12, key
    for (n, m), want in zip(_nms(fx['nms_single']), fx['q2d_single']):
        got = QP.evaluate(QP.plan([(n, m)], QP.Q2D), u, v, 1, coords)[0]
        assert _rel(got, want) < 1e-12, (n, m)


def test_numpy_walk_float32_tables(fx):
    ns = list(range(21))
    for fam, key in ((QP.QBFS, 'qbfs_seq'), (QP.QCON, 'qcon_seq')):
        got = QP.evaluate(QP.plan(ns, fam, np.float32), fx['u'].astype(np.float32), None, 21, QP.RADIAL)
        assert got.dtype == np.float32 and _rel_per_mode(got.astype(np.float64), fx[key]) < 5e-5
    for key, seq in (('nms8', 'q2d_seq8'), ('nms20', 'q2d_seq20')):
        nms = _nms(fx[key])
        got = QP.evaluate(QP.plan(nms, QP.Q2D, np.float32), fx['x'].astype(np.float32), fx['y'].astype(np.float32), len(nms))
        assert _rel_per_mode(got.astype(np.float64), fx[seq]) < 5e-5


def test_numpy_walk_sums_match_compute_z(fx):
    nb = len(fx['zbfs_coefs'])
    basis = QP.evaluate(QP.plan(range(nb), QP.QBFS), fx['u'], None, nb, QP.RADIAL)
    assert _rel(np.tensordot(fx['zbfs_coefs'], basis, axes=(0, 0)), fx['zbfs']) < 1e-12
    nms = _nms(fx['nms8'])
    basis = QP.evaluate(QP.plan(nms, QP.Q2D), fx['x'], fx['y'], len(nms))
    assert _rel(np.tensordot(fx['z2d_coefs'], basis, axes=(0, 0)), fx['z2d']) < 1e-12


def test_table_layout_and_seeds():
    nms = [(4, 0), (1, -1), (3, 1), (5, 1), (0, 0), (3, 1), (2, -3)]
    t = QP.plan(nms, QP.Q2D)
    assert t.dtype.itemsize == 80 and QP.plan(nms, QP.Q2D, np.float32).dtype.itemsize == 48
    assert sorted(int(s) for s in t['slot'] if s >= 0) == list(range(len(nms)))
    starts = np.flatnonzero(t['op'] & QP.RESET)
    assert list(starts) == [0, 5, 12] and int(np.sum(t['dm'])) == 3
    # |m| = 0: Qbfs, P_0 = 2 and P_1 = 6 - 8x are seeds; Q_0 = P_0 / f_0 = 1, Q_1 = (P_1 - g_0 Q_0) / f_1 = (13 - 16x) / sqrt(19)
    g0 = t[:5]
    assert list(g0['op']) == [QP.RESET | QP.SEED, QP.SEED, QP.ADV, QP.ADV, QP.ADV]
    assert (g0['a'][0], g0['a'][1], g0['b'][1]) == (2.0, 6.0, -8.0) and g0['rf'][0] == 0.5
    assert g0['g'][1] == -0.5 and g0['rf'][1] == pytest.approx(2 / np.sqrt(19), rel=1e-15)
    assert (6.0 - g0['g'][1] * 1.0) * g0['rf'][1] == pytest.approx(13 / np.sqrt(19), rel=1e-15)
    assert list(g0['part']) == [QP.BFS, QP.NONE, QP.NONE, QP.NONE, QP.BFS]
    # |m| = 1: P_0 .. P_3 are seeds (P_3 a cubic), the recurrence starts at n = 4 with abc_q2d(3, 1)
    g1 = t[5:12]
    assert list(g1['op'][:5]) == [QP.RESET | QP.SEED, QP.SEED, QP.SEED, QP.SEED, 0]
    assert tuple(g1[3][['a', 'b', 'c', 'd']]) == (0.5, -6.0, 12.0, -6.4)
    assert g1['op'][5] == QP.ADV and np.allclose(tuple(g1[5][['a', 'b', 'c']]), QP.abc_q2d(3, 1), rtol=1e-15)
    # the duplicate (3, 1) rides on the step of the first one (op 0)
    assert list(g1['slot'][3:5]) == [2, 5] and g1['part'][4] == QP.COS
    assert g1['part'][1] == QP.SIN and g1['slot'][6] == 3
    # Qcon: P_0, P_1 seeds of the Jacobi (0, 4) recurrence in 2x - 1, Q = P
    c = QP.plan([2], QP.QCON)
    assert list(c['op']) == [QP.RESET | QP.SEED, QP.SEED, QP.ADV] and (c['a'][1], c['b'][1]) == (-5.0, 6.0)
    assert np.all(c['g'] == 0) and np.all(c['h'] == 0) and np.all(c['rf'] == 1) and c['part'][2] == QP.CON
    with pytest.raises(TypeError):
        QP.step_dtype(np.float16)
    with pytest.raises(ValueError):
        QP.plan([1], 'zernike')


def test_slot_guard_writes_nothing_outside_the_modes():
    t = QP.plan([(2, 1), (3, -2)], QP.Q2D)
    r = np.linspace(0, 1, 7)
    full = QP.evaluate(t, r, r, 2, QP.POLAR)
    t2 = t.copy()
    t2['slot'][t2['slot'] == 1] = 7
    got = QP.evaluate(t2, r, r, 2, QP.POLAR)
    assert np.array_equal(got[0], full[0]) and not np.any(got[1])


@pytest.mark.parametrize('modes, fam', [([-1], QP.QBFS), ([2.5], QP.QCON), ([(-1, 0)], QP.Q2D), ([(2, 0.5)], QP.Q2D)])
def test_bad_indices_raise_before_anything_else(modes, fam):
    from prysm_amd import polynomials as P
    with pytest.raises(ValueError):
        QP.plan(modes, fam)
    r = np.zeros((4, 4))
    if fam == QP.Q2D:
        calls = (lambda: P.Q2d_seq(modes, r, r), lambda: P.Q2d_sum(np.ones(1), modes, r, r), lambda: P.Q2d_sum_adjoint(r, modes, r, r),
                 lambda: P.Q2d(*modes[0], r, r))
    else:
        fn = P.Qbfs_seq if fam == QP.QBFS else P.Qcon_seq
        calls = (lambda: fn(modes, r), lambda: P.Qcon_sum(np.ones(1), modes, r), lambda: P.Qcon_sum_adjoint(r, modes, r))
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_argument_errors_raise_before_upload():
    # no GPU here: every one of these must be refused by the Python checks, not by a failed upload
    from prysm_amd import polynomials as P
    nms = [(1, 1), (2, 0)]
    a, b = np.zeros((4, 4)), np.zeros((4, 5))
    with pytest.raises(ValueError):
        P.Q2d_sum(np.ones(3), nms, a, a)              # 3 coefficients, 2 modes
    with pytest.raises(ValueError):
        P.Q2d_sum(np.ones((1, 2, 2)), nms, a, a)
    with pytest.raises(ValueError):
        P.Q2d_sum(np.ones(2), nms, a, b)              # coordinates differ in shape
    with pytest.raises(ValueError):
        P.Q2d_seq(nms, a, b)
    with pytest.raises(ValueError):
        P.Q2d_sum_adjoint(a, nms, a, b)
    with pytest.raises(ValueError):
        P.Q2d_sum_adjoint(b, nms, a, a)               # databar does not match the points
    with pytest.raises(ValueError):
        P.Qcon_sum(np.ones((2, 3)), [0, 1], a)
    with pytest.raises(ValueError):
        P.Qcon_sum_adjoint(np.zeros((3, 4, 5)), [0, 1], a)
    with pytest.raises(TypeError):
        P.Q2d_seq(nms, a.astype(complex), a)          # complex coordinates
    with pytest.raises(TypeError):
        P.Qbfs_seq([0, 1], a.astype(np.complex64))
    with pytest.raises(TypeError):
        P.Q2d_sum(np.ones(2, complex), nms, a, a)
    with pytest.raises(TypeError):
        P.Qcon_sum_adjoint(a.astype(complex), [0], a)
    with pytest.raises(TypeError):
        P.compute_z_Q2d([1.0], [], [], a, a.astype(complex))


def test_symbols_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'prysm_amd.h')).read()
    for s in SYMS:
        assert s + '(' in hdr
        assert hasattr(lib, s)
        assert s in L.SIGNATURES
    assert 'PM_QPOLY_RADIAL = 2' in hdr and L.PM_QPOLY_RADIAL == 2


BAD = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation before a launch


@pytest.mark.parametrize('kw, code', [
    (dict(dtype=0), -1), (dict(dtype=7), -1), (dict(coords=3), -1), (dict(coords=-1), -1), (dict(u=None), -1), (dict(v=None), -1),
    (dict(table=None), -1), (dict(out=None), -1), (dict(npts=-1), -1), (dict(nsteps=-1), -1), (dict(nmodes=-1), -1),
])
def test_basis_argument_errors(lib, kw, code):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, coords=L.PM_ZERNIKE_POLAR, npts=16, u=BAD, v=BAD, table=BAD, nsteps=3, nmodes=3, out=BAD)
    a.update(kw)
    assert lib.pm_qpoly_basis(a['dtype'], a['coords'], a['npts'], a['u'], a['v'], a['table'], a['nsteps'], a['nmodes'], a['out'],
                              None) == code
    assert b'pm_qpoly_basis' in lib.pm_last_error()


def test_radial_points_need_no_second_coordinate(lib):
    from prysm_amd import _lib as L
    # v = NULL passes validation for radial points; no points means no launch
    assert lib.pm_qpoly_basis(L.PM_F64, L.PM_QPOLY_RADIAL, 0, BAD, None, BAD, 3, 3, BAD, None) == 0
    assert lib.pm_qpoly_sum(L.PM_F32, L.PM_QPOLY_RADIAL, 0, BAD, None, BAD, 3, 3, 1, BAD, 0, BAD, None) == 0
    # the Zernike entry points do not take them
    assert lib.pm_zernike_basis(L.PM_F64, L.PM_QPOLY_RADIAL, 16, BAD, BAD, BAD, 3, 3, BAD, None) == L.PM_ERR_ARG


@pytest.mark.parametrize('kw', [dict(dtype=1), dict(coords=5), dict(v=None), dict(coefs=None), dict(out=None), dict(batch=-1),
                                dict(npts=-5)])
def test_sum_argument_errors(lib, kw):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F32, coords=L.PM_ZERNIKE_CARTESIAN, npts=16, u=BAD, v=BAD, table=BAD, nsteps=3, nmodes=3, batch=2, coefs=BAD, out=BAD)
    a.update(kw)
    assert lib.pm_qpoly_sum(a['dtype'], a['coords'], a['npts'], a['u'], a['v'], a['table'], a['nsteps'], a['nmodes'], a['batch'],
                            a['coefs'], 0, a['out'], None) == L.PM_ERR_ARG


@pytest.mark.parametrize('kw, code', [
    (dict(dtype=4), -1), (dict(databar=None), -1), (dict(out=None), -1), (dict(batch=-1), -1), (dict(table=None), -1),
    (dict(ws=None), -3), (dict(wsb=8), -3), (dict(nmodes=3000), -2),
])
def test_project_argument_errors(lib, kw, code):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, npts=4096, table=BAD, nmodes=10, batch=2, databar=BAD, out=BAD, ws=BAD, wsb=1 << 24)
    a.update(kw)
    assert lib.pm_qpoly_project(a['dtype'], L.PM_ZERNIKE_CARTESIAN, a['npts'], BAD, BAD, a['table'], 12, a['nmodes'], a['batch'],
                                a['databar'], a['out'], a['ws'], a['wsb'], None) == code


def test_workspace_queries(lib):
    from prysm_amd import _lib as L
    # one partial per (workgroup, b, k); a workgroup covers 256 x 4 points, at most 1024 workgroups
    assert lib.pm_qpoly_project_workspace(L.PM_F64, 1024, 36, 1) == 1 * 36 * 8
    assert lib.pm_qpoly_project_workspace(L.PM_F32, 1025, 36, 3) == 2 * 3 * 36 * 4
    assert lib.pm_qpoly_project_workspace(L.PM_F64, 2048 * 2048, 231, 8) == 1024 * 8 * 231 * 8
    assert lib.pm_qpoly_project_workspace(L.PM_F64, 0, 5, 1) == 5 * 8
    assert lib.pm_qpoly_project_workspace(L.PM_C64, 1024, 36, 1) == 0
    assert lib.pm_qpoly_project_workspace(L.PM_F32, -1, 36, 1) == 0
