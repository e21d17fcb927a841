"""CPU: the Zernike host side without a GPU -- index conventions and norms against the reference fixture, the step table the kernels
walk (a numpy walk of it against the fixture), the Python argument checks, and the C entry points' symbols, argument errors and
workspace queries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from prysm_amd.polynomials import zernike_plan as ZP

SYMS = ('pm_zernike_basis', 'pm_zernike_sum', 'pm_zernike_project', 'pm_zernike_project_workspace', 'pm_modes_dot', 'pm_modes_dot_workspace')


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'zernike.npz'))


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


def test_index_conventions_match_the_reference(fx):
    for j, want in zip(fx['j'], fx['noll']):
        assert ZP.noll_to_nm(int(j)) == tuple(want)
    for j, want in zip(fx['j'], fx['fringe']):
        assert ZP.fringe_to_nm(int(j)) == tuple(want)
    for j, want in zip(fx['j'], fx['ansi']):
        assert ZP.ansi_j_to_nm(int(j)) == tuple(want)
    for (n, m), nf, na, nrm in zip(_nms(fx['nms12']), fx['nm_to_fringe12'], fx['nm_to_ansi12'], fx['norm12']):
        assert ZP.nm_to_fringe(n, m) == nf
        assert ZP.nm_to_ansi_j(n, m) == na
        assert ZP.zernike_norm(n, m) == pytest.approx(nrm, rel=1e-15)
    # the conventions invert each other on their whole range
    for j in range(1, 121):
        assert ZP.nm_to_fringe(*ZP.fringe_to_nm(j)) == j
        assert ZP.nm_to_ansi_j(*ZP.ansi_j_to_nm(j)) == j


def test_public_helpers_are_the_plan_module_ones():
    from prysm_amd import polynomials as P
    assert P.noll_to_nm is ZP.noll_to_nm and P.zernike_norm is ZP.zernike_norm


def test_table_layout_and_order():
    nms = [(4, 0), (1, -1), (3, 1), (1, 1), (2, 0), (3, 1), (6, -2)]
    t = ZP.plan(nms, dtype=np.float64)
    assert t.dtype.itemsize == 48 and ZP.plan(nms, dtype=np.float32).dtype.itemsize == 32
    assert sorted(int(s) for s in t['slot'] if s >= 0) == list(range(len(nms)))
    # |m| never decreases and every group starts with RESET; the z^|m| steps add up to the largest |m|
    starts = np.flatnonzero(t['op'] & ZP.RESET)
    assert starts[0] == 0 and int(np.sum(t['dm'])) == 2
    # (6, -2) has Jacobi order 2 at |m| = 2: orders 0 and 1 are walked without output
    g2 = t[starts[-1]:]
    assert list(g2['part']) == [ZP.NONE, ZP.NONE, ZP.SIN] and list(g2['slot'])[-1] == 6
    # the duplicate (3, 1) rides on the step of the first one (op 0)
    dup = t[t['slot'] == 5][0]
    assert dup['op'] == 0 and dup['part'] == ZP.COS
    with pytest.raises(TypeError):
        ZP.step_dtype(np.float16)


@pytest.mark.parametrize('polar', [False, True])
def test_numpy_walk_of_the_table_matches_the_reference(fx, polar):
    u, v = (fx['r'], fx['t']) if polar else (fx['x'], fx['y'])
    nms = _nms(fx['nms12'])
    got = ZP.evaluate(ZP.plan(nms), u, v, len(nms), polar=polar)
    assert _rel_per_mode(got, fx['seq12']) < 1e-12
    u20, v20 = (fx['r20'], fx['t20']) if polar else (fx['x20'], fx['y20'])
    nms20 = _nms(fx['nms20'])
    assert _rel_per_mode(ZP.evaluate(ZP.plan(nms20), u20, v20, len(nms20), polar=polar), fx['seq20']) < 1e-12
    odd = ZP.evaluate(ZP.plan([tuple(fx['odd_nm'])]), u, v, 1, polar=polar)[0]
    assert np.max(np.abs(odd - fx['odd'])) / np.max(np.abs(fx['odd'])) < 1e-12
    raw = _nms(fx['nms_raw'])
    assert _rel_per_mode(ZP.evaluate(ZP.plan(raw, norm=False), u, v, len(raw), polar=polar), fx['seq_raw']) < 1e-12


def test_numpy_walk_float32_table(fx):
    nms = _nms(fx['nms12'])
    got = ZP.evaluate(ZP.plan(nms, dtype=np.float32), fx['x'], fx['y'], len(nms))
    assert got.dtype == np.float32
    assert _rel_per_mode(got.astype(np.float64), fx['seq12']) < 2e-5


def test_numpy_walk_sums_and_modes_adjoint(fx):
    nms = _nms(fx['nms8'])
    basis = ZP.evaluate(ZP.plan(nms), fx['x'], fx['y'], len(nms))
    for c, want in zip(fx['coefs'], fx['sums']):
        got = np.tensordot(c, basis, axes=(0, 0))
        assert np.max(np.abs(got - want)) / np.max(np.abs(want)) < 1e-12
    adj = np.tensordot(basis, fx['databar'])
    assert np.max(np.abs(adj - fx['modes_adj'])) / np.max(np.abs(fx['modes_adj'])) < 1e-12


@pytest.mark.parametrize('nms', [[(-1, 0)], [(2, 4)], [(3, -5)], [(2, 0), (1, 2)], [(2.5, 0)]])
def test_bad_indices_raise_before_anything_else(nms):
    from prysm_amd import polynomials as P
    with pytest.raises(ValueError):
        ZP.plan(nms)
    r = np.zeros((4, 4))
    for call in (lambda: P.zernike_nm_seq(nms, r, r), lambda: P.zernike_sum(np.ones(len(nms)), nms, r, r),
                 lambda: P.zernike_sum_adjoint(r, nms, r, r)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        P.zernike_nm(*nms[-1], r, r)


def test_argument_errors_raise_before_upload():
    # no GPU here: every one of these must be refused by the Python checks, not by a failed upload
    from prysm_amd import polynomials as P
    nms = [(1, 1), (2, 0)]
    a, b = np.zeros((4, 4)), np.zeros((4, 5))
    with pytest.raises(ValueError):
        P.zernike_sum(np.ones(3), nms, a, a)              # 3 coefficients, 2 modes
    with pytest.raises(ValueError):
        P.zernike_sum(np.ones((2, 3)), nms, a, a)
    with pytest.raises(ValueError):
        P.zernike_sum(np.ones((1, 2, 2)), nms, a, a)
    with pytest.raises(ValueError):
        P.zernike_sum(np.ones(2), nms, a, b)              # coordinates differ in shape
    with pytest.raises(ValueError):
        P.zernike_nm_seq(nms, a, b)
    with pytest.raises(ValueError):
        P.zernike_sum_adjoint(a, nms, a, b)
    with pytest.raises(ValueError):
        P.zernike_sum_adjoint(b, nms, a, a)               # databar does not match the points
    with pytest.raises(TypeError):
        P.zernike_nm_seq(nms, a.astype(complex), a)       # complex coordinates
    with pytest.raises(TypeError):
        P.zernike_sum(np.ones(2), nms, a, a.astype(np.complex64))
    with pytest.raises(TypeError):
        P.zernike_sum(np.ones(2, complex), nms, a, a)
    with pytest.raises(ValueError):
        P.zernike_sum_adjoint(np.zeros((3, 4, 5)), nms, a, a)
    with pytest.raises(ValueError):
        P.sum_of_2d_modes(np.zeros((2, 4, 4)), np.ones(3))    # 3 weights, 2 modes
    with pytest.raises(ValueError):
        P.sum_of_2d_modes_adjoint(np.zeros((2, 4, 4)), b)
    with pytest.raises(TypeError):
        P.sum_of_2d_modes_adjoint(np.zeros((2, 4, 4), complex), a)


def test_symbols_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'prysm_amd.h')).read()
    for s in SYMS:
        assert s + '(' in hdr
        assert hasattr(lib, s)
        assert s in L.SIGNATURES


BAD = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation before a launch


@pytest.mark.parametrize('kw, code', [
    (dict(dtype=0), -1), (dict(dtype=7), -1), (dict(coords=2), -1), (dict(u=None), -1), (dict(table=None), -1), (dict(out=None), -1),
    (dict(npts=-1), -1), (dict(nsteps=-1), -1), (dict(nmodes=-1), -1),
])
def test_basis_argument_errors(lib, kw, code):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, coords=L.PM_ZERNIKE_POLAR, npts=16, u=BAD, v=BAD, table=BAD, nsteps=3, nmodes=3, out=BAD)
    a.update(kw)
    assert lib.pm_zernike_basis(a['dtype'], a['coords'], a['npts'], a['u'], a['v'], a['table'], a['nsteps'], a['nmodes'], a['out'],
                                None) == code
    assert b'pm_zernike_basis' in lib.pm_last_error()


@pytest.mark.parametrize('kw', [dict(dtype=1), dict(coords=-1), dict(v=None), dict(coefs=None), dict(out=None), dict(batch=-1),
                                dict(npts=-5)])
def test_sum_argument_errors(lib, kw):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F32, coords=L.PM_ZERNIKE_CARTESIAN, npts=16, u=BAD, v=BAD, table=BAD, nsteps=3, nmodes=3, batch=2, coefs=BAD, out=BAD)
    a.update(kw)
    assert lib.pm_zernike_sum(a['dtype'], a['coords'], a['npts'], a['u'], a['v'], a['table'], a['nsteps'], a['nmodes'], a['batch'],
                              a['coefs'], 0, a['out'], None) == L.PM_ERR_ARG


@pytest.mark.parametrize('kw, code', [
    (dict(dtype=4), -1), (dict(databar=None), -1), (dict(out=None), -1), (dict(batch=-1), -1), (dict(table=None), -1),
    (dict(ws=None), -3), (dict(wsb=8), -3), (dict(nmodes=3000), -2),
])
def test_project_argument_errors(lib, kw, code):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, npts=4096, table=BAD, nmodes=10, batch=2, databar=BAD, out=BAD, ws=BAD, wsb=1 << 24)
    a.update(kw)
    assert lib.pm_zernike_project(a['dtype'], L.PM_ZERNIKE_CARTESIAN, a['npts'], BAD, BAD, a['table'], 12, a['nmodes'], a['batch'],
                                  a['databar'], a['out'], a['ws'], a['wsb'], None) == code


@pytest.mark.parametrize('kw, code', [
    (dict(dtype=0), -1), (dict(modes=None), -1), (dict(v=None), -1), (dict(out=None), -1), (dict(nmodes=-1), -1), (dict(npts=-1), -1),
    (dict(stride=100), -1), (dict(ws=None), -3), (dict(wsb=4), -3),
])
def test_modes_dot_argument_errors(lib, kw, code):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F32, nmodes=5, npts=1000, modes=BAD, stride=1000, v=BAD, out=BAD, ws=BAD, wsb=1 << 20)
    a.update(kw)
    assert lib.pm_modes_dot(a['dtype'], a['nmodes'], a['npts'], a['modes'], a['stride'], a['v'], a['out'], a['ws'], a['wsb'], None) == code


def test_workspace_queries(lib):
    from prysm_amd import _lib as L
    # projection: one partial per (workgroup, b, k); a workgroup covers 256 x 4 points, at most 1024 workgroups
    assert lib.pm_zernike_project_workspace(L.PM_F64, 1024, 36, 1) == 1 * 36 * 8
    assert lib.pm_zernike_project_workspace(L.PM_F32, 1025, 36, 3) == 2 * 3 * 36 * 4
    assert lib.pm_zernike_project_workspace(L.PM_F64, 2048 * 2048, 231, 8) == 1024 * 8 * 231 * 8
    assert lib.pm_zernike_project_workspace(L.PM_F64, 0, 5, 1) == 5 * 8
    assert lib.pm_zernike_project_workspace(L.PM_C64, 1024, 36, 1) == 0
    # modes dot: one partial per (chunk of 2048 points, k)
    assert lib.pm_modes_dot_workspace(L.PM_F64, 231, 2048 * 2048) == 2048 * 231 * 8
    assert lib.pm_modes_dot_workspace(L.PM_F32, 10, 4097) == 3 * 10 * 4
    assert lib.pm_modes_dot_workspace(L.PM_F32, -1, 4097) == 0
