"""CPU: the host side of the masked modal fits -- the argument checks of every entry point of csrc/modalfit.hip (refused before anything
is launched, so no device is needed), the workspace and record queries, the numpy model of every kernel (prysm_amd/polynomials/
fit_plan.py) against the reference's outputs in tests/golden/modalfit.npz, the reference's ValueErrors and the Python-side TypeError /
ValueError checks, which fire before anything is uploaded.  Cases and bounds: tests/modalfit_common.py."""
import ctypes

import numpy as np
import pytest

import modalfit_common as C
from prysm_amd import _lib as L
from prysm_amd.polynomials import fit_plan as FP

P = ctypes.c_void_p(16)         # never dereferenced
ARG, WS, UNSUPPORTED = L.PM_ERR_ARG, L.PM_ERR_WORKSPACE, L.PM_ERR_UNSUPPORTED
F32, F64 = L.PM_F32, L.PM_F64
BIG = 1 << 40
K, N = 5, 100
BOTH = L.PM_MODES_GRAM | L.PM_MODES_RHS


@pytest.fixture(scope='module')
def lib():
    return L.load()


@pytest.fixture(scope='module')
def G():
    return C.golden()


# name: call(lib, dt, k, p, stride, ws) -> rc, with k the mode count, p the modes pointer, stride the modes' stride, ws the workspace bytes
CALLS = {
    'pm_modes_gram': lambda lib, dt, k, p, st, ws: lib.pm_modes_gram(dt, BOTH, k, N, p, st, 1, P, N, None, 1, P, P, ws, None),
    'pm_modes_small': lambda lib, dt, k, p, st, ws: lib.pm_modes_small(dt, L.PM_MODES_FACTOR, k, 1, p, None, None, None),
    'pm_modes_transform': lambda lib, dt, k, p, st, ws: lib.pm_modes_transform(dt, L.PM_MODES_LOWER, 0, k, N, p, st, P, None, P, N, None),
    'pm_modes_stats': lambda lib, dt, k, p, st, ws: lib.pm_modes_stats(dt, k, N, p, st, None, P, P, ws, None),
}
WITH_WORKSPACE = ('pm_modes_gram', 'pm_modes_stats')
WITHOUT_STRIDE = ('pm_modes_small',)


def refused(lib, rc, code, word):
    assert rc == code, (rc, lib.pm_last_error())
    assert word.encode() in lib.pm_last_error(), lib.pm_last_error()
    with pytest.raises(NotImplementedError if code == UNSUPPORTED else ValueError):
        L.check(rc)


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_point_refusals(lib, name):
    call = CALLS[name]
    for dt in (L.PM_C64, 99):
        refused(lib, call(lib, dt, K, P, N, BIG), ARG, 'dtype')
        refused(lib, call(lib, dt, 0, None, N - 1, 0), ARG, 'dtype')      # the dtype is looked at first
    for dt in (F32, F64):
        refused(lib, call(lib, dt, K, None, N, BIG), ARG, 'null pointer')
        refused(lib, call(lib, dt, 0, P, N, BIG), ARG, 'at least 1')
        refused(lib, call(lib, dt, 129, P, N, BIG), UNSUPPORTED, 'PM_MODES_FIT_MAX')
        assert call(lib, dt, 128, None, N, BIG) == ARG                    # the cap itself passes the count check
        if name not in WITHOUT_STRIDE:
            refused(lib, call(lib, dt, K, P, N - 1, BIG), ARG, 'stride')
        if name in WITH_WORKSPACE:
            refused(lib, call(lib, dt, K, P, N, 7), WS, 'workspace')
            refused(lib, call(lib, dt, K, P, N - 1, 7), ARG, 'stride')    # ... and the shape before the workspace


def test_refusals_of_parts_ops_and_forms(lib):
    refused(lib, lib.pm_modes_gram(F64, 0, K, N, P, N, 1, P, N, None, 1, P, P, BIG, None), ARG, 'parts')
    refused(lib, lib.pm_modes_gram(F64, 4, K, N, P, N, 1, P, N, None, 1, P, P, BIG, None), ARG, 'parts')
    refused(lib, lib.pm_modes_gram(F64, BOTH, K, N, P, N, 1, None, N, None, 0, P, P, BIG, None), ARG, 'null pointer')      # data
    refused(lib, lib.pm_modes_gram(F64, BOTH, K, N, P, N, 1, P, N - 1, None, 0, P, P, BIG, None), ARG, 'stride')           # data_stride
    refused(lib, lib.pm_modes_gram(F64, L.PM_MODES_GRAM, K, N, P, N, 0, None, 0, None, 1, P, P, BIG, None), ARG, 'finite_from_data')
    refused(lib, lib.pm_modes_gram(F64, BOTH, K, N, P, N, -1, P, N, None, 0, P, P, BIG, None), ARG, 'negative')
    refused(lib, lib.pm_modes_gram(F64, BOTH, K, N, P, N, 1, P, N, None, 0, ctypes.c_void_p(12), P, BIG, None), ARG, 'alignment')
    refused(lib, lib.pm_modes_small(F64, 5, K, 1, P, None, None, None), ARG, 'op')
    refused(lib, lib.pm_modes_small(F64, L.PM_MODES_SOLVE, K, 1, P, None, None, None), ARG, 'coefficients')
    refused(lib, lib.pm_modes_small(F64, L.PM_MODES_NORMS_STD, K, 0, P, None, None, None), ARG, 'statistics')
    refused(lib, lib.pm_modes_transform(F64, 2, 0, K, N, P, N, P, None, P, N, None), ARG, 'form')
    refused(lib, lib.pm_modes_transform(F64, L.PM_MODES_LOWER, 1, K, N, P, N, P, None, P, N, None), ARG, 'mask')
    refused(lib, lib.pm_modes_transform(F64, L.PM_MODES_LOWER, 0, K, N, P, N, P, None, P, N - 1, None), ARG, 'stride')    # out_stride
    assert lib.pm_modes_transform(F64, L.PM_MODES_LOWER, 0, K, 0, P, 0, P, None, P, 0, None) == 0                        # no point: nothing to do
    assert lib.pm_modes_small(F32, L.PM_MODES_SOLVE, K, 0, P, None, None, None) == 0                                    # no vector


def test_record_and_workspace_queries(lib):
    for k, nrhs in ((1, 0), (37, 1), (128, 8)):
        assert lib.pm_modes_record_doubles(k, nrhs) == FP.record_doubles(k, nrhs) == 2 + 3 * k * k + k + 2 * nrhs * k
    assert lib.pm_modes_record_doubles(0, 1) == 0 and lib.pm_modes_record_doubles(129, 1) == 0 and lib.pm_modes_record_doubles(4, -1) == 0
    assert lib.pm_modes_gram_workspace(F64, 0, N, 1) == 0 and lib.pm_modes_gram_workspace(F64, 129, N, 1) == 0
    assert lib.pm_modes_gram_workspace(L.PM_C64, K, N, 1) == 0 and lib.pm_modes_gram_workspace(F64, K, 0, 1) == 0
    assert lib.pm_modes_stats_workspace(0, N) == 0 and lib.pm_modes_stats_workspace(129, N) == 0
    # one workgroup per 1024 points until the cap, then flat; the cap is read the way tests/modal_scale_common.py reads the others
    for k, nrhs in ((3, 0), (3, 1), (37, 1), (128, 3)):
        per = lib.pm_modes_gram_workspace(F64, k, 1, nrhs)
        assert per > 0 and lib.pm_modes_gram_workspace(F32, k, 1, nrhs) == per      # the partials are doubles in both precisions
        groups = [lib.pm_modes_gram_workspace(F64, k, n, nrhs) // per for n in (1, 1024, 1025, 5 * 1024, 5 * 1024 + 1)]
        assert groups == [1, 1, 2, 5, 6]
        cap = gram_cap(lib, k, nrhs)
        assert cap == 1024
        assert lib.pm_modes_gram_workspace(F64, k, cap * 1024 + 1, nrhs) == lib.pm_modes_gram_workspace(F64, k, 1 << 30, nrhs) == cap * per
    # the accumulators: 256 doubles per (split, block pair) and one count per workgroup
    assert lib.pm_modes_gram_workspace(F64, 16, 1, 0) == (4 * 256 + 1) * 8                  # one pair, the waves split the points four ways
    assert lib.pm_modes_gram_workspace(F64, 37, 1, 1) == ((6 + 3) * 256 + 1) * 8            # 6 pairs of G, 3 of b
    assert lib.pm_modes_gram_workspace(F64, 128, 1, 100) == ((36 + 8) * 256 + 1) * 8        # vectors beyond 16 take launches of their own
    last = 0
    for n in (1, 255, 256, 257, 1 << 12, 1 << 16, 1 << 20, 1 << 24):
        got = lib.pm_modes_stats_workspace(K, n)
        assert got >= last and got % (K * 5 * 8) == 0
        last = got
    assert lib.pm_modes_stats_workspace(K, 1 << 24) == lib.pm_modes_stats_workspace(K, 1 << 20) == K * 256 * 5 * 8


def gram_cap(lib, k=3, nrhs=0):
    per = lib.pm_modes_gram_workspace(F64, k, 1, nrhs)
    g = 1
    while g <= 1 << 22:
        got = lib.pm_modes_gram_workspace(F64, k, 1024 * g, nrhs) // per
        if got < g:
            return got
        g *= 2
    raise AssertionError('the workgroup count never stops growing')


# ----------------------------------------------------------------------------- the numpy model against the golden file
@pytest.mark.parametrize('dt', (np.float64, np.float32))
def test_model_lstsq(G, dt):
    B = C.basis('z37', dt)
    got = FP.lstsq(B, G['z37_data'].astype(dt))
    assert got.dtype == dt
    C.compare('host', 'coef', got, G[f'z37_coef_{C.tag(dt)}'], dt, 'lstsq z37', case='z37')


@pytest.mark.parametrize('dt', (np.float64, np.float32))
def test_model_orthogonalize(G, dt):
    A, mask = C.basis('z11a', dt), G['z11a_mask']
    Q = FP.orthogonalize_modes(A, mask)
    assert Q.dtype == dt and not Q[:, ~mask].any()
    C.compare('host', 'Q', Q[:, mask], G[f'z11a_Q_{C.tag(dt)}'], dt, 'orthogonalize z11a', case='z11a')
    assert np.any(G['z11a_rdiag'] < 0)       # the reference's raw R flips signs on this case: the convention is really tested
    C.check_orthogonality(Q, mask, dt, float(G[f'z11a_ortho_{C.tag(dt)}']), 'model z11a')


@pytest.mark.parametrize('dt', (np.float64, np.float32))
@pytest.mark.parametrize('to', ('std', 'ptp'))
def test_model_normalize(G, dt, to):
    A, mask = C.basis('z11a', dt), G['z11a_mask']
    f = C.tag(dt)
    C.compare('host', 'norm', FP.normalize_modes(A, mask, to)[:, C.NORM_ROWS], G[f'z11a_norm_{to}_3d_{f}'], dt, f'normalize {to} 3-D')
    piston = FP.normalize_modes(A[0], mask, to)
    assert np.array_equal(piston, A[0])          # the loophole: a norm below 1e-9 counts as 1
    C.compare('host', 'norm', piston[C.NORM_ROWS], G[f'z11a_norm_{to}_piston_{f}'], dt, f'normalize {to} piston')
    C.compare('host', 'norm', FP.normalize_modes(A[4], mask, to)[C.NORM_ROWS], G[f'z11a_norm_{to}_m4_{f}'], dt, f'normalize {to} mode 4')


def test_model_hopkins(G):
    for i, (a, b, c) in enumerate(C.HOPKINS):
        C.compare('host', 'hopkins', FP.hopkins(a, b, c, G['z37_r'], G['z37_t'], C.HOPKINS_H), G[f'hopkins_{i}'], np.float64, f'hopkins {a} {b} {c}')
    assert any(a < 0 for a, _, _ in C.HOPKINS)


def test_model_small_algebra():
    """the factor, the substitutions and the inverse on a random Gram matrix, against numpy; a duplicated mode is dropped"""
    rng = np.random.default_rng(2)
    A = rng.standard_normal((6, 200))
    Gm = A @ A.T
    Lm, drop, rank = FP.factor(Gm)
    assert rank == 6 and not drop.any() and np.allclose(Lm @ Lm.T, Gm, rtol=1e-13) and np.allclose(Lm, np.linalg.cholesky(Gm), rtol=1e-12)
    b = rng.standard_normal((3, 6))
    assert np.allclose(FP.solve(Lm, drop, b), np.linalg.solve(Gm, b.T).T, rtol=1e-10)
    assert np.allclose(FP.invert(Lm, drop) @ Lm, np.eye(6), atol=1e-12)
    A2 = np.vstack([A[:3], A[1], A[3:]])                 # mode 3 repeats mode 1
    L2, d2, r2 = FP.factor(A2 @ A2.T)
    assert r2 == 6 and list(np.flatnonzero(d2)) == [3] and not L2[3].any() and not L2[:, 3].any()
    b2 = rng.standard_normal((1, 7))
    x2 = FP.solve(L2, d2, b2)
    keep = [0, 1, 2, 4, 5, 6]
    assert x2[0, 3] == 0.0 and np.allclose(x2[0, keep], np.linalg.solve(Gm, b2[0, keep]), rtol=1e-10)
    T2 = FP.invert(L2, d2)
    assert not T2[3].any() and not T2[:, 3].any()


def test_model_predicate_is_a_select():
    """NaN at an invalid point leaves no trace; a NaN at a valid point propagates"""
    m, d, mask = C.integer_case(5, 255, 3, np.float64)
    n, Gm, b = FP.gram(m, d, mask, True)
    ok = (mask != 0) & np.isfinite(d[0])
    assert n == ok.sum() and np.isfinite(Gm).all() and np.isfinite(b).all()
    assert np.array_equal(Gm, (m[:, ok] @ m[:, ok].T)) and np.array_equal(b, d[:, ok] @ m[:, ok].T)
    m[1, np.flatnonzero(ok)[0]] = np.nan
    assert np.isnan(FP.gram(m, d, mask, True)[1][1]).all()


# ----------------------------------------------------------------------------- the Python-side checks, before anything is uploaded
def test_python_checks_fire_before_any_upload():
    from prysm_amd import polynomials as PO
    z = np.zeros((4, 5, 6))
    with pytest.raises(TypeError):
        PO.lstsq(z.astype(np.complex128), z[0])
    with pytest.raises(TypeError):
        PO.lstsq(z, z[0].astype(np.complex64))
    with pytest.raises(ValueError):
        PO.lstsq(z, np.zeros((5, 7)))
    with pytest.raises(ValueError):
        PO.lstsq(z[0], z[0])
    with pytest.raises(ValueError):
        PO.lstsq(z[:0], z[0])
    with pytest.raises(NotImplementedError):
        PO.lstsq(np.zeros((129, 2, 2)), np.zeros((2, 2)))
    with pytest.raises(ValueError):
        PO.lstsq([z[0], np.zeros((5, 7))], z[0])
    with pytest.raises(ValueError):
        PO.normalize_modes(z, np.ones((5, 6), dtype=bool), to='rms')
    with pytest.raises(ValueError):
        PO.normalize_modes(z, np.ones((5, 7), dtype=bool))
    with pytest.raises(ValueError):
        PO.normalize_modes(z[0, 0], np.ones((6,), dtype=bool))
    with pytest.raises(TypeError):
        PO.normalize_modes(z.astype(np.complex64), np.ones((5, 6), dtype=bool))
    with pytest.raises(ValueError):
        PO.orthogonalize_modes(z, np.ones((6, 5), dtype=bool))
    with pytest.raises(TypeError):
        PO.orthogonalize_modes(z.astype(np.complex128), np.ones((5, 6), dtype=bool))
    with pytest.raises(ValueError):
        PO.prepare_lstsq(z, np.ones((6, 5), dtype=bool))
    with pytest.raises(NotImplementedError):
        PO.prepare_lstsq(np.zeros((130, 2, 2)), np.ones((2, 2), dtype=bool))


def test_the_references_value_errors():
    """pvr without a radius needs a square map (interferogram.py:771-774): refused from the shape, before the coordinates are made"""
    from prysm_amd.interferogram import Interferogram
    with pytest.raises(ValueError, match='square'):
        Interferogram.pvr_check(C.PVR_CASES['rect'][0], None)
    assert Interferogram.pvr_check((48, 48), None) is None and Interferogram.pvr_check(C.PVR_CASES['rect'][0], 5.5) is None
