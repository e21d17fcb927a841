"""GPU: csrc/modalfit.hip at the C ABI and through prysm_amd.polynomials and Interferogram.pvr.

Exact Gram: integer modes and data make every product and every sum exact in double in any order, so COUNT, G and b must equal numpy's
integers to the bit -- over the ragged sizes, an odd base pointer (element-wise path), a stride above npts, both sides of a 16-block
edge and the mode cap, 0, 1 and 3 data vectors, both halves of the predicate alone and together, a NaN mode value at an invalid point,
and the second trip of the grid-stride loop.  Then determinism, the small algebra against the numpy model on the device's own record,
and the public functions against tests/golden/modalfit.npz in both precisions.  Cases and bounds: tests/modalfit_common.py."""
import numpy as np
import pytest
import torch

import modalfit_common as C
from prysm_amd import _lib as L
from prysm_amd.polynomials import fit_plan as FP

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)
BOTH = L.PM_MODES_GRAM | L.PM_MODES_RHS


@pytest.fixture(scope='module')
def lib():
    return L.load()


@pytest.fixture(scope='module')
def G():
    return C.golden()


def code(dt):
    return L.PM_F32 if np.dtype(dt) == np.float32 else L.PM_F64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_gram(lib, modes, data, mask, ffd, parts=BOTH, nrhs=None, offset=0, stride=None, rec=None):
    """pm_modes_gram on host arrays -> the record on the host.  offset: the planes start that many elements into their buffers (an odd
    offset takes the element-wise path); stride: elements between planes"""
    K, npts = modes.shape
    dt = modes.dtype
    nrhs = data.shape[0] if nrhs is None else nrhs
    stride = npts if stride is None else stride
    mbuf = torch.full((offset + K * stride,), 7.0, dtype=torch.from_numpy(modes).dtype, device='cuda')
    mbuf[offset:].view(K, stride)[:, :npts] = dev(modes)
    dbuf = torch.full((offset + max(nrhs, 1) * stride,), 7.0, dtype=mbuf.dtype, device='cuda')
    dbuf[offset:].view(max(nrhs, 1), stride)[:, :npts] = dev(data[:max(nrhs, 1)])
    mk = dev(mask) if mask is not None else None
    if rec is None:
        rec = torch.full((lib.pm_modes_record_doubles(K, nrhs),), np.nan, dtype=torch.float64, device='cuda')
    ws = L.workspace(lib.pm_modes_gram_workspace(code(dt), K, npts, nrhs))
    item = mbuf.element_size()
    need_data = nrhs > 0 or ffd
    L.check(lib.pm_modes_gram(code(dt), parts, K, npts, mbuf.data_ptr() + offset * item, stride, nrhs,
                              dbuf.data_ptr() + offset * item if need_data else None, stride if nrhs else 0, L.ptr(mk), int(ffd), L.ptr(rec), L.ptr(ws),
                              ws.numel(), L.stream_ptr()))
    torch.cuda.synchronize()
    return rec


def want_gram(modes, data, mask, ffd, nrhs):
    ok = FP.valid(modes.shape[1], mask, data[0] if ffd else None)
    mv = modes[:, ok].astype(np.float64)
    return float(ok.sum()), mv @ mv.T, data[:nrhs][:, ok].astype(np.float64) @ mv.T


def check_exact(rec, K, nrhs, want, label):
    rec = rec.cpu().numpy()
    n, Gm, b = want
    assert rec[L.PM_MODES_REC_COUNT] == n, (label, rec[0], n)
    got_G = FP.piece(rec, 'G', K, nrhs)
    assert np.array_equal(got_G, Gm), (label, np.argwhere(got_G != Gm)[:4])
    assert np.array_equal(FP.piece(rec, 'b', K, nrhs), b.reshape(nrhs, K)), label


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('K', C.EXACT_K)
def test_gram_is_exact_on_integers(lib, dt, K):
    for npts in C.EXACT_NPTS:
        for nrhs in C.EXACT_NRHS:
            modes, data, mask = C.integer_case(K, npts, nrhs, dt)
            # the two halves of the predicate together, with data[0] finite-tested even when no vector is multiplied
            if nrhs:
                rec = run_gram(lib, modes, data, mask, True, nrhs=nrhs)
                check_exact(rec, K, nrhs, want_gram(modes, data, mask, True, nrhs), f'K={K} n={npts} nrhs={nrhs} both')
            else:
                clean = np.where(mask[None, :] != 0, modes, 0).astype(dt)
                rec = run_gram(lib, modes, data, mask, False, parts=L.PM_MODES_GRAM, nrhs=0)
                check_exact(rec, K, 0, want_gram(clean, data, mask, False, 0), f'K={K} n={npts} mask alone')


@pytest.mark.parametrize('dt', DTYPES)
def test_gram_predicate_halves_paths_and_strides(lib, dt):
    K, npts, nrhs = 17, 1027, 3
    modes, data, mask = C.integer_case(K, npts, nrhs, dt)
    nan_at = 3
    assert mask[nan_at] == 0 and np.isnan(modes[0, nan_at])
    # the mask alone: data must then be finite where the mask is set
    d2 = np.where(np.isnan(data), 5, data).astype(dt)
    check_exact(run_gram(lib, modes, d2, mask, False), K, nrhs, want_gram(modes, d2, mask, False, nrhs), 'mask alone')
    # isfinite(data[0]) alone: the NaN of mode 0 moves under a NaN of data[0]
    m2 = modes.copy()
    m2[0, nan_at] = 1
    m2[0, 11] = np.nan
    assert np.isnan(data[0, 11])
    check_exact(run_gram(lib, m2, data, None, True), K, nrhs, want_gram(m2, data, None, True, nrhs), 'finite alone')
    # inf in data[0] is invalid too
    d3 = data.copy()
    d3[0, 5] = np.inf
    check_exact(run_gram(lib, m2, d3, None, True), K, nrhs, want_gram(m2, d3, None, True, nrhs), 'inf')
    # a base pointer one element in (element-wise path) and planes further apart than npts; 1028 points on the 16-byte path
    check_exact(run_gram(lib, modes, data, mask, True, offset=1, stride=npts + 5), K, nrhs, want_gram(modes, data, mask, True, nrhs), 'offset 1')
    mm, dd, kk = C.integer_case(K, 1028, nrhs, dt)
    check_exact(run_gram(lib, mm, dd, kk, True, stride=1032), K, nrhs, want_gram(mm, dd, kk, True, nrhs), 'vector path, stride 1032')
    check_exact(run_gram(lib, mm, dd, kk, True, offset=4 if dt == np.float32 else 2, stride=1032), K, nrhs, want_gram(mm, dd, kk, True, nrhs),
                'vector path, offset of 16 bytes')
    # a NaN at a VALID point propagates into its row and column only
    m4 = np.where(np.isnan(modes), 0, modes).astype(dt)
    valid = np.flatnonzero(FP.valid(npts, mask, data[0]))
    m4[2, valid[7]] = np.nan
    rec = run_gram(lib, m4, data, mask, True).cpu().numpy()
    Gm = FP.piece(rec, 'G', K, nrhs)
    assert np.isnan(Gm[2]).all() and np.isnan(Gm[:, 2]).all() and np.isfinite(np.delete(np.delete(Gm, 2, 0), 2, 1)).all()
    # RHS alone leaves COUNT and G as they are, and 20 vectors take two launches
    big = np.random.default_rng(1).integers(-100, 100, (20, npts), endpoint=True).astype(dt)
    rec = run_gram(lib, m2, big, mask, False)
    before = rec.clone()
    rec = run_gram(lib, m2, (2 * big).astype(dt), mask, False, parts=L.PM_MODES_RHS, rec=rec)
    head = FP.offsets(K, 20)['b'][0]
    assert torch.equal(rec[:head][2:2 + K * K], before[:head][2:2 + K * K]) and rec[0] == before[0]
    assert np.array_equal(FP.piece(rec.cpu().numpy(), 'b', K, 20), 2 * FP.piece(before.cpu().numpy(), 'b', K, 20))
    check_exact(before, K, 20, want_gram(m2, big, mask, False, 20), '20 vectors')


def gram_cap(lib):
    per = lib.pm_modes_gram_workspace(L.PM_F64, 3, 1, 0)
    g = 1
    while lib.pm_modes_gram_workspace(L.PM_F64, 3, FP.TILE * g, 0) // per == g:
        g *= 2
        assert g <= 1 << 22
    return lib.pm_modes_gram_workspace(L.PM_F64, 3, FP.TILE * g, 0) // per


@pytest.mark.parametrize('dt', DTYPES)
def test_gram_second_trip(lib, dt):
    """K = 3 past the workgroup cap: one point of a second trip, and six workgroup tiles of one with a ragged last wave tile"""
    cap = gram_cap(lib)
    for npts in (cap * FP.TILE + 1, cap * FP.TILE + 5 * FP.TILE + 516):
        rng = np.random.default_rng(npts)
        modes = rng.integers(-8, 8, (3, npts), endpoint=True).astype(dt)
        data = rng.integers(-100, 100, (1, npts), endpoint=True).astype(dt)
        data[0, ::13] = np.nan
        mask = (rng.random(npts) < 0.9).astype(np.uint8)
        mask[-1] = 1
        data[0, -1] = 3
        check_exact(run_gram(lib, modes, data, mask, True), 3, 1, want_gram(modes, data, mask, True, 1), f'second trip n={npts}')


@pytest.mark.parametrize('dt', DTYPES)
def test_gram_is_deterministic(lib, dt):
    rng = np.random.default_rng(8)
    K, npts = 37, 70001
    modes = rng.standard_normal((K, npts)).astype(dt)
    data = rng.standard_normal((2, npts)).astype(dt)
    data[0, rng.random(npts) < 0.1] = np.nan
    a = run_gram(lib, modes, data, None, True)
    b = run_gram(lib, modes, data, None, True)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    n, Gm, bm = FP.gram(modes, data, None, True)
    rec = a.cpu().numpy()
    assert rec[0] == n
    scale = np.abs(Gm).max()
    assert np.abs(FP.piece(rec, 'G', K, 2) - Gm).max() <= 64 * C.eps(np.float64) * scale      # sums of 70001 terms in double, any order


@pytest.mark.parametrize('K', (5, 37, 128))
def test_small_algebra_against_the_model(lib, K):
    """FACTOR, SOLVE and INVERT on the device's own record: the same operations in the same order, so the same numbers"""
    rng = np.random.default_rng(K)
    npts, nrhs = 4 * K + 300, 3
    modes = rng.standard_normal((K, npts))
    if K == 37:
        modes[20] = modes[4]           # a dependent mode: dropped
    data = rng.standard_normal((nrhs, npts))
    rec = run_gram(lib, modes, data, None, False)
    coef = torch.empty((nrhs, K), dtype=torch.float64, device='cuda')
    for op in (L.PM_MODES_FACTOR, L.PM_MODES_SOLVE, L.PM_MODES_INVERT):
        L.check(lib.pm_modes_small(L.PM_F64, op, K, nrhs, L.ptr(rec), None, L.ptr(coef), L.stream_ptr()))
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    Lm, drop, rank = FP.factor(FP.piece(r, 'G', K, nrhs))
    assert r[L.PM_MODES_REC_RANK] == rank == (K - 1 if K == 37 else K)
    assert np.array_equal(FP.piece(r, 'drop', K, nrhs), drop)
    C.compare('golden', 'small', FP.piece(r, 'L', K, nrhs), Lm, np.float64, f'factor K={K}')
    x = FP.solve(Lm, drop, FP.piece(r, 'b', K, nrhs))
    C.compare('golden', 'small', FP.piece(r, 'coef', K, nrhs), x, np.float64, f'solve K={K}')
    assert np.array_equal(coef.cpu().numpy(), FP.piece(r, 'coef', K, nrhs))
    C.compare('golden', 'small', FP.piece(r, 'T', K, nrhs), FP.invert(Lm, drop), np.float64, f'invert K={K}')
    # the transform of the cap's worth of modes: all K values of a point in LDS, in place
    mk = dev((rng.random(npts) < 0.7).astype(np.uint8))
    m = dev(modes)
    L.check(lib.pm_modes_transform(L.PM_F64, L.PM_MODES_LOWER, 1, K, npts, L.ptr(m), npts, L.ptr(rec), L.ptr(mk), L.ptr(m), npts, L.stream_ptr()))
    want = FP.transform(FP.piece(r, 'T', K, nrhs), modes, mk.cpu().numpy(), zero_outside=True)
    C.compare('golden', 'small', m.cpu().numpy(), want, np.float64, f'transform in place K={K}')


# ----------------------------------------------------------------------------- the public functions against the golden file
@pytest.mark.parametrize('dt', DTYPES)
def test_lstsq_against_the_reference(G, dt):
    from prysm_amd.polynomials import lstsq
    B, data = C.basis('z37', dt), G['z37_data'].astype(dt)
    got = lstsq(dev(B), dev(data))
    assert got.shape == (37,) and got.dtype == dev(B).dtype and got.is_cuda
    C.compare('golden', 'coef', got.cpu().numpy(), G[f'z37_coef_{C.tag(dt)}'], dt, 'lstsq z37', case='z37')
    again = lstsq([b for b in B], data)          # a sequence of host planes
    assert torch.equal(again, got)


@pytest.mark.parametrize('dt', DTYPES)
def test_orthogonalize_against_the_reference(G, dt):
    from prysm_amd.polynomials import orthogonalize_modes
    A, mask = C.basis('z11a', dt), G['z11a_mask']
    Q = orthogonalize_modes(dev(A), dev(mask)).cpu().numpy()
    assert Q.dtype == dt and not Q[:, ~mask].any() and not np.signbit(Q[:, ~mask]).any()      # exact zeros outside the mask
    C.compare('golden', 'Q', Q[:, mask], G[f'z11a_Q_{C.tag(dt)}'], dt, 'orthogonalize z11a', case='z11a')
    C.check_orthogonality(Q, mask, dt, float(G[f'z11a_ortho_{C.tag(dt)}']), 'device z11a')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('to', ('std', 'ptp'))
def test_normalize_against_the_reference(G, dt, to):
    from prysm_amd.polynomials import normalize_modes
    A, mask = C.basis('z11a', dt), G['z11a_mask']
    f = C.tag(dt)
    got = normalize_modes(dev(A), dev(mask), to=to).cpu().numpy()
    assert got.dtype == dt and got.shape == A.shape
    C.compare('golden', 'norm', got[:, C.NORM_ROWS], G[f'z11a_norm_{to}_3d_{f}'], dt, f'normalize {to} 3-D')
    piston = normalize_modes(dev(A[0]), mask, to=to).cpu().numpy()
    assert piston.shape == A[0].shape and np.array_equal(piston, A[0])      # the loophole
    C.compare('golden', 'norm', normalize_modes(A[4], mask, to=to).cpu().numpy()[C.NORM_ROWS], G[f'z11a_norm_{to}_m4_{f}'], dt, f'normalize {to} mode 4')


@pytest.mark.parametrize('dt', DTYPES)
def test_hopkins(G, dt):
    from prysm_amd.polynomials import hopkins
    for i, (a, b, c) in enumerate(C.HOPKINS):
        got = hopkins(a, b, c, dev(G['z37_r'].astype(dt)), dev(G['z37_t'].astype(dt)), C.HOPKINS_H)
        want = FP.hopkins(a, b, c, G['z37_r'].astype(dt).astype(np.float64), G['z37_t'].astype(dt).astype(np.float64), C.HOPKINS_H)
        assert got.dtype == dev(G['z37_r'].astype(dt)).dtype
        assert np.abs(got.cpu().numpy() - want).max() <= 16 * C.eps(dt) * np.abs(want).max()      # cos, sin and pow of the device's library


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(C.PVR_CASES))
def test_pvr_against_the_reference(G, dt, name):
    from prysm_amd.interferogram import Interferogram
    shape, dx, radius, _ = C.PVR_CASES[name]
    I = Interferogram(dev(G[f'pvr_{name}_data'].astype(dt)), dx=dx)
    got = I.pvr(radius)
    assert isinstance(got, float)
    C.compare('golden', 'pvr', got, float(G[f'pvr_{name}_{C.tag(dt)}']), dt, f'pvr {name}')
    if name == 'rect':
        with pytest.raises(ValueError, match='square'):
            I.pvr()


@pytest.mark.parametrize('dt', DTYPES)
def test_a_duplicated_mode_is_dropped(G, dt):
    from prysm_amd.polynomials import lstsq, orthogonalize_modes, prepare_lstsq
    B, data = C.basis('z37', dt)[:12], G['z37_data'].astype(dt)
    dup = np.concatenate([B[:7], B[2:3], B[7:]])          # mode 7 repeats mode 2
    c = lstsq(dev(dup), dev(data)).cpu().numpy()
    c0 = lstsq(dev(B), dev(data)).cpu().numpy()
    assert c[7] == 0.0 and np.array_equal(np.delete(c, 7), c0)
    mask = np.isfinite(data)
    fit = prepare_lstsq(dev(dup), dev(mask))
    assert fit.rank == 12 and fit.count == mask.sum()
    Q = orthogonalize_modes(dev(dup), dev(mask)).cpu().numpy()
    assert not Q[7].any() and np.array_equal(np.delete(Q, 7, 0), orthogonalize_modes(dev(B), dev(mask)).cpu().numpy())


@pytest.mark.parametrize('dt', DTYPES)
def test_prepared_fit(G, dt):
    from prysm_amd import graph
    from prysm_amd.polynomials import lstsq, prepare_lstsq
    B, data = C.basis('z37', dt), G['z37_data'].astype(dt)
    mask = np.isfinite(data)
    rng = np.random.default_rng(4)
    frames = np.stack([data, np.where(mask, 2 * data + 1, np.nan), np.where(mask, data * rng.standard_normal(data.shape), np.nan)]).astype(dt)
    fit = prepare_lstsq(dev(B), dev(mask))
    assert fit.rank == 37
    got = fit.fit(dev(frames))
    assert got.shape == (3, 37) and got.dtype == dev(B).dtype
    for i in range(3):
        want = lstsq(dev(B), dev(frames[i])).cpu().numpy()
        C.compare('golden', 'frames', got[i].cpu().numpy(), want, dt, f'frame {i} against lstsq', case='z37')
    C.compare('golden', 'coef', fit.fit(dev(data)).cpu().numpy(), G[f'z37_coef_{C.tag(dt)}'], dt, 'prepared fit z37', case='z37')
    # a NaN inside the mask: that frame's coefficients are NaN, the others are untouched
    bad = frames.copy()
    bad[1][tuple(np.argwhere(mask)[50])] = np.nan
    gb = fit.fit(dev(bad)).cpu().numpy()
    assert np.isnan(gb[1]).all() and np.array_equal(gb[[0, 2]], got.cpu().numpy()[[0, 2]])
    # one capture, replayed on new data, equals the eager call
    model = graph.capture(fit.fit, dev(frames))
    fresh = dev((frames[::-1] * 0.5).astype(dt).copy())
    out = model(fresh).clone()
    assert torch.equal(out, fit.fit(fresh))


def test_write_parity_log():
    """last in the file: what the comparisons above measured, for profiles/modalfit/parity.txt (printed; the log is kept by hand)"""
    for row in C.measured:
        print('%-6s %-8s %s %-32s %10.3f eps  bound %8.2f' % row)
