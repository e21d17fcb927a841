"""CPU: what tests/test_gpu_cgemm.py leans on, checked without a device.

* The checks of tests/cgemm_common.py notice faults: a numpy model of a tiled 3M product with masked edges and K slabs (tiled_3m below;
  a model of the technique, not a port of csrc/cgemm.hip) reads NaN-framed operands and writes a NaN-framed C, and the exact check must
  fail for each fault planted in it.
* The rounded-data bound holds for a float32 sequential 3M emulation and fails for one on operands rounded to bfloat16.
* The frame builders give the addresses and leading dimensions they claim.
* The argument checks of pm_cgemm, pm_cgemm_abs2 and pm_cgemm_workspace: what each refuses, under which word, and which of two faults
  is reported, i.e. the ORDER of the checks.  Every call is refused or returns 0 for an empty shape before anything is launched, so the
  pointers are never dereferenced (the style of tests/test_entry_args_host.py).
* The operand checks of _ops.cgemm / _ops.cgemm_abs2.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import cgemm_common as G
from prysm_amd import _lib as L

C64, C128 = L.PM_C64, L.PM_C128
ARG, UNSUP = L.PM_ERR_ARG, L.PM_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the checks notice faults

def tiled_3m(fa, fb, fc, opA, opB, M, N, K, alpha, T=4, BK=4, S=2, fault=''):
    """alpha op(A) @ op(B) in float32 by T x T output tiles, K-tiles of BK and S slabs, as three real chains; operands and C are
    cgemm_common frames on the CPU, addressed flat as a kernel would.  Out-of-range rows are clamped to the last row, the K tail to the
    first k of its tile, and both are zeroed before use."""
    a_flat, b_flat, c_buf = fa.buf.numpy().reshape(-1), fb.buf.numpy().reshape(-1), fc.buf.numpy()
    sa, sb = (-1 if opA & 1 else 1), (-1 if opB & 1 else 1)
    if fault == 'conj on the wrong operand':
        sa, sb = sb, sa

    def tile(flat, f, kfast, r0, R, k0, kend):
        r, k = np.arange(r0, r0 + T), np.arange(k0, k0 + BK)
        rok, kok = r < R, k < kend
        rc = np.where(rok, r, R - 1)
        kc = k if fault == 'K tail read past the edge' else np.where(kok, k, k0)
        at = (1 + rc[:, None]) * f.ld + f.off + kc[None, :] if kfast else (1 + kc[None, :]) * f.ld + f.off + rc[:, None]
        keep = (rok[:, None] | (fault == 'rows not zeroed')) & (kok[None, :] | fault.startswith('K tail'))
        t = np.where(keep, flat[at], 0)
        return t.real.astype(np.float32), t.imag.astype(np.float32)

    ksplit = -(-(-(-K // S)) // BK) * BK
    slabs = list(range(-(-K // ksplit)))
    slabs = slabs[:-1] if fault == 'dropped slab' else slabs + slabs[-1:] if fault == 'doubled slab' else slabs
    ntm, ntn = -(-M // T), -(-N // T)
    for l in range(ntm * ntn):
        tn, tm = divmod(l, ntm)
        if fault == 'tm and tn swapped':
            tm, tn = tn, tm
        m0, n0 = tm * T, tn * T
        p1 = p2 = p3 = np.zeros((T, T), np.float32)
        for s in slabs:
            kend = min((s + 1) * ksplit, K)
            for k0 in range(s * ksplit, kend, BK):
                ar, ai = tile(a_flat, fa, not opA & 2, m0, M, k0, kend)
                br, bi = tile(b_flat, fb, bool(opB & 2), n0, N, k0, kend)
                p1, p2, p3 = p1 + ar @ br.T, p2 + ai @ bi.T, p3 + (ar + sa * ai) @ (br + sb * bi).T
        ss = sa if fault == 'sa sb replaced by sa' else sa * sb
        c = np.float32(alpha) * ((p1 - ss * p2) + 1j * (p3 - p1 - ss * p2))
        rows, cols = np.arange(m0, m0 + T), np.arange(n0, n0 + T)
        ok = (rows[:, None] < M) & (cols[None, :] < N + (fault == 'store one column past N'))
        rr, cc = np.nonzero(ok)
        c_buf[1 + rows[rr], fc.off + cols[cc]] = c[rr, cc]


def _model_case(opA, opB, fault, M=9, N=6, K=7):
    """the model on exact data in wide frames (K = 7 in two slabs: a full K-tile, then a short slab that is one K-tile with a tail of 3)"""
    rng = np.random.default_rng(7)
    sa, sb = G.stored_shapes(opA, opB, M, N, K)
    A, B = G.exact_operand(rng, sa, np.complex64), G.exact_operand(rng, sb, np.complex64)
    fa, fb = G.framed(A, 'wide-aligned', 'cpu'), G.framed(B, 'wide-aligned', 'cpu')
    fc = G.out_frame(M, N, np.complex64, 'cpu')
    tiled_3m(fa, fb, fc, opA, opB, M, N, K, -0.5, fault=fault)
    got = G.read_out(fc)
    G.assert_exact(got, G.exact_ref(A, B, opA, opB, -0.5), fault or 'sound')
    return got


@pytest.mark.parametrize('opA,opB', G.OPS)
def test_the_sound_model_passes_the_exact_check(opA, opB):
    _model_case(opA, opB, '')


# fault -> an op pair at which it changes the result (a conjugation fault needs exactly one conjugated operand to show)
FAULTS = {'K tail not zeroed': (0, 0), 'K tail read past the edge': (2, 3), 'dropped slab': (3, 1), 'doubled slab': (1, 2),
          'sa sb replaced by sa': (0, 1), 'conj on the wrong operand': (1, 0), 'tm and tn swapped': (2, 2), 'store one column past N': (0, 3)}


@pytest.mark.parametrize('fault', list(FAULTS))
def test_the_exact_check_notices_a_planted_fault(fault):
    with pytest.raises(AssertionError):
        _model_case(*FAULTS[fault], fault)


@pytest.mark.parametrize('opA,opB', [(0, 0), (2, 2), (0, 2), (2, 0)])
def test_a_k_tail_read_past_the_edge_meets_the_nan_frame(opA, opB):
    """reading the K tail where it lies instead of clamping it lands in the frame (the guard column of the next row, or the guard row
    below), and unzeroed that NaN reaches every element of the result"""
    with pytest.raises(AssertionError, match='nan'):
        _model_case(opA, opB, 'K tail read past the edge')


def test_unzeroed_clamped_rows_change_no_stored_element():
    """What no output check can see, stated so that nobody looks for it: rows of a tile past M (or N) are clamped to the last row, and
    whether they are then zeroed or not only changes rows of the product that are never stored.  The zeroing is not a correctness
    matter; the clamp is (it keeps the reads inside the matrix)."""
    for opA, opB in G.OPS:
        _model_case(opA, opB, 'rows not zeroed')


# ------------------------------------------------------------------------------------------------ the rounded bound

def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _emulate_3m(A, B, alpha, rnd=lambda x: x):
    """three float32 chains summed sequentially over k"""
    ar, ai, br, bi = (rnd(np.ascontiguousarray(x, dtype=np.float32)) for x in (A.real, A.imag, B.real, B.imag))
    p1 = p2 = p3 = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        p1 = p1 + np.outer(ar[:, k], br[k])
        p2 = p2 + np.outer(ai[:, k], bi[k])
        p3 = p3 + np.outer(ar[:, k] + ai[:, k], br[k] + bi[k])
    al = np.float32(alpha)
    return ((p1 - p2) * al) + 1j * ((p3 - p1 - p2) * al)


@pytest.mark.parametrize('K', [17, 64])
def test_rounded_bound_passes_float32_and_fails_bfloat16(K):
    rng = np.random.default_rng(K)
    A, B = G.crandn(rng, (65, K), np.complex64), G.crandn(rng, (K, 63), np.complex64)
    r32 = G.rounded_ratio(_emulate_3m(A, B, 0.37), A, B, 0, 0, 0.37, 1, G.EPS[C64])
    r16 = G.rounded_ratio(_emulate_3m(A, B, 0.37, _bf16), A, B, 0, 0, 0.37, 1, G.EPS[C64])
    print(f'K = {K}: float32 3M emulation at {r32:.3g} of the bound, bfloat16 operands at {r16:.3g}')
    assert r32 <= 1.0 < r16


# ------------------------------------------------------------------------------------------------ the frame builders

@pytest.mark.parametrize('np_dtype', [np.complex64, np.complex128])
@pytest.mark.parametrize('rows,row', [(64, 16), (5, 48), (1, 64), (0, 64), (64, 0), (7, 17)])
def test_frames_are_where_they_claim(np_dtype, rows, row):
    vals = G.exact_operand(np.random.default_rng(1), (rows, row), np_dtype)
    item = np.dtype(np_dtype).itemsize
    for kind, (pad, off) in G.FRAMES.items():
        if row + pad == 0:
            continue        # a packed frame of empty rows has no bytes
        f = G.framed(vals, kind, 'cpu')
        assert f.ld == row + pad and f.ptr == f.buf.data_ptr() + (f.ld + off) * item and f.residue == f.ptr % 16
        assert np.array_equal(f.view.numpy(), vals) and tuple(f.view.shape) == (rows, row)
        host = f.buf.numpy().copy()
        host[1:1 + rows, off:off + row] = 0
        assert np.isnan(host.real).sum() == host.size - rows * row        # everything around the interior is NaN
        if item == 8 and row % 2 == 0:
            want = {'packed': (0, 0), 'wide-aligned': (0, 0), 'unaligned-base': (8, 0), 'unaligned-ld': (0, 1)}[kind]
            assert (f.residue, f.ld % 2) == want, kind
        if item == 16:
            assert f.residue == 0
    o = G.out_frame(3, 5, np_dtype, 'cpu')
    assert o.ld == 5 + G.OUT_PAD and np.isnan(o.buf.numpy().real).all() and np.isnan(o.buf.numpy().imag).all()


def test_read_out_notices_a_write_outside_the_interior():
    o = G.out_frame(3, 5, np.float32, 'cpu', np.zeros((3, 5)))
    assert np.array_equal(G.read_out(o), np.zeros((3, 5)))
    o.buf[1, 0] = float('nan')          # the same NaN the frame holds, bit for bit: nothing changed
    G.read_out(o)
    o.buf[4, 2] = 1.0
    with pytest.raises(AssertionError, match='outside'):
        G.read_out(o)


# ------------------------------------------------------------------------------------------------ argument checks

@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


P = ctypes.c_void_p(16)        # never dereferenced
BIGLD = 1 << 22


def _gemm(lib, dt=C64, opA=0, opB=0, M=64, N=64, K=64, A=P, B=P, C=P, lda=64, ldb=64, ldc=64):
    return lib.pm_cgemm(dt, opA, opB, M, N, K, 1.0, A, lda, B, ldb, C, ldc, None, 0, None)


def _abs2(lib, dt=C64, opA=0, opB=0, M=64, N=64, K=64, A=P, B=P, C=P, lda=64, ldb=64, ldc=64):
    return lib.pm_cgemm_abs2(dt, opA, opB, M, N, K, 1.0, A, lda, B, ldb, C, ldc, 1.0, 0, None, 0, None)


# label: (knobs, rc, word of pm_last_error).  The order of pm_cgemm's checks: null buffers; sizes and ops; the empty shape; leading
# dimensions of 2^22 or more; the dtype; leading dimensions below the stored row (lda, ldb, ldc in that order).
GEMM_ROWS = {
    'null A': (dict(A=None), ARG, 'null buffer'), 'null B': (dict(B=None), ARG, 'null buffer'), 'null C': (dict(C=None), ARG, 'null buffer'),
    'negative M': (dict(M=-1), ARG, 'bad argument'), 'negative N': (dict(N=-1), ARG, 'bad argument'),
    'negative K': (dict(K=-1), ARG, 'bad argument'), 'opA 4': (dict(opA=4), ARG, 'bad argument'), 'opA -1': (dict(opA=-1), ARG, 'bad argument'),
    'opB 4': (dict(opB=4), ARG, 'bad argument'), 'opB -1': (dict(opB=-1), ARG, 'bad argument'),
    'dtype 99': (dict(dt=99), ARG, 'dtype'), 'a real dtype': (dict(dt=L.PM_F32), ARG, 'dtype'),
    'lda 2^22': (dict(lda=BIGLD), UNSUP, 'leading dimensions'), 'ldb 2^22': (dict(ldb=BIGLD), UNSUP, 'leading dimensions'),
    'lda 2^22 - 1 is not refused for its size': (dict(lda=BIGLD - 1, dt=99), ARG, 'dtype'),
    'no row': (dict(M=0), 0, None), 'no column': (dict(N=0), 0, None),
    'the null buffer before the sizes': (dict(A=None, M=-1), ARG, 'null buffer'),
    'the null buffer before the empty shape': (dict(C=None, M=0), ARG, 'null buffer'),
    'the ops before the empty shape': (dict(opB=7, N=0), ARG, 'bad argument'),
    'the empty shape before the leading dimensions': (dict(M=0, lda=BIGLD), 0, None),
    'the empty shape before the dtype': (dict(N=0, dt=99), 0, None),
    'the empty shape before the short row': (dict(M=0, lda=1, ldb=1, ldc=1), 0, None),
    'the sizes before the leading dimensions': (dict(K=-1, ldb=BIGLD), ARG, 'bad argument'),
    'the leading dimensions before the dtype': (dict(dt=99, ldb=BIGLD), UNSUP, 'leading dimensions'),
    'the leading dimensions before the short row': (dict(lda=BIGLD, ldb=63), UNSUP, 'leading dimensions'),
    'the dtype before the short row': (dict(dt=99, lda=63), ARG, 'dtype'),
    'lda below K': (dict(lda=63), ARG, 'lda'), 'lda below M for a transposed A': (dict(opA=2, M=128, lda=127, ldc=64), ARG, 'lda'),
    'ldb below N': (dict(ldb=63), ARG, 'ldb'), 'ldb below K for a transposed B': (dict(opB=3, K=128, lda=128, ldb=127), ARG, 'ldb'),
    'ldc below N': (dict(ldc=63), ARG, 'ldc'), 'complex128 too': (dict(dt=C128, ldc=0), ARG, 'ldc'),
    'lda before ldb': (dict(lda=1, ldb=1, ldc=1), ARG, 'lda'), 'ldb before ldc': (dict(ldb=1, ldc=1), ARG, 'ldb'),
    'one stored row of A has no leading dimension': (dict(M=1, lda=0, ldb=63), ARG, 'ldb'),
    'one stored row of B has no leading dimension': (dict(K=1, lda=1, ldb=0, ldc=63), ARG, 'ldc'),
    'one stored row of a transposed B': (dict(opB=2, N=1, ldb=0, ldc=0), ARG, 'ldc'),
}

# pm_cgemm_abs2: null buffers; sizes and ops; the empty shape; the dtype; the LDS-DMA predicate (PM_ERR_UNSUPPORTED); the short rows
ABS2_ROWS = {
    'null A': (dict(A=None), ARG, 'null buffer'), 'null B': (dict(B=None), ARG, 'null buffer'), 'null R': (dict(C=None), ARG, 'null buffer'),
    'negative M': (dict(M=-1), ARG, 'bad argument'), 'negative N': (dict(N=-1), ARG, 'bad argument'),
    'negative K': (dict(K=-1), ARG, 'bad argument'), 'opA 4': (dict(opA=4), ARG, 'bad argument'), 'opB -1': (dict(opB=-1), ARG, 'bad argument'),
    'dtype 99': (dict(dt=99), ARG, 'dtype'), 'a real dtype': (dict(dt=L.PM_F64), ARG, 'dtype'),
    'no row': (dict(M=0), 0, None), 'no column': (dict(N=0), 0, None),
    'the empty shape before the dtype': (dict(M=0, dt=99), 0, None), 'an empty complex128 call': (dict(N=0, dt=C128), 0, None),
    'the null buffer before the empty shape': (dict(B=None, N=0), ARG, 'null buffer'),
    'the sizes before the dtype': (dict(N=-1, dt=99), ARG, 'bad argument'),
    'complex128': (dict(dt=C128), UNSUP, 'LDS-DMA'), 'ragged K': (dict(K=63), UNSUP, 'LDS-DMA'), 'K below a K-tile': (dict(K=8), UNSUP, 'LDS-DMA'),
    'no K': (dict(K=0), UNSUP, 'LDS-DMA'), 'M below a tile': (dict(M=32, N=64), UNSUP, 'LDS-DMA'), 'ragged M': (dict(M=65), UNSUP, 'LDS-DMA'),
    'ragged N': (dict(N=96), UNSUP, 'LDS-DMA'), 'odd lda': (dict(lda=65), UNSUP, 'LDS-DMA'), 'odd ldb': (dict(ldb=65), UNSUP, 'LDS-DMA'),
    'A at 8 mod 16': (dict(A=ctypes.c_void_p(24)), UNSUP, 'LDS-DMA'), 'B at 8 mod 16': (dict(B=ctypes.c_void_p(40)), UNSUP, 'LDS-DMA'),
    'lda 2^22': (dict(lda=BIGLD), UNSUP, 'LDS-DMA'), 'ldb 2^22': (dict(ldb=BIGLD), UNSUP, 'LDS-DMA'),
    'the dtype before the shape': (dict(dt=99, K=63), ARG, 'dtype'),
    'the shape before the short row': (dict(K=63, lda=2), UNSUP, 'LDS-DMA'), 'the alignment before the short row': (dict(lda=63), UNSUP, 'LDS-DMA'),
    'lda below K': (dict(lda=62), ARG, 'lda'), 'ldb below N': (dict(ldb=62), ARG, 'ldb'), 'ldr below N': (dict(ldc=63), ARG, 'ldr'),
    'ldb below K for a transposed B': (dict(opB=2, K=128, lda=128, ldb=126), ARG, 'ldb'), 'lda before ldr': (dict(lda=2, ldc=1), ARG, 'lda'),
}


def _expect(lib, name, rc, want_rc, word, what):
    msg = lib.pm_last_error().decode()
    assert rc == want_rc, (name, what, rc, msg)
    if want_rc:
        assert (name + ':') in msg and word in msg, (name, what, msg)


@pytest.mark.parametrize('label', list(GEMM_ROWS))
def test_pm_cgemm_argument_checks(lib, label):
    knobs, rc, word = GEMM_ROWS[label]
    _expect(lib, 'pm_cgemm', _gemm(lib, **knobs), rc, word, label)


@pytest.mark.parametrize('label', list(ABS2_ROWS))
def test_pm_cgemm_abs2_argument_checks(lib, label):
    knobs, rc, word = ABS2_ROWS[label]
    _expect(lib, 'pm_cgemm_abs2', _abs2(lib, **knobs), rc, word, label)


def test_pm_cgemm_workspace_sizes(lib):
    """the slab counts tests/test_gpu_cgemm.py relies on, from the query alone (default knobs): the register-staged kernel's for both
    precisions, and the larger of the two kernels' for a complex64 shape that the LDS-DMA kernel may take"""
    for (M, N, K), S in {(65, 65, 1000): 4, (65, 65, 1030): 8, (65, 65, 257): 2, (65, 65, 256): 2, (65, 65, 255): 0, (65, 33, 300): 2,
                         (1, 1, 1): 0, (65, 65, 0): 0, (0, 64, 4096): 0}.items():
        assert lib.pm_cgemm_workspace(C64, M, N, K) == S * M * N * 8, (M, N, K)
        assert lib.pm_cgemm_workspace(C128, M, N, K) == S * M * N * 16, (M, N, K)
    assert lib.pm_cgemm_workspace(C64, 64, 64, 1024) == 16 * 64 * 64 * 8          # 16 LDS-DMA slabs against 8 staged ones
    assert lib.pm_cgemm_workspace(C128, 64, 64, 1024) == 8 * 64 * 64 * 16
    with L.tuning_local(gemm_dma=0):
        assert lib.pm_cgemm_workspace(C64, 64, 64, 1024) == 8 * 64 * 64 * 8
        assert lib.pm_cgemm_workspace(C64, 64, 64, 8200) == 32 * 64 * 64 * 8
    with L.tuning_local(**G.SLABS):
        for K, S in {192: 2, 256: 4, 320: 4, 272: 0}.items():
            assert lib.pm_cgemm_workspace(C64, 64, 64, K) == S * 64 * 64 * 8, K
    assert lib.pm_cgemm_workspace(C64, 64, 64, 1024) == 16 * 64 * 64 * 8          # the thread's knobs are back


# ------------------------------------------------------------------------------------------------ _ops.cgemm's operand checks

@pytest.mark.parametrize('fn', ['cgemm', 'cgemm_abs2'])
def test_ops_cgemm_refuses_operands_the_library_cannot_see(lib, fn):
    """two pointers say nothing of dtype, device, rank or inner stride: a complex128 B behind a complex64 A would be read as the wrong
    bytes.  Every case raises before the library is called (CPU and meta tensors here)."""
    from prysm_amd import _ops
    f = getattr(_ops, fn)
    a = torch.zeros((64, 64), dtype=torch.complex64)
    with pytest.raises(ValueError, match='same dtype'):
        f(a, a.to(torch.complex128))
    with pytest.raises(ValueError, match='same device'):
        f(a, torch.empty((64, 64), dtype=torch.complex64, device='meta'))
    wide = torch.zeros((64, 128), dtype=torch.complex64)
    with pytest.raises(ValueError, match='unit inner stride'):
        f(wide[:, ::2], a)
    with pytest.raises(ValueError, match='unit inner stride'):
        f(a, a.T)
    with pytest.raises(ValueError, match='2-D'):
        f(a[0], a)
    with pytest.raises(ValueError, match='2-D'):
        f(a, a[None])
    with pytest.raises(ValueError, match='inner dimensions'):      # the check that was there before, after the new ones
        f(a, wide, 0, 2)
