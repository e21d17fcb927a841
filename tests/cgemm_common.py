"""What tests/test_cgemm_host.py and tests/test_gpu_cgemm.py share: operands stored inside NaN frames, exact and rounded data, the numpy
references, the checks, and one call of pm_cgemm / pm_cgemm_abs2 with everything around it asserted.  Imports without a GPU.

Frames.  An operand of `rows` stored rows of `row` elements lies inside a buffer of rows + 2 rows of ld = row + pad elements, filled with
NaN, at row 1 and column `off`: one guard row above and below, pad - off guard columns behind every row and `off` in front of it.
  packed          pad 0, off 0
  wide-aligned    pad 2, off 2   complex64 with an even row: base 0 mod 16, ld even -- what the LDS-DMA kernel asks of an operand
  unaligned-base  pad 2, off 1   complex64 with an even row: base 8 mod 16, ld even
  unaligned-ld    pad 1, off 1   complex64 with an even row: base 0 mod 16, ld odd
A kernel that reads past the K edge of an operand where it lies, instead of clamping and zeroing, multiplies a NaN in.  The output (C, or the real image R) is the
interior of such a frame too (pad 3, off 1, so ldc > N and ldc is neither N nor a multiple of anything the kernels tile by); every bit
outside the M x N interior is compared with what it was before the call.

Exact data.  Real and imaginary parts are independent integers in [-3, 3], alpha is 1, -0.5 or 2.  The 3M chains sum products of
|Ar| <= 3, |Ai| <= 3 and |Ar + Ai| <= 6 with the same of B: no partial sum exceeds 36 K, below 2^24 for K <= 8200, so every product,
partial sum, slab sum, K-group sum and the scaling by alpha is exact in float32 and float64 in ANY order.  The reference is the int64
product of the op'ed integer matrices times alpha and the check is np.array_equal: no tolerance, nothing left out.
For the |.|^2 epilogue the parts are in [-2, 2], alpha 1 or 0.5, weight 1 or 2: |Re c|, |Im c| <= 8 K, so weight |alpha c|^2 <=
2 * 2 * (8 K)^2, 2^20 at K = 64 and 2^22 at K = 128 (the shortest K that the slab form of the LDS-DMA kernel takes: two slabs of 64),
a multiple of 1/4 -- exact below 2^24, and so is the sum with a preset image of small integers.

Rounded data (accuracy only: an exact-integer pass would not notice a lower-precision path).  Normal operands, alpha = 0.37, against
numpy complex128, real and imaginary part separately:
  |err| <= 2 (K + 8 + S) eps |alpha| sum_k (|Ar| + |Ai|)(|Br| + |Bi|),   eps = 2^-24 / 2^-53, S the number of slabs (K-groups)
the worst-case forward bound of the three chains (K adds each, of terms bounded by the products of the operand sums), the operand sums,
the two subtractions, the S slab adds and alpha; derived, not measured.  The float32 sequential 3M emulation of
tests/test_cgemm_host.py (products rounded before they are added) reaches 5.3e-2 of it at K = 17 and 1.5e-2 at K = 64; the same with
operands rounded to bfloat16 exceeds it 432 and 82 times.  It loosens with K, which is why the rounded cases stay short and the exact
data carries the long K.

Routes.  pm_cgemm_abs2 accepts a call exactly when pm_cgemm takes the LDS-DMA kernel for it (one predicate), so a complex64 case asks it,
writing into a scratch image; pm_cgemm_workspace / (M N itemsize) is the slab count the query planned.  Forms are forced with
_lib.tuning_local, never the process-wide setter.

Worst |err| / bound of the rounded data per route on an MI355X (tests/test_gpu_cgemm.py::test_accuracy prints them): RECORDED below.
"""
import types

import numpy as np
import torch

from prysm_amd import _lib as L

C64, C128 = L.PM_C64, L.PM_C128
NP_OF = {C64: np.complex64, C128: np.complex128}
ITEM = {C64: 8, C128: 16}
EPS = {C64: 2.0 ** -24, C128: 2.0 ** -53}
OPS = [(a, b) for a in range(4) for b in range(4)]
ALPHAS = (1.0, -0.5, 2.0)
FRAMES = {'packed': (0, 0), 'wide-aligned': (2, 2), 'unaligned-base': (2, 1), 'unaligned-ld': (1, 1)}
OUT_PAD, OUT_OFF = 3, 1

# the four-wave 64 x 64, the 128 x 128, the eight-wave and the slab form of the LDS-DMA kernel; staged: the register-staged kernel
FOUR = dict(gemm_tile=64, gemm_dma_wgs=1)
BIG = dict(gemm_tile=128, gemm_dma_wgs=1)
EIGHT = dict(gemm_tile=0, gemm_wk=1, gemm_dma_wgs=2)
SLABS = dict(gemm_wk=0, gemm_dma_wgs=4, gemm_min_wgs=1)
STAGED = dict(gemm_dma=0)

# worst |err| / bound of the rounded-data check per route as measured on an MI355X; a record, not a bound: the bound is 1
RECORDED = {'staged c64': 0.0586, 'staged c128': 0.0628, 'dma four': 0.0137, 'dma 128': 0.0152, 'dma eight': 0.00885, 'dma slabs': 0.0045}


def _op_np(a, op):
    if op & 1:
        a = np.conj(a)
    if op & 2:
        a = a.T
    return a


def stored_shapes(opA, opB, M, N, K):
    """the shapes A and B are STORED in: A is M x K (op 0 / 1) or K x M (op 2 / 3), B K x N or N x K"""
    return ((K, M) if opA & 2 else (M, K)), ((N, K) if opB & 2 else (K, N))


def frame_claims(kind, row, itemsize):
    """(ld, base mod 16) of an operand of `row` elements per stored row in a frame of this kind, in a 16-byte aligned buffer"""
    pad, off = FRAMES[kind]
    ld = row + pad
    return ld, ((ld + off) * itemsize) % 16


def framed(values, kind, device, pad=None, off=None):
    """`values` (2-D numpy) stored inside a NaN frame on `device`.  Returns the buffer, the interior view, its address, its leading
    dimension and its address mod 16; asserts that the view is where and what frame_claims says."""
    if pad is None:
        pad, off = FRAMES[kind]
    rows, row = values.shape
    ld = row + pad
    host = np.full((rows + 2, ld), np.nan, dtype=values.dtype)     # complex dtypes: both parts NaN
    if np.iscomplexobj(host):
        host.imag = np.nan
    host[1:1 + rows, off:off + row] = values
    buf = torch.empty(host.shape, dtype=torch.from_numpy(host).dtype, device=device)
    buf.copy_(torch.from_numpy(host))
    view = buf[1:1 + rows, off:off + row]
    item = values.dtype.itemsize
    ptr = buf.data_ptr() + (ld + off) * item
    assert buf.data_ptr() % 16 == 0
    if view.numel():
        assert view.data_ptr() == ptr and view.stride(1) == 1
        assert rows == 1 or view.stride(0) == ld
    if kind is not None:
        assert (ld, ptr % 16) == frame_claims(kind, row, item), (kind, row, ld, ptr % 16)
    return types.SimpleNamespace(buf=buf, view=view, ptr=ptr, ld=ld, residue=ptr % 16, before=host, rows=rows, row=row, off=off)


def out_frame(M, N, np_dtype, device, preset=None):
    """the output: the M x N interior of a NaN frame with ld = N + 3 and guard rows, preset with `preset` (accumulate) or left NaN"""
    vals = np.full((M, N), np.nan, dtype=np_dtype) if preset is None else np.asarray(preset, dtype=np_dtype)
    if preset is None and np.iscomplexobj(vals):
        vals.imag = np.nan
    return framed(vals, None, device, OUT_PAD, OUT_OFF)


def read_out(fr):
    """the interior after the call; asserts that every byte of the frame outside it is what it was, bit for bit"""
    after = fr.buf.cpu().numpy()
    item = after.dtype.itemsize
    a = after.view(np.uint8).reshape(fr.rows + 2, fr.ld, item)
    b = fr.before.view(np.uint8).reshape(fr.rows + 2, fr.ld, item)
    outside = np.ones((fr.rows + 2, fr.ld), dtype=bool)
    outside[1:1 + fr.rows, fr.off:fr.off + fr.row] = False
    bad = np.argwhere((a != b).any(axis=2) & outside)
    assert bad.size == 0, f'{len(bad)} elements outside the interior were written, first at frame (row, column) {tuple(bad[0])}'
    return after[1:1 + fr.rows, fr.off:fr.off + fr.row].copy()


def exact_operand(rng, shape, np_dtype, lim=3):
    """independent integer real and imaginary parts in [-lim, lim]"""
    return (rng.integers(-lim, lim + 1, shape) + 1j * rng.integers(-lim, lim + 1, shape)).astype(np_dtype)


def exact_ref(A, B, opA, opB, alpha):
    """alpha op(A) @ op(B) by int64 products (complex128 holds it exactly)"""
    a, b = _op_np(A, opA), _op_np(B, opB)
    ar, ai, br, bi = (np.rint(x).astype(np.int64) for x in (a.real, a.imag, b.real, b.imag))
    assert np.array_equal(ar + 1j * ai, a) and np.array_equal(br + 1j * bi, b)
    cr, ci = ar @ br - ai @ bi, ar @ bi + ai @ br
    assert max(np.abs(cr).max(initial=0), np.abs(ci).max(initial=0)) < 2 ** 24
    return alpha * (cr.astype(np.float64) + 1j * ci.astype(np.float64))


def exact_abs2_ref(A, B, opA, opB, alpha, weight, preset=None):
    c = exact_ref(A, B, opA, opB, alpha)
    r = weight * (c.real ** 2 + c.imag ** 2)
    if preset is not None:
        r = r + preset
    assert np.abs(r).max(initial=0) < 2 ** 24 and np.array_equal(r * 4, np.rint(r * 4))
    return r


def assert_exact(got, ref, what):
    """np.array_equal with a message that says where"""
    got = np.asarray(got)
    ref = np.asarray(ref).astype(np.complex128 if np.iscomplexobj(got) else np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got.astype(ref.dtype), ref):
        bad = np.argwhere(~(got.astype(ref.dtype) == ref))
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ, first at {i}: got {got[i]}, exact {ref[i]}')


def rounded_bound(A, B, opA, opB, alpha, S, eps):
    a, b = _op_np(A, opA), _op_np(B, opB)
    K = a.shape[1]
    amp = (np.abs(a.real) + np.abs(a.imag)).astype(np.float64) @ (np.abs(b.real) + np.abs(b.imag)).astype(np.float64)
    return 2 * (K + 8 + S) * eps * abs(alpha) * amp


def rounded_ratio(got, A, B, opA, opB, alpha, S, eps):
    """worst |err| / bound over the real and the imaginary parts against numpy complex128"""
    ref = alpha * (_op_np(A, opA).astype(np.complex128) @ _op_np(B, opB).astype(np.complex128))
    bound = rounded_bound(A, B, opA, opB, alpha, S, eps)
    got = np.asarray(got).astype(np.complex128)
    assert np.isfinite(got.view(np.float64)).all()
    return float(max((np.abs(got.real - ref.real) / bound).max(), (np.abs(got.imag - ref.imag) / bound).max()))


def crandn(rng, shape, np_dtype):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np_dtype)


# ---------------------------------------------------------------------------------------------------------------- calls (GPU)

def planned_slabs(lib, dt, M, N, K):
    """the slab count pm_cgemm_workspace planned (1: no workspace), and its bytes"""
    need = lib.pm_cgemm_workspace(dt, M, N, K)
    assert need % (M * N * ITEM[dt]) == 0, (need, M, N)
    return max(1, need // (M * N * ITEM[dt])), need


def dma_accepts(lib, opA, opB, M, N, K, fa, fb):
    """does pm_cgemm take the LDS-DMA kernel for these complex64 operands?  pm_cgemm_abs2 answers (it runs into a scratch image)"""
    R = torch.empty((M, N), dtype=torch.float32, device=fa.buf.device)
    rc = lib.pm_cgemm_abs2(C64, opA, opB, M, N, K, 1.0, fa.ptr, fa.ld, fb.ptr, fb.ld, R.data_ptr(), N, 1.0, 0, None, 0, L.stream_ptr())
    assert rc in (0, L.PM_ERR_UNSUPPORTED), (rc, lib.pm_last_error().decode())
    return rc == 0


GUARD = 4096


def _workspace(need, mode, device):
    """(tensor, pointer, bytes) for mode 'query' (exactly `need` bytes between two sentinel guards), 'null' or 'short' (need - 1)"""
    if mode == 'null' or need == 0:
        return None, None, 0
    w = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
    assert w.data_ptr() % 16 == 0
    return w, w.data_ptr() + GUARD, need if mode == 'query' else need - 1


def _guards_intact(w, need):
    if w is not None:
        h = w.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + need:] == 0xA5).all(), 'the workspace was written outside [0, need)'


def run_cgemm(lib, dt, opA, opB, M, N, K, alpha, A, B, kindA='wide-aligned', kindB='wide-aligned', ws='query', device='cuda'):
    """one pm_cgemm call on framed operands into a framed C.  Returns the result, the route (complex64: did the LDS-DMA kernel take
    it) and the planned slab count; asserts the return code, the C frame and the workspace guards."""
    fa, fb = framed(A, kindA, device), framed(B, kindB, device)
    fc = out_frame(M, N, NP_OF[dt], device)
    S, need = planned_slabs(lib, dt, M, N, K)
    w, wp, wb = _workspace(need, ws, device)
    rc = lib.pm_cgemm(dt, opA, opB, M, N, K, float(alpha), fa.ptr, fa.ld, fb.ptr, fb.ld, fc.ptr, fc.ld, wp, wb, L.stream_ptr())
    assert rc == 0, (rc, lib.pm_last_error().decode())
    got = read_out(fc)
    _guards_intact(w, need)
    for f, x in ((fa, A), (fb, B)):        # the operands are inputs: not a bit of their frames may change either
        assert np.array_equal(f.buf.cpu().numpy().view(np.uint8), f.before.view(np.uint8))
    dma = dma_accepts(lib, opA, opB, M, N, K, fa, fb) if dt == C64 else False
    return types.SimpleNamespace(got=got, dma=dma, S=S, need=need)


def run_exact(lib, dt, opA, opB, M, N, K, alpha, seed, **kw):
    """exact data through run_cgemm, compared with np.array_equal"""
    rng = np.random.default_rng(seed)
    sa, sb = stored_shapes(opA, opB, M, N, K)
    A, B = exact_operand(rng, sa, NP_OF[dt]), exact_operand(rng, sb, NP_OF[dt])
    r = run_cgemm(lib, dt, opA, opB, M, N, K, alpha, A, B, **kw)
    assert_exact(r.got, exact_ref(A, B, opA, opB, alpha), f'dtype {dt} op ({opA}, {opB}) {M} x {N} x {K} alpha {alpha} {kw}')
    return r


def run_abs2_exact(lib, opA, opB, M, N, K, alpha, weight, seed, kindA='wide-aligned', kindB='wide-aligned', ws='query', device='cuda'):
    """pm_cgemm_abs2 on exact data: store into a framed R, then accumulate onto a preset one; both exact.  Returns the planned slabs."""
    rng = np.random.default_rng(seed)
    sa, sb = stored_shapes(opA, opB, M, N, K)
    A, B = exact_operand(rng, sa, np.complex64, 2), exact_operand(rng, sb, np.complex64, 2)
    fa, fb = framed(A, kindA, device), framed(B, kindB, device)
    S, need = planned_slabs(lib, C64, M, N, K)
    preset = rng.integers(-4, 5, (M, N)).astype(np.float32)
    for acc, pre in ((0, None), (1, preset)):
        fr = out_frame(M, N, np.float32, device, pre)
        w, wp, wb = _workspace(need, ws, device)
        rc = lib.pm_cgemm_abs2(C64, opA, opB, M, N, K, float(alpha), fa.ptr, fa.ld, fb.ptr, fb.ld, fr.ptr, fr.ld, float(weight), acc, wp, wb,
                               L.stream_ptr())
        assert rc == 0, (rc, lib.pm_last_error().decode())
        got = read_out(fr)
        _guards_intact(w, need)
        assert_exact(got, exact_abs2_ref(A, B, opA, opB, alpha, weight, pre),
                     f'abs2 op ({opA}, {opB}) {M} x {N} x {K} alpha {alpha} weight {weight} accumulate {acc}')
    return S
