"""Thin Python wrappers over the C ABI: build descriptors, allocate outputs, enqueue.

Everything here operates on torch tensors resident in HBM and enqueues on
torch's current stream.  No arithmetic happens in Python.
"""
import ctypes
import math
import threading

import torch

from . import _lib as L
from .graph import sequenced


# The kernels write through raw pointers, which torch's version counters do not see: a caller-supplied `out=` tensor is marked
# modified here, so caches keyed on (tensor identity, version) -- polychromatic.packed_pupil -- notice maps rewritten in place.
_bump = torch.autograd.graph.increment_version


def _axis(n, length=None, off=0, shift=0):
    return L.pm_axis(int(n), int(n if length is None else length), int(off), int(shift))


def _fill_views(d, x, shape, in_off, in_shift, out_shape, out_off, out_shift):
    """Common part of the 2-D descriptors: views, leading dimensions and the batch (leading axis of a 3-D x)."""
    if x.dim() not in (2, 3):
        raise ValueError('2-D transforms take a 2-D array or a (batch, rows, cols) stack of them')
    if x.stride(-1) != 1:
        x = x.contiguous()
    m, n = x.shape[-2:]
    M, N = (m, n) if shape is None else shape
    om, on = (M, N) if out_shape is None else out_shape
    d.dtype = L.code(x)
    d.in_y = _axis(M, m, in_off[0], in_shift[0])
    d.in_x = _axis(N, n, in_off[1], in_shift[1])
    d.out_y = _axis(M, om, out_off[0], out_shift[0])
    d.out_x = _axis(N, on, out_off[1], out_shift[1])
    d.in_ld = x.stride(-2) if m > 1 else n
    if not x.is_complex():
        d.flags |= L.PM_FLAG_REAL_INPUT      # float32 / float64 field read as it is
    if x.dim() == 3:
        d.batch = x.shape[0]
        d.in_bstride = x.stride(0) if x.shape[0] > 1 else m * n
    return x, (M, N), (om, on)


def _fill_mul(d, x, mul, mul_x, mul_conj, keep):
    """Multiplier: full (M, N) array or the (hy, hx) vector pair; with a batch, optionally one per field."""
    batched = x.dim() == 3
    if mul is not None and mul_x is not None:
        d.mul_kind = L.PM_MUL_SEPARABLE
        if batched and mul.dim() == 2:
            mul, mul_x = mul.contiguous(), mul_x.contiguous()
            d.mul_bstride, d.mul_x_bstride = mul.stride(0), mul_x.stride(0)
        d.mul = mul.data_ptr()
        d.mul_x = mul_x.data_ptr()
        keep += [mul, mul_x]
    elif mul is not None:
        d.mul_kind = L.PM_MUL_FULL
        if batched and mul.dim() == 3:
            d.mul_bstride = mul.stride(0)
        d.mul = mul.data_ptr()
        d.mul_ld = mul.stride(-2) if mul.shape[-2] > 1 else mul.shape[-1]
        keep.append(mul)
    d.mul_conj = 1 if mul_conj else 0


def _is_mix_length(n):
    """lengths the mixed-radix kernel takes (csrc/fft_mixed.h): 32 .. 8192, not a power of two, primes <= 19"""
    if n < 32 or n > 8192 or (n & (n - 1)) == 0:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19):
        while n % p == 0:
            n //= p
    return n == 1


def synth_supported(opd, amp, N):
    """Whether pm_fft2 can synthesise amp * exp(i k opd) while loading (PM_FLAG_SYNTH_INPUT): a 2-D float32 / float64 OPD map
    (complex64 / complex128 transform), a row length that is a power of two or (round 4) a composite of primes <= 19 -- the two row
    kernels whose loaders synthesise --, real / bool amplitude."""
    if opd.dim() != 2 or opd.dtype not in (torch.float32, torch.float64) or not (_is_pow2_engine(N) or _is_mix_length(N)):
        return False
    if not _is_pow2_engine(N) and opd.stride(0) >= 1 << 24:
        return False
    return amp is None or (amp.dtype in _AMP_CODE and amp.dim() == 2 and amp.shape == opd.shape and amp.stride(-1) == 1)


# Filled descriptors and their workspace sizes, keyed by everything in them that is not a pointer or a per-call scalar: a
# repeated propagation (the inner loop of every model) then costs one struct copy, four pointer stores and ONE library
# call pair instead of ~40 ctypes field stores.
_fft2_plans = {}


def _check_out(out, x, oshape, odt):
    """A caller-supplied output / accumulator must be exactly what the kernel writes (it only receives a pointer and a
    leading dimension): anything else would be silent corruption or an out-of-bounds write."""
    if not isinstance(out, torch.Tensor) or out.device != x.device:
        raise ValueError('fft2: `out` must be a tensor on the device of the input')
    if out.dtype != odt:
        raise ValueError(f'fft2: `out` must be {odt} for this input and epilogue, got {out.dtype}')
    if tuple(out.shape) != tuple(oshape):
        raise ValueError(f'fft2: `out` must have shape {tuple(oshape)}, got {tuple(out.shape)}')
    if out.stride(-1) != 1:
        raise ValueError('fft2: the last axis of `out` must be contiguous')


def fft2(x, *, synth=None, spectral=None, **kw):
    """Fused 2-D transform (pm_fft2); see _fft2_call for the arguments.

    synth (pupil synthesis inside the row pass) is a property of the ROUTE the library's planner picks -- this module's
    synth_supported() restates the planner's test without its inputs (the mix / mix_min knobs, a tuning_local block, workspace
    limits), so it can say yes where the planner then says PM_ERR_UNSUPPORTED.  When that happens for a single 2-D field the pupil
    is materialised (pm_pupil_synth, what the call would have cost before the fusion existed) and the transform runs on it:
    a disagreement costs time, never an exception."""
    if synth is None or spectral is not None or x.dim() != 2:
        return _fft2_call(x, synth=synth, spectral=spectral, **kw)
    try:
        return _fft2_call(x, synth=synth, **kw)
    except NotImplementedError:
        cdt = L._COMPLEX_OF[x.dtype] if not x.is_complex() else x.dtype
        if isinstance(synth[0], str):       # ('packed', k): (amplitude, OPD) pairs
            pairs = torch.view_as_real(x)
            field = pupil_synth(pairs[..., 0].contiguous(), pairs[..., 1].contiguous(), synth[1], cdt)
        else:
            field = pupil_synth(synth[0], x, synth[1], cdt)
        return _fft2_call(field, **kw)


def _fft2_call(x, *, direction, scale, shape=None, in_off=(0, 0), in_shift=(0, 0),
               out_shape=None, out_off=(0, 0), out_shift=(0, 0), epilogue=L.PM_EPI_NONE,
               mul=None, mul_x=None, mul_conj=False, out=None, weight=1.0, flags=0, synth=None, spectral=None):
    """Fused 2-D transform (pm_fft2).

    x          : (m, n) complex tensor, or a (B, m, n) stack transformed in one launch pair; each field sits at
                 `in_off` inside the logical `shape` = (M, N) array (zero elsewhere), which is then rotated by
                 `in_shift`
    out_shape  : stored window of the output (crop), at `out_off` of the rotated result
    mul, mul_x : None | full (M, N) multiplier | (column vector hy (M,), row vector hx (N,)); with a stack,
                 (B, M, N) / ((B, M), (B, N)) give one multiplier per field
    synth      : (amp | None, k): x is the real float32 OPD map and the transformed field is amp * exp(i k x),
                 synthesised while the row pass loads it (see synth_supported); ('packed', k): x is a complex64 tensor
                 holding (amplitude, OPD) pairs (pack_amp_opd)
    spectral   : (k values, weights) with synth and PM_EPI_ABS2_ACCUM: out += sum_b weights[b] |transform at k[b]|^2, the whole
                 wavelength loop in one call (pm_fft2_spectral: groups of wavelengths share one launch pair); synth[1] is ignored
    out        : optional result / accumulator (PM_EPI_ABS2_ACCUM); must match the dtype and shape the call produces
    """
    lib = L.load()
    if x.dim() not in (2, 3):
        raise ValueError('2-D transforms take a 2-D array or a (batch, rows, cols) stack of them')
    if x.stride(-1) != 1:
        x = x.contiguous()
    m, n = x.shape[-2:]
    M, N = (m, n) if shape is None else shape
    om, on = (M, N) if out_shape is None else out_shape
    cdt = L.cdtype_of(x)
    odt = cdt if epilogue == L.PM_EPI_NONE else L._REAL_OF[cdt]
    oshape = (om, on) if x.dim() == 2 else (x.shape[0], om, on)
    if out is None:
        out = torch.empty(oshape, dtype=odt, device=x.device)
    else:
        _check_out(out, x, oshape, odt)
        _bump(out)
    packed = synth is not None and isinstance(synth[0], str)
    amp = synth[0] if (synth is not None and not packed) else None
    if mul is not None and mul_x is not None and x.dim() == 3 and mul.dim() == 2:
        mul, mul_x = mul.contiguous(), mul_x.contiguous()      # per-field (hy, hx) vectors: rows of two (B, .) arrays
    key = (x.dtype, tuple(x.shape), x.stride(), M, N, tuple(in_off), tuple(in_shift), om, on, tuple(out_off), tuple(out_shift),
           direction, epilogue, flags, float(scale), bool(mul_conj), out.stride(),
           None if synth is None else (True, packed, None if amp is None else (amp.dtype, amp.stride())),
           None if mul is None else (tuple(mul.shape), mul.stride()), None if mul_x is None else (tuple(mul_x.shape), mul_x.stride()))
    plan = _fft2_plans.get(key)
    if plan is None:
        d = L.pm_fft2_desc()
        d.flags = flags
        _fill_views(d, x, shape, in_off, in_shift, out_shape, out_off, out_shift)
        d.direction = direction
        d.epilogue = epilogue
        d.scale = float(scale)
        d.weight = 1.0
        if synth is not None:
            d.flags = (d.flags & ~L.PM_FLAG_REAL_INPUT) | L.PM_FLAG_SYNTH_INPUT | (L.PM_FLAG_SYNTH_PACKED if packed else 0)
            if amp is not None:
                d.synth_amp_dtype = _AMP_CODE[amp.dtype]
                d.synth_amp_ld = amp.stride(0) if amp.shape[0] > 1 else amp.shape[1]
        keep = []
        _fill_mul(d, x, mul, mul_x, mul_conj, keep)
        d.out_ld = out.stride(-2) if om > 1 else on
        if x.dim() == 3:
            d.out_bstride = out.stride(0) if out.shape[0] > 1 else om * d.out_ld
        if synth is not None:     # the workspace query validates the descriptor: give it the pointers of this call
            d.synth_k = float(synth[1])
            d.synth_amp = amp.data_ptr() if amp is not None else None
        nbytes = lib.pm_fft2_workspace(ctypes.byref(d))
        if nbytes == 0:
            L.check(lib.pm_fft2(ctypes.byref(d), L.ptr(x), L.ptr(out), None, 0, L.stream_ptr()))  # raises with the reason
        plan = (d,)
        if len(_fft2_plans) > 512:
            _fft2_plans.clear()
        _fft2_plans[key] = plan
    d = L.pm_fft2_desc.from_buffer_copy(plan[0])
    d.weight = float(weight)
    if synth is not None:
        d.synth_k = float(synth[1])
        d.synth_amp = amp.data_ptr() if amp is not None else None
    if mul is not None:
        d.mul = mul.data_ptr()
        if mul_x is not None:
            d.mul_x = mul_x.data_ptr()
    if spectral is not None:
        ks, wts = spectral
        cnt = len(ks)
        if synth is None or epilogue != L.PM_EPI_ABS2_ACCUM or len(wts) != cnt:
            raise ValueError('spectral=(k, weights) needs synth, the accumulate epilogue and as many weights as wavenumbers')
        ka = (ctypes.c_double * cnt)(*[float(v) for v in ks])
        wa = (ctypes.c_double * cnt)(*[float(v) for v in wts])
        nbytes = lib.pm_fft2_spectral_workspace(ctypes.byref(d), cnt)
        ws = L.workspace(nbytes)
        L.check(lib.pm_fft2_spectral(ctypes.byref(d), cnt, ka, wa, x.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None,
                                     nbytes, L.stream_ptr()))
        return out
    nbytes = lib.pm_fft2_workspace(ctypes.byref(d))      # not cached: it follows the tuning knobs (pm_set_tuning)
    ws = L.workspace(nbytes)
    rc = lib.pm_fft2(ctypes.byref(d), x.data_ptr(), out.data_ptr(), ws.data_ptr() if ws is not None else None, nbytes, L.stream_ptr())
    if rc:
        L.check(rc)
    return out


def real_pairs_ok(x):
    """Whether a real 2-D array can be read as rows of complex pairs (fft2_real): float32 / float64, contiguous rows of EVEN length, even
    row pitch, base address aligned like a complex element."""
    return (isinstance(x, torch.Tensor) and not x.is_complex() and x.dim() == 2 and x.dtype in (torch.float32, torch.float64) and
            x.shape[1] >= 2 and x.shape[1] % 2 == 0 and x.shape[0] >= 1 and x.stride(1) == 1 and (x.stride(0) % 2 == 0 or x.shape[0] == 1) and
            x.data_ptr() % (2 * x.element_size()) == 0)


def fft2_real(x, *, scale=1.0, in_shift=(0, 0), out_shift=(0, 0), epilogue=L.PM_EPI_NONE, norm_dc=False):
    """fft2 of a REAL (M, N) array, N even, on any lengths: the array read as (M, N/2) complex pairs, one half-size pm_fft2 on whatever
    route those lengths take, and one untangling sweep (pm_r2c_untangle) that also applies the input rotation, the optional division by
    the DC bin, `scale`, the epilogue (complex, |.|, |.|^2, angle) and the output rotation.  What the library's Hermitian path does for
    powers of two, for every other size (1000^2, 3000^2, 1536 x 2000 ...): prysm/otf.py:28-33, 62-135."""
    lib = L.load()
    if not real_pairs_ok(x):
        raise ValueError('fft2_real: a real float32 / float64 2-D array with contiguous rows of even length is required')
    M, N = x.shape
    z = torch.view_as_complex(x.as_strided((M, N // 2, 2), (x.stride(0) if M > 1 else N, 2, 1)))
    zf = _fft2_call(z, direction=-1, scale=1.0)
    cdt = zf.dtype
    out = torch.empty((M, N), dtype=cdt if epilogue == L.PM_EPI_NONE else L._REAL_OF[cdt], device=x.device)
    L.check(lib.pm_r2c_untangle(L._COMPLEX_CODE[cdt], M, N, L.ptr(zf), zf.stride(0), int(in_shift[0]) % M, int(in_shift[1]) % N,
                                int(out_shift[0]) % M, int(out_shift[1]) % N, int(epilogue), 1 if norm_dc else 0, float(scale),
                                L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


_REGISTER_ROUTES = {}


def on_register_engine(M, N, cdtype):
    """Whether BOTH passes of a plain complex (M, N) transform run on the composite register engine (csrc/fft_ce.h) -- the composite
    grids whose (B, M, N) stacks go out as one launch pair.  Asked of the library's planner (pm_plan_explain: host logic, no GPU work),
    once per shape, precision and set of open tuning_local blocks OF THE CALLING THREAD (the knobs are per thread: an answer cached
    under another thread's block, or under a process-wide epoch, could be wrong for this one -- ADVICE r5).  A process-wide
    pm_set_tuning after the first question is not seen: call _REGISTER_ROUTES.clear()."""
    key = (int(M), int(N), cdtype, L.tuning_local.signature())
    hit = _REGISTER_ROUTES.get(key)
    if hit is None:
        lib = L.load()
        d = L.pm_fft2_desc()
        d.dtype, d.direction = L._COMPLEX_CODE[cdtype], -1
        d.in_y, d.in_x, d.in_ld = L.pm_axis(M, M, 0, 0), L.pm_axis(N, N, 0, 0), N
        d.out_y, d.out_x, d.out_ld = L.pm_axis(M, M, 0, 0), L.pm_axis(N, N, 0, 0), N
        buf = ctypes.create_string_buffer(256)
        hit = lib.pm_plan_explain(ctypes.byref(d), 0, buf, 256) == 0 and buf.value.count(b'mixed-radix-registers') == 2
        if len(_REGISTER_ROUTES) > 256:
            _REGISTER_ROUTES.clear()
        _REGISTER_ROUTES[key] = hit
    return hit


def pack_amp_opd(amp, opd):
    """(amplitude, OPD) pairs in the OPD map's precision as a complex tensor -- the input of fft2(..., synth=('packed', k)).  A loop
    over wavelengths packs its two maps once and then reads ONE element per sample in every transform."""
    rd = opd.dtype if opd.dtype in (torch.float32, torch.float64) else torch.float32
    a = torch.ones_like(opd, dtype=rd) if amp is None else amp.to(rd)
    return torch.view_as_complex(torch.stack((a, opd.to(rd)), dim=-1).contiguous())


def _is_pow2_engine(n):
    return 2 <= n <= 8192 and (n & (n - 1)) == 0


def fft2_mul_ifft2(x, *, scale, mul, mul_x=None, mul_conj=False, shape=None, in_off=(0, 0), in_shift=(0, 0),
                   out_shape=None, out_off=(0, 0), out_shift=(0, 0), real_out=False):
    """window(ifft2(fft2(pad(x)) * H)) * scale.

    real_out: for a REAL x return the real part of the result as a real tensor -- on half spectra end to end when the shapes allow
    (PM_FLAG_REAL_OUTPUT: unpadded power-of-two sizes, a full multiplier), else `.real` of the complex result.

    Power-of-two transform sizes run the fused three-pass kernel chain (pm_fft2_mul_ifft2: the multiply and
    both column transforms happen in registers); so do composite grids whose column length has primes <= 19 (round 4: the middle
    pass keeps the column in LDS through forward stages, multiplier and transposed stages); what is left composes two pm_fft2 calls.
    """
    lib = L.load()
    m, n = x.shape[-2:]
    M, N = (m, n) if shape is None else shape
    def composed():
        # two fused transforms, the multiplier in the first one's column store (measured, profiles/r01/fused_as.log: the 3-pass chain wins
        # at every engine size, e.g. 4096^2 complex128 448 vs 473 us, 2048^2 complex64 55 vs 75 us)
        F = fft2(x, direction=-1, scale=1.0, shape=shape, in_off=in_off, in_shift=in_shift, mul=mul, mul_x=mul_x,
                 mul_conj=mul_conj)
        r = fft2(F, direction=+1, scale=scale, out_shape=out_shape, out_off=out_off, out_shift=out_shift)
        return r.real if (real_out and not x.is_complex()) else r
    pow2 = _is_pow2_engine(M) and _is_pow2_engine(N)
    if not pow2 and x.dim() != 2:
        return composed()
    d = L.pm_fft2_desc()
    x, (M, N), (om, on) = _fill_views(d, x, shape, in_off, in_shift, out_shape, out_off, out_shift)
    d.direction = -1
    d.scale = float(scale)
    d.weight = 1.0
    keep = [x]
    _fill_mul(d, x, mul, mul_x, mul_conj, keep)
    oshape = (om, on) if x.dim() == 2 else (x.shape[0], om, on)
    if real_out and not x.is_complex() and x.dim() == 2 and mul_x is None and x.data_ptr() % (2 * x.element_size()) == 0:
        # the half-spectrum chain: the workspace query answers whether this descriptor is one it takes
        d.flags |= L.PM_FLAG_REAL_OUTPUT
        out = torch.empty(oshape, dtype=L._REAL_OF[L.cdtype_of(x)], device=x.device)
        d.out_ld = out.stride(-2) if om > 1 else on
        nbytes = lib.pm_fft2_mul_ifft2_workspace(ctypes.byref(d))
        if nbytes:
            ws = L.workspace(int(nbytes))
            L.check(lib.pm_fft2_mul_ifft2(ctypes.byref(d), L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()))
            return out
        d.flags &= ~L.PM_FLAG_REAL_OUTPUT
    out = torch.empty(oshape, dtype=L.cdtype_of(x), device=x.device)
    d.out_ld = out.stride(-2) if om > 1 else on
    if x.dim() == 3:
        d.out_bstride = out.stride(0) if out.shape[0] > 1 else om * d.out_ld
    nbytes = lib.pm_fft2_mul_ifft2_workspace(ctypes.byref(d))
    if not nbytes and not pow2:
        # not a shape of the composite-grid chain (a column length with a prime above 13, a Bluestein row length ...)
        del out
        return composed()
    ws = L.workspace(max(int(nbytes), 16))
    L.check(lib.pm_fft2_mul_ifft2(ctypes.byref(d), L.ptr(x), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return out.real if (real_out and not x.is_complex()) else out


def fft1(x, n=None, axis=-1, direction=-1, scale=1.0, out_len=None, out_off=0, in_off=0):
    """Batched 1-D transform along `axis` of a 2-D tensor (pm_fft1).

    The input is zero padded (placed at `in_off`) or truncated to length n; the stored output is the
    window [out_off, out_off + out_len) of the n bins.  direction -1: exp(-2 pi i ..); +1: exp(+..).
    """
    lib = L.load()
    if x.dim() == 1:
        return fft1(x[None, :], n, 1, direction, scale, out_len, out_off, in_off)[0]
    axis = axis % 2
    rows, cols = x.shape
    length = rows if axis == 0 else cols
    n = length if n is None else int(n)
    batch = cols if axis == 0 else rows
    olen = n if out_len is None else int(out_len)
    t_in = _axis(n, min(length, n - in_off), in_off, 0)
    t_out = _axis(n, olen, out_off, 0)
    oshape = (olen, cols) if axis == 0 else (rows, olen)
    out = torch.empty(oshape, dtype=x.dtype, device=x.device)
    nbytes = lib.pm_fft1_workspace(L.code(x), axis, batch, n)   # non-zero: a non power-of-two length on the Bluestein path
    ws = L.workspace(nbytes) if nbytes else None
    L.check(lib.pm_fft1_ws(L.code(x), direction, axis, batch, ctypes.byref(t_in), ctypes.byref(t_out), float(scale),
                           L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), L.ptr(ws), nbytes, L.stream_ptr()))
    return out


def czt_vectors(N, M, K, shift, half, cdtype):
    """The chirps (b, a, h) of one chirp-Z axis from its scalars in one launch (pm_czt_vectors)."""
    lib = L.load()
    dev = L.device()
    b = torch.empty(N, dtype=cdtype, device=dev)
    a = torch.empty(M, dtype=cdtype, device=dev)
    h = torch.empty(K, dtype=cdtype, device=dev)
    L.check(lib.pm_czt_vectors(L.code(b), N, M, K, float(shift), float(half), L.ptr(b), L.ptr(a), L.ptr(h), L.stream_ptr()))
    return b, a, h


def czt_axis(x, K, axis, H, *, pre=None, post=None, out_len, in_off=0, out_off=0, conj=False, scale=1.0):
    """One axis of a chirp-Z transform in one kernel (pm_czt_axis): scale * post * IFFT_K(FFT_K(pad_K(pre * x)) * H)[out_off : out_off
    + out_len] along `axis` of the 2-D tensor x; `conj` conjugates pre, H and post (the adjoint).  K must be an engine length."""
    lib = L.load()
    axis = axis % 2
    rows, cols = x.shape
    nseq, in_len = (rows, cols) if axis == 1 else (cols, rows)
    oshape = (rows, out_len) if axis == 1 else (out_len, cols)
    out = torch.empty(oshape, dtype=x.dtype, device=x.device)
    c = 1 if conj else 0
    L.check(lib.pm_czt_axis(L.code(x), axis, nseq, int(K), in_len, int(in_off), int(out_len), int(out_off), L.ptr(pre), c, L.ptr(H), c,
                            L.ptr(post), c, float(scale), L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def fft1_ramp(x, K, axis, direction, *, pre=None, post=None, out_len, conj=False, scale=1.0):
    """One axis of an FFT-accelerated DFT in one kernel (pm_fft1_ramp): scale * post * T_K(pad_K(pre * x))[:out_len] along `axis` of
    the 2-D tensor x, T_K unnormalised with the sign of `direction`; `conj` conjugates pre and post (the adjoint).  K must be an
    engine length."""
    lib = L.load()
    axis = axis % 2
    rows, cols = x.shape
    nseq, in_len = (rows, cols) if axis == 1 else (cols, rows)
    oshape = (rows, out_len) if axis == 1 else (out_len, cols)
    out = torch.empty(oshape, dtype=x.dtype, device=x.device)
    c = 1 if conj else 0
    L.check(lib.pm_fft1_ramp(L.code(x), int(direction), axis, nseq, int(K), in_len, 0, int(out_len), 0, L.ptr(pre), c, L.ptr(post), c,
                             float(scale), L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def _rows2d(t):
    """`t` as the kernels address a 2-D array: unit column stride, rows at least a row apart.  A column-strided, transposed or
    row-broadcast view is copied (the entry points take one leading dimension per array and nothing else)."""
    if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def cmul(a, b, conj_b=False):
    lib = L.load()
    a, b = _rows2d(a), _rows2d(b)
    rows, cols = a.shape
    out = torch.empty((rows, cols), dtype=a.dtype, device=a.device)
    L.check(lib.pm_cmul(L.code(a), 1 if conj_b else 0, rows, cols, L.ptr(a), a.stride(0), L.ptr(b), b.stride(0),
                        L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def rmul(r, a, scale=1.0):
    """scale * r * a for a REAL image r and a complex field a of the matching precision (pm_rmul; one sweep)."""
    lib = L.load()
    r, a = _rows2d(r), _rows2d(a)
    rows, cols = a.shape
    out = torch.empty((rows, cols), dtype=a.dtype, device=a.device)
    L.check(lib.pm_rmul(L.code(a), rows, cols, L.ptr(r), r.stride(0), L.ptr(a), a.stride(0), float(scale), L.ptr(out), out.stride(0),
                        L.stream_ptr()))
    return out


def scale_sep(x, row_vec=None, col_vec=None, row_conj=False, col_conj=False, scale=1.0):
    """out[i, j] = x[i, j] * row_vec[i] * col_vec[j] * scale (row_vec indexes rows, col_vec columns)."""
    lib = L.load()
    x = _rows2d(x)
    rows, cols = x.shape
    out = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    L.check(lib.pm_scale_sep(L.code(x), rows, cols, L.ptr(x), x.stride(0), L.ptr(row_vec), 1 if row_conj else 0,
                             L.ptr(col_vec), 1 if col_conj else 0, float(scale), L.ptr(out), out.stride(0),
                             L.stream_ptr()))
    return out


def abs2(x, out=None, weight=None):
    """|x|^2, or out += weight * |x|^2 when `out` and `weight` are given."""
    lib = L.load()
    x = _rows2d(x)
    rows, cols = x.shape
    acc = 0
    if out is None:
        out = torch.empty((rows, cols), dtype=L._REAL_OF[x.dtype], device=x.device)
    else:
        if out.stride(-1) != 1 or (rows > 1 and out.stride(0) < cols):
            raise ValueError('abs2: `out` must have unit column stride and rows that do not overlap')
        _bump(out)
        if weight is not None:
            acc = 1
    L.check(lib.pm_abs2(L.code(x), rows, cols, L.ptr(x), x.stride(0), L.ptr(out), out.stride(0), acc,
                        float(1.0 if weight is None else weight), L.stream_ptr()))
    return out


def abs_arg(x):
    """(|x|, angle(x)) of a complex 2-D array in one sweep (pm_abs_arg)."""
    lib = L.load()
    x = _rows2d(x)
    rows, cols = x.shape
    rd = L._REAL_OF[x.dtype]
    oabs = torch.empty((rows, cols), dtype=rd, device=x.device)
    oarg = torch.empty((rows, cols), dtype=rd, device=x.device)
    L.check(lib.pm_abs_arg(L.code(x), rows, cols, L.ptr(x), x.stride(0), L.ptr(oabs), oabs.stride(0), L.ptr(oarg), oarg.stride(0),
                           L.stream_ptr()))
    return oabs, oarg


def sum_modes(modes, weights, out=None, accumulate=False):
    """sum_b weights[b] * modes[b] over a (B, rows, cols) stack of real images (pm_sum_modes);
    with `out` and accumulate=True adds into `out`."""
    lib = L.load()
    if modes.dim() != 3 or modes.is_complex():
        raise ValueError('sum_modes takes a (B, rows, cols) stack of real images')
    if modes.stride(-1) != 1:
        modes = modes.contiguous()
    B, rows, cols = modes.shape
    w = [float(v) for v in weights]
    if len(w) != B:
        raise ValueError('one weight per mode is required')
    if out is None:
        out = torch.empty((rows, cols), dtype=modes.dtype, device=modes.device)
        accumulate = False
    else:
        _bump(out)
    code = L.PM_C64 if modes.dtype == torch.float32 else L.PM_C128
    if modes.dtype not in (torch.float32, torch.float64):
        raise TypeError('sum_modes: float32 or float64 images')
    arr = (ctypes.c_double * max(B, 1))(*w)
    L.check(lib.pm_sum_modes(code, B, rows, cols, L.ptr(modes), modes.stride(0) if B > 1 else rows * cols, modes.stride(1),
                             arr, 1 if accumulate else 0, L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def encircled_energy(mtf, df, radii_mm):
    """EE(r) for every r of radii_mm (host floats, mm) from the real centre-normalised MTF (pm_encircled_energy):
    a float64 device vector."""
    lib = L.load()
    if mtf.dim() != 2 or mtf.dtype not in (torch.float32, torch.float64):
        raise TypeError('encircled_energy: the MTF is a real 2-D float32 / float64 array')
    if mtf.stride(-1) != 1:
        mtf = mtf.contiguous()
    rows, cols = mtf.shape
    r = [float(v) for v in radii_mm]
    arr = (ctypes.c_double * max(len(r), 1))(*r)
    out = torch.empty(len(r), dtype=torch.float64, device=mtf.device)
    nbytes = lib.pm_encircled_energy_workspace()
    ws = L.workspace(nbytes)
    code = L.PM_C64 if mtf.dtype == torch.float32 else L.PM_C128
    L.check(lib.pm_encircled_energy(code, rows, cols, L.ptr(mtf), mtf.stride(0), float(df), len(r), arr, L.ptr(out), L.ptr(ws),
                                    ws.numel(), L.stream_ptr()))
    return out


def encircled_energy_adjoint(shape, df, radii_mm, ee_bar, rdtype):
    """sum_r ee_bar_r r J1(2 pi r nu) / nu df^2 on the frequency grid of `shape` (pm_encircled_energy_adjoint)."""
    lib = L.load()
    rows, cols = shape
    r = [float(v) for v in radii_mm]
    b = [float(v) for v in ee_bar]
    if len(r) != len(b):
        raise ValueError('one ee_bar value per radius is required')
    ra = (ctypes.c_double * max(len(r), 1))(*r)
    ba = (ctypes.c_double * max(len(b), 1))(*b)
    out = torch.empty((rows, cols), dtype=rdtype, device=L.device())
    code = L.PM_C64 if rdtype == torch.float32 else L.PM_C128
    L.check(lib.pm_encircled_energy_adjoint(code, rows, cols, float(df), len(r), ra, ba, L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def spline_prefilter(measurement, order):
    """B-spline coefficients of a measured complex map for orders 2 .. 5 (pm_spline_prefilter): complex128,
    (rows + 24, cols + 24) -- scipy's edge padding by 12 included."""
    lib = L.load()
    m = L.as_field(measurement)
    if not m.is_complex():
        m = m.to(L.cdtype_of(m))
    m = m.contiguous()
    coeff = torch.empty((m.shape[0] + 24, m.shape[1] + 24), dtype=torch.complex128, device=m.device)
    L.check(lib.pm_spline_prefilter(L.code(m), int(order), m.shape[0], m.shape[1], L.ptr(m), m.stride(0), L.ptr(coeff), coeff.stride(0),
                                    L.stream_ptr()))
    return coeff


def sample_map(measurement, dx, center, xf, yf, fill=1.0, order=1, coeff=None):
    """Complex map resampled at focal coordinates (pm_sample_map / pm_sample_spline): map_coordinates(order 0 .. 5, mode='nearest')
    inside the measured extent, `fill` (scalar or array of the shape of xf) outside.  xf / yf broadcast against each other."""
    lib = L.load()
    m = L.as_field(measurement)
    if not m.is_complex():
        m = m.to(L.cdtype_of(m))
    m = m.contiguous()
    rdt = torch.float32 if m.dtype == torch.complex64 else torch.float64
    xf, yf = L.as_device(xf).to(rdt), L.as_device(yf).to(rdt)
    shape = torch.broadcast_shapes(xf.shape, yf.shape)
    if len(shape) != 2:
        raise ValueError('sample_map: focal coordinates must broadcast to a 2-D grid')
    xb, yb = xf.expand(shape), yf.expand(shape)
    rows, cols = shape
    out = torch.empty(shape, dtype=m.dtype, device=m.device)
    fill_t, fre, fim = None, 0.0, 0.0
    if isinstance(fill, (int, float, complex)):
        fre, fim = float(complex(fill).real), float(complex(fill).imag)
    else:
        fill_t = torch.broadcast_to(L.as_device(fill).to(m.dtype), shape).contiguous()
    cxo, cyo = center
    if order >= 2:   # coeff: the prefiltered map (spline_prefilter), made once per measured map by the caller
        if coeff is None:
            coeff = spline_prefilter(m, order)
        L.check(lib.pm_sample_spline(L.code(m), int(order), m.shape[0], m.shape[1], L.ptr(coeff), coeff.stride(0), float(dx), float(cxo),
                                     float(cyo), rows, cols, L.ptr(xb), xb.stride(0), xb.stride(1), L.ptr(yb), yb.stride(0),
                                     yb.stride(1), L.ptr(fill_t) if fill_t is not None else None,
                                     fill_t.stride(0) if fill_t is not None else 0, fre, fim, L.ptr(out), out.stride(0), L.stream_ptr()))
        return out
    L.check(lib.pm_sample_map(L.code(m), int(order), m.shape[0], m.shape[1], L.ptr(m), m.stride(0), float(dx), float(cxo),
                              float(cyo), rows, cols, L.ptr(xb), xb.stride(0), xb.stride(1), L.ptr(yb), yb.stride(0),
                              yb.stride(1), L.ptr(fill_t) if fill_t is not None else None,
                              fill_t.stride(0) if fill_t is not None else 0, fre, fim, L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


_AMP_CODE = {torch.float32: L.PM_F32, torch.float64: L.PM_F64, torch.bool: L.PM_BOOL, torch.uint8: L.PM_BOOL}


def pupil_synth(amp, opd, k, cdtype, out=None):
    """amp * exp(i k opd); opd real tensor of the real dtype of `cdtype`; `out`: e.g. one field of a stack."""
    lib = L.load()
    rows, cols = opd.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=cdtype, device=opd.device)
    else:
        _bump(out)
    a_code, a_ld = L.PM_F32, cols
    if amp is not None:
        if amp.dtype not in _AMP_CODE:
            amp = amp.to(L._REAL_OF[cdtype])
        a_code, a_ld = _AMP_CODE[amp.dtype], amp.stride(0)
    L.check(lib.pm_pupil_synth(L._COMPLEX_CODE[cdtype], rows, cols, L.ptr(amp), a_code, a_ld, L.ptr(opd),
                               opd.stride(0), float(k), L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def quadratic_phase(x, y, c, cdtype):
    lib = L.load()
    rows, cols = x.shape
    out = torch.empty((rows, cols), dtype=cdtype, device=x.device)
    L.check(lib.pm_quadratic_phase(L._COMPLEX_CODE[cdtype], rows, cols, L.ptr(x), x.stride(0), L.ptr(y), y.stride(0),
                                   float(c), L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


# (shape, wavelength, dx, z, dtype, device, stream) -> (hy, hx): a model that steps the same distance again and again (a time series,
# the planes of a relay, an optimiser's forward passes) re-uses the two vectors instead of re-synthesising them (one launch of 5 us
# against a 320 us step at 4096^2 complex128 -- and nothing at all to wait for at small sizes, where the launch is the cost).  The key
# is scalars only, so nothing can go stale; the values are READ-ONLY by contract (angular_spectrum never hands them out).  Keyed on
# the stream because the vectors are produced on it: another stream would have to wait for that work.
_AS_TF_CACHE = {}
_AS_TF_CACHE_MAX = 16
_AS_TF_LOCK = threading.Lock()      # one pipeline per host thread is the advertised use: lookups, inserts and evictions are serialised


def clear_tf_cache(stream=None):
    """Forget the cached transfer-function vectors -- all of them, or those made on one stream (its raw handle): a destroyed stream's
    handle can be handed out again, and a new stream with an old handle must not find vectors it never waited for."""
    with _AS_TF_LOCK:
        if stream is None:
            _AS_TF_CACHE.clear()
        else:
            for k in [k for k in _AS_TF_CACHE if k[-1] == stream]:
                _AS_TF_CACHE.pop(k, None)


def as_tf_vectors(shape, wvl, dx, z, cdtype, cache=True):
    lib = L.load()
    rows, cols = shape
    key = (int(rows), int(cols), float(wvl), float(dx), float(z), cdtype, L._cur_dev(), L._cur_stream())
    if cache and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        cache = False       # tensors made during a graph capture live in the graph's pool: never handed to eager code
    if cache:
        with _AS_TF_LOCK:
            hit = _AS_TF_CACHE.get(key)
        if hit is not None:
            return hit
    hy = torch.empty(rows, dtype=cdtype, device=L.device())
    hx = torch.empty(cols, dtype=cdtype, device=L.device())
    L.check(lib.pm_as_tf_vectors(L._COMPLEX_CODE[cdtype], rows, cols, float(wvl), float(dx), float(z), L.ptr(hy),
                                 L.ptr(hx), L.stream_ptr()))
    if cache:
        with _AS_TF_LOCK:
            while len(_AS_TF_CACHE) >= _AS_TF_CACHE_MAX:
                _AS_TF_CACHE.pop(next(iter(_AS_TF_CACHE)), None)
            _AS_TF_CACHE[key] = (hy, hx)
    return hy, hx


def outer(hy, hx):
    lib = L.load()
    rows, cols = hy.numel(), hx.numel()
    out = torch.empty((rows, cols), dtype=hy.dtype, device=hy.device)
    L.check(lib.pm_outer(L.code(hy), rows, cols, L.ptr(hy), L.ptr(hx), L.ptr(out), out.stride(0), L.stream_ptr()))
    return out


def embed(x, out_shape, off, fill=0):
    """out = fill; out[off_y:off_y+m, off_x:off_x+n] = x (negative offsets crop)."""
    lib = L.load()
    m, n = x.shape
    om, on = out_shape
    out = torch.empty((om, on), dtype=x.dtype, device=x.device)
    es = x.element_size()
    if es == 2:   # float16: no kernel for 2-byte elements; widen is not acceptable silently
        raise NotImplementedError('pad2d of 2-byte element arrays is not supported')
    fill_t = torch.tensor([fill], dtype=x.dtype)   # host scalar, passed by pointer
    L.check(lib.pm_embed(es, m, n, L.ptr(x), x.stride(0) if m > 1 else n, om, on, int(off[0]), int(off[1]),
                         ctypes.c_void_p(fill_t.data_ptr()), L.ptr(out), out.stride(0) if om > 1 else on,
                         L.stream_ptr()))
    return out


_PAD_MODES = {'edge': 1, 'reflect': 2, 'symmetric': 3, 'wrap': 4}


def pad_index(x, out_shape, off, mode):
    """np.pad(x, ..., mode=mode) for the index-mapping modes ('edge', 'reflect', 'symmetric', 'wrap'): x lands at `off` of `out_shape`."""
    lib = L.load()
    m, n = x.shape
    om, on = out_shape
    if x.stride(-1) != 1:
        x = x.contiguous()
    es = x.element_size()
    if es == 2:
        raise NotImplementedError('pad2d of 2-byte element arrays is not supported')
    out = torch.empty((om, on), dtype=x.dtype, device=x.device)
    L.check(lib.pm_pad_index(es, _PAD_MODES[mode], m, n, L.ptr(x), x.stride(0) if m > 1 else n, om, on, int(off[0]), int(off[1]),
                             L.ptr(out), out.stride(0) if om > 1 else on, L.stream_ptr()))
    return out


def mdft_basis(f, x, sign, cdtype):
    """E[m, n] = exp(sign 2 pi i f[m] x[n])."""
    lib = L.load()
    M, N = f.numel(), x.numel()
    E = torch.empty((M, N), dtype=cdtype, device=f.device)
    L.check(lib.pm_mdft_basis(L._COMPLEX_CODE[cdtype], M, N, L.ptr(f), L.ptr(x), int(sign), L.ptr(E), E.stride(0),
                              L.stream_ptr()))
    return E


def mdft_basis_grid(M, N, f_step, f_shift, f_scale, x_step, sign, cdtype):
    """E[m, n] = exp(sign 2 pi i f[m] x[n]) for x = fftrange(N) * x_step, f = (fftrange(M) * f_step + f_shift) * f_scale, each
    rounded in the real type of cdtype as the elementwise array expressions would (pm_mdft_basis_grid)."""
    lib = L.load()
    E = torch.empty((M, N), dtype=cdtype, device=L.device())
    L.check(lib.pm_mdft_basis_grid(L._COMPLEX_CODE[cdtype], M, N, float(f_step), float(f_shift), float(f_scale), float(x_step),
                                   int(sign), L.ptr(E), E.stride(0), L.stream_ptr()))
    return E


def _gemm_operands(name, A, B):
    """what the library cannot see behind two pointers: both operands 2-D, of one complex dtype, on one device, rows contiguous"""
    for which, t in (('A', A), ('B', B)):
        if t.dim() != 2:
            raise ValueError(f'{name}: {which} must be 2-D, got {t.dim()} dimensions')
        if t.shape[1] > 1 and t.stride(1) != 1:     # the stride of an axis of one element means nothing
            raise ValueError(f'{name}: {which} must have a unit inner stride, got {t.stride(1)} (pass the transposed storage and op 2 / 3)')
    if A.dtype != B.dtype:
        raise ValueError(f'{name}: A and B must have the same dtype, got {A.dtype} and {B.dtype}')
    if A.device != B.device:
        raise ValueError(f'{name}: A and B must be on the same device, got {A.device} and {B.device}')


def cgemm(A, B, opA=0, opB=0, alpha=1.0):
    """alpha * op(A) @ op(B) on the MFMA cores.  op: 0 none, 1 conj, 2 transpose, 3 conjugate transpose."""
    lib = L.load()
    _gemm_operands('cgemm', A, B)
    M, K = (A.shape[1], A.shape[0]) if opA & 2 else A.shape
    K2, N = (B.shape[1], B.shape[0]) if opB & 2 else B.shape
    if K != K2:
        raise ValueError(f'matmul: inner dimensions differ ({K} vs {K2})')
    C = torch.empty((M, N), dtype=A.dtype, device=A.device)
    nbytes = lib.pm_cgemm_workspace(L.code(A), M, N, K)
    ws = L.workspace(nbytes)
    L.check(lib.pm_cgemm(L.code(A), opA, opB, M, N, K, float(alpha), L.ptr(A), A.stride(0), L.ptr(B), B.stride(0),
                         L.ptr(C), C.stride(0), L.ptr(ws), 0 if ws is None else ws.numel(), L.stream_ptr()))
    return C


def cgemm_abs2(A, B, opA=0, opB=0, alpha=1.0, out=None, weight=1.0):
    """weight * |alpha op(A) @ op(B)|^2 as a REAL image, added to `out` when given (pm_cgemm_abs2: the |.|^2 and the weighted
    accumulate in the product's epilogue, no complex result in memory).  Returns None when the shapes are not the LDS-DMA
    kernel's (the caller composes cgemm + abs2)."""
    lib = L.load()
    _gemm_operands('cgemm_abs2', A, B)
    M, K = (A.shape[1], A.shape[0]) if opA & 2 else A.shape
    K2, N = (B.shape[1], B.shape[0]) if opB & 2 else B.shape
    if K != K2:
        raise ValueError(f'matmul: inner dimensions differ ({K} vs {K2})')
    if A.dtype != torch.complex64 or B.dtype != torch.complex64 or M % 64 or N % 64 or K % 16 or M < 64 or N < 64:
        return None
    acc = 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
        acc = 0
    else:
        if out.dtype != torch.float32 or tuple(out.shape) != (M, N) or out.stride(1) != 1 or out.device != A.device:
            raise ValueError('cgemm_abs2: `out` must be a float32 (M, N) image on the device of the operands')
    nbytes = lib.pm_cgemm_workspace(L.code(A), M, N, K)
    ws = L.workspace(nbytes)
    rc = lib.pm_cgemm_abs2(L.code(A), opA, opB, M, N, K, float(alpha), L.ptr(A), A.stride(0), L.ptr(B), B.stride(0), L.ptr(out),
                           out.stride(0), float(weight), acc, L.ptr(ws), 0 if ws is None else ws.numel(), L.stream_ptr())
    if rc == L.PM_ERR_UNSUPPORTED:
        return None
    L.check(rc)
    if acc:
        _bump(out)      # written: caches keyed on (identity, version) must notice (not before the early return above: nothing was written)
    return out


# --------------------------------------------------------------------------- thin films (csrc/thinfilm.hip)

class TfOperands:
    """The operands of the thin-film kernels for K flat samples, on the device: wvl and theta (radians) real, n0 and nsub complex,
    each of K values or of one (shared by all samples); the layer tables n (complex) and d (real), (L, K) or (L, 1).  `d` is used
    where it lies when it already is a contiguous device tensor of the real type (an optimizer's x at a fixed address)."""
    __slots__ = ('cdtype', 'rdtype', 'K', 'L', 'wvl', 'theta', 'n', 'd', 'nsub', 'n0')

    def __init__(self, cdtype, K, wvl, theta, n, d, nsub, n0):
        if cdtype not in (torch.complex64, torch.complex128):
            raise TypeError(f'thin films compute in complex64 or complex128, got {cdtype}')
        self.cdtype, self.rdtype, self.K = cdtype, L._REAL_OF[cdtype], int(K)
        self.wvl, self.theta = self._vector(wvl, self.rdtype, 'wavelength'), self._vector(theta, self.rdtype, 'angle')
        self.nsub, self.n0 = self._vector(nsub, cdtype, 'substrate index'), self._vector(n0, cdtype, 'ambient index')
        self.n = self._table(n, cdtype, 'indices')
        self.L = self.n.shape[0]
        self.d = None
        self.set_thicknesses(d)

    def _vector(self, v, dtype, what):
        t = L.as_device(v, dtype).reshape(-1)
        if t.numel() not in (1, self.K):
            raise ValueError(f'{what}: {t.numel()} values for {self.K} samples')
        return t

    def _table(self, v, dtype, what):
        t = L.as_device(v, dtype)
        if t.numel() == 0:      # no layers: a bare interface
            return torch.empty((0, 1), dtype=dtype, device=t.device)
        t = t.reshape(t.shape[0], -1) if t.dim() >= 1 else t.reshape(1, 1)
        if t.shape[1] not in (1, self.K):
            raise ValueError(f'{what}: {t.shape[1]} values per layer for {self.K} samples')
        return t.contiguous()

    def set_thicknesses(self, d):
        t = self._table(d, self.rdtype, 'thicknesses')
        if t.shape[0] != self.L:
            raise ValueError(f'thicknesses describe {t.shape[0]} layers, indices {self.L}')
        self.d = t
        return self

    def args(self):
        """the operand block of both entry points, after (dtype, pol, ..., K, L)"""
        def ss(t):
            return 0 if t.numel() == 1 and self.K != 1 else 1

        def table(t):
            if self.L == 0:
                return [L.ptr(None), 0, 0]
            per = t.shape[1] != 1 or self.K == 1
            return [L.ptr(t), t.shape[1], 1 if per else 0]
        return ([L.ptr(self.wvl), ss(self.wvl), L.ptr(self.theta), ss(self.theta)] + table(self.n) + table(self.d)
                + [L.ptr(self.nsub), ss(self.nsub), L.ptr(self.n0), ss(self.n0)])


_TF_POLS = {'s': L.PM_TF_S, 'p': L.PM_TF_P, 'both': L.PM_TF_BOTH}


def tf_stack(op, pol, t_convention=L.PM_TF_T_STACK, want=()):
    """pm_tf_stack on a TfOperands: a dict with r and t and whatever `want` names of 'R', 'T', 'fields' (E and H) and 'A'.  pol is
    's', 'p' or 'both'; every array has the leading axis of polarisations (1 or 2), then boundaries or layers, then the K samples.
    One launch."""
    code = _TF_POLS[pol]
    NP, K, Ly = (2 if pol == 'both' else 1), op.K, op.L
    dev = L.device()
    out = {'r': torch.empty((NP, K), dtype=op.cdtype, device=dev), 't': torch.empty((NP, K), dtype=op.cdtype, device=dev)}
    if 'R' in want:
        out['R'] = torch.empty((NP, K), dtype=op.rdtype, device=dev)
    if 'T' in want:
        out['T'] = torch.empty((NP, K), dtype=op.rdtype, device=dev)
    if 'fields' in want:
        out['E'] = torch.empty((NP, Ly + 1, K), dtype=op.cdtype, device=dev)
        out['H'] = torch.empty((NP, Ly + 1, K), dtype=op.cdtype, device=dev)
    if 'A' in want:
        out['A'] = torch.empty((NP, Ly, K), dtype=op.rdtype, device=dev)
    if K:
        lib = L.load()
        L.check(lib.pm_tf_stack(L._COMPLEX_CODE[op.cdtype], code, int(t_convention), K, Ly, *op.args(), L.ptr(out['r']), L.ptr(out['t']),
                                L.ptr(out.get('R')), L.ptr(out.get('T')), L.ptr(out.get('E')), L.ptr(out.get('H')), L.ptr(out.get('A')),
                                L.stream_ptr()))
    return out


def tf_thickness_grad(op, pol, dR=None, dT=None, grad=None):
    """pm_tf_thickness_grad on a TfOperands: the (L,) gradient of sum_k F with respect to the thicknesses from the seeds dR, dT (K
    values shared by the polarisations, or (2, K) with pol 'both'; either may be None).  Added to `grad` when that is given.  Two
    launches; the sum over samples is in double and in a fixed order."""
    code = _TF_POLS[pol]
    NP, K, Ly = (2 if pol == 'both' else 1), op.K, op.L
    acc = grad is not None
    if acc:
        if grad.dtype != op.rdtype or grad.numel() != Ly or not grad.is_contiguous() or grad.device != L.device():
            raise ValueError('thickness gradient: `grad` must be a contiguous device tensor of one real value per layer')
    else:
        grad = torch.zeros(Ly, dtype=op.rdtype, device=L.device())
    ps = 0

    def seed(s):
        nonlocal ps
        if s is None:
            return None
        t = L.as_device(s, op.rdtype).reshape(-1)
        if t.numel() == NP * K and NP == 2:
            ps = K
        elif t.numel() != K:
            raise ValueError(f'a seed has {t.numel()} values for {K} samples')
        return t
    r, t = seed(dR), seed(dT)
    if r is not None and t is not None and r.numel() != t.numel():
        raise ValueError('dR and dT must have the same shape')
    if K == 0 or Ly == 0 or (r is None and t is None):
        return grad
    lib = L.load()
    cd = L._COMPLEX_CODE[op.cdtype]
    ws = L.workspace(int(lib.pm_tf_thickness_grad_workspace(cd, code, K, Ly)))
    L.check(lib.pm_tf_thickness_grad(cd, code, K, Ly, *op.args(), L.ptr(r), L.ptr(t), ps, int(acc), L.ptr(grad), L.ptr(ws), ws.numel(),
                                     L.stream_ptr()))
    return grad


# --------------------------------------------------------------------------- ray trace (csrc/raytrace.hip)

def rt_trace(table, n_launch, tol_sag, P, S, history=True):
    """pm_rt_trace: N rays P, S ((N, 3) device tensors of float32 or float64, any strides) through the J records of `table` (a device
    tensor of float64, x/raytrace_plan.py pack_table).  Returns P, S ((J + 1, N, 3), or (N, 3) without history), OPL ((J + 1, N) or
    (N,)) and the int32 status tensors surface and code.  One launch; nothing is read on the host and nothing copied to the device."""
    dev = L.device()
    if P.dtype not in (torch.float32, torch.float64) or S.dtype != P.dtype:
        raise TypeError(f'rays are float32 or float64 and P and S of one type, got {P.dtype} and {S.dtype}')
    if P.dim() != 2 or P.shape[1] != 3 or S.shape != P.shape:
        raise ValueError(f'P and S are (N, 3), got {tuple(P.shape)} and {tuple(S.shape)}')
    if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != L.PM_RT_RECORD or not table.is_contiguous():
        raise ValueError('the surface table is a contiguous (J, PM_RT_RECORD) float64 tensor')
    P, S = P.contiguous(), S.contiguous()
    N, J = P.shape[0], table.shape[0]
    rows = (J + 1,) if history else ()
    Po, So = torch.empty(rows + (N, 3), dtype=P.dtype, device=dev), torch.empty(rows + (N, 3), dtype=P.dtype, device=dev)
    Oo = torch.empty(rows + (N,), dtype=P.dtype, device=dev)
    surface, code = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    if J == 0:      # no surface: the launch is the result
        (Po[0] if history else Po).copy_(P), (So[0] if history else So).copy_(S)
        Oo.zero_(), surface.zero_(), code.zero_()
    L.check(L.load().pm_rt_trace(L.PM_F32 if P.dtype == torch.float32 else L.PM_F64, N, J, L.ptr(table), float(n_launch), float(tol_sag),
                                 int(bool(history)), L.ptr(P), L.ptr(S), L.ptr(Po), L.ptr(So), L.ptr(Oo), L.ptr(surface), L.ptr(code),
                                 L.stream_ptr()))
    return Po, So, Oo, surface, code


def ceil_half(d):
    return math.ceil(d / 2)


# Inside a ``prysm_amd.graph.sequence()`` block every array-level entry point asks the block for its stream (independent calls alternate
# between the streams of a ring, dependent ones follow their producer); outside of one the wrapper is one thread-local read.
for _name in ('fft2', 'fft2_real', 'pack_amp_opd', 'fft2_mul_ifft2', 'fft1', 'czt_vectors', 'czt_axis', 'fft1_ramp', 'cmul', 'rmul', 'scale_sep', 'abs2',
              'abs_arg', 'sum_modes', 'encircled_energy', 'encircled_energy_adjoint', 'spline_prefilter', 'sample_map', 'pupil_synth',
              'quadratic_phase', 'as_tf_vectors', 'outer', 'embed', 'pad_index', 'mdft_basis', 'mdft_basis_grid', 'cgemm', 'cgemm_abs2'):
    globals()[_name] = sequenced(globals()[_name])
del _name


# --------------------------------------------------------------------------- the image chain (csrc/imagechain.hip)

def _rows(t, dtype):
    """a device tensor as rows with unit element stride: (2-D tensor, elements between its rows).  Strided row views pass as they are."""
    as_is = (isinstance(t, torch.Tensor) and t.device == L.device() and t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1
             and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) and not t.is_conj() and not t.is_neg())
    if not as_is:
        t = L.as_device(t, dtype)
        t = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _vector(t, dtype):
    """a 1-D device tensor and the elements between its values (a column of a 2-D array passes as it is)"""
    if isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == L.device() and t.dim() == 1 and t.stride(0) >= 1:
        return t, t.stride(0)
    t = L.as_device(t, dtype).reshape(-1)
    return t, 1


def object_render(kind, flags, p, dtype, coords, ny, nx, *, a=None, lda=0, b=None, ldb=0, dx=0.0, polar=False):
    """pm_object_render: a target of kind / flags / parameters p on ny x nx samples; a torch.bool mask for the slit and the pinhole"""
    from . import imagechain_plan as IP
    obj = L.pm_object()
    obj.kind, obj.flags = int(kind), int(flags)
    for i, v in enumerate(p):
        obj.p[i] = float(v)
    odt = torch.bool if kind in (IP.SLIT, IP.PINHOLE) else dtype
    out = torch.empty((ny, nx), dtype=odt, device=L.device())
    L.check(L.load().pm_object_render(L.PM_F32 if dtype == torch.float32 else L.PM_F64, coords, int(bool(polar)), ny, nx, L.ptr(a), lda, L.ptr(b),
                                      ldb, float(dx), ctypes.byref(obj), L.ptr(out), nx, L.stream_ptr()))
    return out


def tf_product(shape, factors, dtype, *, dx=None, shift=False, fx=None, fy=None, fr=None, real_out=False):
    """pm_tf_product: H (m, n) = the product of the factors -- imagechain_plan Records and arrays of shape (m, n) -- with its origin at
    [0, 0], in one launch.  dtype: the REAL working precision; H is complex of it unless real_out.  Frequencies: dx (generated), or 1-D
    fx (n) and fy (m), or 2-D arrays fx / fy / fr of shape (m, n); with shift they and the arrays are centred."""
    from . import imagechain_plan as IP
    m, n = int(shape[0]), int(shape[1])
    cdt = L._COMPLEX_OF[dtype]
    keep, packed = [], []
    for f in IP.flatten(factors):
        if isinstance(f, IP.Record):
            packed.append(f)
            continue
        t = f if isinstance(f, torch.Tensor) else L.as_device(f)
        cplx = t.is_complex()
        if tuple(t.shape) != (m, n):
            t = torch.broadcast_to(L.as_device(t), (m, n)).contiguous()
        t, ld = _rows(t, cdt if cplx else dtype)
        if cplx and real_out:
            raise ValueError('a complex array among the transfer functions needs a complex result')
        keep.append(t)
        packed.append((IP.MAP_COMPLEX if cplx else IP.MAP_REAL, ld, t.data_ptr()))
    table = IP.pack_records(packed)
    fq = L.pm_tf_freq()
    fq.shift = int(bool(shift))
    if dx is not None:
        fq.mode, fq.dx = L.PM_FREQ_GRID, float(dx)
    elif all(v is None or (isinstance(v, torch.Tensor) and v.dim() == 1) for v in (fx, fy)) and fr is None:
        fq.mode = L.PM_FREQ_VECTORS
        for name, v, length in (('fx', fx, n), ('fy', fy, m)):
            if v is None:
                continue
            t, st = _vector(v, dtype)
            if t.numel() != length or (name == 'fx' and st != 1):
                if t.numel() != length:
                    raise ValueError(f'{name} has {t.numel()} values for an axis of {length}')
                t, st = t.contiguous(), 1
            keep.append(t)
            setattr(fq, name, t.data_ptr())
            if name == 'fy':
                fq.ldy = st
    else:
        fq.mode = L.PM_FREQ_POINTWISE
        for name, v, ldn in (('fx', fx, 'ldx'), ('fy', fy, 'ldy'), ('fr', fr, 'ldr')):
            if v is None:
                continue
            t = v if isinstance(v, torch.Tensor) else L.as_device(v, dtype)
            if tuple(t.shape) != (m, n):
                t = torch.broadcast_to(t.reshape(1, -1) if t.dim() == 1 else t, (m, n)).contiguous()
            t, ld = _rows(t, dtype)
            keep.append(t)
            setattr(fq, name, t.data_ptr())
            setattr(fq, ldn, ld)
    out = torch.empty((m, n), dtype=dtype if real_out else cdt, device=L.device())
    recs = table.ctypes.data_as(ctypes.POINTER(L.pm_tf_record)) if len(table) else None
    L.check(L.load().pm_tf_product(L.PM_F32 if dtype == torch.float32 else L.PM_F64, m, n, ctypes.byref(fq), recs, len(table),
                                   int(not real_out), L.ptr(out), n, L.stream_ptr()))
    return out


def polar_resample(x, y, x_step, y_step, rho, phi, data):
    """pm_polar_resample: data (ny, nx) on the axes x, y gathered onto rho (nx) x phi (ny), all device tensors of data's dtype"""
    ny, nx = data.shape
    out = torch.empty((ny, nx), dtype=data.dtype, device=data.device)
    L.check(L.load().pm_polar_resample(L.PM_F32 if data.dtype == torch.float32 else L.PM_F64, ny, nx, L.ptr(x), L.ptr(y), float(x_step),
                                       float(y_step), L.ptr(rho), L.ptr(phi), L.ptr(data), data.stride(0) if ny > 1 else nx, L.ptr(out), nx,
                                       L.stream_ptr()))
    return out


def centroid(data):
    """pm_centroid: the centre of mass (row, col) of a 2-D real device tensor as a float64 device 2-vector; nothing is read back"""
    lib = L.load()
    m, n = data.shape
    out = torch.empty(2, dtype=torch.float64, device=data.device)
    nbytes = lib.pm_centroid_workspace(m, n)
    ws = L.workspace(nbytes)
    L.check(lib.pm_centroid(L.PM_F32 if data.dtype == torch.float32 else L.PM_F64, m, n, L.ptr(data), data.stride(0) if m > 1 else n,
                            L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()))
    return out


def psf_size(polar, r, relative, value, last):
    """pm_psf_size: (mean crossing radius, count) of a polar map as a float64 device 2-vector; nothing is read back"""
    lib = L.load()
    rows, cols = polar.shape
    out = torch.empty(2, dtype=torch.float64, device=polar.device)
    nbytes = lib.pm_psf_size_workspace(rows)
    ws = L.workspace(nbytes)
    L.check(lib.pm_psf_size(L.PM_F32 if polar.dtype == torch.float32 else L.PM_F64, rows, cols, L.ptr(polar),
                            polar.stride(0) if rows > 1 else cols, L.ptr(r), int(relative), float(value), int(last), L.ptr(out), L.ptr(ws),
                            nbytes, L.stream_ptr()))
    return out


# --------------------------------------------------------------------------- the wavefront sensors (csrc/sensors.hip)

_FRAME_CODE = {torch.float32: L.PM_F32, torch.float64: L.PM_F64, torch.uint8: L.PM_U8, torch.uint16: L.PM_U16}


def _rcode(dtype):
    return L.PM_F32 if dtype == torch.float32 else L.PM_F64


def psi(frames, s, c, out_dtype, want=(True, True, True)):
    """pm_psi: (num, den, phase) -- None where `want` is False -- of K frames, device tensors of one shape (rows, cols), one dtype and one
    row stride, each read where it lies (a (K, rows, cols) tensor passes as the list of its planes).  s, c: K host floats."""
    K = len(frames)
    f0 = frames[0]
    rows, cols = f0.shape
    ld = f0.stride(0) if rows > 1 else cols
    tab = L.pm_psi_frames()
    for k, f in enumerate(frames):
        tab.frame[k] = f.data_ptr()
        tab.s[k], tab.c[k] = float(s[k]), float(c[k])
    outs = [torch.empty((rows, cols), dtype=out_dtype, device=f0.device) if w else None for w in want]
    L.check(L.load().pm_psi(_FRAME_CODE[f0.dtype], _rcode(out_dtype), K, rows, cols, ctypes.byref(tab), ld, L.ptr(outs[0]), L.ptr(outs[1]),
                            L.ptr(outs[2]), cols, L.stream_ptr()))
    return tuple(outs)


def lenslet_screen(par, dtype, coords, ny, nx, *, x=None, ldx=0, y=None, ldy=0, dx=0.0):
    """pm_lenslet_screen: the complex screen (ny, nx) of the lenslet array `par` (x/sensors_plan.lenslet_params)"""
    lens = L.pm_lenslets()
    for name, v in par.items():
        setattr(lens, name, v)
    out = torch.empty((ny, nx), dtype=L._COMPLEX_OF[dtype], device=L.device())
    L.check(L.load().pm_lenslet_screen(_rcode(dtype), coords, ny, nx, L.ptr(x), ldx, L.ptr(y), ldy, float(dx), ctypes.byref(lens), L.ptr(out), nx,
                                       L.stream_ptr()))
    return out


def grating(kind, p, dtype, coords, rows, cols, *, x=None, ldx=0, dx=0.0, shift=0.0, field=None):
    """pm_grating: the grating `kind` with parameters p at x + shift -- real (rows, cols) -- or `field` (complex of dtype) times it"""
    arr = (ctypes.c_double * 5)(*[float(v) for v in p])
    fld = 0
    if field is not None:
        field = _rows2d(field)
        fld = field.stride(0) if rows > 1 else cols
    out = torch.empty((rows, cols), dtype=dtype if field is None else L._COMPLEX_OF[dtype], device=L.device())
    L.check(L.load().pm_grating(_rcode(dtype), kind, coords, rows, cols, L.ptr(x), ldx, float(dx), float(shift), arr, L.ptr(field), fld, L.ptr(out),
                                cols, L.stream_ptr()))
    return out


def beam_combine(a, ca, b, cb, want_total=False, want_intensity=True):
    """pm_beam_combine: (|ca a + cb b|^2, ca a + cb b) of two complex 2-D device tensors of one dtype; None where not wanted"""
    a, b = _rows2d(a), _rows2d(b)
    rows, cols = a.shape
    inten = torch.empty((rows, cols), dtype=L._REAL_OF[a.dtype], device=a.device) if want_intensity else None
    total = torch.empty((rows, cols), dtype=a.dtype, device=a.device) if want_total else None
    L.check(L.load().pm_beam_combine(L.code(a), rows, cols, L.ptr(a), a.stride(0) if rows > 1 else cols, float(ca), L.ptr(b),
                                     b.stride(0) if rows > 1 else cols, float(cb), L.ptr(inten), cols, L.ptr(total), cols, L.stream_ptr()))
    return inten, total


def fiber_scale(efib, power, eta, phase_shift=0.0):
    """pm_fiber_scale: efib sqrt(power eta) exp(i phase_shift); power, eta: 0-d (or 1-element) device tensors of efib's dtype"""
    efib = _rows2d(efib)
    rows, cols = efib.shape
    out = torch.empty((rows, cols), dtype=L._COMPLEX_OF[efib.dtype], device=efib.device)
    L.check(L.load().pm_fiber_scale(_rcode(efib.dtype), rows, cols, L.ptr(efib), efib.stride(0) if rows > 1 else cols, L.ptr(power), L.ptr(eta),
                                    math.cos(phase_shift), math.sin(phase_shift), L.ptr(out), cols, L.stream_ptr()))
    return out


# --------------------------------------------------------------------------- measured maps with invalid pixels (csrc/interferogram.hip)

def _ld(t):
    """elements between the rows of a 2-D tensor with unit column stride (one row: its length)"""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def ifg_window2d(t):
    """a real 2-D device tensor as the unit's kernels address it, in place: unit column stride and rows at least a row apart -- a
    contiguous array or a view of one such as Interferogram.crop leaves.  Nothing is copied: the edits write through"""
    if t.dim() != 2 or t.dtype not in (torch.float32, torch.float64) or not t.is_cuda:
        raise TypeError('a 2-D float32 / float64 device tensor is required')
    if t.numel() and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise ValueError('the rows of the map must be contiguous and must not overlap')
    return t


def ifg_coords(dtype, mode, *, x=None, y=None, origin=(0, 0), dx=0.0, linspace=None):
    """(pm_ifg_coords, tensors to keep alive, the arrays' shapes or None).  GRID: origin (oy, ox) and step dx, or linspace = (x0, dx, y0, dy); SEPARABLE: 1-D x and y;
    POINTWISE: 2-D x and y"""
    co = L.pm_ifg_coords()
    co.mode = mode
    keep = []
    shapes = None
    if mode != L.PM_COORDS_GRID:
        shapes = (tuple(x.shape), tuple(y.shape))      # as given: checked against the data by ifg_fit / ifg_remove, nothing broadcasts
    if mode == L.PM_COORDS_GRID:
        if linspace is not None:
            co.linspace = 1
            co.x0, co.dx, co.y0, co.dy = (float(v) for v in linspace)
        else:
            co.oy, co.ox = int(origin[0]), int(origin[1])
            co.dx = co.dy = float(dx)
    elif mode == L.PM_COORDS_SEPARABLE:
        x, _ = _vector(x, dtype)
        y, co.ldy = _vector(y, dtype)
        if x.stride(0) != 1:
            x = x.contiguous()
        co.x, co.y = x.data_ptr(), y.data_ptr()
        keep += [x, y]
    else:
        x, co.ldx = _rows(x, dtype)
        y, co.ldy = _rows(y, dtype)
        co.x, co.y = x.data_ptr(), y.data_ptr()
        keep += [x, y]
    return co, keep, shapes


def _check_coords(co, data):
    if co[2] is not None:
        from .interferogram_plan import check_coord_shapes
        check_coord_shapes(co[2][0], co[2][1], tuple(data.shape))


def ifg_stats(data):
    """pm_ifg_stats: the record of PM_IFG_RECORD float64 values of a 2-D real device tensor, on the device; nothing is read back"""
    lib = L.load()
    data = ifg_window2d(data)
    rows, cols = data.shape
    rec = torch.empty(L.PM_IFG_RECORD, dtype=torch.float64, device=data.device)
    nbytes = lib.pm_ifg_stats_workspace(rows, cols)
    ws = L.workspace(nbytes)
    L.check(lib.pm_ifg_stats(_rcode(data.dtype), rows, cols, L.ptr(data), _ld(data), L.ptr(rec), L.ptr(ws), nbytes, L.stream_ptr()))
    return rec


def ifg_fit(data, terms, co):
    """pm_ifg_fit: the four coefficients (piston, x, y, x^2 + y^2) as a float64 device vector; co from ifg_coords"""
    lib = L.load()
    data = ifg_window2d(data)
    _check_coords(co, data)
    rows, cols = data.shape
    coef = torch.empty(4, dtype=torch.float64, device=data.device)
    nbytes = lib.pm_ifg_fit_workspace(rows, cols)
    ws = L.workspace(nbytes)
    L.check(lib.pm_ifg_fit(_rcode(data.dtype), int(terms), rows, cols, L.ptr(data), _ld(data), ctypes.byref(co[0]), L.ptr(coef), L.ptr(ws), nbytes,
                           L.stream_ptr()))
    return coef


def ifg_remove(data, terms, co, coef):
    """pm_ifg_remove: data -= the chosen terms, on the finite pixels, in place"""
    data = ifg_window2d(data)
    _check_coords(co, data)
    rows, cols = data.shape
    L.check(L.load().pm_ifg_remove(_rcode(data.dtype), int(terms), rows, cols, L.ptr(data), _ld(data), ctypes.byref(co[0]), L.ptr(coef), L.stream_ptr()))
    return data


def ifg_edit(data, op, value=0.0, mask=None, record=None):
    """pm_ifg_edit in place: PM_IFG_FILL (NaN -> value), PM_IFG_MASK (NaN where the bool / uint8 mask is false), PM_IFG_CLIP (NaN where
    |z| > value * record[PM_IFG_STD])"""
    data = ifg_window2d(data)
    rows, cols = data.shape
    mld = 0
    if mask is not None:
        mask = L.as_device(mask) if not isinstance(mask, torch.Tensor) else mask.to(data.device)
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask != 0
        if tuple(mask.shape) != (rows, cols):
            raise ValueError(f'the mask has shape {tuple(mask.shape)}, the data {(rows, cols)}')
        mask = _rows2d(mask)
        mld = _ld(mask)
    L.check(L.load().pm_ifg_edit(_rcode(data.dtype), int(op), rows, cols, L.ptr(data), _ld(data), float(value), L.ptr(mask), mld, L.ptr(record),
                                 L.stream_ptr()))
    return data


def ifg_slope(data, dx):
    """pm_ifg_slope: (gx, gy, hypot(gx, gy)) of np.gradient(data, dx)"""
    data = ifg_window2d(data)
    rows, cols = data.shape
    gx, gy, gr = (torch.empty((rows, cols), dtype=data.dtype, device=data.device) for _ in range(3))
    L.check(L.load().pm_ifg_slope(_rcode(data.dtype), rows, cols, L.ptr(data), _ld(data), float(dx), L.ptr(gx), L.ptr(gy), L.ptr(gr), cols, L.stream_ptr()))
    return gx, gy, gr


def ifg_window(kind, shape, dtype, *, height=None, dx=0.0, alpha=4.0, window=None):
    """pm_ifg_window: (height x window -- the window itself without a height --, S2 as a one-element float64 device tensor)"""
    lib = L.load()
    rows, cols = int(shape[0]), int(shape[1])
    dev = L.device()
    hld = wld = 0
    if height is not None:
        height = ifg_window2d(height)
        hld = _ld(height)
    if window is not None:
        window, wld = _rows(window, dtype)
        if tuple(window.shape) != (rows, cols):
            raise ValueError(f'the window has shape {tuple(window.shape)}, the data {(rows, cols)}')
    out = torch.empty((rows, cols), dtype=dtype, device=dev)
    s2 = torch.empty(1, dtype=torch.float64, device=dev)
    nbytes = lib.pm_ifg_window_workspace(rows, cols)
    ws = L.workspace(nbytes)
    L.check(lib.pm_ifg_window(_rcode(dtype), int(kind), rows, cols, L.ptr(height), hld, float(dx), float(alpha), L.ptr(window), wld, L.ptr(out), cols,
                              L.ptr(s2), L.ptr(ws), nbytes, L.stream_ptr()))
    return out, s2


def ifg_psd_scale(data, s2, fs):
    """pm_ifg_psd_scale: data /= s2[0] * fs * fs in place"""
    data = ifg_window2d(data)
    rows, cols = data.shape
    L.check(L.load().pm_ifg_psd_scale(_rcode(data.dtype), rows, cols, L.ptr(data), _ld(data), L.ptr(s2), float(fs), L.stream_ptr()))
    return data


def ifg_band(psd, flow, fhigh, *, nu=None, dx=0.0):
    """pm_ifg_band: (integral, spacing) as a float64 device 2-vector.  psd 2-D with nu None (generated from dx) or 2-D; psd 1-D with nu 1-D"""
    lib = L.load()
    ndim = psd.dim()
    p = psd.reshape(-1, 1) if ndim == 1 else psd
    if ndim == 1 and not p.is_contiguous():
        p = p.contiguous()
    p = ifg_window2d(p)
    rows, cols = p.shape
    nld = 0
    if nu is not None:
        nu = nu.reshape(-1, 1) if nu.dim() == 1 else nu
        nu, nld = _rows(nu, p.dtype)
        if tuple(nu.shape) != (rows, cols):
            raise ValueError(f'the frequencies have shape {tuple(nu.shape)}, the spectrum {(rows, cols)}')
    out = torch.empty(2, dtype=torch.float64, device=p.device)
    nbytes = lib.pm_ifg_band_workspace(rows, cols)
    ws = L.workspace(nbytes)
    L.check(lib.pm_ifg_band(_rcode(p.dtype), L.PM_COORDS_GRID if nu is None else L.PM_COORDS_POINTWISE, ndim, rows, cols, L.ptr(p), _ld(p), L.ptr(nu), nld,
                            float(dx), float(flow), float(fhigh), L.ptr(out), L.ptr(ws), nbytes, L.stream_ptr()))
    return out


def ifg_iir(shape, dtype, dx, fcn_low, fcn_high=None, *, r=None, origin=(0, 0), r_dx=0.0, parts=L.PM_IFG_IIR_HANN | L.PM_IFG_IIR_LPF):
    """pm_ifg_iir: (h'_low, h'_high or None), r generated from (origin, r_dx) or a 2-D array; parts: the window, the impulse response or
    their product"""
    rows, cols = int(shape[0]), int(shape[1])
    dev = L.device()
    rld = 0
    if r is not None:
        r, rld = _rows(r, dtype)
        if tuple(r.shape) != (rows, cols):
            raise ValueError(f'the radial coordinate has shape {tuple(r.shape)}, the filter {(rows, cols)}')
    lo = torch.empty((rows, cols), dtype=dtype, device=dev)
    hi = torch.empty((rows, cols), dtype=dtype, device=dev) if fcn_high is not None else None
    L.check(L.load().pm_ifg_iir(_rcode(dtype), int(parts), L.PM_COORDS_GRID if r is None else L.PM_COORDS_POINTWISE, rows, cols, L.ptr(r), rld, int(origin[0]),
                                int(origin[1]), float(r_dx), float(dx), float(fcn_low), float(fcn_high or 0.0), L.ptr(lo), L.ptr(hi), cols, L.stream_ptr()))
    return lo, hi


def ifg_combine(typ, Hl, Hh=None, complex_out=False):
    """pm_ifg_combine: the transfer function of a filter type from |fft2(h')|, real or as a complex multiplier"""
    Hl = _rows2d(Hl)
    rows, cols = Hl.shape
    hld = 0
    if Hh is not None:
        Hh = _rows2d(Hh)
        if tuple(Hh.shape) != (rows, cols) or Hh.dtype != Hl.dtype:
            raise ValueError('the two spectra of a band filter differ in shape or precision')
        hld = _ld(Hh)
    out = torch.empty((rows, cols), dtype=L._COMPLEX_OF[Hl.dtype] if complex_out else Hl.dtype, device=Hl.device)
    L.check(L.load().pm_ifg_combine(_rcode(Hl.dtype), int(typ), int(bool(complex_out)), rows, cols, L.ptr(Hl), _ld(Hl), L.ptr(Hh), hld, L.ptr(out), cols,
                                    L.stream_ptr()))
    return out


def ifg_psd_model(kind, nu, a, b, c=0.0):
    """pm_ifg_psd_model: abc_psd / ab_psd of a real device tensor of any shape"""
    nu = nu.contiguous()
    out = torch.empty_like(nu)
    L.check(L.load().pm_ifg_psd_model(_rcode(nu.dtype), int(kind), nu.numel(), L.ptr(nu), float(a), float(b), float(c), L.ptr(out), L.stream_ptr()))
    return out


# --------------------------------------------------------------------------- surfaces synthesised from a PSD (csrc/psdsynth.hip)

def _stack3(t):
    """a real or complex (B, m, n) device tensor as the unit addresses it: unit column stride, rows and members that do not overlap"""
    if t.dim() != 3 or not t.is_cuda:
        raise TypeError('a (batch, rows, cols) device tensor is required')
    B, m, n = t.shape
    if t.numel() and (t.stride(2) != 1 or (m > 1 and t.stride(1) < n) or (B > 1 and t.stride(0) < m * (t.stride(1) if m > 1 else n))):
        raise ValueError('the rows of a surface must be contiguous, and rows and surfaces must not overlap')
    return t, (t.stride(1) if m > 1 else n), (t.stride(0) if B > 1 else m * (t.stride(1) if m > 1 else n))


def psd_uniform(shape, dtype, seed, surface0=0, out=None):
    """pm_psd_uniform: a (B, m, n) tensor of uniform numbers in [0, 1), surface b drawn with surface index surface0 + b"""
    B, m, n = (int(v) for v in shape)
    if out is None:
        out = torch.empty((B, m, n), dtype=dtype, device=L.device())
    out, ld, bs = _stack3(out)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    L.check(L.load().pm_psd_uniform(_rcode(dtype), B, m, n, seed - (1 << 64) if seed >> 63 else seed, int(surface0), L.ptr(out), ld, bs, L.stream_ptr()))
    return out


def psd_signal(spectrum, area, *, psd=None, model=None):
    """pm_psd_signal in place on a complex (B, m, n) spectrum: psd a real (m, n) array, or model = (kind, a, b, c, dxg)"""
    spectrum, ld, bs = _stack3(spectrum)
    B, m, n = spectrum.shape
    rdt = L._REAL_OF[spectrum.dtype]
    pld, rec = 0, None
    if psd is not None:
        psd, pld = _rows(psd, rdt)
        if tuple(psd.shape) != (m, n):
            raise ValueError(f'the psd has shape {tuple(psd.shape)}, the spectrum {(m, n)}')
    if model is not None:
        rec = L.pm_psd_model(int(model[0]), 0, float(model[1]), float(model[2]), float(model[3]), float(model[4]))
    L.check(L.load().pm_psd_signal(_rcode(rdt), B, m, n, L.ptr(spectrum), ld, bs, L.ptr(psd), pld, ctypes.byref(rec) if rec is not None else None,
                                   float(area), L.stream_ptr()))
    return spectrum


def psd_finish(field, *, mask=None, circle=None, out=None):
    """pm_psd_finish: (z = real(field) with NaN outside the mask, the (B, 2) float64 device tensor of counts and sums of squares).
    mask: a bool / uint8 (m, n) device tensor; circle: (radius, step)"""
    lib = L.load()
    field, ld, bs = _stack3(field)
    B, m, n = field.shape
    rdt = L._REAL_OF[field.dtype]
    if out is None:
        out = torch.empty((B, m, n), dtype=rdt, device=field.device)
    out, old, obs = _stack3(out)
    if tuple(out.shape) != (B, m, n) or out.dtype != rdt:
        raise ValueError('the output differs from the field in shape or precision')
    kind, mld, radius, step = L.PM_PSD_MASK_NONE, 0, 0.0, 0.0
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (m, n):
            raise ValueError(f'the mask must be a bool or uint8 array of shape {(m, n)}')
        mask = _rows2d(mask)
        kind, mld = L.PM_PSD_MASK_ARRAY, _ld(mask)
    elif circle is not None:
        kind, radius, step = L.PM_PSD_MASK_CIRCLE, float(circle[0]), float(circle[1])
    sums = torch.empty((B, 2), dtype=torch.float64, device=field.device)
    nbytes = lib.pm_psd_finish_workspace(B, m, n)
    ws = L.workspace(nbytes)
    L.check(lib.pm_psd_finish(_rcode(rdt), kind, B, m, n, L.ptr(field), ld, bs, L.ptr(mask), mld, radius, step, L.ptr(out), old, obs, L.ptr(sums),
                              L.ptr(ws), nbytes, L.stream_ptr()))
    return out, sums


def psd_scale(z, sums, rms):
    """pm_psd_scale in place: each surface times rms / sqrt(sum / count), the sums read on the device"""
    z, ld, bs = _stack3(z)
    B, m, n = z.shape
    L.check(L.load().pm_psd_scale(_rcode(z.dtype), B, m, n, L.ptr(z), ld, bs, L.ptr(sums), float(rms), L.stream_ptr()))
    return z
