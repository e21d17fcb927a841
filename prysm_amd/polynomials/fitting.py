"""Mode sums, their adjoint and masked fits (prysm/polynomials/fitting.py) over a stored basis.

The fits run on csrc/modalfit.hip; prysm_amd/polynomials/fit_plan.py restates its kernels in numpy.  Launches and host reads per call:

  lstsq                   4 launches (pm_modes_gram: the Gram pass and its fold; pm_modes_small FACTOR and SOLVE), no host read
  normalize_modes         6 launches (pm_modes_stats 4, NORMS, pm_modes_transform DIAGONAL), no host read
  orthogonalize_modes     5 launches (Gram pass and fold, FACTOR, INVERT, pm_modes_transform LOWER with zero_outside), no host read
  prepare_lstsq           3 launches (Gram pass and fold, FACTOR); ModalFit.fit 3 (the right-hand sides and their fold, SOLVE) for up
                          to 16 frames, 2 more per further 16; .rank is one host read
  hopkins                 tensor operations, not a kernel

At most PM_MODES_FIT_MAX = 128 modes per fit (normalize_modes takes any number, 128 at a time).
"""
import numpy as np
import torch

from .. import _lib as L
from .. import _ops
from . import fit_plan as FP

__all__ = ['sum_of_2d_modes', 'sum_of_2d_modes_adjoint', 'lstsq', 'normalize_modes', 'orthogonalize_modes', 'hopkins', 'prepare_lstsq',
           'ModalFit']


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


def _is_complex(a):
    return a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a)


def _modes(modes):
    if isinstance(modes, (list, tuple)):
        modes = torch.stack([L.as_device(m) for m in modes])
    m = L.as_device(modes)
    if m.dim() < 2 or m.is_complex() or m.dtype not in (torch.float32, torch.float64):
        raise TypeError('modes must be a (K, ...) float32 or float64 array')
    return m


def sum_of_2d_modes(modes, weights):
    """sum_k weights[k] modes[k] over a (K, rows, cols) stack (fitting.py:7-37), in the modes' dtype (pm_sum_modes).

    The weights are read on the HOST when the call is made: a captured graph keeps the weights it was captured with.  To change the
    weights of a captured model, use zernike_sum, which reads its coefficients on the device."""
    shape = _shape(modes)
    if len(shape) != 3:
        raise ValueError('sum_of_2d_modes takes a (K, rows, cols) stack of modes')
    w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
    if w.ndim != 1 or len(w) != shape[0]:
        raise ValueError(f'{np.shape(w)} weights do not match {shape[0]} modes')
    m = _modes(modes)
    return _ops.sum_modes(m, [float(v) for v in w])


def sum_of_2d_modes_adjoint(modes, databar):
    """np.tensordot(modes, databar) of the reference (fitting.py:40-57): (K,) in the modes' dtype, sum_p modes[k][p] databar[p] over
    every point (pm_modes_dot).  Deterministic: two launches, no atomics."""
    shape, shape_g = _shape(modes), _shape(databar)
    if shape_g != tuple(shape[1:]):
        raise ValueError(f'databar of shape {shape_g} does not match modes of shape {shape}')
    if _is_complex(databar) or _is_complex(modes):
        raise TypeError('modes and databar must be real')
    m = _modes(modes)
    g = L.as_device(databar, m.dtype)
    K, npts = m.shape[0], g.numel()
    code = L.PM_F32 if m.dtype == torch.float32 else L.PM_F64
    out = torch.empty((K,), dtype=m.dtype, device=m.device)
    if K:
        lib = L.load()
        ws = L.workspace(lib.pm_modes_dot_workspace(code, K, npts))
        L.check(lib.pm_modes_dot(code, K, npts, L.ptr(m), m.stride(0), L.ptr(g), L.ptr(out), L.ptr(ws), ws.numel() if ws is not None else 0,
                                 L.stream_ptr()))
    return out


# ----------------------------------------------------------------------------- masked fits (csrc/modalfit.hip)
def _code(dt):
    return L.PM_F32 if dt == torch.float32 else L.PM_F64


def _check_real(a, what):
    if _is_complex(a):
        raise TypeError(f'{what} must be real')


def _stack(modes):
    """(K, rows, cols) contiguous float32 / float64 device tensor of a stack, a sequence of planes or an array; the shape and dtype checks
    come before anything is uploaded"""
    if isinstance(modes, (list, tuple)):
        for m in modes:
            _check_real(m, 'modes')
        shapes = {_shape(m) for m in modes}
        if len(shapes) > 1:
            raise ValueError(f'the modes differ in shape: {sorted(shapes)}')
        shape = (len(modes), *next(iter(shapes), ()))
    else:
        _check_real(modes, 'modes')
        shape = _shape(modes)
    if len(shape) != 3:
        raise ValueError(f'modes must be a (K, rows, cols) stack, not of shape {shape}')
    FP.check_count(shape[0])
    return shape


def _mask_bytes(mask):
    m = L.as_device(mask)
    return (m != 0).to(torch.uint8).contiguous()


def _new_record(K, nrhs, dev):
    return torch.empty(FP.record_doubles(K, nrhs), dtype=torch.float64, device=dev)


def _gram(m, parts, rec, data=None, mask=None, finite_from_data=False):
    K, npts = m.shape[0], m[0].numel()
    nrhs = 0 if data is None else data.shape[0]
    lib, code = L.load(), _code(m.dtype)
    ws = L.workspace(lib.pm_modes_gram_workspace(code, K, npts, nrhs))
    L.check(lib.pm_modes_gram(code, parts, K, npts, L.ptr(m), m.stride(0), nrhs, L.ptr(data), data.stride(0) if nrhs else 0, L.ptr(mask),
                              int(finite_from_data), L.ptr(rec), L.ptr(ws), ws.numel(), L.stream_ptr()))


def _small(dt, op, K, nrhs, rec, stats=None, coef=None):
    L.check(L.load().pm_modes_small(_code(dt), op, K, nrhs, L.ptr(rec), L.ptr(stats), L.ptr(coef), L.stream_ptr()))


def _transform(m, form, zero_outside, rec, mask, out):
    K, npts = m.shape[0], m[0].numel()
    L.check(L.load().pm_modes_transform(_code(m.dtype), form, int(zero_outside), K, npts, L.ptr(m), m.stride(0), L.ptr(rec), L.ptr(mask), L.ptr(out),
                                        out.stride(0), L.stream_ptr()))


def lstsq(modes, data):
    """Least-squares fit of the modes to the finite points of data (fitting.py:103-126): (K,) device tensor in the modes' dtype.

    The normal equations G c = b over the mask isfinite(data), with every product and sum of G and b in double on the matrix cores
    (pm_modes_gram), an unpivoted Cholesky factor and two substitutions on the device (pm_modes_small): four launches, no host read.
    The error grows with the square of the condition number of the masked basis, against the reference's SVD with the first power:
    K kappa^2 eps64 is its size.  For a rank-deficient basis the reference returns the minimum-norm solution; this returns the basic
    solution, with each mode that depends on the modes before it at 0.  float32 and float64 only; at most 128 modes."""
    shape = _stack(modes)
    _check_real(data, 'data')
    if FP.check_shapes(shape, _shape(data)) is not None:
        raise ValueError('lstsq takes one (rows, cols) map; use prepare_lstsq(modes, mask).fit for a stack')
    m = _modes(modes)
    d = L.as_device(data, m.dtype).reshape(1, -1)
    K = shape[0]
    rec = _new_record(K, 1, m.device)
    coef = torch.empty((1, K), dtype=m.dtype, device=m.device)
    _gram(m, L.PM_MODES_GRAM | L.PM_MODES_RHS, rec, d, None, True)
    _small(m.dtype, L.PM_MODES_FACTOR, K, 1, rec)
    _small(m.dtype, L.PM_MODES_SOLVE, K, 1, rec, coef=coef)
    return coef[0]


def normalize_modes(modes, mask, to='std'):
    """Scale one (rows, cols) mode or a (K, rows, cols) stack to unit std ('std') or unit peak-to-valley ('ptp') over the mask
    (fitting.py:129-162); a norm below 1e-9 counts as 1, the reference's loophole for piston.  The whole plane is scaled, as in the
    reference.  The norms stay on the device (pm_modes_stats, two-pass variance in double): six launches per 128 modes, no host read."""
    FP.check_to(to)
    _check_real(modes, 'modes')
    shape = _shape(modes)
    if len(shape) not in (2, 3):
        raise ValueError(f'normalize_modes takes a (rows, cols) mode or a (K, rows, cols) stack, not shape {shape}')
    FP.check_mask(shape, _shape(mask))
    m = _modes(modes)
    single = m.dim() == 2
    if single:
        m = m.unsqueeze(0)
    mk = _mask_bytes(mask)
    out = torch.empty_like(m)
    lib, code, npts = L.load(), _code(m.dtype), m[0].numel()
    op = L.PM_MODES_NORMS_STD if to == 'std' else L.PM_MODES_NORMS_PTP
    for k0 in range(0, m.shape[0], FP.FIT_MAX):
        part, K = m[k0:k0 + FP.FIT_MAX], min(FP.FIT_MAX, m.shape[0] - k0)
        st = torch.empty(K * L.PM_MODES_STAT_RECORD, dtype=torch.float64, device=m.device)
        ws = L.workspace(lib.pm_modes_stats_workspace(K, npts))
        L.check(lib.pm_modes_stats(code, K, npts, L.ptr(part), part.stride(0), L.ptr(mk), L.ptr(st), L.ptr(ws), ws.numel(), L.stream_ptr()))
        rec = _new_record(K, 0, m.device)
        _small(m.dtype, op, K, 0, rec, stats=st)
        _transform(part, L.PM_MODES_DIAGONAL, False, rec, None, out[k0:k0 + K])
    return out[0] if single else out


def orthogonalize_modes(modes, mask):
    """Orthonormalise the modes over the mask in their order, zero outside it (fitting.py:165-187).

    Cholesky QR: G = A^T A over the mask, G = L L^T, Q = A L^-T.  R = L^T has a positive diagonal, which is what the reference's
    Q * sign(diag R) produces, so the two agree in sign by construction.  One pass: Q's orthogonality error is kappa(A)^2 eps64, the
    reference's Householder QR has eps64; for the Zernike and Q bases over annular or segmented apertures (kappa below 100) both sit
    at tens of eps64, and there is no second pass.  A mode that depends on those before it comes out as an exact zero plane.
    Five launches, no host read."""
    shape = _stack(modes)
    FP.check_mask(shape, _shape(mask))
    m = _modes(modes)
    mk = _mask_bytes(mask)
    K = shape[0]
    rec = _new_record(K, 0, m.device)
    _gram(m, L.PM_MODES_GRAM, rec, None, mk, False)
    _small(m.dtype, L.PM_MODES_FACTOR, K, 0, rec)
    _small(m.dtype, L.PM_MODES_INVERT, K, 0, rec)
    out = torch.empty_like(m)
    _transform(m, L.PM_MODES_LOWER, True, rec, mk, out)
    return out


def hopkins(a, b, c, r, t, H):
    """Hopkins' aberration term W_abc: cos(a t) r^b H^c, or sin(|a| t) r^b H^c for a < 0 (fitting.py:60-100).  A few tensor operations
    on the device, not a kernel of the unit: it is evaluated once per term of a model, not per iteration."""
    r, t = L.as_device(r), L.as_device(t)
    if not isinstance(H, (int, float)):
        H = L.as_device(H)
    c1 = torch.sin(abs(a) * t) if a < 0 else torch.cos(a * t)
    return c1 * r ** b * H ** c


class ModalFit:
    """A basis factored once over a fixed aperture (prepare_lstsq): fit(data) then costs the right-hand sides and the substitutions."""

    def __init__(self, modes, mask):
        shape = _stack(modes)
        FP.check_mask(shape, _shape(mask))
        self.modes = _modes(modes)
        self.mask = _mask_bytes(mask)
        self.K = shape[0]
        self._head = FP.record_doubles(self.K, 0)
        self._rec = _new_record(self.K, 0, self.modes.device)
        self._by_frames = {}
        self._rank = None
        _gram(self.modes, L.PM_MODES_GRAM, self._rec, None, self.mask, False)
        _small(self.modes.dtype, L.PM_MODES_FACTOR, self.K, 0, self._rec)

    def _record(self, nrhs):
        """the record for nrhs frames: the factored head copied once, then its own b and coefficients"""
        rec = self._by_frames.get(nrhs)
        if rec is None:
            rec = self._by_frames[nrhs] = _new_record(self.K, nrhs, self.modes.device)
            rec[:self._head].copy_(self._rec)
        return rec

    def fit(self, data):
        """Coefficients of a (rows, cols) map, (K,), or of a (B, rows, cols) stack, (B, K), over the prepared mask, in the modes' dtype.
        Three launches per 16 frames, no host read; capturable with prysm_amd.graph.capture on one stream.  The mask is the prepared
        one, not isfinite(data): a NaN in data inside the mask makes that frame's coefficients NaN (every coefficient of the frame,
        and of no other frame)."""
        _check_real(data, 'data')
        B = FP.check_shapes(tuple(self.modes.shape), _shape(data))
        d = L.as_device(data, self.modes.dtype).reshape(1 if B is None else B, -1)
        nrhs = d.shape[0]
        coef = torch.empty((nrhs, self.K), dtype=self.modes.dtype, device=self.modes.device)
        if nrhs:
            rec = self._record(nrhs)
            _gram(self.modes, L.PM_MODES_RHS, rec, d, self.mask, False)
            _small(self.modes.dtype, L.PM_MODES_SOLVE, self.K, nrhs, rec, coef=coef)
        return coef[0] if B is None else coef

    __call__ = fit

    @property
    def rank(self):
        """the number of modes the factorisation kept (one host read, then remembered)"""
        if self._rank is None:
            self._rank = int(self._rec[L.PM_MODES_REC_RANK].item())
        return self._rank

    @property
    def count(self):
        """the number of points inside the mask (one host read)"""
        return int(self._rec[L.PM_MODES_REC_COUNT].item())


def prepare_lstsq(modes, mask):
    """Factor the normal equations of the modes over a fixed byte mask once (beyond the reference): ModalFit, whose fit(data) fits one
    map or a stack of maps that share the aperture."""
    return ModalFit(modes, mask)
