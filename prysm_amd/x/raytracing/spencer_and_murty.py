"""Spencer & Murty's general ray trace on the device (prysm/x/raytracing/spencer_and_murty.py): raytrace on pm_rt_trace.

`raytrace(surfaces, P, S, wvl)` walks a bundle through a list of Surface objects in one launch and returns the reference's
RayTraceResult: P and S of (J + 1, N, 3), OPL of (J + 1, N), row 0 the launch, and the complex status -- real part the 1-based surface
of a ray's first failure (or J), imaginary part the STATUS_* code.  `history=False` (not in the reference) keeps only the last row and
the summed path.  `prepare(surfaces, wvl)` packs the surface table once and keeps it on the device; a trace of a Prescription reads
nothing on the host and copies nothing to the device, so it can be captured with prysm_amd.graph.capture.

keep_intermediates and the differential and adjoint traces are not implemented.
"""
import numpy as np
import torch

from ... import _lib as L
from ... import _ops
from ...conf import config
from .. import raytrace_plan as plan
from ..raytrace_plan import STYPE_EVAL, STYPE_IMG, STYPE_OBJ, STYPE_REFLECT, STYPE_REFRACT, resolve_tol_sag  # noqa: F401

SURFACE_INTERSECTION_DEFAULT_MAXITER = plan.NEWTON_ITERS
DEFAULT_TOL_SAG = plan.DEFAULT_TOL_SAG

STATUS_OK = 0
STATUS_NEWTON = 1       # Newton-Raphson did not converge
STATUS_CLIP = 2         # clipped by the surface's aperture
STATUS_MISS = -1        # no closed-form intersection
STATUS_TIR = -2         # total internal reflection
STATUS_EVANESCENT = -3  # of the reference's gratings; never produced here

_STATUS_LABELS = {STATUS_OK: 'OK', STATUS_NEWTON: 'NEWTON', STATUS_CLIP: 'CLIPPED', STATUS_MISS: 'MISS', STATUS_TIR: 'TIR',
                  STATUS_EVANESCENT: 'EVANESCENT'}

__all__ = ['raytrace', 'prepare', 'Prescription', 'RayTraceResult', 'RayStatus', 'decode_status', 'valid_mask', 'resolve_tol_sag',
           'STATUS_OK', 'STATUS_NEWTON', 'STATUS_CLIP', 'STATUS_MISS', 'STATUS_TIR', 'STATUS_EVANESCENT']


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class RayStatus:
    """the status as two integer arrays: surface and code"""
    __slots__ = ('surface', 'code')

    def __init__(self, surface, code):
        self.surface, self.code = surface, code

    @classmethod
    def from_encoded(cls, status):
        if isinstance(status, torch.Tensor):
            return cls(status.real.to(torch.int64), status.imag.to(torch.int64))
        status = np.asarray(status)
        return cls(status.real.astype(int), status.imag.astype(int))

    @property
    def encoded(self):
        if isinstance(self.surface, torch.Tensor):
            return torch.complex(self.surface.to(torch.float64), self.code.to(torch.float64))
        return self.surface + 1j * self.code

    @property
    def text(self):
        return decode_status(self.encoded)


class RayTraceResult:
    """what raytrace returns: P, S, OPL, status (complex128) and status_record (the RayStatus of the kernel's two int32 arrays)"""
    __slots__ = ('P', 'S', 'OPL', 'status', 'status_record', 'intermediates')

    def __init__(self, P, S, OPL, status, status_record=None):
        self.P, self.S, self.OPL, self.status = P, S, OPL, status
        self.status_record = RayStatus.from_encoded(status) if status_record is None else status_record
        self.intermediates = None

    def __repr__(self):
        return f'RayTraceResult(N_rays={self.status.shape[0]}, N_surfaces={self.P.shape[0] - 1})'


def _decode_status_scalar(status):
    surface, code = int(status.real), int(status.imag)
    label = _STATUS_LABELS.get(code, f'UNKNOWN({code})')
    return label if code == STATUS_OK else f'{label} at surface {surface}'


def decode_status(status):
    """the status as text: a string for a scalar, an object array of strings for an array (spencer_and_murty.py:125-144)"""
    arr = _host(status)
    if arr.ndim == 0:
        return _decode_status_scalar(arr.item())
    return np.asarray([_decode_status_scalar(v) for v in arr.ravel()], dtype=object).reshape(arr.shape)


def valid_mask(status, P=None):
    """the rays whose code is OK and, with P, whose position is finite (spencer_and_murty.py:153-177); tensors give a tensor"""
    if isinstance(status, torch.Tensor) or isinstance(P, torch.Tensor):
        finite = None if P is None else torch.isfinite(torch.as_tensor(P)).all(dim=-1)
        if status is None:
            return finite
        valid = torch.as_tensor(status).imag == STATUS_OK
        return valid if finite is None else valid & finite.to(valid.device)
    finite = None if P is None else np.isfinite(np.asarray(P)).all(axis=-1)
    if status is None:
        return finite
    valid = np.asarray(status).imag == STATUS_OK
    return valid if finite is None else valid & finite


class Prescription:
    """A list of surfaces at one wavelength, packed for the kernel: `table`, the (J, PM_RT_RECORD) float64 tensor on the device, built
    once, and `n_launch`, the index the rays start in.  raytrace accepts it in place of the list.  `host_table` is the numpy array the
    device tensor was made from."""
    __slots__ = ('table', 'host_table', 'n_launch', 'wvl', 'J')

    def __init__(self, surfaces, wvl):
        self.host_table = plan.pack_table(surfaces, wvl)
        self.n_launch = plan.launch_index(surfaces, wvl)
        self.wvl, self.J = wvl, len(surfaces)
        self.table = torch.from_numpy(self.host_table).to(L.device())

    def __len__(self):
        return self.J


def prepare(surfaces, wvl, dtype=None):
    """Pack `surfaces` at wavelength `wvl` into a Prescription.  `dtype` names the precision of the rays it is meant for, float32 or
    float64 (None: config.precision); anything else is a TypeError.  The table itself is always double -- the kernel converts to the
    rays' type as it reads -- so one Prescription serves rays of either precision."""
    _check_sequence(surfaces)
    if dtype is not None:
        try:
            ok = L.torch_dtype(dtype) in (torch.float32, torch.float64)
        except (KeyError, TypeError):
            ok = False
        if not ok:
            raise TypeError(f'prepare: dtype must be float32 or float64, got {dtype!r}')
    return Prescription(surfaces, wvl)


def _check_sequence(surfaces):
    if hasattr(surfaces, 'to_surfaces'):
        raise TypeError('raytrace requires a compiled surface sequence; call system.trace(...) for an OpticalSystem or pass '
                        'lens.to_surfaces() explicitly')
    try:
        len(surfaces)
    except TypeError as e:
        raise TypeError('raytrace requires a sized compiled surface sequence') from e


def _rays(a):
    """a device tensor of float32 / float64; integers (and anything else that is not floating) are cast to config.precision"""
    if isinstance(a, torch.Tensor):
        t = a if a.is_floating_point() and a.dtype in (torch.float32, torch.float64) else a.to(L.torch_dtype(config.compute_precision))
        return t if t.is_cuda else L.as_device(t)
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.floating) or a.dtype.itemsize < 4:
        a = a.astype(config.compute_precision)
    return L.as_device(a)


def raytrace(surfaces, P, S, wvl, tol_sag=None, keep_intermediates=False, history=True):
    """Trace the rays P, S ((N, 3), or (3,) for one ray) through `surfaces` -- a list of Surface, or a Prescription -- at wavelength
    wvl (microns).  tol_sag: the Newton convergence tolerance on |Z - sag|, None for resolve_tol_sag of the rays' type.  One launch."""
    if keep_intermediates:
        raise NotImplementedError('raytrace(keep_intermediates=True) is not implemented: the kernel keeps nothing per surface but the '
                                  'history')
    if isinstance(surfaces, Prescription):
        rx = surfaces
    else:
        _check_sequence(surfaces)
        L.device()      # no device: refuse before any host work
        rx = Prescription(surfaces, wvl)
    P, S = _rays(P), _rays(S)
    if S.dtype != P.dtype:
        S = S.to(P.dtype)
    squeeze = P.dim() == 1
    if squeeze:
        P, S = P[None, :], S[None, :]
    tol = resolve_tol_sag(tol_sag, np.float32 if P.dtype == torch.float32 else np.float64)
    Po, So, Oo, surface, code = _ops.rt_trace(rx.table, rx.n_launch, tol, P, S, history)
    status = torch.complex(surface.to(torch.float64), code.to(torch.float64))
    if squeeze:      # the status stays of length 1
        Po, So, Oo = Po.squeeze(-2), So.squeeze(-2), Oo.squeeze(-1)
    return RayTraceResult(Po, So, Oo, status, RayStatus(surface, code))
