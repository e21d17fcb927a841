"""Step-index optical fibres on the device (prysm/x/fibers.py): LP modes, mode sums and coupling without a stored basis.

The names and conventions are the reference's: find_all_modes returns {l: b descending} with the keys 0, 1, -1, 2, -2, ...;
compute_LP_modes walks each family's list reversed and takes r <= a as the core; smf_mode_field takes r (1/a) < 1 and the J1(U), K1(W)
normalisers.  The roots are solved on the host (fibers_plan.py, numpy, a few hundred scalar roots); fields stay torch tensors on the
device.

prepare(V, mode_dict, a, r, t) returns a ModeSet: the record table on the device and sum_p mode_k^2 cached.  Its modes() writes every
mode in one launch (pm_fiber_modes), sum(coefs) is the field of a coefficient vector (pm_fiber_sum), project(E) the sums
sum_p E[p] mode_k[p] (pm_fiber_project), and coupling(E) multimode_coupling without the stored modes: two launches for every mode,
nothing read on the host, results left on the device -- all of it capturable with prysm_amd.graph.capture.  mode_overlap_integral is
one pass over both fields (pm_overlap).
"""
import numpy as np
import torch

from .. import _lib as L
from ..polynomials._modal import _code, _projector
from . import fibers_plan as plan

__all__ = ['critical_angle', 'numerical_aperture', 'V', 'find_all_modes', 'compute_LP_modes', 'smf_mode_field', 'marcuse_mfr_from_V',
           'petermann_mfr_from_V', 'mode_overlap_integral', 'multimode_coupling', 'overlap', 'prepare', 'ModeSet']


def critical_angle(n_core, n_clad, deg=True):
    """Angle at which TIR happens in a step index fiber (fibers.py:13-35)."""
    ang = np.arcsin(n_clad / n_core)
    return np.degrees(ang) if deg else ang


def numerical_aperture(n_core, n_clad):
    """NA of a step-index fiber (fibers.py:38-54)."""
    return np.sqrt(n_core * n_core - n_clad * n_clad)


def V(radius, NA, wavelength):
    """V-number of a fiber: k r NA (fibers.py:57-83)."""
    return 2 * np.pi / wavelength * radius * NA


def marcuse_mfr_from_V(V):
    """Marcuse's estimate of w/a, mode field radius over core radius (fibers.py:462-479)."""
    return 0.65 + 1.619 * V ** -1.5 + 2.879 * V ** -6


def petermann_mfr_from_V(V):
    """Petermann's estimate of w/a (fibers.py:482-502)."""
    return marcuse_mfr_from_V(V) - 0.016 - 1.567 * V ** -7


def find_all_modes(V, count_only=False):
    """The modes of a step-index fiber: {l: b for each m, descending}, or the counts from cutoff theory (fibers.py:289-340).  Host
    arithmetic in float64 (fibers_plan.find_all_modes)."""
    return plan.find_all_modes(V, count_only=count_only)


# --------------------------------------------------------------------------- tensors
def _real_dtype(*arrays):
    """float32 when every array is float32 / complex64, else float64"""
    def single(a):
        dt = a.dtype if isinstance(a, torch.Tensor) else L.torch_dtype(np.asarray(a).dtype)
        return dt in (torch.float32, torch.complex64)
    return torch.float32 if all(single(a) for a in arrays) else torch.float64


def _np_dtype(dt):
    return np.float32 if dt == torch.float32 else np.float64


def _coords(r, t):
    sr, st = tuple(np.shape(r)), tuple(np.shape(t))
    if sr != st:
        raise ValueError(f'coordinate arrays differ in shape: {sr} and {st}')
    for c in (r, t):
        if (c.is_complex() if isinstance(c, torch.Tensor) else np.iscomplexobj(c)):
            raise TypeError('fibre coordinates must be real')
    dt = _real_dtype(r, t)
    return L.as_device(r, dt), L.as_device(t, dt), dt, sr


def _planes(E, dt, shape, what):
    """(planes, fields, complex?, stacked?) of a field or a (B, ...) stack of fields: contiguous (B or 2B, npts) real planes, for a
    complex field Re then Im of each member, and the fields themselves as a contiguous (B, npts) array in the points' precision"""
    e = L.as_device(E)
    se = tuple(e.shape)
    if se != shape and se[1:] != shape:
        raise ValueError(f'{what} of shape {se} does not match coordinates of shape {shape} (or a (B, ...) stack of them)')
    stacked = se != shape
    B = se[0] if stacked else 1
    if e.is_complex():
        e = e.to(torch.complex64 if dt == torch.float32 else torch.complex128).reshape(B, -1)
        e = e.contiguous()
        return torch.view_as_real(e).permute(0, 2, 1).contiguous().reshape(2 * B, -1), e, True, stacked
    e = e.to(dt).reshape(B, -1).contiguous()
    return e, e, False, stacked


class ModeSet:
    """The LP modes of one fibre on one set of points, never stored: what prepare returns."""

    def __init__(self, V, mode_dict, a, r, t, table=None, nmodes=None):
        self.V, self.a = float(V), float(a)
        if not self.a > 0:
            raise ValueError('the core radius a must be positive')
        self.mode_dict = mode_dict
        self.r, self.t, self.dtype, self.shape = _coords(r, t)
        if table is None:
            table, nmodes = plan.mode_table(self.V, mode_dict, _np_dtype(self.dtype))
        self.nmodes, self.nrec = int(nmodes), len(table)
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(L.device())
        self.npts = self.r.numel()
        self._norm = None

    def _head(self):
        return (self.npts, L.ptr(self.r), L.ptr(self.t), self.a, L.ptr(self.table), self.nrec, self.nmodes)

    def modes(self):
        """every mode, (nmodes, *shape), in the order compute_LP_modes emits them; one launch"""
        out = torch.empty((self.nmodes, *self.shape), dtype=self.dtype, device=self.r.device)
        if self.nmodes and self.npts:
            L.check(L.load().pm_fiber_modes(_code(self.dtype), *self._head(), L.ptr(out), L.stream_ptr()))
        return out

    def as_dict(self, flat):
        """a flat sequence in mode order -> {l: list} with the structure of compute_LP_modes"""
        return plan.as_dict(self.mode_dict, flat)

    def sum(self, coefs, out=None, accumulate=False):
        """sum_k coefs[k] mode_k: (K,) coefficients give a field of the points' shape, (B, K) a (B, ...) stack; complex coefficients a
        complex field.  The coefficients are read on the device when the kernel runs.  out / accumulate: add into a real field."""
        c = L.as_device(coefs)
        sc = tuple(c.shape)
        if len(sc) not in (1, 2) or sc[-1] != self.nmodes:
            raise ValueError(f'coefs of shape {sc} do not match the {self.nmodes} modes (want ({self.nmodes},) or (B, {self.nmodes}))')
        B = 1 if len(sc) == 1 else sc[0]
        cplx = c.is_complex()
        if cplx:
            c = c.to(torch.complex64 if self.dtype == torch.float32 else torch.complex128).reshape(B, -1)
            c = torch.view_as_real(c).permute(0, 2, 1).contiguous().reshape(2 * B, -1)
        else:
            c = c.to(self.dtype).reshape(B, -1).contiguous()
        nb = c.shape[0]
        if out is not None:
            if cplx or out.dtype != self.dtype or tuple(out.shape) != ((B, *self.shape) if len(sc) == 2 else self.shape) \
                    or not out.is_contiguous():
                raise ValueError('out must be a contiguous real field of the result\'s shape and the points\' precision')
            planes = out
        else:
            if accumulate:
                raise ValueError('accumulate needs the field to add into (out)')
            planes = torch.empty((nb, *self.shape), dtype=self.dtype, device=self.r.device)
        if self.npts and nb:
            L.check(L.load().pm_fiber_sum(_code(self.dtype), *self._head(), nb, L.ptr(c), int(bool(accumulate)), L.ptr(planes),
                                          L.stream_ptr()))
        if out is not None:
            return out
        if cplx:
            planes = torch.complex(planes[0::2], planes[1::2])
        return planes[0] if len(sc) == 1 else planes

    def _project(self, g, nb):
        out = torch.empty((nb, self.nmodes), dtype=self.dtype, device=self.r.device)
        if self.nmodes and nb:
            _projector('fiber', self.dtype, self.npts, self.nmodes, nb)(*self._head(), nb, L.ptr(g), L.ptr(out))
        return out

    def project(self, E):
        """sum_p E[p] mode_k[p] for a field of the points' shape, (K,), or a (B, ...) stack of fields, (B, K); complex for a complex
        field.  Deterministic: two launches, no atomics."""
        g, _, cplx, stacked = _planes(E, self.dtype, self.shape, 'E')
        out = self._project(g, g.shape[0])
        if cplx:
            out = torch.complex(out[0::2], out[1::2])
        return out if stacked else out[0]

    def norms(self):
        """sum_p mode_k[p]^2, (K,), computed once"""
        if self._norm is None:
            self._norm = self._project(None, 1)[0]
        return self._norm

    def coupling(self, E, as_dict=False):
        """multimode_coupling without the stored modes: eta_k = |sum E conj(mode_k)|^2 / (sum mode_k^2 sum |E|^2), a (K,) tensor on the
        device, (B, K) for a (B, ...) stack of fields (sum |E|^2 is pm_overlap's, one call per field); as_dict=True gives the reference's {l: list} of 0-d tensors (single field)."""
        g, e, cplx, stacked = _planes(E, self.dtype, self.shape, 'E')
        p = self._project(g, g.shape[0])
        num = p[0::2] ** 2 + p[1::2] ** 2 if cplx else p * p
        power = torch.stack([overlap(eb, eb)[2] for eb in e])          # sum |E|^2 of each field (pm_overlap)
        eta = num / (self.norms()[None, :] * power[:, None])
        if as_dict:
            if stacked:
                raise ValueError('as_dict takes a single field')
            return self.as_dict(eta[0])
        return eta if stacked else eta[0]


def prepare(V, mode_dict, a, r, t):
    """The modes of mode_dict (as find_all_modes returns it, or a part of it) at the polar points (r, t) of a fibre of V-number V and
    core radius a, prepared once: the table on the device, in the points' precision (float32 for float32 points)."""
    return ModeSet(V, mode_dict, a, r, t)


def compute_LP_modes(V, mode_dict, a, r, t):
    """LP modes of a step-index fiber on the device (fibers.py:343-421): {l: [mode per b, in REVERSED order of mode_dict[l]]}, each a
    view of one (nmodes, ...) stack written in one launch."""
    ms = prepare(V, mode_dict, a, r, t)
    return ms.as_dict(ms.modes())


def smf_mode_field(V, a, b, r):
    """Mode field of a single mode fiber (fibers.py:424-459): J0(U rn) / J1(U) for rn = r (1/a) < 1, K0(W rn) / K1(W) outside."""
    dt = _real_dtype(r)
    table, n = plan.smf_table(V, b, _np_dtype(dt))
    r = L.as_device(r, dt)
    return ModeSet(V, {0: [b]}, a, r, r, table=table, nmodes=n).modes()[0]


# --------------------------------------------------------------------------- overlap
def _field(E, dt):
    e = L.as_device(E)
    if e.is_complex():
        return e.to(torch.complex64 if dt == torch.float32 else torch.complex128), 1
    return e.to(dt), 0


def overlap(E1, E2):
    """(5,) on the device: Re S, Im S, I1, I2, eta with S = sum E1 conj(E2), I1 = sum |E1|^2, I2 = sum |E2|^2, eta = |S|^2 / (I1 I2);
    one pass over both fields and a fixed-order second launch (pm_overlap).  Real or complex fields of one shape."""
    s1, s2 = tuple(np.shape(E1)), tuple(np.shape(E2))
    if s1 != s2:
        raise ValueError(f'fields differ in shape: {s1} and {s2}')
    dt = _real_dtype(E1, E2)
    e1, c1 = _field(E1, dt)
    e2, c2 = _field(E2, dt)
    out = torch.empty(5, dtype=dt, device=e1.device)
    lib = L.load()
    ws = L.workspace(lib.pm_overlap_workspace(_code(dt), e1.numel()))
    L.check(lib.pm_overlap(_code(dt), e1.numel(), L.ptr(e1), c1, L.ptr(e2), c2, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return out


def mode_overlap_integral(E1, E2, E2conj=None, I1sum=None, I2sum=None):
    """eta = |sum E1 conj(E2)|^2 / (sum I1 sum I2) (fibers.py:505-548), a 0-d tensor on the device.  E2conj, when given, takes the place
    of E2.conj(); I1sum / I2sum take the place of the sums computed here."""
    if E2conj is not None:
        E2 = torch.conj(L.as_device(E2conj)).resolve_conj() if L.as_device(E2conj).is_complex() else E2conj
    res = overlap(E1, E2)
    if I1sum is None and I2sum is None:
        return res[4]
    i1 = res[2] if I1sum is None else I1sum
    i2 = res[3] if I2sum is None else I2sum
    return (res[0] * res[0] + res[1] * res[1]) / (i1 * i2)


def multimode_coupling(E_in, mode_fields):
    """Per-LP-mode coupling efficiency of an incident field (fibers.py:551-588): {l: [eta per mode]} of 0-d tensors on the device.
    mode_fields is a ModeSet (nothing stored: ModeSet.coupling) or the dictionary compute_LP_modes returns, whose stored modes are
    read once by pm_modes_dot."""
    if isinstance(mode_fields, ModeSet):
        return mode_fields.coupling(E_in, as_dict=True)
    from ..polynomials.fitting import sum_of_2d_modes_adjoint
    flat = [m for modes in mode_fields.values() for m in modes]
    if not flat:
        return {l: [] for l in mode_fields}
    dt = _real_dtype(E_in, *flat)
    stack = torch.stack([L.as_device(m, dt) for m in flat])
    e = L.as_device(E_in)
    parts = (e.real, e.imag) if e.is_complex() else (e,)
    parts = [p.to(dt).contiguous() for p in parts]
    num = sum(sum_of_2d_modes_adjoint(stack, p) ** 2 for p in parts)
    power = sum((p * p).sum() for p in parts)
    eta = num / ((stack * stack).reshape(len(flat), -1).sum(dim=1) * power)
    return plan.as_dict(mode_fields, eta)
