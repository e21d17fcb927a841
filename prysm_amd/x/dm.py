"""Deformable mirror (prysm/x/dm.py) -- SURVEY 8(f) rank 4: the producer of the pupil phase in closed-loop WFSC models.

DM.render is four steps on the device: the actuator lattice scattered into the poke grid (pm_lattice), the convolution with the
influence function as ONE fused fft2 x H ifft2 chain (pm_fft2_mul_ifft2, the wfe scale and 1/MN folded into it), the projection
into the beam normal (pm_warp: map_coordinates(order=3, mode='constant') of the rotation's homography, with the Nout window
fused), and the pad / crop to Nout.  render_adjoint runs the same pieces backwards and gathers the lattice samples out.  A
(B, rows, cols) stack goes through each piece as one launch sequence (render_stack, render_adjoint of a 3-D protograd).

Only the construction touches the host (lattice geometry, homographies, Ifn by one pm_fft2, the shift ramps).
"""
import copy
import math

import numpy as np
import torch

from .. import _lib as L
from .. import _ops
from ..fttools import fourier_resample, pad2d, crop_center

__all__ = ['DM', 'prepare_actuator_lattice', 'make_rotation_matrix', 'projection_homographies', 'apply_homography']


def _pair(v):
    return (v, v) if isinstance(v, (int, np.integer)) else tuple(v)


def prepare_actuator_lattice(shape, Nact, sep):
    """Lattice geometry of prepare_actuator_lattice (prysm/x/dm.py:18-61): Nact and sep in (X, Y) order; returns
    (y0, x0, sy, sx, nact_y, nact_x), lattice point (i, j) at grid sample (y0 + i sy, x0 + j sx)."""
    cy, cx = [s // 2 for s in shape]
    nact_x, nact_y = Nact
    sep_x, sep_y = sep
    off_x = 0 if nact_x % 2 else sep_x // 2
    off_y = 0 if nact_y % 2 else sep_y // 2
    x0 = cx + -nact_x // 2 * sep_x + off_x          # floor division: odd counts put the extra actuator on the negative side
    y0 = cy + -nact_y // 2 * sep_y + off_y
    return int(y0), int(x0), int(sep_y), int(sep_x), int(nact_y), int(nact_x)


def make_rotation_matrix(zyx, radians=False):
    """3 x 3 rotation Rx @ Ry @ Rz for (Z, Y, X) angles (prysm/coordinates.py:381-429); missing trailing angles are 0."""
    ang = np.zeros(3)
    ang[:len(zyx)] = zyx
    if not radians:
        ang = np.radians(ang)
    gamma, beta, alpha = ang
    ca, cb, cg = np.cos(alpha), np.cos(beta), np.cos(gamma)
    sa, sb, sg = np.sin(alpha), np.sin(beta), np.sin(gamma)
    Rx = np.asarray([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.asarray([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.asarray([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def projection_homographies(shape, rot):
    """(Mfwd, Mifwd): the 3 x 3 homographies of prepare_fwd_reverse_projection_coordinates (prysm/x/dm.py:64-82) -- the rotation
    about the array centre ((n - 1) / 2) with z dropped, and its inverse.  render pulls through Mifwd, render_adjoint through Mfwd."""
    oy, ox = [(s - 1) / 2 for s in shape]
    R = np.zeros((4, 4))
    R[:3, :3] = make_rotation_matrix(rot)
    R[3, 3] = 1
    Tin, Tout = np.eye(4), np.eye(4)
    Tin[0, 3], Tin[1, 3] = -ox, -oy
    Tout[0, 3], Tout[1, 3] = ox, oy
    keep = [0, 1, 3]
    Mfwd = np.ascontiguousarray((Tout @ (R @ Tin))[keep][:, keep])
    return Mfwd, np.linalg.inv(Mfwd)


def apply_homography(M, x, y):
    """(x', y') = (M (x, y, 1))[:2] / w, numpy, in the reference's order of operations (prysm/coordinates.py:545-570)."""
    pts = np.empty((3, x.size))
    pts[0], pts[1], pts[2] = x.ravel(), y.ravel(), 1
    xp, yp, w = M @ pts
    return np.reshape(xp / w, x.shape), np.reshape(yp / w, x.shape)


def _window(inner, Nout):
    """The reference's pad / crop decision (dm.py:267-271, axis 0 only -- kept verbatim) as an output window of `inner`:
    (out_shape, (off_y, off_x)) with output pixel (r, c) = inner pixel (r + off_y, c + off_x), or None for no change."""
    if inner[0] < Nout[0]:          # pad2d(out_shape=Nout): the data lands at ceil((Nout - n) / 2)
        return tuple(Nout), tuple(-math.ceil((o - i) / 2) for i, o in zip(inner, Nout))
    if inner[0] > Nout[1]:          # crop_center(out_shape=Nout): the window starts at ceil((n - Nout) / 2)
        if any(o > i for i, o in zip(inner, Nout)):
            raise ValueError(f'DM: Nout {tuple(Nout)} crops axis 0 of the {tuple(inner)} surface but is larger along axis 1')
        return tuple(Nout), tuple(math.ceil((i - o) / 2) for i, o in zip(inner, Nout))
    return None


class DM:
    """A DM whose actuators fill a rectangular region on a perfect grid, and have the same influence function
    (prysm/x/dm.py:85-331), rendered on the device.

    Arguments and attributes are the reference's: `ifn` (2-D real; float32 runs the complex64 chain, float64 complex128), `Nout`,
    `Nact` / `sep` / `shift` in (X, Y) order, `rot` (Z, Y, X) degrees, `upsample`, `project_centering` (accepted and, as in the
    reference, unused).  `actuators` is a (Nact_y, Nact_x) device tensor that may be written in place (``dm.actuators[25, 25] = 1``).

    Reference behaviour kept as it is:
      - The surface sits HALF AN ARRAY away from the lattice.  Ifn = fft2(ifn) has no ifftshift (dm.py:155) while the shifts of
        apply_transfer_functions cancel (convolution.py:86, 113), so a single poke at lattice sample p renders as np.roll(ifn, p):
        the influence function's centre lands on p + N // 2 (mod N), and a full command map wraps into the corners.
      - The pad / crop decision looks at axis 0 only (dm.py:267-271).
      - render_adjoint derives its resample factor as ifn.shape[0] / protograd.shape[0] and needs a prior render
        (Nintermediate).  It is the exact adjoint of render only without rotation and upsample, as in the reference.

    Stacks: render_stack((B, Nact_y, Nact_x)) -> (B, *Nout) and render_adjoint of a (B, rows, cols) protograd run the lattice, the
    chain and the warp once for the whole stack; with upsample != 1 the Fourier resample (2-D only) loops over the fields, and
    a pad without rotation (pm_embed, 2-D) does as well.
    """

    def __init__(self, ifn, Nout, Nact=50, sep=10, shift=(0, 0), rot=(0, 0, 0), upsample=1, project_centering='fft'):
        Nout, Nact, sep = _pair(Nout), _pair(Nact), _pair(sep)
        ifn = L.as_device(ifn)
        if ifn.dim() != 2 or ifn.dtype not in (torch.float32, torch.float64):
            raise ValueError('DM: ifn must be a 2-D float32 or float64 array')
        s = tuple(ifn.shape)
        self.ifn = ifn
        self.Ifn = _ops.fft2(ifn, direction=-1, scale=1.0)
        self.Nout = Nout
        self.Nact = Nact
        self.sep = sep
        self.shift = shift
        self.rot = rot
        self.upsample = upsample
        self.project_centering = project_centering
        self.obliquity = float(make_rotation_matrix(rot)[2, 2])

        self.lattice = prepare_actuator_lattice(s, Nact, sep)
        y0, x0, sy, sx, ny, nx = self.lattice
        if y0 < 0 or x0 < 0 or y0 + (ny - 1) * sy >= s[0] or x0 + (nx - 1) * sx >= s[1]:
            raise ValueError(f'DM: {nx} x {ny} actuators at separation {sep} do not fit inside the {s[1]} x {s[0]} influence function array')
        self.actuators = torch.zeros((ny, nx), dtype=ifn.dtype, device=ifn.device)

        self.needs_rot = not np.allclose(rot, [0, 0, 0])
        if self.needs_rot:
            self.Mfwd, self.Mifwd = projection_homographies(s, rot)
            x, y = np.meshgrid(np.arange(s[1], dtype=np.float64), np.arange(s[0], dtype=np.float64))
            self.projx, self.projy = [L.as_device(a) for a in apply_homography(self.Mifwd, x, y)]
            self.invprojx, self.invprojy = [L.as_device(a) for a in apply_homography(self.Mfwd, x, y)]
        else:
            self.Mfwd = self.Mifwd = None
            self.projx = self.projy = self.invprojx = self.invprojy = None

        if shift[0] != 0 or shift[1] != 0:
            # 2 pi / px phase ramps (forward_ft_unit(1, n, shift=False) = fftfreq(n)), fp64 on the host, applied once here
            Y, X = [np.fft.fftfreq(n) for n in s]
            Xramp = np.exp(X * (-2j * np.pi * shift[0]))
            Yramp = np.exp(Y * (-2j * np.pi * shift[1]))
            self.Xramp = L.as_device(np.broadcast_to(Xramp, s))
            self.Yramp = L.as_device(np.broadcast_to(Yramp[:, None], s))
            tf = (self.Ifn.to(torch.complex128) * self.Xramp * self.Yramp).to(self.Ifn.dtype)
        else:
            tf = self.Ifn
        self.tf = [tf.contiguous()]

    # ------------------------------------------------------------------ state
    def copy(self):
        """Make a (deep) copy of this DM."""
        return copy.deepcopy(self)

    def update(self, actuators):
        """Copy new commands into `actuators` (dm.py:200-207)."""
        self.actuators[:] = L.as_device(actuators).to(self.actuators.dtype)

    # ------------------------------------------------------------------ pieces
    def _scatter(self, acts, scale=1.0):
        """(B, nact_y, nact_x) commands -> (B, rows, cols) poke grid, one launch."""
        y0, x0, sy, sx, ny, nx = self.lattice
        rows, cols = self.ifn.shape
        if tuple(acts.shape[-2:]) != (ny, nx):
            raise ValueError(f'DM: actuator commands must have shape (..., {ny}, {nx}), got {tuple(acts.shape)}')
        if acts.dtype != self.ifn.dtype or acts.device != self.ifn.device or acts.stride(-1) != 1:
            acts = L.as_device(acts, self.ifn.dtype)
        B = acts.shape[0]
        poke = torch.empty((B, rows, cols), dtype=self.ifn.dtype, device=self.ifn.device)
        L.check(L.load().pm_lattice(L.PM_F32 if acts.dtype == torch.float32 else L.PM_F64, L.PM_LATTICE_SCATTER, B, rows, cols, ny, nx,
                                    y0, x0, sy, sx, float(scale), L.ptr(acts), acts.stride(-2), acts.stride(0) if B > 1 else ny * nx,
                                    L.ptr(poke), cols, rows * cols, L.stream_ptr()))
        return poke

    def _gather(self, field, scale=1.0):
        """real part of a (B, rows, cols) real or complex field at the lattice points -> (B, nact_y, nact_x), one launch."""
        y0, x0, sy, sx, ny, nx = self.lattice
        rows, cols = field.shape[-2:]
        code = {torch.float32: L.PM_F32, torch.float64: L.PM_F64, torch.complex64: L.PM_C64, torch.complex128: L.PM_C128}[field.dtype]
        B = field.shape[0]
        out = torch.empty((B, ny, nx), dtype=L._REAL_OF.get(field.dtype, field.dtype), device=field.device)
        L.check(L.load().pm_lattice(code, L.PM_LATTICE_GATHER, B, rows, cols, ny, nx, y0, x0, sy, sx, float(scale), L.ptr(field),
                                    field.stride(-2), field.stride(0) if B > 1 else rows * cols, L.ptr(out), nx, ny * nx,
                                    L.stream_ptr()))
        return out

    def _warp(self, field, M, scale, window=None):
        """scale * map_coordinates(real part of field (B, rows, cols), M (c, r, 1)), order 3, mode 'constant'), through `window`."""
        lib = L.load()
        rows, cols = field.shape[-2:]
        B = field.shape[0]
        (orows, ocols), (oy, ox) = window if window is not None else ((rows, cols), (0, 0))
        code = {torch.float32: L.PM_F32, torch.float64: L.PM_F64, torch.complex64: L.PM_C64, torch.complex128: L.PM_C128}[field.dtype]
        out = torch.empty((B, orows, ocols), dtype=L._REAL_OF.get(field.dtype, field.dtype), device=field.device)
        nbytes = lib.pm_warp_workspace(code, B, rows, cols)
        ws = L.workspace(nbytes)
        H = (L.c_f64 * 9)(*[float(v) for v in np.asarray(M, dtype=np.float64).ravel()])
        L.check(lib.pm_warp(code, 3, B, rows, cols, L.ptr(field), field.stride(-2), field.stride(0) if B > 1 else rows * field.stride(-2),
                            H, float(scale), orows, ocols, oy, ox, L.ptr(out), ocols, orows * ocols, L.ptr(ws), nbytes, L.stream_ptr()))
        return out

    def _chain(self, x, scale, **kw):
        """real part of ifft2(fft2(x) * tf) * scale (pm_fft2_mul_ifft2).  The chain reads the multiplier in x's precision, so x must be
        in the influence function's: anything else is refused here rather than read past the end of tf."""
        if x.dtype != self.ifn.dtype:
            raise TypeError(f'DM: the convolution input is {x.dtype}, the influence function {self.ifn.dtype}')
        return _ops.fft2_mul_ifft2(x, scale=scale, mul=self.tf[0], **kw)

    @staticmethod
    def _pad_fields(x, window):
        """pm_embed of each field of a (B, m, n) stack into the window (zero fill); complex or real, 2-D kernel per field."""
        (orows, ocols), (oy, ox) = window
        out = torch.empty((x.shape[0], orows, ocols), dtype=x.dtype, device=x.device)
        lib = L.load()
        fill = torch.zeros(1, dtype=x.dtype)
        for b in range(x.shape[0]):
            f = x[b]
            L.check(lib.pm_embed(f.element_size(), f.shape[0], f.shape[1], L.ptr(f), f.stride(0), orows, ocols, -oy, -ox,
                                 L.ptr(fill), L.ptr(out[b]), ocols, L.stream_ptr()))
        return out

    # ------------------------------------------------------------------ forward
    def _render(self, acts, wfe):
        rows, cols = self.ifn.shape
        B = acts.shape[0]
        scale = 2 * self.obliquity if wfe else 1.0
        poke = self._scatter(acts)
        x = poke[0] if B == 1 else poke
        if self.upsample == 1:
            self.Nintermediate = (rows, cols)
            win = _window((rows, cols), self.Nout)
            if self.needs_rot:
                F = self._chain(x, 1.0 / (rows * cols))
                return self._warp(F.reshape((B, rows, cols)), self.Mifwd, scale, win)
            sc = scale / (rows * cols)
            if win is None:
                return self._chain(x, sc, real_out=True).reshape((B, rows, cols))
            (orows, ocols), off = win
            if off[0] >= 0:         # crop: the chain's store window
                F = self._chain(x, sc, out_shape=(orows, ocols), out_off=off)
                return F.reshape((B, orows, ocols)).real
            F = self._chain(x, sc).reshape((B, rows, cols))
            return self._pad_fields(F, win).real
        # upsample != 1: chain (+ warp), then the Fourier resample and the window field by field
        if self.needs_rot:
            F = self._chain(x, 1.0 / (rows * cols))
            sfe = self._warp(F.reshape((B, rows, cols)), self.Mifwd, scale)
        else:
            sfe = self._chain(x, scale / (rows * cols), real_out=True).reshape((B, rows, cols))
        outs = []
        for b in range(B):
            w = fourier_resample(sfe[b], self.upsample).to(self.ifn.dtype)     # it resamples in config.compute_precision
            self.Nintermediate = tuple(w.shape)
            win = _window(tuple(w.shape), self.Nout)
            if win is not None:
                w = pad2d(w, out_shape=self.Nout) if win[1][0] < 0 else crop_center(w, self.Nout)
            outs.append(w)
        return outs[0][None] if B == 1 else torch.stack(outs)

    def render(self, wfe=True):
        """Render the DM's surface figure or, with wfe, reflected wavefront error (2 x obliquity x surface), projected into the beam
        normal by self.rot and padded / cropped to Nout (dm.py:219-273).  Returns a 2-D device tensor."""
        return self._render(self.actuators[None], wfe)[0]

    def render_stack(self, actuators, wfe=True):
        """render() of each of B command maps (B, Nact_y, Nact_x) in one launch sequence -> (B, *Nout); self.actuators is untouched."""
        acts = actuators if isinstance(actuators, torch.Tensor) else L.as_device(actuators)
        if acts.dim() != 3:
            raise ValueError('render_stack: actuators must be (B, Nact_y, Nact_x)')
        return self._render(acts, wfe)

    # ------------------------------------------------------------------ adjoint
    def render_adjoint(self, protograd, wfe=True):
        """The adjoint of render() (dm.py:275-331): protograd (rows, cols), or a (B, rows, cols) stack, -> gradient with respect to
        the actuators, (Nact_y, Nact_x) or (B, Nact_y, Nact_x).  Needs a prior render (Nintermediate)."""
        g = L.as_device(protograd) if not isinstance(protograd, torch.Tensor) else protograd
        if g.is_complex():
            raise TypeError('render_adjoint: protograd must be real (the reference does not support complex protograd either)')
        if g.device != self.ifn.device or g.dtype != self.ifn.dtype or g.stride(-1) != 1:
            g = L.as_device(g, self.ifn.dtype)
        single = g.dim() == 2
        if single:
            g = g[None]
        Nint = self.Nintermediate
        rows, cols = self.ifn.shape
        B = g.shape[0]
        scale = 2 * self.obliquity if wfe else 1.0
        inner = tuple(g.shape[-2:])
        pad = None
        if inner[0] > Nint[0]:          # forward padded: crop (a view)
            g = crop_center(g, Nint) if g.dim() == 2 else g[(slice(None),) + tuple(
                slice(math.ceil((i - o) / 2), math.ceil((i - o) / 2) + o) for i, o in zip(inner, Nint))]
        elif inner[0] < Nint[0]:        # forward cropped: pad
            pad = (tuple(Nint), tuple(-math.ceil((o - i) / 2) for i, o in zip(inner, Nint)))
        if self.upsample != 1:
            if pad is not None:
                g = self._pad_fields(g, pad)
            factor = rows / g.shape[-2]
            g = torch.stack([fourier_resample(g[b], factor) for b in range(B)]).to(self.ifn.dtype)
            pad = None
        chain_kw = {}
        if self.needs_rot:
            if pad is not None:
                g = self._pad_fields(g, pad)
            g = self._warp(g, self.Mfwd, scale)
            sc = 1.0 / (rows * cols)
        else:
            sc = scale / (rows * cols)
            if pad is not None:
                if any(o < 0 for o in pad[1]):
                    g = self._pad_fields(g, pad)
                else:               # the chain reads the padded field through its input window
                    chain_kw = dict(shape=(rows, cols), in_off=tuple(-o for o in pad[1]))
        if tuple(g.shape[-2:]) != (rows, cols) and not chain_kw:
            raise ValueError(f'render_adjoint: protograd resolves to {tuple(g.shape[-2:])}, not the influence function shape {(rows, cols)}')
        x = g[0] if B == 1 else g
        F = self._chain(x, sc, mul_conj=True, **chain_kw)
        out = self._gather(F.reshape((B, rows, cols)))
        return out[0] if single else out
