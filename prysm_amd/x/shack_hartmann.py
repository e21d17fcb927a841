"""Shack-Hartmann phase screens on the device (prysm/x/shack_hartmann.py).

The reference builds the screen in a Python double loop over the lenslets (shack_hartmann.py:102-114), each iteration slicing a
window, evaluating an aperture and accumulating: 4096 iterations for the 64 x 64 array its docstring recommends.  Its windows
(_local_window, 2 x samples_per_lenslet wide around an aperture of half-width pitch / 2) never clip an aperture, so the screen is a
closed-form function of the sample and pm_lenslet_screen (csrc/sensors.hip) forms it in ONE launch: a sample tests the 3 x 3
lenslets around the nearest centre and adds the quadratic phase of those whose aperture holds it.

  geometry.rectangle (optional height=, angle 0 or absent) and geometry.circle take that path.  Membership is decided with the
  reference's own expressions in the coordinates' precision, so a sample on the shared edge of two lenslets belongs to both and gets
  both terms, as in the reference.
  Any other callable, a rotated rectangle, or a rectangle taller than a pitch takes the reference's loop written with this
  library's tensor operations: one window per lenslet, slow but correct.

Coordinates: 2-D arrays as the reference takes them, 1-D vectors x (nx) and y (ny), or shape= / dx= (the grid of make_xy_grid,
generated in the kernel).  The screen is complex in the coordinates' precision (config.precision for a generated grid).  Kept from
the reference: n = (n0, n1) makes n1 centres along x and n0 along y, while shift=True moves xc by half a pitch when n0 is even and yc
when n1 is even.
"""
import inspect
import math

import numpy as np
import torch

from .. import _lib as L
from .. import _ops
from .. import geometry
from ..conf import config
from ..coordinates import _real_dtype, make_xy_grid
from ..geometry_plan import grid_spacing
from . import sensors_plan as SP

__all__ = ['shack_hartmann']

rectangle = geometry.rectangle


def _np_dtype(dt):
    return np.float32 if dt == torch.float32 else np.float64


def _loop(pitch, n, efl, wavelength, x, y, aperture, aperture_kwargs, shift):
    """shack_hartmann.py:70-117 with tensor operations, one window per lenslet.  x, y: 2-D tensors of one real dtype; the work is done
    where they live."""
    from ..segmented import _local_window
    if not hasattr(n, '__iter__'):
        n = (n, n)
    dt = x.dtype
    params = inspect.signature(aperture).parameters
    callxy = 'x' in params and 'y' in params
    dx = float(x[0, 1] - x[0, 0])
    samples_per_lenslet = int(pitch / dx + 1)
    par = dict(nx=n[1], ny=n[0], pitch=float(pitch), shift_x=pitch / 2 if (shift and n[0] % 2 == 0) else 0.0,
               shift_y=pitch / 2 if (shift and n[1] % 2 == 0) else 0.0)
    xc, yc = SP.lenslet_centres(par, _np_dtype(dt))
    cx, cy = math.ceil(x.shape[1] / 2), math.ceil(y.shape[0] / 2)
    lenslet_rsq = (pitch / 2) ** 2
    total = torch.zeros_like(x)
    for yy in yc:
        for xx in xc:
            win = _local_window(cy, cx, (float(xx), float(yy)), dx, samples_per_lenslet, x, y)
            lx = x[win] - float(xx)
            ly = y[win] - float(yy)
            if lx.numel() == 0:
                continue
            rsq = lx * lx + ly * ly
            phase = rsq / (2 * efl)
            if callxy:
                m = aperture(pitch / 2, x=lx, y=ly, **aperture_kwargs)
            else:
                m = aperture(lenslet_rsq, r=rsq, **aperture_kwargs)
            total[win] += phase * torch.as_tensor(m, device=x.device).to(dt)
    arg = total * (-(2 * math.pi) / (wavelength / 1e3))
    return torch.complex(torch.cos(arg), torch.sin(arg))


def shack_hartmann(pitch, n, efl, wavelength, x=None, y=None, aperture=rectangle, aperture_kwargs=None, shift=False, *, shape=None, dx=0):
    """Create the complex screen for a Shack-Hartmann lenslet array (shack_hartmann.py:11-117):
    exp(-2 pi i / (wavelength / 1e3) total), total = the sum over the lenslets whose aperture holds the sample of
    ((x - xc)^2 + (y - yc)^2) / (2 efl).

    pitch: lenslet pitch, mm; n: number of lenslets, an int or (n0, n1); efl: focal length of each lenslet, mm; wavelength: um;
    x, y: coordinates, mm (2-D arrays, 1-D vectors, or shape= / dx= instead); aperture: geometry.rectangle or geometry.circle for the
    one-launch path, any callable taking x= and y= or r= otherwise; shift: move the array by half a pitch in +x / +y."""
    if aperture_kwargs is None:
        aperture_kwargs = {}
    kind = SP.LENSLET_RECTANGLE if aperture is geometry.rectangle else SP.LENSLET_CIRCLE if aperture is geometry.circle else None
    par = SP.lenslet_params(pitch, n, efl, wavelength, kind, aperture_kwargs, shift) if kind is not None else None
    if par is None:
        if shape is not None:
            x, y = make_xy_grid(shape, dx=dx)
        dt = _real_dtype(x, y)
        if len(np.shape(x)) != 2 or np.shape(x) != np.shape(y):
            raise ValueError('the per-lenslet loop takes two 2-D coordinate arrays of one shape')
        return _loop(pitch, n, efl, wavelength, L.as_device(x, dt), L.as_device(y, dt), aperture, aperture_kwargs, shift)
    if shape is not None:
        if x is not None or y is not None:
            raise ValueError('give either shape= with dx=, or x and y')
        (ny, nx), dx = grid_spacing(shape, dx, 0)
        return _ops.lenslet_screen(par, L.torch_dtype(config.compute_precision), L.PM_COORDS_GRID, ny, nx, dx=dx)
    if x is None or y is None:
        raise ValueError('give either shape= with dx=, or x and y')
    dt = _real_dtype(x, y)
    sx, sy = tuple(np.shape(x)), tuple(np.shape(y))
    if len(sx) == 1 and len(sy) == 1:
        xd, _ = _ops._vector(x, dt)
        if xd.stride(0) != 1:
            xd = xd.contiguous()
        yd, ldy = _ops._vector(y, dt)
        return _ops.lenslet_screen(par, dt, L.PM_COORDS_SEPARABLE, sy[0], sx[0], x=xd, y=yd, ldy=ldy)
    if sx != sy or len(sx) != 2:
        raise ValueError(f'coordinates must be two 2-D arrays of one shape or two 1-D vectors, got {sx} and {sy}')
    xd, ldx = _ops._rows(x, dt)
    yd, ldy = _ops._rows(y, dt)
    return _ops.lenslet_screen(par, dt, L.PM_COORDS_POINTWISE, sx[0], sx[1], x=xd, ldx=ldx, y=yd, ldy=ldy)
