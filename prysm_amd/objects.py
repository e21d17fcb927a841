"""Objects for image simulation on the device (prysm/objects.py): slit, pinhole, siemensstar, tiltedsquare, slantededge and the
analytic spectra slit_ft and pinhole_ft.

Each target is ONE launch of pm_object_render (csrc/imagechain.hip) that stores every sample once.  The functions keep the reference's
signatures and defaults; coordinates are accepted the way geometry.render accepts them and are read once by the kernel, never expanded
to a 2-D map on the host:

  2-D arrays as given        x, y (or r, t for the pinhole and the Siemens star), rows may be strided views
  1-D separable vectors      x (nx) and y (ny) give (ny, nx); the polar targets form r = hypot(x, y), t = atan2(y, x) in registers
  shape= / dx=               keyword only: the grid of coordinates.make_xy_grid, generated in the kernel

Kept from the reference: siemensstar paints the background BEFORE the binarisation, so with sinusoidal=False a black background comes
out as bottom = (1 - contrast) / 2 and a white one as top, and samples where the cosine gives exactly 0.5 stay 0.5; an invalid background
raises ValueError before any launch; slit and pinhole return torch.bool masks; slit (like the reference, through
optimize_xy_separable) reads the first row of a 2-D x and the first column of a 2-D y.  slantededge(crossed=True) combines the edge
with its own rot90 and needs a square grid: a non-square one raises ValueError (the reference fails there with a broadcast error).

Precision: coordinates._real_dtype's rule -- float32 when every array argument is float32, float64 otherwise, config.precision for a
generated grid -- NOT the reference's mixed casts (its slit_ft casts to config.precision, its tilted square and slanted edge compute
float32 coordinates in float64 because np.radians returns a float64 scalar).

slit_ft and pinhole_ft are one launch of pm_tf_product each; `slit_ft.spec(width_x, width_y)` and `pinhole_ft.spec(radius)` are their
deferred forms for convolution.apply_transfer_functions / convolution.transfer_function.  slit_ft keeps the reference's exact
`fx == 0` / `fy == 0` band tests and recovers the grid lengths from the spacing of the first two frequencies of each axis.
"""
import numpy as np
import torch

from . import _lib as L
from . import _ops
from . import imagechain_plan as IP
from .conf import config
from .coordinates import _real_dtype
from .geometry_plan import grid_spacing

__all__ = ['slit', 'slit_ft', 'pinhole', 'pinhole_ft', 'siemensstar', 'tiltedsquare', 'slantededge']


def _render(params, a, b, shape, dx, polar=False, first_lines=False, what=('x', 'y')):
    """one target from whichever coordinate form was given"""
    kind, flags, p = params
    if shape is not None:
        if a is not None or b is not None:
            raise ValueError(f'give either shape= with dx=, or {what[0]} and {what[1]}')
        (ny, nx), dx = grid_spacing(shape, dx, 0)
        dt = L.torch_dtype(config.compute_precision)
        return _ops.object_render(kind, flags, p, dt, L.PM_COORDS_GRID, ny, nx, dx=dx)
    if a is None or (b is None and not (polar and kind == IP.PINHOLE)):
        raise ValueError(f'give either shape= with dx=, or {what[0]} and {what[1]}')
    arrays = [v for v in (a, b) if v is not None]
    dt = _real_dtype(*arrays)
    sa = tuple(np.shape(a))
    sb = sa if b is None else tuple(np.shape(b))
    if len(sa) == 2 and first_lines:       # optimize_xy_separable: the first row of x, the first column of y
        if len(sb) != 2:
            raise ValueError(f'coordinate arrays differ in shape: {sa} and {sb}')
        a, b = a[0, :], b[:, 0]
        sa, sb = (sa[1],), (sb[0],)
    if len(sa) == 1 and len(sb) == 1 and not polar:
        ad, _ = _ops._vector(a, dt)
        if ad.stride(0) != 1:
            ad = ad.contiguous()
        bd, ldb = _ops._vector(b, dt)
        return _ops.object_render(kind, flags, p, dt, L.PM_COORDS_SEPARABLE, sb[0], sa[0], a=ad, b=bd, ldb=ldb)
    if sa != sb or len(sa) != 2:
        raise ValueError(f'coordinates must be two 2-D arrays of one shape or two 1-D vectors, got {sa} and {sb}')
    ad, lda = _ops._rows(a, dt)
    bd, ldb = (None, 0) if b is None else _ops._rows(b, dt)
    return _ops.object_render(kind, flags, p, dt, L.PM_COORDS_POINTWISE, sa[0], sa[1], a=ad, lda=lda, b=bd, ldb=ldb, polar=polar)


def slit(x=None, y=None, width_x=None, width_y=None, *, shape=None, dx=0):
    """Rasterize a slit or pair of crossed slits (objects.py:8-37): a torch.bool mask, True where |x| <= width_x / 2 or
    |y| <= width_y / 2 (None draws no slit along that axis).  One launch."""
    return _render(IP.object_params(IP.SLIT, width_x=width_x, width_y=width_y), x, y, shape, dx, first_lines=True)


def pinhole(radius, rho=None, *, x=None, y=None, shape=None, dx=0):
    """Rasterize a pinhole (objects.py:91-107): the torch.bool mask rho <= radius.  rho as the reference takes it, or x= and y= / shape=
    and dx= with rho = hypot(x, y) formed in the kernel.  One launch."""
    params = IP.object_params(IP.PINHOLE, radius=radius)
    if rho is not None:
        if x is not None or y is not None or shape is not None:
            raise ValueError('give rho, or x= and y=, or shape= with dx=')
        r2 = rho if len(np.shape(rho)) == 2 else L.as_device(rho, _real_dtype(rho)).reshape(1, -1)
        return _render(params, r2, None, None, 0, polar=True).reshape(tuple(np.shape(rho)))
    return _render(params, x, y, shape, dx)


def siemensstar(r=None, t=None, spokes=None, oradius=0.9, iradius=0, background='black', contrast=0.9, sinusoidal=False, *, x=None, y=None,
                shape=None, dx=0):
    """Rasterize a Siemens star (objects.py:130-181) in [0, 1]: (contrast cos(spokes / 2 t) + 1) / 2 inside iradius <= r <= oradius, the
    background outside, binarised to bottom / top unless sinusoidal.  r, t as the reference takes them, or x= and y= / shape= and dx=
    with the polar coordinates formed in the kernel.  One launch."""
    if spokes is None:
        raise TypeError('siemensstar() needs the number of spokes')
    params = IP.object_params(IP.SIEMENSSTAR, spokes=spokes, oradius=oradius, iradius=iradius, background=background, contrast=contrast,
                              sinusoidal=sinusoidal)
    if r is not None or t is not None:
        if x is not None or y is not None or shape is not None:
            raise ValueError('give r and t, or x= and y=, or shape= with dx=')
        return _render(params, r, t, None, 0, polar=True, what=('r', 't'))
    return _render(params, x, y, shape, dx)


def tiltedsquare(x=None, y=None, angle=4, radius=0.5, contrast=0.9, background='white', *, shape=None, dx=0):
    """Rasterize a tilted square (objects.py:184-224): delta = (1 - contrast) / 2 inside and 1 - delta outside on a white background,
    the other way round on a black one.  One launch."""
    return _render(IP.object_params(IP.TILTEDSQUARE, angle=angle, radius=radius, contrast=contrast, background=background), x, y, shape, dx)


def slantededge(x=None, y=None, angle=4, contrast=0.9, crossed=False, *, shape=None, dx=0):
    """Rasterize a slanted edge (objects.py:227-258): (1 - contrast) / 2 where x cos(angle) - y sin(angle) > 0, one minus that elsewhere;
    crossed=True draws four edges (the mask and its rot90, square grids only).  One launch."""
    params = IP.object_params(IP.SLANTEDEDGE, angle=angle, contrast=contrast, crossed=crossed)
    if crossed:
        s = grid_spacing(shape, dx, 0)[0] if shape is not None else (tuple(np.shape(y))[:1] + tuple(np.shape(x))[-1:])
        if len(s) == 2 and s[0] != s[1]:
            raise ValueError(f'crossed edges need a square grid, got {s[0]} x {s[1]}')
    return _render(params, x, y, shape, dx)


def _eager(spec, fx=None, fy=None, fr=None):
    """one analytic transfer function on given frequencies: a real map in the working precision, one launch"""
    given = [v for v in (fx, fy, fr) if v is not None]
    dt = _real_dtype(*given, what='frequencies')
    if fr is not None:
        shp = tuple(np.shape(fr))
        t, _ = _ops._rows(fr, dt)
        return _ops.tf_product(t.shape, spec.records, dt, fr=t, real_out=True).reshape(shp)
    sx, sy = tuple(np.shape(fx)), tuple(np.shape(fy))
    if (len(sx) == 1 and len(sy) == 1) or (len(sx) == 2 and len(sy) == 2 and sx[0] == 1 and sy[1] == 1):
        vx, vy = L.as_device(fx, dt).reshape(-1), L.as_device(fy, dt).reshape(-1)
        return _ops.tf_product((vy.numel(), vx.numel()), spec.records, dt, fx=vx, fy=vy, real_out=True)
    shp = tuple(np.broadcast_shapes(sx, sy))
    if len(shp) != 2:
        raise ValueError(f'frequencies must be 1-D vectors or broadcast to a 2-D array, got {sx} and {sy}')
    return _ops.tf_product(shp, spec.records, dt, fx=L.as_device(fx, dt) if not isinstance(fx, torch.Tensor) else fx,
                           fy=L.as_device(fy, dt) if not isinstance(fy, torch.Tensor) else fy, real_out=True)


def slit_ft(width_x, width_y, fx, fy):
    """Analytic Fourier transform of a slit, normalized to 1 at DC (objects.py:40-88).  fx, fy: 2-D meshgrids (their first row / first
    column are read, as the reference does) or 1-D vectors, fftshifted so that they contain 0.  Both widths empty raises ValueError."""
    spec = IP.slit_spec(width_x, width_y)
    dt = _real_dtype(fx, fy, what='frequencies')
    if len(np.shape(fx)) == 2:
        fx, fy = fx[0, :], fy[:, 0]
    vx, _ = _ops._vector(fx, dt)
    vy, _ = _ops._vector(fy, dt)
    return _ops.tf_product((vy.numel(), vx.numel()), spec.records, dt, fx=vx, fy=vy, real_out=True)


def pinhole_ft(radius, fr):
    """Analytic Fourier transform of a pinhole (objects.py:110-127): jinc(2 pi radius fr), jinc from the unit's own J1 series."""
    return _eager(IP.pinhole_spec(radius), fr=fr)


slit_ft.spec = IP.slit_spec
pinhole_ft.spec = IP.pinhole_spec
