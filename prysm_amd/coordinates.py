"""Coordinate grids and conversions on the device (prysm/coordinates.py:11-125, 344-378).

make_xy_grid, cart_to_polar and polar_to_cart are one launch each, both outputs from one kernel (csrc/geometry.hip); the two view
helpers are host logic on tensors.  uniform_cart_to_polar (coordinates.py:269-316) is one gather launch (csrc/imagechain.hip).  Grids come back in config.precision, conversions in the inputs' precision (float32 when every
input is float32, float64 otherwise).  The pose helpers of the ray trace -- promote_3d_point, coerce_3d_rotation,
apply_tilt_decenter and make_rotation_matrix (coordinates.py:168-266, 381-429) -- are host code on numpy: a Surface's pose is built on
the host.  The rest of the reference module (homographies, warps, resample_2d, quadratures) is not here.
"""
import numpy as np
import torch

from . import _lib as L
from .conf import config
from .geometry_plan import grid_spacing

__all__ = ['make_xy_grid', 'cart_to_polar', 'polar_to_cart', 'optimize_xy_separable', 'broadcast_1d_to_2d', 'uniform_cart_to_polar', 'promote_3d_point',
           'coerce_3d_rotation', 'apply_tilt_decenter', 'make_rotation_matrix']


def _real_dtype(*arrays, what='coordinates'):
    """float32 when every array is float32, float64 for any other real input; TypeError for complex"""
    f32 = True
    for a in arrays:
        if isinstance(a, torch.Tensor):
            cplx, single = a.is_complex(), a.dtype == torch.float32
        else:
            dt = np.asarray(a).dtype
            cplx, single = np.issubdtype(dt, np.complexfloating), dt == np.float32
        if cplx:
            raise TypeError(f'{what} must be real')
        f32 = f32 and single
    return torch.float32 if f32 else torch.float64


def _code(dt):
    return L.PM_F32 if dt == torch.float32 else L.PM_F64


def _tensor(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))


def optimize_xy_separable(x, y):
    """x as a (1, nx) row and y as an (ny, 1) column: views of the first row / first column of 2-D meshgrids, or of 1-D vectors
    (coordinates.py:11-45)."""
    x, y = _tensor(x), _tensor(y)
    if x.ndim == 2:
        return x[0, :].reshape(1, -1), y[:, 0].reshape(-1, 1)
    return x.reshape(1, -1), y.reshape(-1, 1)


def broadcast_1d_to_2d(x, y):
    """vectors x (n,) and y (m,) as (m, n) views (coordinates.py:48-70)."""
    x, y = _tensor(x), _tensor(y)
    return x.reshape(1, -1).expand(y.numel(), x.numel()), y.reshape(-1, 1).expand(y.numel(), x.numel())


def make_xy_grid(shape, *, dx=0, diameter=0, grid=True):
    """x, y of a grid of `shape` = (rows, cols) samples (a scalar: square) spaced dx apart, or diameter / max(shape) when a diameter is
    given, with the origin at sample n // 2: meshgrids, or 1-D vectors when grid=False (coordinates.py:344-378).  Element j of an axis
    is (j - n // 2) in config.precision times dx rounded once to it, the reference's fftrange(n) * dx bit for bit.  One launch."""
    (ny, nx), dx = grid_spacing(shape, dx, diameter)
    dt = L.torch_dtype(config.compute_precision)
    dev = L.device()
    if grid:
        x, y = torch.empty((ny, nx), dtype=dt, device=dev), torch.empty((ny, nx), dtype=dt, device=dev)
    else:
        x, y = torch.empty(nx, dtype=dt, device=dev), torch.empty(ny, dtype=dt, device=dev)
    L.check(L.load().pm_xy_grid(_code(dt), ny, nx, dx, int(bool(grid)), L.ptr(x), L.ptr(y), L.stream_ptr()))
    return x, y


def cart_to_polar(x, y, vec_to_grid=True):
    """rho = hypot(x, y), phi = atan2(y, x) (coordinates.py:73-102).  1-D vectors give (ny, nx) grids when vec_to_grid; otherwise the
    inputs broadcast.  One launch."""
    dt = _real_dtype(x, y)
    sx, sy = tuple(np.shape(x)), tuple(np.shape(y))
    separable = vec_to_grid and len(sx) == 1
    if separable:
        if len(sy) != 1:
            raise ValueError(f'x is a vector of {sx} but y has shape {sy}')
        shape = (sy[0], sx[0])
    else:
        shape = tuple(np.broadcast_shapes(sx, sy))
    xd, yd = L.as_device(x, dt), L.as_device(y, dt)
    if not separable and (sx != shape or sy != shape):
        xd, yd = xd.expand(shape).contiguous(), yd.expand(shape).contiguous()
    rho, phi = torch.empty(shape, dtype=dt, device=xd.device), torch.empty(shape, dtype=dt, device=xd.device)
    n = rho.numel()
    ny, nx = (shape if separable else (1, n))
    L.check(L.load().pm_cart_to_polar(_code(dt), ny, nx, int(separable), L.ptr(xd), L.ptr(yd), L.ptr(rho), L.ptr(phi), L.stream_ptr()))
    return rho, phi


def polar_to_cart(rho, phi):
    """x = rho cos(phi), y = rho sin(phi) (coordinates.py:105-125).  One launch."""
    dt = _real_dtype(rho, phi)
    shape = tuple(np.broadcast_shapes(tuple(np.shape(rho)), tuple(np.shape(phi))))
    r, p = L.as_device(rho, dt), L.as_device(phi, dt)
    if tuple(r.shape) != shape or tuple(p.shape) != shape:
        r, p = r.expand(shape).contiguous(), p.expand(shape).contiguous()
    x, y = torch.empty(shape, dtype=dt, device=r.device), torch.empty(shape, dtype=dt, device=r.device)
    L.check(L.load().pm_polar_to_cart(_code(dt), x.numel(), L.ptr(r), L.ptr(p), L.ptr(x), L.ptr(y), L.stream_ptr()))
    return x, y


def uniform_cart_to_polar(x, y, data):
    """data, sampled uniformly on the sorted 1-D coordinates x (columns) and y (rows), interpolated onto polar coordinates
    (coordinates.py:269-316): returns (rho, phi, polar) on the device with rho = linspace(0, max|x, y extremes|, len(x)),
    phi = linspace(0, 2 pi, len(y)) and polar[i, j] the bilinear interpolation at rho[j] (cos phi[i], sin phi[i]) -- scipy's
    RegularGridInterpolator(method='linear', bounds_error=False, fill_value=0): 0 outside [min, max] of either axis, the boundary
    inside.  One gather launch (pm_polar_resample); the axes are built on the host from x and y (device vectors are read back, numpy
    ones are not).  Everything is in the precision of _real_dtype(x, y, data), not in the reference's float64."""
    from . import _ops
    from . import imagechain_plan as IP
    dt = _real_dtype(x, y, data)
    hx, hy = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (x, y))
    if hx.ndim != 1 or hy.ndim != 1 or hx.size < 2 or hy.size < 2:
        raise ValueError('x and y must be sorted 1-D arrays of at least two sample points')
    npdt = np.float32 if dt == torch.float32 else np.float64
    hx, hy = hx.astype(npdt), hy.astype(npdt)
    if tuple(np.shape(data)) != (hy.size, hx.size):
        raise ValueError(f'data has shape {tuple(np.shape(data))}, the coordinates describe {(hy.size, hx.size)}')
    rho, phi, _ = IP.polar_axes(hx, hy)
    d, _ = _ops._rows(data, dt)
    xd, yd = L.as_device(hx), L.as_device(hy)
    rd, pd = L.as_device(rho.astype(npdt)), L.as_device(phi.astype(npdt))
    x_step, y_step = (float(hx[-1]) - float(hx[0])) / (hx.size - 1), (float(hy[-1]) - float(hy[0])) / (hy.size - 1)
    return rd, pd, _ops.polar_resample(xd, yd, x_step, y_step, rd, pd, d)


# --------------------------------------------------------------------------- poses (host, numpy)

def promote_3d_point(P, dtype=None):
    """A point from a z, a (y, z) or an (x, y, z): a scalar is z, a sequence fills the coordinates from the right; more than three
    (or no) values are a ValueError"""
    coords = list(P) if hasattr(P, '__iter__') else [P]
    if len(coords) not in (1, 2, 3):
        raise ValueError('P must contain one to three coordinates')
    return np.array([0] * (3 - len(coords)) + coords, dtype=config.precision if dtype is None else dtype)


def make_rotation_matrix(zyx, radians=False):
    """The rotation Rx(a) Ry(b) Rz(g) from up to three angles given in the order (g about z, b about y, a about x), missing ones zero;
    degrees unless `radians`.  Written out as one matrix from the six sines and cosines."""
    g, b, a = (tuple(float(v) for v in zyx) + (0.0, 0.0, 0.0))[:3]
    if not radians:
        g, b, a = np.radians(g), np.radians(b), np.radians(a)
    sa, ca, sb, cb, sg, cg = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(g), np.cos(g)
    return np.array([[cb * cg, -cb * sg, sb],
                     [sa * sb * cg + ca * sg, ca * cg - sa * sb * sg, -sa * cb],
                     [sa * sg - ca * sb * cg, ca * sb * sg + sa * cg, ca * cb]])


def coerce_3d_rotation(R):
    """a list or tuple is (z, y, x) angles in degrees and becomes their matrix; a matrix, or None for no rotation, passes through"""
    return make_rotation_matrix(R) if type(R) in (list, tuple) else R


def apply_tilt_decenter(P, R, tilt=None, decenter=None, tilt_radians=False, dtype=None):
    """The pose (P, R) moved by `decenter` (three values, else a ValueError) and turned by `tilt` ((z, y, x) angles, applied on the right
    of R).  R None is no rotation and stays None when there is no tilt."""
    if decenter is not None:
        shift = np.asarray(decenter, dtype=config.precision if dtype is None else dtype)
        if shift.shape != (3,):
            raise ValueError(f'decenter must be a length-3 vector, got shape {shift.shape}')
        P = P + shift
    if tilt is None:
        return P, R
    turn = make_rotation_matrix(tilt, radians=tilt_radians)
    return P, (turn if R is None else R @ turn)
