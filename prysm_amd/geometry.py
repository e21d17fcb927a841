"""Aperture geometry on the device: the signed-distance shapes of prysm/geometry.py, and whole apertures rendered in one launch.

The reference's functions are here under their names, with their arguments, argument checks and quirks: circle[_sdf],
annulus[_sdf], rectangle[_sdf], rotated_ellipse[_sdf], polygon_sdf, regular_polygon[_sdf], spider[_sdf], offset_circle,
rectangle_with_corner_fillets[_sdf], gaussian, square, antialias, union, intersect, subtract.  The functions that the reference
passes through optimize_xy_separable (rectangle_sdf at angle 0, polygon_sdf, regular_polygon_sdf, offset_circle, gaussian,
rectangle_with_corner_fillets_sdf at rotation 0) take 2-D meshgrids or 1-D vectors and give (ny, nx); the others are elementwise with
numpy broadcasting.  Masks are torch.bool; distances and coverage are float32 when every array argument is float32 and float64
otherwise.  One deliberate difference: on float32 input the reference's rotated_ellipse_sdf and spider_sdf return float64 (np.radians
hands them a float64 scalar); here they stay float32.  Complex input raises TypeError; arguments are checked before any upload.

New, beyond the reference: `shape` builds a whole aperture symbolically --

    ap = shape.circle(3.0).intersect(shape.regular_polygon(6, 2.7, rotation=11.3)).subtract(shape.circle(0.7)) \
              .subtract(shape.spider(3, 0.14, rotation=13.7))
    amp = render(ap, shape=(4096, 4096), dx=dx, antialias=True)

-- and render() evaluates it per pixel in ONE kernel (pm_sdf_render) that writes each output element once: the coordinates come from
the pixel index (or from given vectors / arrays), the shape from a step table of a few hundred bytes built by geometry_plan.plan and
cached on the device.  Every function above is the one-node case of the same kernel.  union / intersect / subtract / antialias on
TENSORS are thin torch calls (one full-array sweep each); on shape nodes they build the tree.

multisample is left out on purpose: the reference calls it a fallback for shapes without a distance function, and every shape here
has one.
"""
import numpy as np
import torch

from . import _lib as L
from . import geometry_plan as GP
from .conf import config
from .coordinates import _real_dtype, _code
from .geometry_plan import Node

__all__ = ['shape', 'render', 'Node', 'antialias', 'union', 'intersect', 'subtract', 'gaussian', 'rectangle_sdf', 'rectangle',
           'rotated_ellipse_sdf', 'rotated_ellipse', 'square', 'circle_sdf', 'circle', 'annulus_sdf', 'annulus', 'polygon_sdf',
           'regular_polygon_sdf', 'regular_polygon', 'spider_sdf', 'spider', 'offset_circle', 'rectangle_with_corner_fillets_sdf',
           'rectangle_with_corner_fillets']

_TABLES = {}
_TABLES_MAX = 64
_KINDS = {'mask': L.PM_SDF_MASK, 'sdf': L.PM_SDF_DISTANCE, 'coverage': L.PM_SDF_COVERAGE}


class shape:
    """Constructors of shape nodes: the primitives of the reference (with center= where it has one) and the three combinations.
    Nodes also combine by method: a.union(b, c), a.intersect(b), a.subtract(b)."""
    circle = staticmethod(GP.circle)
    offset_circle = staticmethod(GP.offset_circle)
    annulus = staticmethod(GP.annulus)
    rectangle = staticmethod(GP.rectangle)
    rectangle_with_corner_fillets = staticmethod(GP.rectangle_with_corner_fillets)
    rotated_ellipse = staticmethod(GP.rotated_ellipse)
    polygon = staticmethod(GP.polygon)
    spider = staticmethod(GP.spider)
    gaussian = staticmethod(GP.gaussian)
    union = staticmethod(GP.union)
    intersect = staticmethod(GP.intersect)
    subtract = staticmethod(GP.subtract)

    @staticmethod
    def regular_polygon(sides, radius, center=(0, 0), rotation=0):
        """vertices R sin(k 2 pi / sides + rot) + x0, R cos(...) + y0, generated on the host in config.precision"""
        return GP.regular_polygon(sides, radius, center, rotation, dtype=config.precision)


def _table(programs, dtype):
    """the step table of a tuple of programs on the current device: (uint8 device tensor, steps per program)"""
    key = (tuple(p.key for p in programs), dtype, L._cur_dev())
    hit = _TABLES.get(key)
    if hit is None:
        t = GP.plan(programs, np.float32 if dtype == torch.float32 else np.float64)
        if len(_TABLES) >= _TABLES_MAX:
            _TABLES.pop(next(iter(_TABLES)))
        hit = _TABLES[key] = (torch.from_numpy(t.view(np.uint8).copy()).to(L.device()), t.shape[1])
    return hit


def _launch(programs, dt, coords, ny, nx, xd, yd, ox, oy, dx, kind, aa, out, out_ld, out_bstride):
    tab, nsteps = _table(programs, dt)
    L.check(L.load().pm_sdf_render(_code(dt), coords, ny, nx, L.ptr(xd), L.ptr(yd), ox, oy, dx, dx, L.ptr(tab), nsteps, len(programs),
                                   _KINDS[kind], aa, L.ptr(out), out_ld, out_bstride, L.stream_ptr()))


def _shapes(x, y):
    return tuple(np.shape(x)), tuple(np.shape(y))


def _programs(program):
    single = isinstance(program, Node)
    programs = (program,) if single else tuple(program)
    if not programs or not all(isinstance(p, Node) for p in programs):
        raise TypeError('render() takes a shape node or a non-empty sequence of them')
    return programs, single


def render(program, *, shape=None, dx=0, diameter=0, x=None, y=None, output=None, antialias=None, dtype=None, out=None):
    """Evaluate a shape tree (or a sequence of B of them: a (B, ...) stack) in one launch.

    Where: either a grid -- `shape` (rows, cols) with `dx` or `diameter`, make_xy_grid's rule, the coordinates computed from the pixel
    index and never stored -- or coordinates `x`, `y`: two 1-D vectors give (ny, nx); two arrays of one shape (a meshgrid, warped
    points) give that shape.
    What: output 'mask' (torch.bool, d <= 0; the default), 'sdf' (the signed distance) or 'coverage' (antialias's one-pixel ramp).
    antialias=True means coverage with the grid's spacing, antialias=<number> coverage with that sample spacing.
    dtype: the working precision, torch.float32 / float64 (default: config.precision for a grid, else float32 when x and y both are,
    float64 otherwise).  out: a device tensor to write into; its last dimension must be contiguous, rows and programs may be strided.
    Allocates only its output once the table is cached, so it can be captured in a graph."""
    programs, single = _programs(program)
    if output is None:
        output = 'coverage' if (antialias is not None and antialias is not False) else 'mask'
    if output not in _KINDS:
        raise ValueError(f"output must be 'mask', 'sdf' or 'coverage', got {output!r}")
    if any(p.kind == 'gaussian' for p in programs) and output != 'sdf':
        raise ValueError("a gaussian is a value, not a distance: render it with output='sdf'")
    grid = shape is not None
    if grid == (x is not None or y is not None) or (x is None) != (y is None):
        raise ValueError('give either shape= with dx= / diameter=, or x= and y=')
    if dtype is not None:
        dtype = L.torch_dtype(dtype)
        if dtype not in (torch.float32, torch.float64):
            raise TypeError('dtype must be float32 or float64')
    aa = 0.0
    if grid:
        (ny, nx), dx = GP.grid_spacing(shape, dx, diameter)
        dt = dtype or L.torch_dtype(config.compute_precision)
        oshape, coords = (ny, nx), L.PM_COORDS_GRID
        if antialias is True or (output == 'coverage' and antialias is None):
            aa = dx
    else:
        dt = dtype or _real_dtype(x, y)
        _real_dtype(x, y)
        sx, sy = _shapes(x, y)
        if len(sx) == 1 and len(sy) == 1:
            oshape, coords = (sy[0], sx[0]), L.PM_COORDS_SEPARABLE
        elif sx == sy:
            oshape, coords = sx, L.PM_COORDS_POINTWISE
        else:
            raise ValueError(f'coordinate arrays differ in shape: {sx} and {sy}')
        if antialias is True or (output == 'coverage' and antialias is None):
            raise ValueError('coverage on given coordinates needs the sample spacing: antialias=dx')
        ny, nx = oshape if len(oshape) == 2 else (1, int(np.prod(oshape, dtype=np.int64)))
    if output == 'coverage':
        if antialias is not None and antialias is not True:
            aa = float(antialias)
        if not aa > 0:
            raise ValueError('coverage needs a sample spacing > 0')
    for p in programs:
        if GP.depth(p) > GP.MAX_SLOTS:
            raise ValueError(f'the shape tree nests composites deeper than the {GP.MAX_SLOTS} accumulators of the kernel')
    B = len(programs)
    full = oshape if single else (B, *oshape)
    odt = torch.bool if output == 'mask' else dt
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(full) or out.dtype != odt:
            raise ValueError(f'out must be a {odt} tensor of shape {tuple(full)}')
    # ---- everything is checked: the device from here on
    dev = L.device()
    xd = yd = None
    if not grid:
        xd, yd = L.as_device(x, dt), L.as_device(y, dt)
    if out is None:
        out = torch.empty(full, dtype=odt, device=dev)
    elif out.device != dev:
        raise ValueError('out must be on the current device')
    if out.numel() == 0:
        return out
    o = out if not single else out.unsqueeze(0)
    if len(oshape) == 2 and o.stride(-1) == 1 and o.stride(-2) >= nx and (B == 1 or o.stride(0) >= ny * o.stride(-2)):
        out_ld, out_bs = o.stride(-2), (o.stride(0) if B > 1 else ny * o.stride(-2))
    elif o[0].is_contiguous() and (B == 1 or o.stride(0) >= ny * nx):
        out_ld, out_bs = nx, (o.stride(0) if B > 1 else ny * nx)
    else:
        raise ValueError('out: the last dimension must be contiguous and rows / programs must not overlap')
    _launch(programs, dt, coords, ny, nx, xd, yd, nx // 2, ny // 2, dx if grid else 0.0, output, aa, out, out_ld, out_bs)
    return out


# ---------------------------------------------------------------- the one-node forms behind the reference's functions
def _separable(node, output, x, y, aa=0.0):
    """x, y as optimize_xy_separable takes them: 2-D meshgrids (first row / first column are read) or 1-D vectors -> (ny, nx)"""
    dt = _real_dtype(x, y)
    sx, sy = _shapes(x, y)
    if len(sx) == 2:
        if sx != sy:
            raise ValueError(f'coordinate arrays differ in shape: {sx} and {sy}')
        x, y = x[0, :], y[:, 0]
    elif len(sx) > 2 or len(sy) > 2:
        raise ValueError(f'coordinates must be 2-D meshgrids or 1-D vectors, got {sx} and {sy}')
    else:
        x, y = x.reshape(-1), y.reshape(-1)
    return render(node, x=x, y=y, output=output, antialias=aa or None, dtype=dt)


def _elementwise(node, output, x, y, vec_to_grid=False):
    """x, y broadcast against each other (1-D vectors to a grid first when vec_to_grid, cart_to_polar's rule)"""
    dt = _real_dtype(x, y)
    sx, sy = _shapes(x, y)
    if vec_to_grid and len(sx) == 1:
        if len(sy) != 1:
            raise ValueError(f'x is a vector of {sx} but y has shape {sy}')
        return render(node, x=x, y=y, output=output, dtype=dt)
    full = tuple(np.broadcast_shapes(sx, sy))
    if sx != full or sy != full:
        x, y = L.as_device(x, dt).expand(full).contiguous(), L.as_device(y, dt).expand(full).contiguous()
    if len(full) == 1:      # two equal vectors are points, not the axes of a grid
        x, y = x.reshape(1, -1), y.reshape(1, -1)
        return render(node, x=x, y=y, output=output, dtype=dt).reshape(full)
    return render(node, x=x, y=y, output=output, dtype=dt)


def antialias(d, dx):
    """signed distance -> coverage with a one-pixel edge ramp: min(max(0.5 - d / dx, 0), 1) (geometry.py:11-34).  A thin torch call;
    render(..., antialias=...) does it inside the kernel."""
    return torch.clamp(0.5 - d / dx, 0, 1)


def _combine(ds, fn, node_fn):
    if all(isinstance(d, Node) for d in ds):
        return node_fn(*ds)
    out = ds[0]
    for d in ds[1:]:
        out = fn(out, d)
    return out


def union(*ds):
    """signed distance of the union: the minimum (geometry.py:37-54).  Shape nodes give a node."""
    return _combine(ds, torch.minimum, GP.union)


def intersect(*ds):
    """signed distance of the intersection: the maximum (geometry.py:57-74).  Shape nodes give a node."""
    return _combine(ds, torch.maximum, GP.intersect)


def subtract(d1, d2):
    """signed distance of shape 1 with shape 2 removed: max(d1, -d2) (geometry.py:77-93).  Shape nodes give a node."""
    if isinstance(d1, Node) and isinstance(d2, Node):
        return GP.subtract(d1, d2)
    return torch.maximum(d1, -d2)


def gaussian(sigma, x, y, center=(0, 0)):
    """exp(-4 ln 2 ((x - x0)^2 + (y - y0)^2) / sigma^2) (geometry.py:154-179); x, y 2-D meshgrids or vectors."""
    return _separable(GP.gaussian(sigma, center), 'sdf', x, y)


def rectangle_sdf(width, x, y, height=None, angle=0):
    """signed distance to a rectangle of half-width `width` and half-height `height` (None: square) (geometry.py:182-222).  angle 0:
    x, y meshgrids or vectors; angle 90 swaps x and y, elementwise; any other angle rotates the coordinates by +angle degrees (the
    kernel rotates directly where the reference goes through polar coordinates: a rounding-level difference)."""
    node = GP.rectangle(width, height, angle)
    if angle == 0:
        return _separable(node, 'sdf', x, y)
    return _elementwise(node, 'sdf', x, y, vec_to_grid=angle != 90)


def rectangle(width, x, y, height=None, angle=0):
    """mask of rectangle_sdf (geometry.py:225-248)."""
    node = GP.rectangle(width, height, angle)
    if angle == 0:
        return _separable(node, 'mask', x, y)
    return _elementwise(node, 'mask', x, y, vec_to_grid=angle != 90)


def rotated_ellipse_sdf(width_major, width_minor, x, y, major_axis_angle=0):
    """first-order signed distance F / max(|grad F|, 1e-15) to an ellipse about the origin (geometry.py:251-290); ValueError when
    minor > major.  float32 input gives float32 (the reference: float64)."""
    return _elementwise(GP.rotated_ellipse(width_major, width_minor, major_axis_angle), 'sdf', x, y)


def rotated_ellipse(width_major, width_minor, x, y, major_axis_angle=0):
    """mask of rotated_ellipse_sdf (geometry.py:293-315)."""
    return _elementwise(GP.rotated_ellipse(width_major, width_minor, major_axis_angle), 'mask', x, y)


def square(x, y):
    """ones like x (geometry.py:318-334)."""
    _real_dtype(x, y)
    return torch.ones_like(L.as_device(x))


def circle_sdf(radius, r):
    """r - radius (geometry.py:337-353)."""
    return _elementwise(GP.radial_circle(radius), 'sdf', r, r)


def circle(radius, r):
    """mask of circle_sdf (geometry.py:356-372)."""
    return _elementwise(GP.radial_circle(radius), 'mask', r, r)


def annulus_sdf(rin, rout, r):
    """|r - (rin + rout) / 2| - (rout - rin) / 2 (geometry.py:375-395)."""
    return _elementwise(GP.radial_annulus(rin, rout), 'sdf', r, r)


def annulus(rin, rout, r):
    """mask of annulus_sdf (geometry.py:398-416)."""
    return _elementwise(GP.radial_annulus(rin, rout), 'mask', r, r)


def polygon_sdf(vertices, x, y):
    """signed distance to a polygon of N x 2 vertices, either winding, concave allowed (geometry.py:419-463): the minimum over edges
    of the distance to the clamped segment, the sign by even-odd crossing parity.  x, y meshgrids or vectors."""
    return _separable(GP.polygon(vertices), 'sdf', x, y)


def regular_polygon_sdf(sides, radius, x, y, center=(0, 0), rotation=0):
    """polygon_sdf of a regular polygon (geometry.py:466-491), vertices generated on the host in config.precision."""
    return _separable(shape.regular_polygon(sides, radius, center, rotation), 'sdf', x, y)


def regular_polygon(sides, radius, x, y, center=(0, 0), rotation=0):
    """mask of regular_polygon_sdf (geometry.py:494-518)."""
    return _separable(shape.regular_polygon(sides, radius, center, rotation), 'mask', x, y)


def spider_sdf(vanes, width, x, y, rotation=0, center=(0, 0), rotation_is_rad=False):
    """signed distance to the vanes of a spider: semi-infinite capsules of full width `width` from `center`, `rotation` clockwise, in
    degrees unless rotation_is_rad (geometry.py:550-594).  float32 input gives float32 (the reference: float64)."""
    return _elementwise(GP.spider(vanes, width, rotation, center, rotation_is_rad), 'sdf', x, y)


def spider(vanes, width, x, y, rotation=0, center=(0, 0), rotation_is_rad=False):
    """mask of spider_sdf (geometry.py:597-624)."""
    return _elementwise(GP.spider(vanes, width, rotation, center, rotation_is_rad), 'mask', x, y)


def offset_circle(radius, x, y, center):
    """mask of a circle about `center` (geometry.py:627-653); x, y meshgrids or vectors."""
    return _separable(GP.circle(radius, center), 'mask', x, y)


def rectangle_with_corner_fillets_sdf(width, height, cradius, x, y, center=(0, 0), rotation=0):
    """signed distance to a rectangle with filleted corners (geometry.py:656-696); a rotation (degrees) is about the grid origin,
    applied before `center` is subtracted.  rotation 0: x, y meshgrids or vectors."""
    node = GP.rectangle_with_corner_fillets(width, height, cradius, center, rotation)
    if rotation == 0:
        return _separable(node, 'sdf', x, y)
    return _elementwise(node, 'sdf', x, y, vec_to_grid=True)


def rectangle_with_corner_fillets(width, height, cradius, x, y, center=(0, 0), rotation=0):
    """mask of rectangle_with_corner_fillets_sdf (geometry.py:699-726)."""
    node = GP.rectangle_with_corner_fillets(width, height, cradius, center, rotation)
    if rotation == 0:
        return _separable(node, 'mask', x, y)
    return _elementwise(node, 'mask', x, y, vec_to_grid=True)
