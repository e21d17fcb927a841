"""Shapes, apertures and posed surfaces of the ray trace (prysm/x/raytracing/surfaces.py, aperture.py).

Host code: a shape holds its parameters, a Surface its pose (numpy, built on the host), interaction, material and aperture; the trace
itself reads them from the packed table (prysm_amd/x/raytrace_plan.py) in the kernel of csrc/raytrace.hip.  `sag` and
`sag_and_normal` are for users who call them: torch operations on tensors, where the tensors lie.

Not built, each raising NotImplementedError with its name: gratings, surface coatings, a callable clip, the shapes Q2D, Zernike, XY,
Chebyshev, Jacobi, Toroid, Biconic and CallableShape, and even aspheres of more than 8 coefficients.
"""
import numbers

import torch

from ...conf import config
from ...coordinates import apply_tilt_decenter, coerce_3d_rotation, promote_3d_point
from .. import raytrace_plan as plan
from ..raytrace_plan import STYPE_EVAL, STYPE_IMG, STYPE_OBJ, STYPE_REFLECT, STYPE_REFRACT, DepartureBand

__all__ = ['STYPE_REFLECT', 'STYPE_REFRACT', 'STYPE_EVAL', 'STYPE_OBJ', 'STYPE_IMG', 'Shape', 'Plane', 'Sphere', 'Conic', 'OffAxisConic',
           'EvenAsphere', 'Surface', 'DepartureBand', 'Aperture', 'CircularClip', 'AnnularClip', 'circular_aperture', 'annular_aperture']


_STYPE_NAMES = {'refl': STYPE_REFLECT, 'reflect': STYPE_REFLECT, 'refr': STYPE_REFRACT, 'refract': STYPE_REFRACT, 'eval': STYPE_EVAL,
                'obj': STYPE_OBJ, 'object': STYPE_OBJ, 'img': STYPE_IMG, 'image': STYPE_IMG}


def _map_stype(typ):
    """the STYPE constant of an interaction given by name (any case) or as one of the constants; anything else is a ValueError"""
    if isinstance(typ, numbers.Integral):
        if int(typ) in _STYPE_NAMES.values():
            return int(typ)
    elif typ.lower() in _STYPE_NAMES:
        return _STYPE_NAMES[typ.lower()]
    raise ValueError(f'unknown surface type {typ!r}: it is one of {sorted(_STYPE_NAMES)} or one of the STYPE_* constants')


# --------------------------------------------------------------------------- apertures (aperture.py)

class CircularClip:
    """circular clip predicate carrying its radius"""

    def __init__(self, radius, x0=0.0, y0=0.0):
        self.radius, self.x0, self.y0 = float(radius), float(x0), float(y0)

    def __call__(self, x, y):
        dx, dy = x - self.x0, y - self.y0
        return dx * dx + dy * dy <= self.radius * self.radius

    @property
    def limiting_radius(self):
        return self.radius

    def __repr__(self):
        return f'CircularClip(radius={self.radius:g})'


class AnnularClip:
    """annular clip predicate: passes the ring, blocks the central disk"""

    def __init__(self, inner_radius, outer_radius, x0=0.0, y0=0.0):
        self.inner_radius, self.outer_radius, self.x0, self.y0 = float(inner_radius), float(outer_radius), float(x0), float(y0)

    def __call__(self, x, y):
        dx, dy = x - self.x0, y - self.y0
        rsq = dx * dx + dy * dy
        return (rsq >= self.inner_radius * self.inner_radius) & (rsq <= self.outer_radius * self.outer_radius)

    @property
    def limiting_radius(self):
        return self.outer_radius

    def __repr__(self):
        return f'AnnularClip(inner_radius={self.inner_radius:g}, outer_radius={self.outer_radius:g})'


def circular_aperture(radius, x0=0.0, y0=0.0):
    return CircularClip(radius, x0, y0)


def annular_aperture(inner_radius, outer_radius, x0=0.0, y0=0.0):
    return AnnularClip(inner_radius, outer_radius, x0, y0)


class Aperture:
    """a surface's clip: None, a CircularClip or an AnnularClip; a number is a circular clip of that radius"""

    def __init__(self, clip=None):
        if isinstance(clip, (int, float)) and not isinstance(clip, bool):
            clip = circular_aperture(clip)
        if clip is not None and not isinstance(clip, (CircularClip, AnnularClip)):
            raise NotImplementedError(f'a callable clip ({clip!r}) is not implemented: the kernel tests circular and annular apertures')
        self.clip = clip

    def clips(self, x, y):
        return True if self.clip is None else self.clip(x, y)

    def limiting_radius(self, footprint=None):
        return footprint if self.clip is None else self.clip.limiting_radius

    def __repr__(self):
        return 'Aperture()' if self.clip is None else f'Aperture(clip={self.clip!r})'


def as_aperture(value):
    return value if isinstance(value, Aperture) else Aperture(value)


# --------------------------------------------------------------------------- shapes

def _unit_normal(fx, fy):
    inv = 1.0 / torch.sqrt(1.0 + fx * fx + fy * fy)
    return torch.stack([-fx * inv, -fy * inv, inv], dim=-1)


def _conic_sag(c, k, rsq):
    return (c * rsq) / (1 + torch.sqrt(1 - (1 + k) * c * c * rsq))


def _conic_sag_and_normal(c, k, X, Y):
    """conic_sag_and_normal (sags.py:109-121)"""
    if c == 0.0:
        n = torch.zeros(X.shape + (3,), dtype=X.dtype, device=X.device)
        n[..., 2] = 1.0
        return torch.zeros_like(X), n
    A = X * X + Y * Y
    phi = torch.nan_to_num(torch.sqrt(1 - (1 + k) * c * c * A), nan=0.0, posinf=float('inf'), neginf=float('-inf'))
    mag_sq = 1.0 - k * c * c * A
    mag = torch.sqrt(torch.where(mag_sq < 0.0, torch.ones_like(mag_sq), mag_sq))
    return (c * A) / (1 + phi), torch.stack([-c * X / mag, -c * Y / mag, phi / mag], dim=-1)


class Shape:
    """base of the sag-bearing shapes: parameters in `params`, also readable as attributes"""
    analytic_intersect = False

    def __init__(self, **params):
        self.params = params or None

    def __getattr__(self, name):
        params = self.__dict__.get('params')
        if params is not None and name in params:
            return params[name]
        raise AttributeError(name)

    def sag(self, x, y):
        raise NotImplementedError

    def sag_and_normal(self, x, y):
        raise NotImplementedError


class Plane(Shape):
    analytic_intersect = True

    def __init__(self):
        super().__init__()

    def sag(self, x, y):
        return torch.zeros_like(x)

    def sag_and_normal(self, x, y):
        return _conic_sag_and_normal(0.0, 0.0, x, y)


class Sphere(Shape):
    analytic_intersect = True

    def __init__(self, c):
        super().__init__(c=c)

    def sag(self, x, y):
        return _conic_sag(self.params['c'], 0.0, x * x + y * y)

    def sag_and_normal(self, x, y):
        return _conic_sag_and_normal(self.params['c'], 0.0, x, y)


class Conic(Shape):
    analytic_intersect = True

    def __init__(self, c, k):
        super().__init__(c=c, k=k)

    def sag(self, x, y):
        return _conic_sag(self.params['c'], self.params['k'], x * x + y * y)

    def sag_and_normal(self, x, y):
        return _conic_sag_and_normal(self.params['c'], self.params['k'], x, y)


class OffAxisConic(Shape):
    analytic_intersect = True

    def __init__(self, c, k, dx=0.0, dy=0.0):
        super().__init__(c=c, k=k, dx=dx, dy=dy)

    def sag(self, x, y):
        p = self.params
        X, Y = x + p['dx'], y + p['dy']
        return _conic_sag(p['c'], p['k'], X * X + Y * Y)

    def sag_and_normal(self, x, y):
        p = self.params
        return _conic_sag_and_normal(p['c'], p['k'], x + p['dx'], y + p['dy'])


class EvenAsphere(Shape):
    """conic base plus coefs[i] r^(2 i + 4); intersected by Newton from the seed conic's root"""

    def __init__(self, c, k, coefs):
        coefs = tuple(coefs) if coefs is not None else ()
        if len(coefs) > plan.MAX_COEFS:
            raise NotImplementedError(f'an even asphere of {len(coefs)} coefficients: the surface table holds {plan.MAX_COEFS}')
        super().__init__(c=c, k=k, coefs=coefs)

    def seed_conic(self):
        p = self.params
        return p['c'], p['k'], 0.0, 0.0

    def sag(self, x, y):
        p = self.params
        rsq = x * x + y * y
        z = _conic_sag(p['c'], p['k'], rsq)
        if len(p['coefs']) == 0:
            return z
        poly = 0.0
        for a in reversed(p['coefs']):
            poly = poly * rsq + a
        return z + poly * rsq * rsq

    def sag_and_normal(self, x, y):
        p = self.params
        c, k = p['c'], p['k']
        rsq = x * x + y * y
        phi = torch.sqrt(1 - (1 + k) * c * c * rsq)
        fx, fy = (c * x) / phi, (c * y) / phi
        if len(p['coefs']) > 0:
            poly = 0.0
            for i in range(len(p['coefs']) - 1, -1, -1):
                poly = poly * rsq + (i + 2) * p['coefs'][i]
            common = 2.0 * rsq * poly
            fx, fy = fx + x * common, fy + y * common
        return self.sag(x, y), _unit_normal(fx, fy)


def _not_built_shape(name):
    class _Shape(Shape):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError(f'prysm_amd.x.raytracing: the shape {name} is not implemented (Plane, Sphere, Conic, OffAxisConic and '
                                      'EvenAsphere are)')
    _Shape.__name__ = _Shape.__qualname__ = name
    return _Shape


Q2D, Zernike, XY, Chebyshev, Jacobi, Toroid, Biconic, CallableShape = (
    _not_built_shape(n) for n in ('Q2D', 'Zernike', 'XY', 'Chebyshev', 'Jacobi', 'Toroid', 'Biconic', 'CallableShape'))
__all__ += ['Q2D', 'Zernike', 'XY', 'Chebyshev', 'Jacobi', 'Toroid', 'Biconic', 'CallableShape']


# --------------------------------------------------------------------------- the posed surface

class Surface:
    """A posed optical surface with a shape and an interaction (surfaces.py:1162-1238): shape, interaction ('reflect', 'refract',
    'eval', 'object', 'image' or an STYPE constant), the pose -- (P, R) as `pose` or by keyword, then tilt and decenter --, the material
    (anything with .n(wvl), or a number as a constant index; required of a refracting surface) and the aperture (None, a number for a
    circular clip, circular_aperture / annular_aperture)."""

    def __init__(self, shape=None, interaction=None, pose=None, material=None, aperture=None, grating=None, *, P=None, R=None, tilt=None,
                 decenter=None, tilt_radians=False, coating=None):
        if shape is None:
            raise TypeError('Surface requires a shape')
        if interaction is None:
            raise TypeError('Surface requires an interaction')
        if grating is not None:
            raise NotImplementedError('Surface(grating=...) is not implemented: the kernel bends by reflection and refraction only')
        if coating is not None:
            raise NotImplementedError('Surface(coating=...) is not implemented: surfaces are bare interfaces')
        if not isinstance(shape, (Plane, Sphere, Conic, OffAxisConic, EvenAsphere)):
            raise NotImplementedError(f'the shape {type(shape).__name__} is not implemented (Plane, Sphere, Conic, OffAxisConic and '
                                      'EvenAsphere are)')
        if pose is not None:
            try:
                P, R = pose
            except (TypeError, ValueError):
                P, R = pose.P, pose.R
        if P is None:
            raise TypeError('Surface requires a pose or P')
        typ = _map_stype(interaction)
        P = promote_3d_point(P, dtype=config.precision)
        R = coerce_3d_rotation(R)
        P, R = apply_tilt_decenter(P, R, tilt=tilt, decenter=decenter, tilt_radians=tilt_radians, dtype=config.precision)
        if typ == STYPE_REFRACT and material is None:
            raise ValueError('refractive surfaces must have a material, not None')
        self.shape, self.typ, self.P, self.R, self.material = shape, typ, P, R, material
        self.params = shape.params
        self.aperture = aperture
        self.sag, self.sag_and_normal = shape.sag, shape.sag_and_normal
        self._analytic_intersect = bool(shape.analytic_intersect)
        self._departure_band = None

    @property
    def aperture(self):
        return self._aperture

    @aperture.setter
    def aperture(self, value):
        self._aperture = as_aperture(value)
        self._departure_band = None

    def departure_band(self):
        """the conic-seed departure bounds of the first-root acceptance band; unbounded for a closed-form shape (surfaces.py:1262-1339).
        Computed once, on the host in float64."""
        if self._departure_band is None:
            if isinstance(self.shape, EvenAsphere):
                p = self.shape.params
                self._departure_band = plan.departure_band(p['c'], p['k'], p['coefs'], self.aperture.limiting_radius())
            else:
                self._departure_band = DepartureBand.unbounded()
        return self._departure_band
