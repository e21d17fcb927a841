"""Thin-film calculations (prysm/thinfilm.py): the Fresnel one-liners on the host and multilayer_stack_rt on the device.

brewsters_angle, critical_angle, snell_aor and the four Fresnel coefficients are host arithmetic on Python scalars, numpy arrays or
torch tensors (a tensor stays where it lies), one line each as in the reference.  multilayer_stack_rt runs on pm_tf_stack
(csrc/thinfilm.hip): one thread per sample walks the layers in registers, s or p, one launch.  Its signature, its ValueErrors and
its conventions are the reference's: the first axis of `indices` / `thicknesses` is the layer axis and trailing axes are calculation
axes, `aoi` is in DEGREES, the results keep the calculation shape and come back as device tensors.  `wavelength`, `aoi` and
`ambient_index` may be arrays too and broadcast with the calculation axes (scalar layers over a wavelength x angle grid).

Its `t` for p-polarisation is NOT prysm_amd.x.coatings.stack_rt's: t_thinfilm,p = t_stack,p cos(theta_0) / cos(theta_sub) (the
reference's A00 carries the substrate's cosine), while r is the same; the kernel applies the factor under PM_TF_T_THINFILM.

Precision: complex64 when `indices` or `thicknesses` is a float32 / complex64 array or tensor or config.precision is below 64,
else complex128.
"""
import numpy as np
import torch

from . import _lib as L
from . import _ops
from .conf import config

__all__ = ['brewsters_angle', 'critical_angle', 'snell_aor', 'fresnel_rs', 'fresnel_ts', 'fresnel_rp', 'fresnel_tp', 'multilayer_stack_rt']


def _xp(*args):
    return torch if any(isinstance(a, torch.Tensor) for a in args) else np


def brewsters_angle(n0, n1, deg=True):
    """Brewster's angle of the n0 | n1 interface (thinfilm.py:5-22)."""
    xp = _xp(n0, n1)
    ang = xp.arctan2(*(torch.as_tensor(v, dtype=torch.float64) if xp is torch and not isinstance(v, torch.Tensor) else v for v in (n1, n0)))
    return xp.rad2deg(ang) if deg else ang


def critical_angle(n0, n1, deg=True):
    """The smallest angle of total internal reflection going from n0 into n1 (thinfilm.py:25-47)."""
    xp = _xp(n0, n1)
    ang = xp.arcsin(n1 / n0)
    return xp.rad2deg(ang) if deg else ang


def snell_aor(n0, n1, theta, deg=True):
    """The angle of refraction, complex beyond the critical angle (thinfilm.py:50-72)."""
    xp = _xp(n0, n1, theta)
    if deg:
        theta = xp.deg2rad(theta)
    s = n0 / n1 * xp.sin(theta)
    if xp is torch:
        return torch.asin(s.to(L._COMPLEX_OF.get(s.dtype, s.dtype)) if bool(torch.any(s.abs() > 1)) and not s.is_complex() else s)
    return np.lib.scimath.arcsin(s)


def fresnel_rs(n0, n1, theta0, theta1):
    """r_s of an interface; angles in radians (thinfilm.py:83-107)."""
    xp = _xp(n0, n1, theta0, theta1)
    return (n0 * xp.cos(theta0) - n1 * xp.cos(theta1)) / (n0 * xp.cos(theta0) + n1 * xp.cos(theta1))


def fresnel_ts(n0, n1, theta0, theta1):
    """t_s of an interface (thinfilm.py:110-134)."""
    xp = _xp(n0, n1, theta0, theta1)
    return (2 * n0 * xp.cos(theta0)) / (n0 * xp.cos(theta0) + n1 * xp.cos(theta1))


def fresnel_rp(n0, n1, theta0, theta1):
    """r_p of an interface (thinfilm.py:137-161)."""
    xp = _xp(n0, n1, theta0, theta1)
    return (n0 * xp.cos(theta1) - n1 * xp.cos(theta0)) / (n0 * xp.cos(theta1) + n1 * xp.cos(theta0))


def fresnel_tp(n0, n1, theta0, theta1):
    """t_p of an interface (thinfilm.py:164-188)."""
    xp = _xp(n0, n1, theta0, theta1)
    return (2 * n0 * xp.cos(theta0)) / (n0 * xp.cos(theta1) + n1 * xp.cos(theta0))


def _array(v):
    """a tensor as it is, anything else as a numpy array"""
    return v if isinstance(v, torch.Tensor) else np.asarray(v)


def _broadcast_to(v, shape):
    return torch.broadcast_to(v, shape) if isinstance(v, torch.Tensor) else np.broadcast_to(v, shape)


def _single(v):
    return (v.dtype in (torch.float32, torch.complex64)) if isinstance(v, torch.Tensor) else (v.dtype in (np.float32, np.complex64))


def flat_operand(v, shape):
    """v for the kernels: its one value when it has one (a shared operand), else broadcast to `shape` and flattened"""
    v = _array(v)
    size = v.numel() if isinstance(v, torch.Tensor) else v.size
    if size == 1:
        return v.reshape(1)
    return _broadcast_to(v, shape).reshape(-1)


def _as_layer_arrays(indices, thicknesses):
    """thinfilm.py:191-210: the two arrays broadcast against each other, the layer axis first"""
    if isinstance(indices, (list, tuple)) and any(isinstance(i, torch.Tensor) for i in indices):
        indices = torch.stack([torch.as_tensor(i) for i in indices])
    if isinstance(thicknesses, (list, tuple)) and any(isinstance(i, torch.Tensor) for i in thicknesses):
        thicknesses = torch.stack([torch.as_tensor(i) for i in thicknesses])
    indices, thicknesses = _array(indices), _array(thicknesses)
    if indices.ndim == 0:
        indices = indices[None]
    if thicknesses.ndim == 0:
        thicknesses = thicknesses[None]
    try:
        shape = np.broadcast_shapes(tuple(indices.shape), tuple(thicknesses.shape))
    except ValueError as exc:
        raise ValueError('indices and thicknesses must be broadcastable to the same shape') from exc
    if len(shape) < 1 or shape[0] == 0:
        raise ValueError('indices and thicknesses must contain at least one film layer')
    return indices, thicknesses, shape


def multilayer_stack_rt(indices, thicknesses, wavelength, polarization, substrate_index, aoi=0, ambient_index=1):
    """r and t of a stack of films (thinfilm.py:213-316), on the device.

    indices, thicknesses: the layer axis first, ambient side first; trailing axes are calculation axes.  wavelength and thicknesses
    in the same unit; polarization 'p' or 's'; aoi in degrees.  Returns (r, t) as device tensors of the calculation shape.
    """
    polarization = polarization.lower()
    if polarization not in ('p', 's'):
        raise ValueError("unknown polarization, use p or s")
    indices, thicknesses, layer_shape = _as_layer_arrays(indices, thicknesses)
    nlayers, calc = layer_shape[0], tuple(layer_shape[1:])
    substrate_index = _array(substrate_index)
    if len(layer_shape) > 1:
        try:
            np.broadcast_shapes(tuple(substrate_index.shape), calc)
            if len(substrate_index.shape) > len(calc):
                raise ValueError
        except ValueError as exc:
            raise ValueError('substrate_index must be broadcastable to the trailing layer dimensions') from exc
    wavelength, aoi, ambient_index = _array(wavelength), _array(aoi), _array(ambient_index)
    shape = np.broadcast_shapes(calc, *(tuple(v.shape) for v in (substrate_index, wavelength, aoi, ambient_index)))
    K = int(np.prod(shape, dtype=np.int64))
    single = _single(indices) or _single(thicknesses) or config.compute_precision is np.float32
    cd = torch.complex64 if single else torch.complex128

    def table(a):
        b = _broadcast_to(a, layer_shape)
        strides = b.stride() if isinstance(b, torch.Tensor) else b.strides
        if all(st == 0 or sz == 1 for st, sz in zip(strides[1:], layer_shape[1:])):      # the same value for every sample: a shared table
            return b[(slice(None),) + (0,) * len(calc)].reshape(nlayers, 1)
        b = b.reshape((nlayers,) + (1,) * (len(shape) - len(calc)) + calc)
        return _broadcast_to(b, (nlayers,) + tuple(shape)).reshape(nlayers, -1)
    theta = flat_operand(aoi, shape)
    theta = torch.deg2rad(theta.to(torch.float64)) if isinstance(theta, torch.Tensor) else np.radians(theta.astype(np.float64))
    op = _ops.TfOperands(cd, K, flat_operand(wavelength, shape), theta, table(indices), table(thicknesses),
                         flat_operand(substrate_index, shape), flat_operand(ambient_index, shape))
    out = _ops.tf_stack(op, polarization, L.PM_TF_T_THINFILM)
    return out['r'][0].reshape(tuple(shape)), out['t'][0].reshape(tuple(shape))
