"""Multilayer stacks on the device (prysm/x/coatings/stack.py): Stack, stack_rt, internal_fields and RTA on pm_tf_stack.

Layers are ambient side first.  Angles are radians; thicknesses and wavelengths share a unit (microns in the reference).  `wvl` and
`theta0` broadcast against each other, against indices that depend on wavelength and against per-sample thicknesses; the results
keep that calculation shape and are device tensors.  A Stack holds its thicknesses as a device tensor: float32 / float64 tensors
keep their dtype (and their storage, so an optimizer's x can be the stack's thicknesses), anything else is taken in
config.precision.  That dtype decides the precision of every evaluation: float32 -> complex64, float64 -> complex128.  Indices are
constants, callables of wavelength or objects with .nk, resolved on the host into the layer table the kernel reads.
"""
import numpy as np
import torch

from ... import _lib as L
from ... import _ops
from ...conf import config

__all__ = ['Stack', 'stack_rt', 'internal_fields', 'RTA', 'field_at_depth', 'stack_characteristic_matrices', 'forward_products',
           'backward_products']


def _resolve(index, wvl):
    """a constant, a callable of wavelength or a material with .nk at wavelength wvl (stack.py:13-20)"""
    nk = getattr(index, 'nk', None)
    if callable(nk):
        return nk(wvl)
    if callable(index):
        return index(wvl)
    return index


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def resolve_table(indices, wvl, shape=None):
    """the per-layer indices at wvl as one host array: (L, 1) when no layer depends on the sample, else (L, K) over `shape`"""
    vals = [np.asarray(_host(_resolve(n, wvl)), dtype=np.complex128) for n in indices]
    if not vals:
        return np.zeros((0, 1), dtype=np.complex128)
    if all(v.size == 1 for v in vals):
        return np.array([v.reshape(()) for v in vals]).reshape(-1, 1)
    shape = np.broadcast_shapes(*(v.shape for v in vals)) if shape is None else tuple(shape)
    return np.stack([np.broadcast_to(v, shape).reshape(-1) for v in vals])


class Stack:
    """A multilayer thin-film stack (stack.py:60-99).

    indices: per-layer refractive index, ambient side first.  thicknesses: per-layer physical thicknesses (a scalar is repeated
    per layer).  substrate_index, ambient_index: constants, callables of wavelength or objects with .nk.
    """

    __slots__ = ('indices', 'thicknesses', 'substrate_index', 'ambient_index')

    def __init__(self, indices, thicknesses, substrate_index, ambient_index=1.0):
        indices = list(indices)
        if isinstance(thicknesses, torch.Tensor):
            t = thicknesses if thicknesses.dtype in (torch.float32, torch.float64) else thicknesses.to(L.torch_dtype(config.compute_precision))
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(thicknesses, dtype=config.compute_precision)))
        if t.dim() == 0:
            t = t.expand(len(indices)).contiguous()
        if len(indices) != t.shape[0]:
            raise ValueError('indices and thicknesses must describe the same number of layers')
        self.indices = indices
        self.thicknesses = L.as_device(t)
        self.substrate_index = substrate_index
        self.ambient_index = ambient_index

    def __len__(self):
        return self.thicknesses.shape[0]

    def resolved_indices(self, wvl):
        """List of per-layer indices evaluated at wavelength wvl."""
        return [_resolve(n, wvl) for n in self.indices]

    def __repr__(self):
        return f'Stack({len(self)} layers, substrate={self.substrate_index!r})'


def operands(stack, wvl, theta0):
    """(TfOperands, calculation shape) of a stack over wvl x theta0: the indices resolved on the host, everything else as it is"""
    d = stack.thicknesses
    if d.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'the thicknesses must be float32 or float64, got {d.dtype}')
    cd = L._COMPLEX_OF[d.dtype]
    w = _host(wvl)
    n0, nsub = _host(_resolve(stack.ambient_index, w)), _host(_resolve(stack.substrate_index, w))
    layers = [_host(_resolve(n, w)) for n in stack.indices]
    theta_shape = tuple(theta0.shape) if hasattr(theta0, 'shape') else ()
    shape = np.broadcast_shapes(w.shape, theta_shape, n0.shape, nsub.shape, tuple(d.shape[1:]), *(v.shape for v in layers))
    K = int(np.prod(shape, dtype=np.int64))
    from ...thinfilm import flat_operand
    table = resolve_table(layers, w, shape)
    dd = d if d.dim() == 1 else torch.broadcast_to(d.reshape((d.shape[0],) + (1,) * (len(shape) - d.dim() + 1) + tuple(d.shape[1:])),
                                                    (d.shape[0],) + shape).reshape(d.shape[0], -1)
    op = _ops.TfOperands(cd, K, flat_operand(wvl, shape), flat_operand(theta0, shape), table, dd, flat_operand(nsub, shape),
                         flat_operand(n0, shape))
    return op, tuple(shape)


def _pol(pol):
    pol = pol.lower()
    if pol not in ('p', 's'):
        raise ValueError("unknown polarization, use 'p' or 's'")
    return pol


def stack_rt(stack, wvl, theta0, pol):
    """Amplitude reflection and transmission coefficients r, t for a unit-amplitude incident wave (stack.py:206-226)."""
    pol = _pol(pol)
    op, shape = operands(stack, wvl, theta0)
    out = _ops.tf_stack(op, pol)
    return out['r'][0].reshape(shape), out['t'][0].reshape(shape)


def internal_fields(stack, wvl, theta0, pol):
    """Tangential E and H at every boundary, the leading axis from the ambient side (stack.py:229-249)."""
    pol = _pol(pol)
    op, shape = operands(stack, wvl, theta0)
    out = _ops.tf_stack(op, pol, want=('fields',))
    return out['E'][0].reshape((-1,) + shape), out['H'][0].reshape((-1,) + shape)


def RTA(stack, wvl, theta0, pol):
    """Reflectance, transmittance and per-layer absorptance; A has one leading entry per layer (stack.py:304-334)."""
    pol = _pol(pol)
    op, shape = operands(stack, wvl, theta0)
    out = _ops.tf_stack(op, pol, want=('R', 'T', 'A'))
    return out['R'][0].reshape(shape), out['T'][0].reshape(shape), out['A'][0].reshape((-1,) + shape)


def field_at_depth(stack, z, wvl, theta0, pol):
    """Not built: the field at arbitrary depths (stack.py:252-301)."""
    raise NotImplementedError('prysm_amd.x.coatings.field_at_depth is not implemented: internal_fields gives the boundaries only')


def _matrices(name):
    def missing(*args, **kwargs):
        raise NotImplementedError(f'prysm_amd.x.coatings.{name} is not implemented: the kernels keep no per-layer matrices '
                                  '(stack_rt, internal_fields and RTA sweep them in registers)')
    missing.__name__ = name
    return missing


stack_characteristic_matrices = _matrices('stack_characteristic_matrices')
forward_products = _matrices('forward_products')
backward_products = _matrices('backward_products')
