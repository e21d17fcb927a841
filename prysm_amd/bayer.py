"""Bayer mosaics on the device (prysm/bayer.py): white balance, (de/re)compositing and demosaicing.

The reference's names, signatures, argument checks and error types; inputs numpy arrays or torch tensors, results torch tensors on
the device.  demosaic_malvar is ONE kernel (pm_bayer_demosaic: the mosaic read once -- the Detector's integer DN as stored -- and
the RGB image stored once); composite / recomposite / deinterlace are one sweep each; safe white balance is two launches without a
host read (pm_bayer_class_max, pm_bayer_scale), so it can be captured in a graph.  prysm_amd/bayer_plan.py restates the kernels in
numpy.

Differences from the reference, all deliberate:
- wb_prescale / wb_postscale scale a floating DEVICE tensor in place and RETURN it (the reference scales in place and returns None);
  a numpy array (or an integer tensor) is copied to the device first and the scaled tensor returned.  The safe ratio is formed in
  the data's precision.
- demosaic_malvar takes a stack (B, m, n) -> (B, m, n, 3) in one launch, and `layout='chw'` returns (..., 3, m, n).
- composite_bayer / recomposite_bayer / demosaic_deinterlace take stacks too.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import _ops
from . import bayer_plan as BP
from .bayer_plan import kernel_G_at_R_or_B, kernel_R_at_G_in_RB, kernel_R_at_G_in_BR, kernel_R_at_B_in_BB  # noqa: F401
from .conf import config
from .coordinates import _code
from .detector import _stack_view

__all__ = ['wb_prescale', 'wb_postscale', 'composite_bayer', 'decomposite_bayer', 'recomposite_bayer', 'demosaic_deinterlace',
           'assemble_superresolved', 'demosaic_malvar', 'top_left', 'top_right', 'bottom_left', 'bottom_right', 'ErrBadCFA',
           'kernel_G_at_R_or_B', 'kernel_R_at_G_in_RB', 'kernel_R_at_G_in_BR', 'kernel_R_at_B_in_BB']

top_left = (slice(0, None, 2), slice(0, None, 2))
top_right = (slice(0, None, 2), slice(1, None, 2))
bottom_left = (slice(1, None, 2), slice(0, None, 2))
bottom_right = (slice(1, None, 2), slice(1, None, 2))

ErrBadCFA = NotImplementedError('only rggb, bggr bayer patterns currently implemented')

_INT_CODE = {torch.uint8: L.PM_U8, torch.uint16: L.PM_U16, torch.uint32: L.PM_U32}
_FLOATS = (torch.float32, torch.float64)
_f64x4 = ctypes.c_double * 4


def _cfa(cfa):
    code = BP.cfa_code(cfa)
    if code is None:
        raise ErrBadCFA
    return code


def _tensor(a):
    """numpy array or tensor -> a tensor that keeps its dtype and strides (moved to the device by the caller)"""
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))


def _real(a, what):
    """a float32 / float64 device tensor, strides kept; anything else real becomes float64 (complex: TypeError)"""
    t = _tensor(a)
    if t.is_complex():
        raise TypeError(f'{what} must be real')
    t = t.to(L.device())
    if t.dtype not in _FLOATS:
        t = t.to(torch.float64)
    return t


def _planes(r, g1, g2, b):
    ts = [_real(p, 'a color plane') for p in (r, g1, g2, b)]
    dt = torch.float32 if all(t.dtype == torch.float32 for t in ts) else torch.float64
    ts = [t if t.dtype == dt else t.to(dt) for t in ts]
    if any(t.shape != ts[0].shape for t in ts) or ts[0].ndim not in (2, 3):
        raise ValueError('the four color planes must have one shape, (m, n) or (B, m, n)')
    return ts, dt


def _plane_args(t):
    """(pointer, row stride, element stride, batch stride) of a (m, n) or (B, m, n) tensor with non-negative strides"""
    if t.numel() and min(t.stride()) < 0:
        t = t.contiguous()
    s = t.stride()
    return t, [L.ptr(t), s[-2], s[-1], s[0] if t.ndim == 3 else 0]


def _out_view(output, shape, dt):
    if output is None:
        return torch.empty(shape, dtype=dt, device=L.device())
    if not isinstance(output, torch.Tensor) or output.device != L.device() or output.dtype != dt or tuple(output.shape) != tuple(shape):
        raise ValueError(f'output must be a device tensor of shape {tuple(shape)} and dtype {dt}')
    return output


def _weave(mode, r, g1, g2, b, cfa, output):
    code = _cfa(cfa)
    ts, dt = _planes(r, g1, g2, b)
    shape = tuple(ts[0].shape)
    if mode == L.PM_BAYER_RECOMPOSITE:
        shape = shape[:-2] + (2 * shape[-2], 2 * shape[-1])
    out = _out_view(output, shape, dt)
    if out.numel() == 0:
        return out
    ov, ld, bs = _stack_view(out, 'output')
    if ov.data_ptr() != out.data_ptr() or (ov.numel() > 1 and ov.stride(-1) != 1):
        raise ValueError('output must have contiguous rows')
    B, m, n = ov.shape
    keep, args = [], []
    for t in ts:
        t, a = _plane_args(t)
        keep.append(t)
        args += a
    L.check(L.load().pm_bayer_weave(_code(dt), mode, code, B, m, n, *args, L.ptr(ov), ld, bs, L.stream_ptr()))
    return out


def composite_bayer(r, g1, g2, b, cfa='rggb', output=None):
    """Composite an interleaved image from densely sampled color planes (bayer.py:130-171): out takes r, g1, g2, b at the sites of
    their color.  Planes (m, n) or (B, m, n), any strides.  One launch."""
    return _weave(L.PM_BAYER_COMPOSITE, r, g1, g2, b, cfa, output)


def decomposite_bayer(img, cfa='rggb'):
    """The four color planes r, g1, g2, b of a mosaic (bayer.py:174-210) as stride-2 VIEWS of the (device) image: no kernel."""
    code = _cfa(cfa)
    t = _tensor(img).to(L.device())
    a, g1, g2, d = t[..., 0::2, 0::2], t[..., 0::2, 1::2], t[..., 1::2, 0::2], t[..., 1::2, 1::2]
    return (a, g1, g2, d) if code == 0 else (d, g1, g2, a)


def recomposite_bayer(r, g1, g2, b, cfa='rggb', output=None):
    """The reciprocal of decomposite_bayer (bayer.py:213-257): planes (m, n) -> mosaic (2m, 2n).  The views decomposite_bayer returns
    are read where they lie.  One launch."""
    return _weave(L.PM_BAYER_RECOMPOSITE, r, g1, g2, b, cfa, output)


def _mosaic_view(t, what):
    if t.ndim not in (2, 3):
        raise ValueError(f'{what} must be (m, n) or a stack (B, m, n)')
    return _stack_view(t, what)


def demosaic_deinterlace(img, cfa='rggb'):
    """(m, n) -> (m//2, n//2, 3) as r, (g1 + g2) / 2, b (bayer.py:260-282).  m and n even.  One launch."""
    code = _cfa(cfa)
    t = _real(img, 'img')
    shape = tuple(t.shape)
    v, ld, bs = _mosaic_view(t, 'img')
    B, m, n = v.shape
    if m % 2 or n % 2:
        raise ValueError(f'demosaic_deinterlace needs even dimensions, got {(m, n)}')
    out = torch.empty(shape[:-2] + (m // 2, n // 2, 3), dtype=t.dtype, device=t.device)
    if out.numel():
        L.check(L.load().pm_bayer_deinterlace(_code(t.dtype), code, B, m, n, L.ptr(v), ld, bs, L.ptr(out), L.stream_ptr()))
    return out


def demosaic_malvar(img, cfa='rggb', layout='hwc'):
    """Demosaic with the Malvar-He-Cutler filters (bayer.py:378-447): (m, n) -> (m, n, 3) R, G, B; a stack (B, m, n) ->
    (B, m, n, 3) in the same launch.  A float mosaic keeps its dtype; an integer one (the Detector's uint8 / uint16 / uint32 are read
    as stored) gives config.precision.  layout='chw' returns (..., 3, m, n).  The border is scipy's mode='reflect', as in the
    reference: the edge sample is repeated, which breaks the color parity there."""
    code = _cfa(cfa)
    if layout not in ('hwc', 'chw'):
        raise ValueError("layout must be 'hwc' or 'chw'")
    t = _tensor(img)
    if t.is_complex():
        raise TypeError('img must be real')
    t = t.to(L.device())
    if t.dtype in _FLOATS:
        odt, icode = t.dtype, _code(t.dtype)
    else:
        odt = L.torch_dtype(config.precision)
        if t.dtype not in _INT_CODE:
            t = t.to(odt)
        icode = _INT_CODE.get(t.dtype, _code(odt))
    shape = tuple(t.shape)
    v, ld, bs = _mosaic_view(t, 'img')
    B, m, n = v.shape
    oshape = shape[:-2] + ((3, m, n) if layout == 'chw' else (m, n, 3))
    out = torch.empty(oshape, dtype=odt, device=t.device)
    if out.numel():
        L.check(L.load().pm_bayer_demosaic(icode, _code(odt), code, int(layout == 'chw'), B, m, n, L.ptr(v), ld, bs, L.ptr(out),
                                           L.stream_ptr()))
    return out


def _scalable(a, what):
    """the tensor the white balance scales in place: the argument itself when it is a floating device tensor, else a device copy"""
    t = _tensor(a)
    if t.is_complex():
        raise TypeError(f'{what} must be real')
    if t.device != L.device() or t.dtype not in _FLOATS:
        t = t.to(L.device(), torch.float64 if t.dtype not in _FLOATS else t.dtype)
    return t


def _scale(t, classes, code, view, gains, saturation):
    v, ld, bs = view
    B, m, n = v.shape
    if classes == L.PM_BAYER_RGB:
        n //= 3
    lib = L.load()
    maxima = None
    if saturation is not None:
        maxima = torch.empty(4, dtype=torch.float64, device=t.device)
        ws = L.workspace(int(lib.pm_bayer_class_max_workspace()))
        L.check(lib.pm_bayer_class_max(_code(t.dtype), classes, B, m, n, L.ptr(v), ld, bs, L.ptr(maxima), L.ptr(ws), ws.numel(), L.stream_ptr()))
    g = _f64x4(*[float(x) for x in gains], *([1.0] * (4 - len(gains))))
    s = _f64x4(*(list(saturation) + [1.0] * (4 - len(saturation)))) if saturation is not None else None
    L.check(lib.pm_bayer_scale(_code(t.dtype), classes, code, B, m, n, L.ptr(v), ld, bs, g, int(saturation is not None), s, L.ptr(maxima),
                               L.stream_ptr()))
    return t


def wb_prescale(mosaic, wr, wg1, wg2, wb, cfa='rggb', safe=False, saturation=None):
    """White-balance prescaling of a mosaic (bayer.py:13-75): the planes r, g1, g2, b times their gains.  With safe=True all gains
    are first divided by the largest max(plane) * gain / saturation above 1; the maxima and the ratio stay on the device (two
    launches, no host read).  A floating device tensor is scaled IN PLACE and returned; anything else is copied to the device and
    the scaled tensor returned (the reference returns None)."""
    cfa = cfa.lower()
    saturation = BP.check_saturation(safe, saturation, 4)
    code = _cfa(cfa)
    t = _scalable(mosaic, 'mosaic')
    if t.ndim not in (2, 3):
        raise ValueError('mosaic must be (m, n) or a stack (B, m, n)')
    if t.numel() == 0:
        return t
    if safe and (t.shape[-2] < 2 or t.shape[-1] < 2):
        raise ValueError('zero-size array to reduction operation maximum which has no identity')
    view = _stack_view(t, 'mosaic')
    if view[0].data_ptr() != t.data_ptr() or (t.shape[-1] > 1 and view[0].stride(-1) != 1):
        raise ValueError('mosaic must have contiguous rows to be scaled in place')
    return _scale(t, L.PM_BAYER_MOSAIC, code, view, (wr, wg1, wg2, wb), saturation)


def wb_postscale(rgb, wr, wg, wb, safe=False, saturation=None):
    """White-balance post scaling of an (..., 3) image (bayer.py:78-127); safe as in wb_prescale, over the three channels.  A
    contiguous floating device tensor is scaled IN PLACE and returned; anything else is copied to the device first."""
    saturation = BP.check_saturation(safe, saturation, 3)
    t = _scalable(rgb, 'rgb')
    if t.ndim < 2 or t.shape[-1] != 3:
        raise ValueError('rgb must have shape (..., 3)')
    if t.numel() == 0:
        return t
    if not t.is_contiguous():
        raise ValueError('rgb must be contiguous to be scaled in place')
    rows = t.numel() // (3 * t.shape[-2])
    v = t.view(1, rows, 3 * t.shape[-2])
    return _scale(t, L.PM_BAYER_RGB, 0, (v, v.shape[2], v.shape[1] * v.shape[2]), (wr, wg, wb), saturation)


def assemble_superresolved(r, g1, g2, b, zoomfactor, cfa='rggb', out=None):
    """Assemble a trichromatic image from super-resolved color planes (bayer.py:285-336): r, b and g2 are moved onto g1's grid by
    Fourier shifts of zoomfactor samples -- fft2, the separable multiplier of ndimage.fourier_shift (exp(-2 pi i shift f), f =
    fftfreq(N) per axis) and ifft2 in one _ops.fft2_mul_ifft2 each -- then one sweep stores r', (g2' + g1) / 2, b' as (m, n, 3)."""
    if cfa != 'rggb':
        raise NotImplementedError('assemble_superresolved: only rggb patterns supported at this time')
    ts, dt = _planes(r, g1, g2, b)
    if ts[0].ndim != 2:
        raise ValueError('the color planes must be (m, n)')
    m, n = ts[0].shape
    res = _out_view(out, (m, n, 3), dt)
    if not res.is_contiguous():
        raise ValueError('out must be contiguous')
    shifts = BP.superres_shifts(zoomfactor)
    f = [torch.fft.fftfreq(k, dtype=torch.float64, device=res.device) for k in (m, n)]
    cdt = L._COMPLEX_OF[dt]

    def moved(p, shift):
        hy, hx = (torch.polar(torch.ones_like(fk), (-2 * np.pi * float(s)) * fk).to(cdt) for fk, s in zip(f, shift))
        return _ops.fft2_mul_ifft2(p.contiguous(), scale=1.0 / (m * n), mul=hy, mul_x=hx).real

    rp, bp, g2p = moved(ts[0], shifts['r']), moved(ts[3], shifts['b']), moved(ts[2], shifts['g2'])
    keep, args = [], []
    for t in (rp, ts[1], g2p, bp):
        t, a = _plane_args(t)
        keep.append(t)
        args += a
    L.check(L.load().pm_bayer_assemble(_code(dt), 1, m, n, *args, L.ptr(res), L.stream_ptr()))
    return res
