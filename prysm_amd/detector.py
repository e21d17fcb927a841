"""The detector on the device (prysm/detector.py): bindown, tile, and Detector.expose as one fused kernel.

The reference's names, signatures, argument checks and error types; inputs numpy arrays or torch tensors, results torch tensors on
the device.  bindown / tile are one launch each (pm_bindown, pm_tile) with a fixed summation order, so results are bitwise
reproducible.  Detector.expose is one launch (pm_detector_expose) that computes the Poisson mean and the sampler's constants once
per pixel, loops over the frames and stores every sample once, in its final width.  prysm_amd/detector_plan.py restates the kernels
in numpy.

New beyond the reference: `seed=` / Detector.seed(n) / Detector.seed_value (the noise is a pure function of seed, exposure index,
frame and pixel), Detector.digitize (the deterministic tail alone), Detector.mean_electrons (the mean the sampler sees).
"""
import numbers
import os

import numpy as np
import torch

from . import _lib as L
from . import detector_plan as DP
from .coordinates import _real_dtype, _code

__all__ = ['apply_lut', 'Detector', 'olpf_ft', 'pixel_ft', 'pixel', 'bindown', 'tile']


def _index(img):
    """an integer tensor as gather indices (torch indexes with int32 / int64)"""
    return img.to(torch.int64)


def apply_lut(img, lut):
    """lut[img] (detector.py:8-26): img an array of an unsigned integer dtype, lut a 1-D table.  A thin torch gather."""
    img, lut = L.as_device(img), L.as_device(lut)
    return torch.take(lut, _index(img))


def _stack_view(t, what):
    """a real tensor of (..., m, n) as (B, m, n) with the strides the kernels take: last dimension contiguous, rows and members strided"""
    if t.ndim < 2:
        raise ValueError(f'{what} must have at least two dimensions')
    if t.ndim == 2:
        v = t.unsqueeze(0)
    elif t.ndim == 3:
        v = t
    else:
        v = t.reshape((-1,) + tuple(t.shape[-2:]))
    B, m, n = v.shape
    ok = (n <= 1 or v.stride(2) == 1) and (m <= 1 or v.stride(1) >= n) and (B <= 1 or v.stride(0) >= m * max(v.stride(1), n))
    if not ok or (v.numel() and min(v.stride()) < 0):
        v = v.contiguous()
    ld = v.stride(1) if m > 1 else n
    bs = v.stride(0) if B > 1 else m * ld
    return v, int(ld), int(bs)


def _to_device(a, dt):
    """like _lib.as_device, but a strided tensor keeps its strides (the kernels read them)"""
    dev = L.device()
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.device != dev:
        t = t.to(dev)
    if t.dtype != dt:
        t = t.to(dt)
    if t.is_conj() or t.is_neg():
        t = t.resolve_conj().resolve_neg()
    return t


def bindown(array, factor, mode='avg'):
    """Bin an array by `factor` (detector.py:222-274): an int (every axis) or one factor per axis; a stack (B, m, n) takes
    [1, fy, fx].  mode 'avg' / 'average' / 'mean' or 'sum'.  One launch; each bin is one running sum in the array's precision, in a
    fixed order.  A shape that is not a multiple of the factors raises ValueError before any launch."""
    shape = tuple(array.shape)
    fy, fx = DP.factors_of(shape, factor)
    mode = DP.bin_mode(mode)
    m, n = shape[-2:]
    if m % fy or n % fx:
        raise ValueError(f'cannot bin an array of shape {shape} by {(fy, fx)}: not a multiple')
    dt = _real_dtype(array, what='bindown input')
    v, ld, bs = _stack_view(_to_device(array, dt), 'array')
    B = v.shape[0]
    out = torch.empty((B, m // fy, n // fx), dtype=dt, device=v.device)
    L.check(L.load().pm_bindown(_code(dt), B, m // fy, n // fx, fy, fx, L.PM_BIN_AVG if mode == 'avg' else L.PM_BIN_SUM, L.ptr(v), ld, bs,
                                L.ptr(out), n // fx, (m // fy) * (n // fx), L.stream_ptr()))
    return out.reshape(shape[:-2] + (m // fy, n // fx))


def tile(array, factor, scaling='sum'):
    """Repeat every element `factor` times along each axis (detector.py:277-339), the adjoint of bindown: scaling 'sum' multiplies by
    1 / prod(factor) (the adjoint of bindown 'avg'), 'avg' by 1 (the adjoint of bindown 'sum').  One launch."""
    shape = tuple(array.shape)
    fy, fx = DP.factors_of(shape, factor)
    if scaling == 'sum':
        sf = 1 / (fy * fx)
    elif scaling in ('avg', 'average', 'mean'):
        sf = 1.0
    else:
        raise ValueError('scaling must be average or sum')
    m, n = shape[-2:]
    dt = _real_dtype(array, what='tile input')
    v, ld, bs = _stack_view(_to_device(array, dt), 'array')
    B = v.shape[0]
    out = torch.empty((B, m * fy, n * fx), dtype=dt, device=v.device)
    L.check(L.load().pm_tile(_code(dt), B, m, n, fy, fx, float(sf), L.ptr(v), ld, bs, L.ptr(out), n * fx, m * fy * n * fx, L.stream_ptr()))
    return out.reshape(shape[:-2] + (m * fy, n * fx))


class Detector:
    """Model of a detector (detector.py:29-148) whose exposure is one fused kernel.

    Differences from the reference, all deliberate:
    - The noise is a pure function of (seed, exposure index, frame, pixel): Philox4x32-10 counters, not a global generator.  The
      exposure index counts the frames this Detector has exposed since seed(); it lives on the device and advances there, so
      expose(img, frames=F) equals F successive expose(img) calls bit for bit, and a captured graph draws fresh frames per replay.
      seed=None takes 64 bits from os.urandom and keeps them in seed_value, so any run can be repeated.
    - The Poisson mean is computed in fp64 whatever the image's dtype (the reference keeps a float32 image's products in float32).
    - numpy raises ValueError for a negative or NaN mean before it draws.  Here the kernel sets a flag in a device status word;
      expose(..., validate=True) (the default) reads it back after the launch (one host synchronisation) and raises ValueError; with
      validate=False, and always under graph capture, such pixels get zero shot electrons and no host read happens.
    """

    def __init__(self, dark_current, read_noise, bias, fwc, conversion_gain, bits, exposure_time, prnu=None, dcnu=None, lut=None,
                 seed=None):
        self.dark_current = dark_current
        self.read_noise = read_noise
        self.bias = bias
        self.fwc = fwc
        self.conversion_gain = conversion_gain
        self.bits = bits
        self.exposure_time = exposure_time
        self.prnu = prnu
        self.dcnu = dcnu
        self.lut = lut
        self._state = None
        self._maps = {}
        self.seed(seed)

    def seed(self, n=None):
        """Restart the noise sequence from seed n (None: 64 bits of host entropy); the exposure index returns to 0."""
        if n is None:
            n = int.from_bytes(os.urandom(8), 'little')
        if not isinstance(n, numbers.Integral):
            raise TypeError('the seed must be an integer')
        self.seed_value = int(n) & 0xFFFFFFFFFFFFFFFF
        if self._state is not None:
            self._state.zero_()
        return self

    # ---- device-side pieces
    def _device_state(self):
        if self._state is None or self._state.device != L.device():
            self._state = torch.zeros(2, dtype=torch.int64, device=L.device())
        return self._state

    @property
    def exposure_index(self):
        """frames exposed since seed() (a host read of the device state: it synchronises)"""
        return 0 if self._state is None else int(self._state[0].item())

    def _map(self, name, shape):
        """prnu / dcnu as a contiguous fp64 device map of the image's shape (cached per source object)"""
        src = getattr(self, name)
        if src is None:
            return None
        hit = self._maps.get(name)
        if hit is None or hit[0] is not src or hit[1].device != L.device():
            t = L.as_device(src, torch.float64)
            hit = self._maps[name] = (src, t)
        t = hit[1]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{name} has shape {tuple(t.shape)}, the image {tuple(shape)}')
        return t

    def _tail(self):
        """(lut tensor or None, lut length, bytes per output element, torch dtype of the output)"""
        if self.bits > 32:
            raise ValueError("numpy's random functionality is inadequate for > 32 unsigned bits")
        if self.bits < 1:
            raise ValueError('bits must be at least 1')
        if self.lut is not None:
            hit = self._maps.get('lut')
            if hit is None or hit[0] is not self.lut or hit[1].device != L.device():
                t = L.as_device(self.lut)
                if t.ndim != 1:
                    raise ValueError('lut must be 1-dimensional')
                hit = self._maps['lut'] = (self.lut, t)
            lut = hit[1]
            if lut.numel() < 2 ** self.bits:
                raise ValueError(f'lut has {lut.numel()} entries, a {self.bits}-bit ADC needs {2 ** self.bits}')
            if lut.element_size() not in (1, 2, 4, 8) or lut.is_complex():
                raise TypeError(f'lut dtype {lut.dtype} is not supported')
            return lut, lut.numel(), lut.element_size(), lut.dtype
        odt = torch.uint8 if self.bits <= 8 else torch.uint16 if self.bits <= 16 else torch.uint32
        return None, 0, torch.empty((), dtype=odt).element_size(), odt

    def _signed_seed(self):
        s = self.seed_value
        return s - (1 << 64) if s >= (1 << 63) else s

    # ---- the public pieces
    def mean_electrons(self, aerial_img):
        """The Poisson mean per pixel, img * t * prnu + dark * t * dcnu in fp64 (thin torch calls; expose computes it in its kernel)."""
        _real_dtype(aerial_img, what='aerial_img')
        img = L.as_device(aerial_img, torch.float64)
        e = img * float(self.exposure_time)
        prnu, dcnu = self._map('prnu', img.shape[-2:]), self._map('dcnu', img.shape[-2:])
        if prnu is not None:
            e = e * prnu
        d = float(self.dark_current) * float(self.exposure_time)
        if dcnu is not None:
            d = d * dcnu
        return e + d

    def digitize(self, electrons):
        """The deterministic tail of an exposure on electrons the caller brings (any shape (..., m, n), fp32 / fp64, strided): + bias,
        clip at fwc, * (1 / conversion_gain), clip to [0, 2**bits - 1], truncating cast, LUT; computed in fp64.  One launch."""
        lut, lut_len, obytes, odt = self._tail()
        dt = _real_dtype(electrons, what='electrons')
        t = _to_device(electrons, dt)
        shape = tuple(t.shape)
        v, ld, bs = _stack_view(t, 'electrons')
        B, m, n = v.shape
        out = torch.empty(shape, dtype=odt, device=v.device)
        L.check(L.load().pm_detector_digitize(_code(dt), B, m, n, L.ptr(v), ld, bs, float(self.bias), float(self.fwc),
                                              float(self.conversion_gain), int(self.bits), L.ptr(lut), lut_len, obytes, L.ptr(out),
                                              L.stream_ptr()))
        return out

    def expose(self, aerial_img, frames=1, validate=True, pixel_offset=0):
        """Form `frames` exposures of an aerial image in e-/sec (detector.py:83-148): (m, n) or a stack (B, m, n), fp32 / fp64,
        strided.  Returns (frames, *aerial_img.shape) DN, the first dimension squeezed when frames == 1; dtype uint8 / uint16 /
        uint32 by `bits`, or the LUT's.  ValueError above 32 bits.

        validate: read the status word back and raise ValueError when a mean was negative, NaN or infinite (the class docstring).
        pixel_offset: added to the row-major pixel index that addresses the noise stream; member b of a stack exposed by itself with
        pixel_offset=b * m * n (and the same seed and exposure index) gives the frames it has inside the stack."""
        lut, lut_len, obytes, odt = self._tail()
        frames = int(frames)
        if frames < 1:
            raise ValueError('frames must be at least 1')
        dt = _real_dtype(aerial_img, what='aerial_img')
        t = _to_device(aerial_img, dt)
        shape = tuple(t.shape)
        if t.ndim not in (2, 3):
            raise ValueError('aerial_img must be (m, n) or a stack (B, m, n)')
        v, ld, bs = _stack_view(t, 'aerial_img')
        B, m, n = v.shape
        prnu, dcnu = self._map('prnu', (m, n)), self._map('dcnu', (m, n))
        state = self._device_state()
        out = torch.empty((frames,) + shape, dtype=odt, device=v.device)
        validate = validate and not torch.cuda.is_current_stream_capturing()
        if validate:
            state[1:].zero_()           # what an earlier unvalidated call may have left
        L.check(L.load().pm_detector_expose(_code(dt), B, m, n, L.ptr(v), ld, bs, L.ptr(prnu), L.ptr(dcnu), float(self.exposure_time),
                                            float(self.dark_current), float(self.read_noise), float(self.bias), float(self.fwc),
                                            float(self.conversion_gain), int(self.bits), L.ptr(lut), lut_len, obytes, frames,
                                            self._signed_seed(), int(pixel_offset), L.ptr(state), L.ptr(out), L.stream_ptr()))
        if validate:
            if int(state[1].item()):
                raise ValueError('the aerial image gives a negative, NaN or infinite mean number of electrons')
        return out[0] if frames == 1 else out


def olpf_ft(fx, fy, width_x, width_y):
    """Analytic FT of an optical low-pass filter (detector.py:151-171): cos(2 wx fx) cos(2 wy fy).  Thin torch calls."""
    dt = _real_dtype(fx, fy, what='frequencies')
    fx, fy = L.as_device(fx, dt), L.as_device(fy, dt)
    return torch.cos(2 * width_x * fx) * torch.cos(2 * width_y * fy)


def pixel_ft(fx, fy, width_x, width_y):
    """Analytic FT of a rectangular pixel aperture (detector.py:174-194): sinc(fx wx) sinc(fy wy).  Thin torch calls."""
    dt = _real_dtype(fx, fy, what='frequencies')
    fx, fy = L.as_device(fx, dt), L.as_device(fy, dt)
    return torch.sinc(fx * width_x) * torch.sinc(fy * width_y)


def _olpf_spec(width_x, width_y):
    """The deferred form of olpf_ft for convolution.apply_transfer_functions / transfer_function: records only, no device work."""
    from .imagechain_plan import olpf_spec
    return olpf_spec(width_x, width_y)


def _pixel_spec(width_x, width_y):
    """The deferred form of pixel_ft for convolution.apply_transfer_functions / transfer_function: records only, no device work."""
    from .imagechain_plan import pixel_spec
    return pixel_spec(width_x, width_y)


olpf_ft.spec = _olpf_spec
pixel_ft.spec = _pixel_spec


def pixel(x, y, width_x, width_y):
    """Spatial representation of a pixel (detector.py:197-219): a torch.bool mask of |x| <= wx / 2 and |y| <= wy / 2."""
    dt = _real_dtype(x, y, what='coordinates')
    x, y = L.as_device(x, dt), L.as_device(y, dt)
    width_x = width_x / 2
    width_y = width_y / 2
    return (x <= width_x) & (x >= -width_x) & (y <= width_y) & (y >= -width_y)
