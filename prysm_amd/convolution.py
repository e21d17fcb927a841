"""Numerical convolution (prysm/convolution.py) -- SURVEY 8(f) ranks 1 and 4.

conv = fftshift(ifft2(fft2(ifftshift(o)) * fft2(ifftshift(h)))): one fused pm_fft2 for H, then the fused
3-pass fft2 -> x H -> ifft2 chain; the shifts are index rotations, the product with H happens in registers between
the two column transforms and the 1/(MN) rides on the last store.  Real objects / PSFs / actuator maps are read as
they are (PM_FLAG_REAL_INPUT), and a real object's result -- the reference keeps its real part -- comes out of a chain that runs on
half spectra end to end (PM_FLAG_REAL_OUTPUT, csrc/fft_c2r.h) for unpadded power-of-two sizes.  apply_transfer_functions is the same chain with the product of the given
transfer functions as H (the DM surface render of prysm/x/dm.py:254,330).

Analytic transfer functions have a deferred form -- `detector.pixel_ft.spec(wx, wy)`, `detector.olpf_ft.spec`,
`degradations.smear_ft.spec`, `degradations.jitter_ft.spec`, `objects.pinhole_ft.spec`, `objects.slit_ft.spec`, `psf.airydisk_ft.spec`:
small records, no device work.  When `tfs` holds only such records and arrays, apply_transfer_functions builds H with ONE launch
(pm_tf_product, csrc/imagechain.hip: the frequencies generated in the kernel as forward_ft_unit makes them, no fr / ft maps, every
factor multiplied in registers, the ifftshift an index rotation, H stored once in the chain's dtype) and hands it to the chain
unchanged.  transfer_function returns that H for callers who reuse it across frames.  With a plain callable among `tfs` the map-by-map
path below runs as before.
"""
import inspect

import numpy as np
import torch

from . import _lib as L
from . import _ops
from . import imagechain_plan as IP
from .conf import config
from .fttools import forward_ft_unit


def _match(o, h):
    """Bring two fields to one precision (numpy result type)."""
    co, ch = L.cdtype_of(o), L.cdtype_of(h)
    if co != ch:
        if torch.complex128 in (co, ch):
            o = o.to(torch.complex128 if o.is_complex() else torch.float64)
            h = h.to(torch.complex128 if h.is_complex() else torch.float64)
    return o, h


def conv(obj, psf):
    """Convolve an object and psf (arrays of the same shape) (convolution.py:9-31)."""
    o = L.as_field(obj)
    real = not o.is_complex()
    h = L.as_field(psf)
    o, h = _match(o, h)
    M, N = o.shape
    shift = (M // 2, N // 2)
    H = _ops.fft2(h, direction=-1, scale=1.0, in_shift=shift)
    # a real object keeps the real part: the chain then runs on half spectra end to end where the shapes allow (PM_FLAG_REAL_OUTPUT)
    return _ops.fft2_mul_ifft2(o, scale=1.0 / (M * N), mul=H, in_shift=shift, out_shift=shift, real_out=real)


def _ifftshift2(t):
    return torch.roll(t, shifts=(-(t.shape[0] // 2), -(t.shape[1] // 2)), dims=(0, 1))


def _is_double(a):
    dt = a.dtype if isinstance(a, torch.Tensor) else L.torch_dtype(np.asarray(a).dtype)
    return dt in (torch.float64, torch.complex128)


def _working_dtype(tfs, fx, fy, *others):
    """the REAL precision of a fused product, by the rule of the map-by-map path: double as soon as an array, a given frequency vector
    or -- for generated frequencies -- config.precision is double"""
    arrays = [tf for tf in tfs if not isinstance(tf, IP.Spec)] + [v for v in (fx, fy) if v is not None] + list(others)
    generated = (fx is None or fy is None) and any(isinstance(tf, IP.Spec) for tf in tfs)
    double = any(_is_double(a) for a in arrays) or (generated and L.torch_dtype(config.compute_precision) == torch.float64)
    return torch.float64 if double else torch.float32


def _fused_product(shape, dx, tfs, fx, fy, shift, rdt, real_out=False):
    M, N = shape
    if fx is None and fy is None:
        return _ops.tf_product((M, N), tfs, rdt, dx=dx, shift=shift, real_out=real_out)
    # a given axis next to a generated one: the generated one as forward_ft_unit's vector (tiny), so that both are read as vectors
    ux = L.as_device(forward_ft_unit(dx, N, shift=shift) if fx is None else fx)
    uy = L.as_device(forward_ft_unit(dx, M, shift=shift) if fy is None else fy)
    if ux.numel() == N and uy.numel() == M:
        ux, uy = ux.reshape(-1).to(rdt), uy.reshape(-1).to(rdt)
    elif ux.dim() == 2 and uy.dim() == 2 and ux.shape[0] != 1:        # meshgrids: optimize_xy_separable reads their first lines
        ux, uy = ux[0, :].to(rdt), uy[:, 0].to(rdt)
    return _ops.tf_product((M, N), tfs, rdt, fx=ux, fy=uy, shift=shift, real_out=real_out)


def transfer_function(shape, dx, tfs, shift=False, dtype=None, fx=None, fy=None):
    """H = the product of the transfer functions `tfs` -- `.spec(...)` records and arrays of `shape` -- with its origin at sample
    [0, 0], built in one launch: what apply_transfer_functions multiplies into the spectrum, for reuse across frames (pass it back as
    `apply_transfer_functions(obj, dx, [H])`).  shift: arrays (and fx, fy) are centred.  dtype: torch.complex64 / complex128, or
    float32 / float64 for the real part on request; the default is the complex type apply_transfer_functions would use.  Not in the
    reference."""
    if not isinstance(shape, tuple):
        shape = (shape, shape)
    tfs = list(tfs)
    if any(callable(tf) for tf in tfs):
        raise TypeError('transfer_function takes .spec(...) records and arrays; a plain callable cannot be fused')
    rdt = _working_dtype(tfs, fx, fy)
    real_out = False
    if dtype is not None:
        dtype = L.torch_dtype(dtype)
        if dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
            raise TypeError('dtype must be float32, float64, complex64 or complex128')
        real_out = not dtype.is_complex
        rdt = torch.float32 if dtype in (torch.float32, torch.complex64) else torch.float64
    return _fused_product(shape, dx, tfs, fx, fy, shift, rdt, real_out=real_out)


def apply_transfer_functions(obj, dx, tfs, fx=None, fy=None, ft=None, fr=None, shift=False):
    """Blur an object by N transfer functions (convolution.py:34-113).

    tfs: arrays, or callables taking any of fx, fy, fr, ft (frequency grids on the device).  With shift=False the
    transfer functions have their origin at sample [0, 0]; with shift=True at the centre of the array.
    """
    o = L.as_field(obj)
    real = not o.is_complex()
    M, N = o.shape
    tfs = list(tfs)
    if ft is None and fr is None and any(isinstance(tf, IP.Spec) for tf in tfs) and not any(callable(tf) for tf in tfs):
        rdt = _working_dtype(tfs, fx, fy, o)
        H = _fused_product((M, N), dx, tfs, fx, fy, shift, rdt)
        if rdt == torch.float64 and L.cdtype_of(o) != torch.complex128:
            o = o.to(torch.complex128 if o.is_complex() else torch.float64)
        sh = (M // 2, N // 2)
        return _ops.fft2_mul_ifft2(o, scale=1.0 / (M * N), mul=H, in_shift=sh, out_shift=sh, real_out=real)
    if any(callable(tf) or isinstance(tf, IP.Spec) for tf in tfs):
        if fx is None or fy is None:
            uy, ux = [L.as_device(forward_ft_unit(dx, n, shift=shift)) for n in o.shape]
            fx = ux if fx is None else fx
            fy = uy if fy is None else fy
        fx, fy = L.as_device(fx), L.as_device(fy)
        if fx.dim() == 1 or (fx.dim() == 2 and fx.shape[0] != 1 and fy.dim() == 1):   # optimize_xy_separable
            fx, fy = fx.reshape(1, -1), fy.reshape(-1, 1)
        computed_fr, computed_ft = torch.hypot(fx, fy), torch.atan2(fy + 0 * fx, fx + 0 * fy)   # cart_to_polar
        fr = computed_fr if fr is None else L.as_device(fr)
        ft = computed_ft if ft is None else L.as_device(ft)
    cd = L.cdtype_of(o)
    H = None
    for tf in tfs:
        if callable(tf):
            params = inspect.signature(tf).parameters
            kwargs = {k: v for k, v in (('fx', fx), ('fy', fy), ('fr', fr), ('ft', ft)) if k in params}
            if not kwargs:
                raise ValueError(f'{tf} accepts none of fx, fy, fr, ft; a transfer function must accept at least one')
            tf = tf(**kwargs)
        elif isinstance(tf, IP.Spec):       # a record next to a plain callable: its map, from the same frequencies
            tf = _ops.tf_product((M, N), [tf], fr.dtype, fx=torch.broadcast_to(fx, (M, N)), fy=torch.broadcast_to(fy, (M, N)),
                                 fr=torch.broadcast_to(fr, (M, N)), real_out=True)
        tf = L.as_device(tf)
        if tf.dtype == torch.complex128 or tf.dtype == torch.float64:
            if cd == torch.complex64:
                cd = torch.complex128
        tf = torch.broadcast_to(tf, (M, N)) if tuple(tf.shape) != (M, N) else tf
        H = tf if H is None else H * tf
    if H is None:
        H = torch.ones((M, N), dtype=cd, device=o.device)
    H = H.to(cd)
    if cd == torch.complex128 and L.cdtype_of(o) != cd:
        o = o.to(torch.complex128 if o.is_complex() else torch.float64)
    if shift:
        H = _ifftshift2(H)      # centred transfer functions -> origin at [0, 0]
    sh = (M // 2, N // 2)
    return _ops.fft2_mul_ifft2(o, scale=1.0 / (M * N), mul=H.contiguous(), in_shift=sh, out_shift=sh, real_out=real)
