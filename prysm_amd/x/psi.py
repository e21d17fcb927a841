"""Phase Shifting Interferometry on the device (prysm/x/psi.py).

Scheme, ZYGO_THIRTEEN_FRAME, SCHWIDER and design_scheme are host numpy, as in the reference (psi.py:16-28, 112-157): a scheme is a
handful of numbers.  psi_accumulate and degroot_formalism_psi (psi.py:45-71, 74-109) are ONE launch of pm_psi (csrc/sensors.hip):
every frame is read once where it lies -- separately allocated frames are not stacked -- and the numerator, the denominator and
atan2 of them are formed in registers.  The reference reads the frames twice through two sum_of_2d_modes calls, writes and re-reads
both sums, then takes arctan2.

Frames: float32, float64, uint8 or uint16, arrays or RichData (RichData in gives RichData out).  The scheme's weights are read on the
host when the call is made, as polynomials.sum_of_2d_modes documents.

Deliberate departure: every frame dtype is accumulated in double and rounded once, so integer camera frames give the right phase.
The reference casts the weights to the frames' dtype, where the negative weights of SCHWIDER and ZYGO_THIRTEEN_FRAME wrap in uint16
and the phase is off by up to pi.  Float frames give results in their own dtype, integer frames in config.precision.

unwrap_phase (psi.py:160-194) is what the reference makes it: a host wrapper around scikit-image's unwrap_2d, imported inside the
function so that this module imports without scikit-image.
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L
from .. import _ops
from .._richdata import RichData
from ..conf import config
from . import sensors_plan as SP

__all__ = ['Scheme', 'ZYGO_THIRTEEN_FRAME', 'SCHWIDER', 'psi_accumulate', 'degroot_formalism_psi', 'design_scheme', 'unwrap_phase']

Scheme = namedtuple('Scheme', ['shifts', 's', 'c'])


def _fftrange(n):
    return np.arange(-(n // 2), -(n // 2) + n)


ZYGO_THIRTEEN_FRAME = Scheme(
    _fftrange(13) * np.pi / 4,
    np.asarray((-3, -4, 0, 12, 21, 16, 0, -16, -21, -12, 0, 4, 3)),
    np.asarray((0, -4, -12, -12, 0, 16, 24, 16, 0, -12, -12, -4, 0)),
)

SCHWIDER = Scheme(
    _fftrange(5) * np.pi / 2,
    np.asarray((0, 2, 0, -2, 0)),
    np.asarray((-1, 0, 2, 0, -1)),
)

_FRAME_TORCH = (torch.float32, torch.float64, torch.uint8, torch.uint16)


def _frames(gs):
    """the frames as device tensors of one shape, dtype and row stride, each where it lies when it can be read there"""
    if isinstance(gs, (torch.Tensor, np.ndarray)):
        if gs.ndim != 3:
            raise ValueError(f'frames must be a sequence of 2-D images or a (K, rows, cols) array, got shape {tuple(gs.shape)}')
        gs = [gs[k] for k in range(gs.shape[0])]
    gs = [g.data if isinstance(g, RichData) else g for g in gs]
    K = len(gs)
    if not 1 <= K <= SP.MAX_FRAMES:
        raise ValueError(f'{K} frames: between 1 and {SP.MAX_FRAMES} are taken')
    ts = [L.as_device(g) if not (isinstance(g, torch.Tensor) and g.device == L.device()) else g for g in gs]
    dt = ts[0].dtype
    if dt not in _FRAME_TORCH:
        raise TypeError(f'frames must be float32, float64, uint8 or uint16, got {dt}')
    shape = tuple(ts[0].shape)
    if len(shape) != 2:
        raise ValueError(f'a frame must be a 2-D image, got shape {shape}')
    for t in ts:
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError('the frames differ in shape or dtype')
    ts = [_ops._rows2d(t.resolve_conj().resolve_neg() if (t.is_conj() or t.is_neg()) else t) for t in ts]
    ld = ts[0].stride(0)
    if shape[0] > 1 and any(t.stride(0) != ld for t in ts):
        ts = [t.contiguous() for t in ts]
    return ts


def _accumulate(gs, scheme, want):
    ts = _frames(gs)
    s, c = SP.check_scheme(len(ts), scheme.s, scheme.c)
    odt = ts[0].dtype if ts[0].dtype.is_floating_point else L.torch_dtype(config.compute_precision)
    return _ops.psi(ts, s, c, odt, want)


def psi_accumulate(gs, scheme):
    """Accumulate the numerator (sine) and denominator (cosine) for PSI reconstruction (psi.py:45-71): sum_k s[k] g_k and
    sum_k c[k] g_k in one pass over the frames.  RichData frames give RichData sums."""
    num, den, _ = _accumulate(gs, scheme, (True, True, False))
    if isinstance(gs[0], RichData):
        return RichData(num, gs[0].dx, gs[0].wavelength), RichData(den, gs[0].dx, gs[0].wavelength)
    return num, den


def degroot_formalism_psi(gs, scheme):
    """Peter de Groot's formalism for PSI algorithms (psi.py:74-109): the wrapped phase arctan2(sum s g, sum c g) in one launch;
    neither sum is stored.  RichData frames give RichData."""
    _, _, out = _accumulate(gs, scheme, (False, False, True))
    if isinstance(gs[0], RichData):
        return RichData(out, gs[0].dx, gs[0].wavelength)
    return out


def design_scheme(N, stepsize=None, window=None):
    """Design a new PSI scheme (psi.py:112-157): shifts = fftrange(N) stepsize (2 pi / (N - 1) by default), s and c their sine and
    cosine times the window -- None, an array, or the name of a scipy.signal window (sym=False).  Host numpy."""
    if stepsize is None:
        stepsize = (2 * np.pi) / (N - 1)
    shifts = _fftrange(N) * stepsize
    s = np.sin(shifts)
    c = np.cos(shifts)
    if window is not None:
        if isinstance(window, str):
            from scipy import signal
            window = signal.windows.get_window(window, N)
        s *= window
        c *= window
    return Scheme(shifts, s, c)


def unwrap_phase(wrapped, mask):
    """Unwrap a 2-D array of phase wrapped at pi (psi.py:160-194): a host wrapper around scikit-image's unwrap_2d (the data makes a
    round trip through host memory; this is not a hot path).  mask: boolean, True where the data is to be ignored, or None."""
    try:
        from skimage.restoration._unwrap_2d import unwrap_2d as sk_unwrap
    except ImportError as exc:
        raise ImportError('unwrap_phase needs scikit-image (skimage.restoration), which is not installed') from exc
    from ..mathops import array_to_true_numpy
    was_rd = isinstance(wrapped, RichData)
    w0 = wrapped
    if was_rd:
        wrapped = wrapped.data
    w = np.ascontiguousarray(array_to_true_numpy(wrapped) if isinstance(wrapped, torch.Tensor) else wrapped, dtype=np.float64)
    mask2 = np.zeros(w.shape, dtype=np.uint8, order='C')
    if mask is not None:
        mask2[np.asarray(array_to_true_numpy(mask) if isinstance(mask, torch.Tensor) else mask, dtype=bool)] = 255
    out = np.empty(w.shape, dtype=np.float64, order='C')
    sk_unwrap(w, mask2, out, wrap_around=[False, False], seed=None)
    if isinstance(w0.data if was_rd else w0, torch.Tensor):
        out = L.as_device(out)
    if was_rd:
        out = RichData(out, w0.dx, w0.wavelength)
    return out
