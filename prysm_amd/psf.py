"""Evaluation routines for point spread functions on the device (prysm/psf.py).

  airydisk, airydisk_efield, airydisk_ft   one launch of pm_tf_product each (csrc/imagechain.hip), jinc from the unit's own J1 series;
                            `airydisk_ft.spec(fno, wavelength)` is the deferred form for convolution.apply_transfer_functions.
                            airydisk_ft does not clip the caller's array (the reference assigns s[s > 1] = 1 in place).
  centroid_device, centroid sum d, sum row d, sum col d in double: two launches, a fixed summation order, no atomics -- bit-reproducible
                            and capturable.  centroid_device returns the (row, col) 2-vector on the device; centroid reads it and
                            returns Python floats like the reference.
  autocrop                  centroid, int() truncation as the reference does, then ONE launch that writes the px x px window, zero
                            where it leaves the array (no pad-then-slice).
  estimate_size, fwhm, one_over_e, one_over_e_sq   the resample (coordinates.uniform_cart_to_polar), the maximum of the POLAR map, one
                            launch that finds each row's first or last crossing with one wavefront per row, one that averages them:
                            no Python loop over rows, one host read of (mean, count) at the end.

Precision: coordinates._real_dtype's rule on the array arguments, not the reference's mixed casts (its resample runs in float64 whatever
the data's precision).
"""
import numpy as np
import torch

from . import _lib as L
from . import _ops
from . import imagechain_plan as IP
from .coordinates import _real_dtype, uniform_cart_to_polar
from .objects import _eager

__all__ = ['FIRST_AIRY_ZERO', 'SECOND_AIRY_ZERO', 'THIRD_AIRY_ZERO', 'FIRST_AIRY_ENCIRCLED', 'SECOND_AIRY_ENCIRCLED', 'THIRD_AIRY_ENCIRCLED',
           'AIRYDATA', 'estimate_size', 'fwhm', 'one_over_e', 'one_over_e_sq', 'centroid', 'centroid_device', 'autocrop', 'airydisk',
           'airydisk_efield', 'airydisk_ft']

FIRST_AIRY_ZERO = 1.220
SECOND_AIRY_ZERO = 2.233
THIRD_AIRY_ZERO = 3.238
FIRST_AIRY_ENCIRCLED = 0.8377850436212378
SECOND_AIRY_ENCIRCLED = 0.9099305350850819
THIRD_AIRY_ENCIRCLED = 0.9376474743695488

AIRYDATA = {
    1: (FIRST_AIRY_ZERO, FIRST_AIRY_ENCIRCLED),
    2: (SECOND_AIRY_ZERO, SECOND_AIRY_ENCIRCLED),
    3: (THIRD_AIRY_ZERO, THIRD_AIRY_ENCIRCLED)
}


def _data2d(data):
    dt = _real_dtype(data, what='data')
    if len(np.shape(data)) != 2:
        raise ValueError(f'data must be 2-D, got shape {tuple(np.shape(data))}')
    return _ops._rows(data, dt)[0]


def estimate_size(data, metric, dx=None, x=None, y=None, criteria='last'):
    """The radius at which, on average over the azimuth, data crosses a metric (psf.py:27-90): 'fwhm', '1/e', '1/e^2' (fractions of the
    maximum of the polar map) or a number (an absolute level); criteria 'first' or 'last' picks the crossing.  x, y: 1-D sample
    coordinates, which supersede dx.  An unknown metric or criteria raises ValueError before any launch; a metric that no row crosses
    raises the reference's ValueError after the one host read."""
    relative, value = IP.size_threshold(metric)
    last = IP.size_criteria(criteria)
    d = _data2d(data)
    if x is None and y is None:
        if dx is None:
            raise ValueError('estimate_size needs dx, or x and y')
        npdt = np.float32 if d.dtype == torch.float32 else np.float64
        y, x = ((np.arange(s) - s // 2).astype(npdt) * dx for s in d.shape)      # fftrange(s, dtype=data.dtype) * dx
    r, _, polar = uniform_cart_to_polar(x, y, d)
    mean, count = _ops.psf_size(polar, r, relative, value, last).tolist()
    if count == 0:
        raise ValueError('metric does not cross the sampled data')
    return mean


def fwhm(data, dx=None, x=None, y=None, criteria='last'):
    """The full width at half maximum of data (psf.py:93-117): twice estimate_size(metric='fwhm')."""
    return estimate_size(x=x, y=y, dx=dx, data=data, metric='fwhm', criteria=criteria) * 2


def one_over_e(data, dx=None, x=None, y=None, criteria='last'):
    """The 1/e diameter of data (psf.py:120-144)."""
    return estimate_size(x=x, y=y, dx=dx, data=data, metric='1/e', criteria=criteria) * 2


def one_over_e_sq(data, dx=None, x=None, y=None, criteria='last'):
    """The 1/e^2 diameter of data (psf.py:147-171)."""
    return estimate_size(x=x, y=y, dx=dx, data=data, metric='1/e^2', criteria=criteria) * 2


def centroid_device(data):
    """The centre of mass (row, col) of data in samples, corner indexed, as a float64 2-vector ON THE DEVICE: two launches, nothing read
    back, the same bits every call."""
    return _ops.centroid(_data2d(data))


def centroid(data, dx=None, unit='spatial'):
    """The centroid of data (psf.py:174-203) as Python floats (row, col): unit 'pixels' is corner indexed, 'spatial' is
    dx (com - n // 2)."""
    shape = tuple(np.shape(data))
    com = tuple(centroid_device(data).tolist())
    if unit != 'spatial':
        return com
    return tuple(dx * (c - n // 2) for c, n in zip(com, shape))


def autocrop(data, px):
    """Crop to the px x px window around the centroid (psf.py:206-237), zero where the window leaves the array.  One host read (the
    centroid, truncated with int() as the reference does), then one launch."""
    d = _data2d(data)
    cy, cx = (int(c) for c in centroid(d, unit='pixels'))
    w = px // 2
    return _ops.embed(d, (px, px), (w - cy, w - cx))      # row i of the window is row cy - w + i of data


def airydisk(unit_r, fno, wavelength):
    """The Airy pattern |2 jinc(pi r / (wavelength fno))|^2 over radial distances unit_r (psf.py:240-259)."""
    return _eager(IP.airydisk_spec(fno, wavelength), fr=unit_r)


def airydisk_efield(unit_r, fno, wavelength):
    """The same as airydisk, returning the (real-valued) E-field 2 jinc(pi r / (wavelength fno)) (psf.py:262-265)."""
    return _eager(IP.airydisk_spec(fno, wavelength, efield=True), fr=unit_r)


def airydisk_ft(r, fno, wavelength):
    """The Fourier transform of the Airy disk (psf.py:268-292): 2/pi (acos s - s sqrt(1 - s^2)) with s = min(|r| wavelength fno, 1).
    The caller's array is left as it is."""
    return _eager(IP.airydisk_ft_spec(fno, wavelength), fr=r)


airydisk_ft.spec = IP.airydisk_ft_spec
