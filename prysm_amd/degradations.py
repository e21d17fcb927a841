"""Degradations in the image chain on the device (prysm/degradations.py): the smear and jitter transfer functions.

Each function is one launch of pm_tf_product (csrc/imagechain.hip) that returns the map in the working precision --
coordinates._real_dtype's rule: float32 when every frequency array is float32, float64 otherwise; NOT the reference's casts to
config.precision.  Frequencies are 1-D vectors (fx of nx and fy of ny values give (ny, nx)), a (1, nx) row with an (ny, 1) column, or
2-D arrays.  `smear_ft.spec(width, height)` and `jitter_ft.spec(scale)` are the deferred forms: small records, no device work, for
convolution.apply_transfer_functions and convolution.transfer_function, which multiply every factor into H in one launch.
"""
from . import imagechain_plan as IP
from .objects import _eager

__all__ = ['jitter_ft', 'smear_ft']


def smear_ft(fx, fy, width, height):
    """Analytic Fourier transform of smear (degradations.py:7-39): sinc(fx width) sinc(fy height), a zero extent dropping its factor;
    both zero raises ValueError."""
    return _eager(IP.smear_spec(width, height), fx=fx, fy=fy)


def jitter_ft(fr, scale):
    """Analytic Fourier transform of Gaussian jitter (degradations.py:42-59): exp(-2 (pi scale fr)^2)."""
    return _eager(IP.jitter_spec(scale), fr=fr)


smear_ft.spec = IP.smear_spec
jitter_ft.spec = IP.jitter_spec
