"""Generalised Laguerre polynomials (prysm/polynomials/laguerre.py) on the device:
k L_k = (alpha + 2k - 1 - x) L_{k-1} - (alpha + k - 1) L_{k-2} as one table of csrc/recur.hip.
"""
from . import _recur as R

__all__ = ['laguerre', 'laguerre_seq', 'laguerre_der', 'laguerre_der_seq']

laguerre, laguerre_seq, laguerre_der, laguerre_der_seq = R.make_family('laguerre', 'laguerre.py:8-140')
