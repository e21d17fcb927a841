"""Hermite polynomials (prysm/polynomials/hermite.py) on the device: the probabilist's He_k = x He_{k-1} - (k - 1) He_{k-2} and the
physicist's H_k = 2 x H_{k-1} - 2 (k - 1) H_{k-2}, each one table of csrc/recur.hip.
"""
from . import _recur as R

__all__ = ['hermite_He', 'hermite_He_seq', 'hermite_He_der', 'hermite_He_der_seq', 'hermite_H', 'hermite_H_seq', 'hermite_H_der',
           'hermite_H_der_seq']

hermite_He, hermite_He_seq, hermite_He_der, hermite_He_der_seq = R.make_family('hermite_He', 'hermite.py:79-98')
hermite_H, hermite_H_seq, hermite_H_der, hermite_H_der_seq = R.make_family('hermite_H', 'hermite.py:101-120')
