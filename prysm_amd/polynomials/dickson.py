"""Dickson polynomials of the first and second kind (prysm/polynomials/dickson.py) on the device: both obey
P_k = x P_{k-1} - alpha P_{k-2} and differ in P_0 (2 and 1), each one table of csrc/recur.hip.
"""
from . import _recur as R

__all__ = ['dickson1', 'dickson1_seq', 'dickson1_der', 'dickson1_der_seq', 'dickson2', 'dickson2_seq', 'dickson2_der', 'dickson2_der_seq']

dickson1, dickson1_seq, dickson1_der, dickson1_der_seq = R.make_family('dickson1', 'dickson.py:8-186')
dickson2, dickson2_seq, dickson2_der, dickson2_der_seq = R.make_family('dickson2', 'dickson.py:49-275')
