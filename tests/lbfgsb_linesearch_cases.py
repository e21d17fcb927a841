"""Scalar functions for the strong-Wolfe search, shared by tests/golden/make_golden_lbfgsb.py (which records what the reference's search
does on them) and tests/test_lbfgsb_host.py: name -> (phi(alpha) -> (phi, phi'), maxalpha, c2, maxiter); c1 = 1e-4.  Between them
they reach: immediate acceptance, bracket by increase, bracket by positive slope, doubling, the pinned cap, alpha1 == 0, the cubic
step accepted, cubic rejected -> quadratic -> bisection, zoom exhausted and the bracket phase exhausted."""
import math

CASES = {
    'accept': (lambda a: ((a - 1) ** 2, 2 * (a - 1)), None, 0.9, 30),
    'increase': (lambda a: ((a - 0.3) ** 2, 2 * (a - 0.3)), None, 0.9, 30),
    'slope': (lambda a: ((a - 0.8) ** 2, 2 * (a - 0.8)), None, 0.1, 30),
    'doubling': (lambda a: ((a - 5) ** 2, 2 * (a - 5)), None, 0.1, 30),
    'pinned': (lambda a: ((a - 5) ** 2, 2 * (a - 5)), 0.5, 0.1, 30),
    'zero': (lambda a: ((a - 5) ** 2, 2 * (a - 5)), 0.0, 0.9, 30),
    'wall': (lambda a: ((0.0, -1.0) if a == 0 else (1.0, -1.0)), None, 0.9, 30),      # a table: phi0 = 0, 1 everywhere else
    'more-thuente': (lambda a: (-a / (a * a + 2), (a * a - 2) / (a * a + 2) ** 2), None, 0.001, 30),
    'quartic': (lambda a: ((a - 0.07) ** 4 * 50 - a * 0.01, 200 * (a - 0.07) ** 3 - 0.01), None, 0.01, 30),
    'exp': (lambda a: (math.exp(8 * a) - 20 * a, 8 * math.exp(8 * a) - 20), None, 0.01, 30),
    'oscillating': (lambda a: (-a + 0.3 * math.sin(25 * a), -1 + 7.5 * math.cos(25 * a)), None, 0.05, 30),
    'runaway': (lambda a: (-a, -1.0), None, 0.9, 6),
}
