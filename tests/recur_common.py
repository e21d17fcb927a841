"""What the CPU and GPU tests of the recurrence families share (tests/test_recur_host.py, tests/test_gpu_recur.py): the fixture's cases,
the package's tolerances and the error measures."""
import numpy as np

# fixture case -> (family, shape parameters, the key of its points)
CASES = {
    'cheby1': ('cheby1', (), 'x_unit'), 'cheby2': ('cheby2', (), 'x_unit'), 'cheby3': ('cheby3', (), 'x_unit'),
    'cheby4': ('cheby4', (), 'x_unit'), 'legendre': ('legendre', (), 'x_unit'),
    'hermite_He': ('hermite_He', (), 'x_hermite'), 'hermite_H': ('hermite_H', (), 'x_hermite'),
    'laguerre': ('laguerre', (1.5,), 'x_laguerre'),
    'dickson1': ('dickson1', (0.75,), 'x_unit'), 'dickson2': ('dickson2', (0.75,), 'x_unit'),
    'jacobi_0_2': ('jacobi', (0.0, 2.0), 'x_unit'), 'jacobi_h_mh': ('jacobi', (0.5, -0.5), 'x_unit'),
    'jacobi_0_0': ('jacobi', (0.0, 0.0), 'x_unit'),
}
# relative per mode, max |delta| / max |ref|: the tolerances of tests/test_gpu_zernike.py
TOL = {np.float64: 1e-12, np.float32: 2e-5}


def rel_per_mode(got, ref):
    """max |got - ref| / max |ref| per plane; a plane that is zero in the reference (the derivative of order 0) must be zero"""
    ax = tuple(range(1, ref.ndim))
    err, scale = np.max(np.abs(got - ref), axis=ax), np.max(np.abs(ref), axis=ax)
    assert np.all(err[scale == 0] == 0)
    return np.max(err[scale > 0] / scale[scale > 0])


def rel(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def mns_of(a):
    return [tuple(int(v) for v in row) for row in a]
