"""CPU: the order of the argument checks of the entry points of csrc/pointwise.hip that take a dtype.  Every call here is refused (or
returns for an empty shape) before anything is launched, so the pointers are never dereferenced and no device is needed.

Most entry points check their arguments, then the leading dimensions, then return 0 for an empty shape, and only then look at the
dtype: an empty call with a bad dtype returns 0.  pm_sum_modes looks at the dtype first, and the entry points without an empty
return refuse a zero length as a bad argument.  The table states which."""
import ctypes
import os

import pytest

from prysm_amd import _lib as L

P = ctypes.c_void_p(16)         # never dereferenced
W = (ctypes.c_double * 1)(1.0)
R, C = 2, 3
CLD = C + 24                    # spline coefficients: the map's columns and 12 samples of padding on either side

COMPLEX_BAD = (L.PM_F32, 99)
ELEM_BAD = (2,)
AMP_BAD = (L.PM_C64,)

# name: (call(lib, dtype, rows, cols, ld), the bad dtypes, the word its refusal names, what an EMPTY call (rows = 0) with a bad dtype
#        returns, whether `ld` goes through the rule "one row takes any leading dimension")
ENTRIES = {
    'pm_cmul': (lambda lib, dt, r, c, ld: lib.pm_cmul(dt, 0, r, c, P, ld, P, ld, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_rmul': (lambda lib, dt, r, c, ld: lib.pm_rmul(dt, r, c, P, ld, P, ld, 1.0, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_scale_sep': (lambda lib, dt, r, c, ld: lib.pm_scale_sep(dt, r, c, P, ld, P, 0, P, 1, 1.0, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_abs2': (lambda lib, dt, r, c, ld: lib.pm_abs2(dt, r, c, P, ld, P, ld, 1, 0.5, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_abs_arg': (lambda lib, dt, r, c, ld: lib.pm_abs_arg(dt, r, c, P, ld, P, ld, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_sum_modes': (lambda lib, dt, r, c, ld: lib.pm_sum_modes(dt, 1, r, c, P, R * C, ld, W, 0, P, ld, None), COMPLEX_BAD, 'dtype',
                     L.PM_ERR_ARG, True),
    'pm_sample_map': (lambda lib, dt, r, c, ld: lib.pm_sample_map(dt, 1, R, C, P, C, 1.0, 0.0, 0.0, r, c, P, c, 1, P, c, 1, P, ld, 0.0, 0.0,
                                                                  P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_sample_spline': (lambda lib, dt, r, c, ld: lib.pm_sample_spline(dt, 3, R, C, P, CLD, 1.0, 0.0, 0.0, r, c, P, c, 1, P, c, 1, P, ld, 0.0,
                                                                        0.0, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_pupil_synth': (lambda lib, dt, r, c, ld: lib.pm_pupil_synth(dt, r, c, P, L.PM_F32, ld, P, ld, 1.0, P, ld, None), COMPLEX_BAD, 'dtype', 0,
                       True),
    'pm_pupil_synth (amplitude)': (lambda lib, dt, r, c, ld: lib.pm_pupil_synth(L.PM_C64, r, c, P, dt, ld, P, ld, 1.0, P, ld, None), AMP_BAD,
                                   'amp_dtype', 0, True),
    'pm_pupil_synth (amplitude, complex128)': (lambda lib, dt, r, c, ld: lib.pm_pupil_synth(L.PM_C128, r, c, P, dt, ld, P, ld, 1.0, P, ld, None),
                                               AMP_BAD, 'amp_dtype', 0, True),
    'pm_quadratic_phase': (lambda lib, dt, r, c, ld: lib.pm_quadratic_phase(dt, r, c, P, ld, P, ld, 1.0, P, ld, None), COMPLEX_BAD, 'dtype', 0,
                           True),
    'pm_outer': (lambda lib, dt, r, c, ld: lib.pm_outer(dt, r, c, P, P, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_embed': (lambda lib, dt, r, c, ld: lib.pm_embed(dt, r, c, P, ld, r, c, 0, 0, None, P, ld, None), ELEM_BAD, 'elem_bytes', 0, True),
    # the input of pm_pad_index has at least one row: the empty shape is the output's
    'pm_pad_index': (lambda lib, dt, r, c, ld: lib.pm_pad_index(dt, 1, max(r, 1), c, P, ld, r, c, 0, 0, P, ld, None), ELEM_BAD, 'elem_bytes', 0,
                     True),
    'pm_mdft_basis': (lambda lib, dt, r, c, ld: lib.pm_mdft_basis(dt, r, c, P, P, 1, P, ld, None), COMPLEX_BAD, 'dtype', 0, True),
    'pm_mdft_basis_grid': (lambda lib, dt, r, c, ld: lib.pm_mdft_basis_grid(dt, r, c, 0.1, 0.0, 1.0, 0.1, -1, P, ld, None), COMPLEX_BAD, 'dtype',
                           0, True),
    # no empty return: a zero length is a bad argument.  Their leading dimensions (where they have any) follow rules of their own
    'pm_spline_prefilter': (lambda lib, dt, r, c, ld: lib.pm_spline_prefilter(dt, 3, r, c, P, ld, P, CLD, None), COMPLEX_BAD, 'dtype',
                            L.PM_ERR_ARG, False),
    'pm_as_tf_vectors': (lambda lib, dt, r, c, ld: lib.pm_as_tf_vectors(dt, r, c, 0.6328, 0.01, 10.0, P, P, None), COMPLEX_BAD, 'dtype',
                         L.PM_ERR_ARG, False),
    'pm_czt_vectors': (lambda lib, dt, r, c, ld: lib.pm_czt_vectors(dt, r, c, r + c, 0.3, 0.01, P, P, P, None), COMPLEX_BAD, 'dtype',
                       L.PM_ERR_ARG, False),
    # the width of the real array is even: 2 x 4, read as 2 x 2 packed complex numbers
    'pm_r2c_untangle': (lambda lib, dt, r, c, ld: lib.pm_r2c_untangle(dt, r, c + 1, P, ld, 0, 0, 0, 0, L.PM_EPI_NONE, 0, 1.0, P, ld + 1, None),
                        COMPLEX_BAD, 'dtype', L.PM_ERR_ARG, False),
}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _refused(lib, rc, name, word):
    msg = lib.pm_last_error().decode()
    assert rc == L.PM_ERR_ARG, (name, rc, msg)
    assert name.split(' ')[0] in msg and word in msg, (name, msg)


@pytest.mark.parametrize('name', list(ENTRIES))
def test_bad_dtype_is_refused(lib, name):
    call, bad, word, _, _ = ENTRIES[name]
    for dt in bad:
        _refused(lib, call(lib, dt, R, C, C), name, word)


@pytest.mark.parametrize('name', list(ENTRIES))
def test_empty_shape_with_bad_dtype(lib, name):
    call, bad, _, empty_rc, _ = ENTRIES[name]
    for dt in bad:
        rc = call(lib, dt, 0, C, C)
        assert rc == empty_rc, (name, dt, rc, lib.pm_last_error())
        if rc:
            assert name.split(' ')[0].encode() in lib.pm_last_error()


@pytest.mark.parametrize('name', [n for n, e in ENTRIES.items() if e[4]])
def test_one_row_takes_a_leading_dimension_below_cols(lib, name):
    """ld = cols - 1 with one row passes the leading-dimension rule: the refusal that follows is the dtype's"""
    call, bad, word, _, _ = ENTRIES[name]
    for dt in bad:
        _refused(lib, call(lib, dt, 1, C, C - 1), name, word)
        assert 'leading dimension' not in lib.pm_last_error().decode()
