"""CPU: the host side of the wavefront sensors (prysm_amd/x/psi.py, shack_hartmann.py, pdi.py, sri.py and x/sensors_plan.py): the numpy
model of every kernel against the reference's outputs in tests/golden/sensors.npz, the PSI schemes, the Python layer's refusals.
Bounds and cases: tests/sensors_common.py."""
import importlib.util

import numpy as np
import pytest
import torch

import sensors_common as C
from prysm_amd.x import psi, shack_hartmann as shmod, pdi, sri, sensors_plan as SP  # noqa: F401


@pytest.fixture(scope='module')
def G():
    return C.golden()


# ----------------------------------------------------------------------------- PSI
@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('name', C.PSI_SCHEMES)
def test_psi_model_against_golden(G, name, dt):
    sch = C.scheme(psi, name)
    fr = C.frames(G['psi_phi'], sch.shifts, dt)
    num, den, w = SP.psi(fr, sch.s, sch.c, dt)
    assert w.dtype == dt and num.dtype == dt
    assert C.wrapped_diff(w, G[f'psi_{name}_{"f64" if dt == np.float64 else "f32"}']).max() <= C.PSI_EPS_MULT[dt] * C.eps(dt)


@pytest.mark.parametrize('idt', [np.uint16, np.uint8])
@pytest.mark.parametrize('name', ['schwider', 'zygo13'])
def test_psi_model_on_integer_frames_against_the_truth(G, name, idt):
    sch = C.scheme(psi, name)
    phi = G['psi_phi']
    fr = C.frames(phi, sch.shifts, idt, C.INT_AMPL[idt])
    assert fr[0].dtype == idt
    for odt in (np.float64, np.float32):
        w = SP.psi(fr, sch.s, sch.c, SP.out_dtype_of(idt, odt))[2]
        assert w.dtype == odt
        assert C.wrapped_diff(w, phi).max() <= C.int_bound(sch, C.INT_AMPL[idt], odt)


@pytest.mark.parametrize('name', ['design7', 'design9', 'hann8', 'schwider', 'zygo13'])
def test_schemes_against_golden(G, name):
    sch = {'design7': lambda: psi.design_scheme(7), 'design9': lambda: psi.design_scheme(9, stepsize=np.pi / 3),
           'hann8': lambda: psi.design_scheme(8, window='hann'), 'schwider': lambda: psi.SCHWIDER, 'zygo13': lambda: psi.ZYGO_THIRTEEN_FRAME}[name]()
    assert isinstance(sch, psi.Scheme)
    for field, v in zip(('shifts', 's', 'c'), sch):
        assert np.array_equal(np.asarray(v, dtype=np.float64), G[f'scheme_{name}_{field}']), field


def test_design_scheme_takes_an_array_window():
    w = np.linspace(0.5, 1.0, 5)
    sch, plain = psi.design_scheme(5, window=w), psi.design_scheme(5)
    assert np.array_equal(sch.s, plain.s * w) and np.array_equal(sch.c, plain.c * w)


def test_psi_refusals_of_the_python_layer():
    with pytest.raises(ValueError, match='between 1 and 32'):
        SP.check_scheme(33, np.zeros(33), np.zeros(33))
    with pytest.raises(ValueError, match='between 1 and 32'):
        SP.check_scheme(0, [], [])
    with pytest.raises(ValueError, match='weights'):
        SP.check_scheme(5, np.zeros(4), np.zeros(5))
    with pytest.raises(TypeError, match='float32, float64, uint8 or uint16'):
        SP.out_dtype_of(np.int32, np.float64)
    assert SP.out_dtype_of(np.uint16, np.float32) == np.float32 and SP.out_dtype_of(np.float32, np.float64) == np.float32


def test_unwrap_phase_without_or_with_scikit_image():
    yy, xx = np.mgrid[0:24, 0:32]
    truth = 0.45 * xx + 0.2 * yy
    wrapped = np.angle(np.exp(1j * truth))
    if importlib.util.find_spec('skimage') is None:
        with pytest.raises(ImportError, match='scikit-image'):
            psi.unwrap_phase(wrapped, None)
    else:
        out = np.asarray(psi.unwrap_phase(wrapped, None))
        d = out - truth
        k = np.round(d.mean() / (2 * np.pi))
        assert np.abs(d - 2 * np.pi * k).max() < 1e-9


# ----------------------------------------------------------------------------- Shack-Hartmann
def _par(name):
    n, shape, shift, pitch, ap, kw = C.SH_CASES[name]
    kind = SP.LENSLET_CIRCLE if ap == 'circle' else SP.LENSLET_RECTANGLE
    return SP.lenslet_params(pitch, n, C.SH_EFL, C.SH_WVL, kind, kw, shift), shape


@pytest.mark.parametrize('name', list(C.SH_CASES))
def test_lenslet_model_against_golden(G, name):
    par, shape = _par(name)
    idx = G[f'sh_{name}_idx']
    for dt, tag in ((np.float64, 'f64'), (np.float32, 'f32')):
        field, count = SP.lenslet_screen(*C.sh_xy(shape, dt), par, dt)
        assert np.array_equal(count, G[f'sh_{name}_count' if dt == np.float64 else f'sh_{name}_count32'])
        keep = (G[f'sh_{name}_count'] == G[f'sh_{name}_count32']).ravel()[idx]
        bound = C.SH_C[dt] * C.eps(dt) * C.sh_max_arg(float(G[f'sh_{name}_maxtotal']))
        assert np.abs(field.ravel()[idx] - G[f'sh_{name}_{tag}'])[keep].max() <= bound
        assert (~keep).sum() <= C.SH_EXCLUDE_CAP * field.size


def test_lenslet_cases_hold_the_ties_the_issue_counts(G):
    for name in C.SH_TIE_CASES:
        count = G[f'sh_{name}_count']
        assert (count == 2).sum() >= 98 and 2 <= (count == 4).sum() <= 9, name
    assert G['sh_n4_61_p093_count'].max() == 1
    for name in ('n4_64', 'n3_50', 'n23_40x56_shift'):
        assert 99 <= (G[f'sh_{name}_count'] == 0).sum() <= 964


def test_lenslet_params_keep_the_reference_pairing():
    par = SP.lenslet_params(1.0, (2, 3), 50.0, 0.5, SP.LENSLET_RECTANGLE, {}, True)
    assert (par['nx'], par['ny']) == (3, 2)
    assert par['shift_x'] == 0.5 and par['shift_y'] == 0.0        # n[0] = 2 is even: xc moves; n[1] = 3 is odd: yc stays
    xc, yc = SP.lenslet_centres(par, np.float64)
    assert np.array_equal(xc, [-0.5, 0.5, 1.5]) and np.array_equal(yc, [-1.0, 0.0])
    # what the one-launch path does not take falls to the loop
    assert SP.lenslet_params(1.0, 3, 50.0, 0.5, SP.LENSLET_RECTANGLE, {'angle': 30}, False) is None
    assert SP.lenslet_params(1.0, 3, 50.0, 0.5, SP.LENSLET_RECTANGLE, {'height': 1.2}, False) is None
    assert SP.lenslet_params(1.0, 3, 50.0, 0.5, SP.LENSLET_RECTANGLE, {'height': 0.3, 'angle': 0}, False)['half_height'] == 0.3
    with pytest.raises(ValueError):
        SP.lenslet_params(1.0, 0, 50.0, 0.5, SP.LENSLET_RECTANGLE, {}, False)


def test_fallback_loop_against_the_model():
    """a callable the kernel does not know (a square written with tensor operations) through the per-lenslet loop, on host tensors"""
    name = 'n4_64_shift'
    par, shape = _par(name)
    x, y = (torch.from_numpy(v) for v in C.sh_xy(shape))

    def square(width, x, y):
        return (x.abs() - width <= 0) & (y.abs() - width <= 0)
    got = shmod._loop(1.0, 4, C.SH_EFL, C.SH_WVL, x, y, square, {}, True).numpy()
    want, _ = SP.lenslet_screen(*C.sh_xy(shape), par, np.float64)
    assert np.abs(got - want).max() <= C.SH_C[np.float64] * C.eps(np.float64) * C.sh_max_arg(4 * 0.5 / (2 * C.SH_EFL))

    def disc(radius, r):
        return r - radius <= 0
    parc = SP.lenslet_params(1.0, 4, C.SH_EFL, C.SH_WVL, SP.LENSLET_CIRCLE, {}, True)
    got = shmod._loop(1.0, 4, C.SH_EFL, C.SH_WVL, x, y, disc, {}, True).numpy()
    want, _ = SP.lenslet_screen(*C.sh_xy(shape), parc, np.float64)
    assert np.abs(got - want).max() <= C.SH_C[np.float64] * C.eps(np.float64) * C.sh_max_arg(4 * 0.5 / (2 * C.SH_EFL))


# ----------------------------------------------------------------------------- gratings, combination, fibre scale
def test_rectangle_pulse_model_against_golden(G):
    got = SP.grating(SP.GRATING_PULSE, C.PULSE_X, SP.pulse_params(**C.PULSE_KW), np.float64)
    assert np.array_equal(got, G['pulse'])
    hi, lo = 0.6 + 0.4, 0.6 - 0.4
    assert got[0] == 0.6 and got[1] == 0.6 and got[4] == lo and got[7] == lo and got[8] == hi      # midpoint, edge, negative x
    with pytest.raises(ValueError, match='period'):
        SP.pulse_params(period=0)


def test_fiber_scale_and_combination_models(G):
    at, efib = G['sri_more_at'], G['sri_efib']
    power = (np.abs(at) ** 2).sum()
    got = SP.fiber_scale(efib, power, float(G['sri_more_coupling']), 0.3)
    assert np.abs(got - G['sri_more_emitted']).max() <= 1e-10 * np.abs(G['sri_more_emitted']).max()
    a = np.array([[1 + 2j, 0.5j]])
    b = np.array([[2 - 1j, 1.0]])
    inten, total = SP.beam_combine(a, 0.5, b, 2.0)
    assert np.allclose(total, 0.5 * a + 2.0 * b, rtol=0, atol=1e-15) and np.allclose(inten, np.abs(0.5 * a + 2.0 * b) ** 2, rtol=1e-15)


def test_pspdi_refuses_an_unknown_grating():
    with pytest.raises(ValueError, match='unsupported grating type'):
        pdi.PSPDI(np.zeros((4, 4)), np.zeros((4, 4)), 100.0, 10.0, 0.6328, grating_type='blazed')
