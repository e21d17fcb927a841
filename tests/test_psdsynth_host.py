"""CPU: the host side of the PSD surface synthesis -- the numpy model of csrc/psdsynth.hip against the reference's outputs in
tests/golden/psdsynth.npz, the generator's uniforms against the detector's Philox words, fit_psd, the placement of
make_random_subaperture_mask, the argument errors of the public functions and of every entry point (refused before anything is
launched, so no device is needed), and the declarations of the new symbols.  Cases and bounds: tests/psdsynth_common.py."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import psdsynth_common as C
from prysm_amd import _lib as L
from prysm_amd import detector_plan as DP
from prysm_amd import interferogram as ifg
from prysm_amd import psdsynth_plan as PP

P = ctypes.c_void_p(16)         # never dereferenced
ARG, WS = L.PM_ERR_ARG, L.PM_ERR_WORKSPACE
F32, F64 = L.PM_F32, L.PM_F64
BIG = 1 << 40
B, R, CO = 2, 4, 6
SYMBOLS = ('pm_psd_uniform', 'pm_psd_signal', 'pm_psd_finish_workspace', 'pm_psd_finish', 'pm_psd_scale')


@pytest.fixture(scope='module')
def lib():
    return L.load()


@pytest.fixture(scope='module')
def G():
    return C.golden()


# ---------------------------------------------------------------- the model against the reference
@pytest.mark.parametrize('dt', C.DTYPES)
@pytest.mark.parametrize('name', list(C.SYNTH))
def test_model_of_synthesize_against_the_reference(G, name, dt):
    shape, seed = C.SYNTH[name]
    psd, _, nu_y = C.synth_case(name)
    dx, f = PP.synthesize(psd.astype(dt), nu_y[0], C.randnums(shape, seed, dt))
    assert f.dtype == PP.cdtype(dt)
    C.compare('host', name, f.real, G[f'{name}_{C.tag(dt)}_z'], dt)
    assert dx == G[f'{name}_{C.tag(dt)}_dx']


def render_model(name, u):
    size, samples, rms, _, which, kw, _ = C.RENDER[name]
    mask = C.render_mask(name)
    if which == 'user':
        nu = PP.freq_vector(samples, size / (samples - 1))
        source = dict(psd=C.gauss_psd(np.hypot(nu[None, :], nu[:, None]), **kw).astype(u.dtype))
    else:
        source = dict(model=PP.model_record(PP.ABC if which == 'abc' else PP.AB, kw))
    kind = PP.MASK_NONE if mask is None else PP.MASK_CIRCLE if isinstance(mask, str) else PP.MASK_ARRAY
    return PP.render(size, samples, u, rms=rms, mask_kind=kind, mask=None if isinstance(mask, str) else mask, **source)


@pytest.mark.parametrize('dt', C.DTYPES)
@pytest.mark.parametrize('name', list(C.RENDER))
def test_model_of_render_against_the_reference(G, name, dt):
    size, samples, rms, _, _, _, seed = C.RENDER[name]
    dx, z = render_model(name, C.randnums((samples, samples), seed, dt))
    assert z.dtype == dt
    want = G[f'render_{name}_{C.tag(dt)}_z']
    C.compare('host', name, z, want, dt)
    assert abs(dx - G[f'render_{name}_{C.tag(dt)}_dx']) <= 2 * C.eps(np.float64) * dx
    if rms is not None:
        fin = np.isfinite(z)
        assert abs(np.sqrt((z[fin].astype(np.float64) ** 2).mean()) - rms) <= 4 * C.eps(dt) * rms


def test_the_reference_acceptance_case(G):
    z = G['render_circle_f64_z']
    fin = np.isfinite(z)
    assert abs(np.sqrt((z[fin] ** 2).mean()) - 5.0) < 1e-12 and np.isnan(z[0, 0])
    assert abs(G['render_circle_f64_dx'] - 100 / 63) < 1e-12


# ---------------------------------------------------------------- the generator
def test_uniforms_are_the_detectors_philox_words_to_the_bit():
    seed, shape = 0x9E3779B97F4A7C15, (5, 7)
    pixel = np.arange(shape[0] * shape[1])
    for surface in (0, 3):
        w = DP.sample_words(seed, 0, surface, pixel, 0)
        u64 = PP.uniform(seed, [surface], shape, np.float64)[0]
        u32 = PP.uniform(seed, [surface], shape, np.float32)[0]
        assert u64.dtype == np.float64 and u32.dtype == np.float32
        assert np.array_equal(u64.ravel(), DP.uniform53(w[0], w[1]))
        assert np.array_equal(u32.ravel().astype(np.float64), (w[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
        assert u64.min() >= 0 and u64.max() < 1 and u32.min() >= 0 and u32.max() < 1
    a, b = PP.uniform(seed, [0, 1], shape, np.float64)
    assert not np.array_equal(a, b)
    assert abs(PP.uniform(1, [0], (64, 64), np.float64).mean() - 0.5) < 0.02


def test_a_seed_comes_from_pythons_random():
    random.seed(5)
    a = PP.draw_seed()
    random.seed(5)
    assert PP.draw_seed() == a and 0 <= a < 1 << 64


# ---------------------------------------------------------------- host logic
def test_window_frequencies_and_routes():
    f = PP.freq_vector(64, 100 / 63)
    want = np.fft.fftshift(np.fft.fftfreq(64, 100 / 63))
    want[32] = want[33] / 10
    assert np.array_equal(f, want)
    dx, area, scale = PP.window(f[0], (64, 64))
    assert abs(dx - 100 / 63) < 1e-13 and abs(area - (63 * dx) ** 2) < 1e-9 and abs(scale - 1 / (64 * 64 * dx * dx)) < 1e-18
    fo = PP.freq_vector(33, 0.1)      # an odd length: fs is not 1 / dx of the grid
    assert abs(PP.window(fo[0], (33, 33))[0] - 1 / (2 * 16 / (33 * 0.1))) < 1e-15
    assert PP.shifts((64, 33)) == (32, 17)
    assert PP.route((64, 128)) == 'hermitian' and PP.route((64, 48)) == 'real_pairs' and PP.route((33, 47)) == 'complex'
    assert PP.route((64, 48), stacked=True) == 'complex' and PP.route((64, 64), stacked=True) == 'hermitian'
    assert PP.model_record(PP.ABC, dict(a=1, b=2, c=3)) == (PP.ABC, 1.0, 2.0, 3.0)
    assert PP.model_record(PP.AB, dict(a=1, b=2)) == (PP.AB, 1.0, 2.0, 0.0)
    with pytest.raises(TypeError):
        PP.model_record(PP.AB, dict(a=1, b=2, c=3))
    with pytest.raises(TypeError):
        PP.model_record(PP.ABC, dict(a=1, b=2))


def test_model_of_the_signal_and_the_scale():
    X = C.spectrum((5, 7), np.float64)
    psd = C.positive((5, 7), np.float64)
    psd[1, 1] = -1.0
    S = PP.signal(X, psd, 2.5)
    want = np.exp(1j * np.angle(X)) * np.sqrt(2.5 * psd.astype(complex)).real
    ok = np.isfinite(S)
    assert np.isnan(S[1, 1]) and ok.sum() == 34
    assert np.abs(S[ok] - want[ok]).max() < 4 * C.eps(np.float64) * np.abs(want[ok]).max()
    assert np.array_equal(S[X == 0].real, np.sqrt(2.5 * psd[X == 0])) and not S[X == 0].imag.any()
    field = C.integer_field((6, 9), np.float64, batch=2)
    mask = np.ones((6, 9), bool)
    mask[1, 2] = False
    z, sums = PP.finish(field, PP.MASK_ARRAY, mask)
    assert np.isnan(z[:, 1, 2]).all() and np.array_equal(sums[:, 0], [53, 53])
    assert np.array_equal(sums[:, 1], [(field[b].real[mask] ** 2).sum() for b in range(2)])
    zs = PP.scale(z, sums, 3.0)
    for b in range(2):
        assert abs(np.sqrt((zs[b][mask] ** 2).mean()) - 3.0) < 1e-14
    dark, s0 = PP.finish(field, PP.MASK_ARRAY, np.zeros((6, 9), bool))
    assert np.isnan(PP.scale(dark, s0, 3.0)).all() and not s0.any()


# ---------------------------------------------------------------- fit_psd, make_random_subaperture_mask
def test_fit_psd_recovers_the_reference_cases(G):
    coefs = ifg.fit_psd(C.FIT_F, PP.abc(C.FIT_F, *C.FIT_ABC))
    np.testing.assert_allclose(coefs, C.FIT_ABC, rtol=C.FIT_RTOL_ABC)
    psd = PP.ab(C.FIT_F, *C.FIT_AB)
    np.testing.assert_allclose(ifg.fit_psd(C.FIT_F, psd, callable=ifg.ab_psd), C.FIT_AB, rtol=C.FIT_RTOL_AB)
    res = ifg.fit_psd(C.FIT_F, psd, callable=ifg.ab_psd, return_='optres')
    assert res.success and res.status == 0 and res.nfev == 1 and res.fun.shape == (195,) and abs(res.cost) < 1e-20
    np.testing.assert_allclose(res.x, C.FIT_AB, rtol=C.FIT_RTOL_AB)
    np.testing.assert_allclose(ifg.fit_psd(C.FIT_F, C.noisy_curve()), G['fit_noisy'], rtol=C.FIT_RTOL_NOISY)
    res = ifg.fit_psd(C.FIT_F, C.noisy_curve(), return_='optres')
    np.testing.assert_allclose(res.x, G['fit_noisy'], rtol=C.FIT_RTOL_NOISY)
    user = ifg.fit_psd(C.FIT_F, PP.abc(C.FIT_F, *C.FIT_ABC), callable=lambda nu, a, b, c: PP.abc(nu, a, b, c), guess=[90, 0.6, 3.0])
    np.testing.assert_allclose(user, C.FIT_ABC, rtol=C.FIT_RTOL_ABC)


def test_the_closed_form_fit_needs_no_scipy(monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split('.')[0] == 'scipy':
            raise ImportError(name)
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, '__import__', no_scipy)
    psd = PP.ab(C.FIT_F, *C.FIT_AB)
    np.testing.assert_allclose(ifg.fit_psd(C.FIT_F, psd, callable=ifg.ab_psd), C.FIT_AB, rtol=C.FIT_RTOL_AB)
    res = ifg.fit_psd(C.FIT_F, psd, callable=ifg.ab_psd, return_='optres')
    assert isinstance(res, PP.FitResult) and res.success and res.status == 0 and res.nfev == 1 and 'closed-form' in res.message
    np.testing.assert_allclose(res.x, C.FIT_AB, rtol=C.FIT_RTOL_AB)
    with pytest.raises(ImportError):
        ifg.fit_psd(C.FIT_F, PP.abc(C.FIT_F, *C.FIT_ABC))


def test_subaperture_offsets_keep_the_mask_inside():
    random.seed(3)
    seen = {PP.subaperture_offsets((7, 9), (3, 4)) for _ in range(400)}
    assert all(0 <= dy <= 4 and 0 <= dx <= 5 for dy, dx in seen) and len(seen) == 30
    assert PP.subaperture_offsets((3, 4), (3, 4)) == (0, 0)
    for bad in ((2, 9), (7, 3)):
        with pytest.raises(ValueError, match='fit inside'):
            PP.subaperture_offsets(bad, (3, 4))
    with pytest.raises(ValueError, match='fit inside'):
        ifg.make_random_subaperture_mask((2, 2), np.ones((3, 3), bool))


# ---------------------------------------------------------------- argument errors
def test_public_argument_errors():
    psd, nu_x, nu_y = C.synth_case('even')
    with pytest.raises(ValueError, match='not both'):
        ifg.synthesize_surface_from_psd(psd, nu_x, nu_y, randnums=C.randnums(C.EVEN, 1), seed=4)
    for shape in ((1, 8), (8, 1), (8,)):
        with pytest.raises(ValueError, match='at least 2'):
            ifg.synthesize_surface_from_psd(np.ones(shape), nu_x, nu_y, seed=1)
    with pytest.raises(ValueError, match="'circle'"):
        ifg.render_synthetic_surface(10, 16, mask='square', a=1, b=1, c=1)
    with pytest.raises(ValueError, match="'circle'"):
        ifg.Interferogram.render_from_psd(10, 16, mask='disc', a=1, b=1, c=1)
    with pytest.raises(ValueError, match='not both'):
        ifg.render_synthetic_surface(10, 16, randnums=np.zeros((16, 16)), seed=1, a=1, b=1, c=1)
    with pytest.raises(ValueError, match='randnums must have shape'):
        ifg.render_synthetic_surface(10, 16, randnums=np.zeros((15, 16)), a=1, b=1, c=1)
    with pytest.raises(ValueError, match='batch'):
        ifg.render_synthetic_surface(10, 16, batch=0, a=1, b=1, c=1)
    with pytest.raises(ValueError, match='batch'):
        ifg.render_synthetic_surface(10, 16, batch=2, randnums=np.zeros((3, 16, 16)), a=1, b=1, c=1)
    with pytest.raises(ValueError, match='samples'):
        ifg.render_synthetic_surface(10, 2, a=1, b=1, c=1)
    with pytest.raises(TypeError):
        ifg.render_synthetic_surface(10, 16, psd_fcn=ifg.ab_psd, a=1, b=1, c=1)
    assert PP.check_random((4, 5), None, None) is None and PP.check_random((4, 5), None, 3, batch=3) == 3
    assert PP.check_random((4, 5), (4, 5), None) is None and PP.check_random((4, 5), (2, 4, 5), None) == 2
    for name in ('synthesize_surface_from_psd', 'render_synthetic_surface', 'fit_psd', 'make_random_subaperture_mask'):
        assert name in ifg.__all__ and callable(getattr(ifg, name))
    assert isinstance(ifg.Interferogram.__dict__['render_from_psd'], staticmethod)


def refused(lib, rc, code, word):
    assert rc == code, (rc, lib.pm_last_error())
    assert word.encode() in lib.pm_last_error(), lib.pm_last_error()
    with pytest.raises(ValueError):
        L.check(rc)


def model(kind=L.PM_IFG_PSD_ABC, dxg=0.1):
    return L.pm_psd_model(kind, 0, 1.0, 2.0, 3.0, dxg)


# name: call(lib, dt, p, ld, bs, ws) -> rc, with p the data pointer, ld / bs its leading dimension and member stride, ws the workspace bytes
CALLS = {
    'pm_psd_uniform': lambda lib, dt, p, ld, bs, ws: lib.pm_psd_uniform(dt, B, R, CO, 7, 0, p, ld, bs, None),
    'pm_psd_signal': lambda lib, dt, p, ld, bs, ws: lib.pm_psd_signal(dt, B, R, CO, p, ld, bs, P, CO, None, 1.0, None),
    'pm_psd_finish': lambda lib, dt, p, ld, bs, ws: lib.pm_psd_finish(dt, L.PM_PSD_MASK_NONE, B, R, CO, p, ld, bs, None, 0, 0.0, 0.0, P, CO, R * CO, P, P,
                                                                      ws, None),
    'pm_psd_scale': lambda lib, dt, p, ld, bs, ws: lib.pm_psd_scale(dt, B, R, CO, p, ld, bs, P, 1.0, None),
}


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_point_refusals(lib, name):
    call = CALLS[name]
    for dt in (L.PM_C64, 99):
        refused(lib, call(lib, dt, P, CO, R * CO, BIG), ARG, 'dtype')
        refused(lib, call(lib, dt, None, CO - 1, 0, 0), ARG, 'dtype')      # the dtype is looked at first
    for dt in (F32, F64):
        refused(lib, call(lib, dt, None, CO, R * CO, BIG), ARG, 'null pointer')
        refused(lib, call(lib, dt, P, CO - 1, R * CO, BIG), ARG, 'leading dimension')
        refused(lib, call(lib, dt, P, CO, R * CO - 1, BIG), ARG, 'overlap')
        if name == 'pm_psd_finish':
            refused(lib, call(lib, dt, P, CO, R * CO, 7), WS, 'workspace')
            refused(lib, call(lib, dt, P, CO - 1, R * CO, 7), ARG, 'leading dimension')      # the shape before the workspace


def test_refusals_of_kinds_shapes_and_records(lib):
    refused(lib, lib.pm_psd_uniform(F64, 0, R, CO, 7, 0, P, CO, R * CO, None), ARG, 'empty')
    refused(lib, lib.pm_psd_uniform(F64, 65536, R, CO, 7, 0, P, CO, R * CO, None), ARG, 'too large')
    refused(lib, lib.pm_psd_uniform(F64, B, R, CO, 7, -1, P, CO, R * CO, None), ARG, 'first surface')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, P, CO, R * CO, None, 0, None, 1.0, None), ARG, 'exactly one')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, P, CO, R * CO, P, CO, ctypes.byref(model()), 1.0, None), ARG, 'exactly one')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, P, CO, R * CO, P, CO - 1, None, 1.0, None), ARG, 'leading dimension')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, P, CO, R * CO, None, 0, ctypes.byref(model(kind=2)), 1.0, None), ARG, 'kind')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, P, CO, R * CO, None, 0, ctypes.byref(model(dxg=0.0)), 1.0, None), ARG, 'spacing')
    refused(lib, lib.pm_psd_signal(F64, B, R, CO, ctypes.c_void_p(8), CO, R * CO, P, CO, None, 1.0, None), ARG, 'aligned')
    fin = lambda kind, mask, mld, radius=1.0, old=CO, obs=R * CO: lib.pm_psd_finish(      # noqa: E731
        F32, kind, B, R, CO, P, CO, R * CO, mask, mld, radius, 0.1, P, old, obs, P, P, BIG, None)
    refused(lib, fin(3, None, 0), ARG, 'mask_kind')
    refused(lib, fin(L.PM_PSD_MASK_ARRAY, None, CO), ARG, 'mask is missing')
    refused(lib, fin(L.PM_PSD_MASK_ARRAY, P, CO - 1), ARG, 'leading dimension')
    refused(lib, fin(L.PM_PSD_MASK_CIRCLE, None, 0, radius=float('nan')), ARG, 'finite')
    refused(lib, fin(L.PM_PSD_MASK_NONE, None, 0, old=CO - 1), ARG, 'leading dimension')
    refused(lib, fin(L.PM_PSD_MASK_NONE, None, 0, obs=R * CO - 1), ARG, 'overlap')
    refused(lib, lib.pm_psd_scale(F64, B, R, CO, P, CO, R * CO, ctypes.c_void_p(20), 1.0, None), ARG, 'alignment')
    # the workspace: one (count, sum of squares) pair per workgroup of 256 threads and surface, at most 1024 workgroups per surface
    assert lib.pm_psd_finish_workspace(B, R, CO) == B * 1 * 2 * 8
    assert lib.pm_psd_finish_workspace(3, 1024, 513) == 3 * 1024 * 2 * 8 and lib.pm_psd_finish_workspace(1, 100, 100) == 40 * 2 * 8
    assert lib.pm_psd_finish_workspace(0, R, CO) == 0 and lib.pm_psd_finish_workspace(1, 1 << 32, 1) == 0


def test_new_symbols_are_declared_exported_and_bound(lib):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(here, 'include', 'prysm_amd.h')).read(), flags=re.S)
    for name in SYMBOLS:
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, f'{name} is not declared in prysm_amd.h'
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert len(L.SIGNATURES[name][1]) == len(m.group(1).split(',')), name
    assert ctypes.sizeof(L.pm_psd_model) == 40 and 'typedef struct pm_psd_model' in src
    assert (L.PM_PSD_MASK_NONE, L.PM_PSD_MASK_ARRAY, L.PM_PSD_MASK_CIRCLE) == (PP.MASK_NONE, PP.MASK_ARRAY, PP.MASK_CIRCLE) == (0, 1, 2)
    assert (L.PM_IFG_PSD_ABC, L.PM_IFG_PSD_AB) == (PP.ABC, PP.AB)
    assert lib.pm_version() == 107
