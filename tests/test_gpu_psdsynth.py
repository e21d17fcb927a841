"""GPU: the PSD surface synthesis on an MI355X -- the public functions against the reference's outputs in tests/golden/psdsynth.npz
and against the numpy model (prysm_amd/psdsynth_plan.py), the device generator against the model's uniforms to the bit, and every
kernel of csrc/psdsynth.hip alone on the smallest shapes that can go wrong.  Cases and bounds: tests/psdsynth_common.py; each
comparison prints measured against bound."""
import random

import numpy as np
import pytest
import torch

import interferogram_common as IC
import psdsynth_common as C
from prysm_amd import psdsynth_plan as PP

pytestmark = pytest.mark.gpu

DTYPES = list(C.DTYPES)
SEED = 0x1234_5678_9ABC_DEF1      # the high word is used too


@pytest.fixture(scope='module')
def G():
    return C.golden()


@pytest.fixture(scope='module')
def ops(pa):
    from prysm_amd import _lib, _ops
    return _ops, _lib


@pytest.fixture(scope='module')
def ifg(pa):
    from prysm_amd import interferogram
    return interferogram


@pytest.fixture
def precision():
    """config.precision for the duration of a test"""
    from prysm_amd.conf import config

    def use(dt):
        config.precision = 32 if np.dtype(dt) == np.float32 else 64
    yield use
    config.precision = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def render_args(ifg, name):
    size, samples, rms, _, which, kw, seed = C.RENDER[name]
    fcn = {'abc': ifg.abc_psd, 'ab': ifg.ab_psd, 'user': C.gauss_psd}[which]
    return (size, samples), dict(rms=rms, mask=C.render_mask(name), psd_fcn=fcn, **kw), seed


def render_model(name, u):
    size, samples, rms, _, which, kw, _ = C.RENDER[name]
    mask = C.render_mask(name)
    if which == 'user':
        nu = PP.freq_vector(samples, size / (samples - 1)).astype(u.dtype)      # the callable sees frequencies of the data's precision
        source = dict(psd=C.gauss_psd(np.hypot(nu[None, :], nu[:, None]), u.dtype.type(kw['a']), u.dtype.type(kw['s'])))
    else:
        source = dict(model=PP.model_record(PP.ABC if which == 'abc' else PP.AB, kw))
    kind = PP.MASK_NONE if mask is None else PP.MASK_CIRCLE if isinstance(mask, str) else PP.MASK_ARRAY
    return PP.render(size, samples, u, rms=rms, mask_kind=kind, mask=None if isinstance(mask, str) else mask, **source)


# ----------------------------------------------------------------------------- the public functions against the reference
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(C.SYNTH))
def test_synthesize_against_the_reference(ifg, G, name, dt):
    shape, seed = C.SYNTH[name]
    psd, nu_x, nu_y = C.synth_case(name)
    u = C.randnums(shape, seed, dt)
    x, y, z = ifg.synthesize_surface_from_psd(psd.astype(dt), nu_x, nu_y, randnums=u)
    assert z.dtype == dev(u).dtype and tuple(z.shape) == shape and tuple(x.shape) == (shape[1],) and tuple(y.shape) == (shape[0],)
    key = f'{name}_{C.tag(dt)}'
    C.compare('golden', name, host(z), G[f'{key}_z'], dt)
    C.compare('model', 'z', host(z), PP.synthesize(psd.astype(dt), nu_y[0], u)[1].real, dt, name)
    assert abs(float(x[1] - x[0]) - G[f'{key}_dx']) <= C.eps(dt) * G[f'{key}_dx'] and float(x[0]) == 0 and float(y[0]) == 0
    stack = np.stack([u, C.randnums(shape, seed + 100, dt)])
    zs = host(ifg.synthesize_surface_from_psd(dev(psd.astype(dt)), nu_x, dev(nu_y), randnums=dev(stack))[2])
    assert zs.shape == (2,) + shape
    C.compare('golden', name, zs[0], G[f'{key}_z'], dt, 'member 0 of a stack')
    C.compare('model', 'z', zs[1], PP.synthesize(psd.astype(dt), nu_y[0], stack[1])[1].real, dt, f'{name} member 1')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name', list(C.RENDER))
def test_render_against_the_reference(ifg, G, precision, name, dt):
    precision(dt)
    (size, samples), kw, seed = render_args(ifg, name)
    u = C.randnums((samples, samples), seed, dt)
    x, y, z = ifg.render_synthetic_surface(size, samples, randnums=u, **kw)
    key = f'render_{name}_{C.tag(dt)}'
    assert host(z).dtype == dt and tuple(z.shape) == (samples, samples)
    C.compare('golden', name, host(z), G[f'{key}_z'], dt)      # NaN positions are compared exactly
    C.compare('model', 'z', host(z), render_model(name, u)[1], dt, name)
    assert abs(float(x[1] - x[0]) - G[f'{key}_dx']) <= C.eps(dt) * G[f'{key}_dx']
    if name == 'circle':
        assert bool(torch.isnan(z[0, 0]))


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize('dt', DTYPES)
def test_uniforms_are_the_models_to_the_bit(ops, dt):
    _ops, L = ops
    tdt = L.torch_dtype(dt)
    for shape, s0 in (((3, 9, 65), 0), ((2, 33, 47), 5)):
        u = host(_ops.psd_uniform(shape, tdt, SEED, surface0=s0))
        assert np.array_equal(u, PP.uniform(SEED, range(s0, s0 + shape[0]), shape[1:], dt)), shape
    frame = torch.full((2, 9 + 2 * C.FRAME[0], 63 + 2 * C.FRAME[1]), float('nan'), dtype=tdt, device='cuda')
    win = frame[:, C.FRAME[0]:-C.FRAME[0], C.FRAME[1]:-C.FRAME[1]]
    _ops.psd_uniform((2, 9, 63), tdt, -3, out=win)      # a negative seed is its two's complement
    assert np.array_equal(host(win), PP.uniform((1 << 64) - 3, [0, 1], (9, 63), dt))
    assert int(torch.isnan(frame).sum()) == frame.numel() - win.numel()


@pytest.mark.parametrize('dt', DTYPES)
def test_the_seed_path_equals_randnums_fed_the_models_uniforms(ifg, precision, dt):
    precision(dt)
    (size, samples), kw, _ = render_args(ifg, 'circle')
    z = host(ifg.render_synthetic_surface(size, samples, seed=SEED, **kw)[2])
    u = PP.uniform(SEED, [0], (samples, samples), dt)[0]
    zr = host(ifg.render_synthetic_surface(size, samples, randnums=u, **kw)[2])
    assert np.array_equal(z, zr, equal_nan=True)      # the same kernels on the same numbers
    C.compare('model', 'z', z, render_model('circle', u)[1], dt, 'seed')
    random.seed(11)
    a = host(ifg.render_synthetic_surface(size, samples, **kw)[2])
    random.seed(11)
    b = host(ifg.render_synthetic_surface(size, samples, **kw)[2])
    c = host(ifg.render_synthetic_surface(size, samples, **kw)[2])
    assert np.array_equal(a, b, equal_nan=True) and not np.array_equal(a, c, equal_nan=True)


@pytest.mark.parametrize('samples', (64, 48, 33))      # the Hermitian path, a stack on the complex transform, an odd width
@pytest.mark.parametrize('dt', DTYPES)
def test_a_batch_is_the_models_surfaces(ifg, precision, dt, samples):
    precision(dt)
    kw = dict(rms=5, mask='circle', psd_fcn=ifg.abc_psd, a=1e4, b=1 / 100, c=2)
    z = host(ifg.render_synthetic_surface(100, samples, seed=SEED, batch=3, **kw)[2])
    assert z.shape == (3, samples, samples)
    model = dict(model=(PP.ABC, 1e4, 1 / 100, 2.0))
    for b in range(3):
        u = PP.uniform(SEED, [b], (samples, samples), dt)[0]
        want = PP.render(100, samples, u, rms=5, mask_kind=PP.MASK_CIRCLE, **model)[1]
        C.compare('model', 'z', z[b], want, dt, f'batch member {b} of {samples}')
        fin = np.isfinite(z[b])
        assert abs(np.sqrt((z[b][fin].astype(np.float64) ** 2).mean()) - 5) <= 4 * C.eps(dt) * 5
    assert not np.array_equal(z[0], z[1], equal_nan=True) and not np.array_equal(z[1], z[2], equal_nan=True)
    one = host(ifg.render_synthetic_surface(100, samples, seed=SEED, batch=1, **kw)[2])
    assert one.shape == (1, samples, samples)
    C.compare('model', 'z', one[0], z[0], dt, 'batch of one')


@pytest.mark.parametrize('dt', DTYPES)
def test_render_from_psd_gives_an_interferogram(ifg, G, precision, dt):
    precision(dt)
    I = ifg.Interferogram.render_from_psd(100, 64, rms=5, seed=SEED, a=1e4, b=1 / 100, c=2)
    assert isinstance(I, ifg.Interferogram) and I.shape == (64, 64) and I.wavelength == ifg.HeNe
    assert abs(I.dx - G['render_circle_f64_dx']) <= 2 * C.eps(np.float64) * I.dx
    assert bool(torch.isnan(I.data[0, 0])) and I.dropout_percentage > 15
    f64, f32, _ = IC.BOUND['stat']
    bound = f32 if dt == np.float32 else f64
    dev_ = abs(I.rms - 5) / (C.eps(dt) * 5)
    print(f'render_from_psd {C.tag(dt)} rms {I.rms!r}: {dev_:.3f} eps, bound {bound}')
    assert dev_ <= bound
    J = ifg.Interferogram.render_from_psd(10, 33, mask=None, psd_fcn=ifg.ab_psd, seed=3, a=1e2, b=2)
    assert J.dropout_percentage == 0


def test_make_random_subaperture_mask(ifg):
    random.seed(2)
    one = np.zeros((3, 4), bool)
    one[1, 2] = True
    for _ in range(5):
        out = ifg.make_random_subaperture_mask((7, 9), one)
        assert out.dtype == torch.bool and tuple(out.shape) == (7, 9) and int(out.sum()) == 1
        r, c = (int(v) for v in torch.nonzero(out)[0])
        assert 1 <= r <= 5 and 2 <= c <= 7
    full = ifg.make_random_subaperture_mask((3, 4), dev(np.ones((3, 4))))
    assert bool(full.all())
    with pytest.raises(ValueError, match='fit inside'):
        ifg.make_random_subaperture_mask((3, 3), one)


def test_fit_psd_takes_device_vectors(ifg, G):
    got = ifg.fit_psd(dev(C.FIT_F), dev(C.noisy_curve()))
    np.testing.assert_allclose(got, G['fit_noisy'], rtol=C.FIT_RTOL_NOISY)
    np.testing.assert_allclose(ifg.fit_psd(dev(C.FIT_F), dev(PP.ab(C.FIT_F, *C.FIT_AB)), callable=ifg.ab_psd), C.FIT_AB, rtol=C.FIT_RTOL_AB)


# ----------------------------------------------------------------------------- the kernels alone
def framed(a, fill=np.nan):
    """(the whole tensor, the window holding `a`) -- a window with ld > cols inside a frame of NaN"""
    fr, fc = C.FRAME
    shape = a.shape[:-2] + (a.shape[-2] + 2 * fr, a.shape[-1] + 2 * fc)
    whole = torch.full(shape, fill, dtype=dev(a[..., :1, :1]).dtype, device='cuda')
    win = whole[..., fr:fr + a.shape[-2], fc:fc + a.shape[-1]]
    win.copy_(dev(a))
    return whole, win


def frame_untouched(whole, win):
    bad = torch.isnan(torch.view_as_real(whole)[..., 0]) if whole.is_complex() else torch.isnan(whole)
    return int(bad.sum()) >= whole.numel() - win.numel() and bool(bad[..., :C.FRAME[0], :].all()) and bool(bad[..., :, :C.FRAME[1]].all()) \
        and bool(bad[..., -C.FRAME[0]:, :].all()) and bool(bad[..., :, -C.FRAME[1]:].all())


def parts(z):
    return np.stack([z.real, z.imag])


@pytest.mark.parametrize('cols', C.COLS)
@pytest.mark.parametrize('dt', DTYPES)
def test_signal_kernel_against_the_model(ops, dt, cols):
    _ops, L = ops
    shape = (C.COLS_ROWS, cols)
    X = C.spectrum(shape, dt, batch=2)      # exact zeros among the elements: the phasor is 1 there
    psd = C.positive(shape, dt)
    psd[3, 5] = -2.0                        # a negative psd: NaN, as in the reference
    assert (X == 0).sum() >= 4 and X[0, 3, 5] != 0
    for label, build in (('contiguous', lambda: (None, dev(X))), ('framed', lambda: framed(X))):
        whole, win = build()
        out = _ops.psd_signal(win, 2.5, psd=dev(psd))
        assert out.data_ptr() == win.data_ptr()
        got, want = host(win), PP.signal(X, psd, 2.5)
        assert np.isnan(got[:, 3, 5]).all() and np.array_equal(got[X == 0], want[X == 0])
        C.compare('model', 'signal', parts(got), parts(want), dt, f'array psd, {cols} columns, {label}')
        assert whole is None or frame_untouched(whole, win)
    for kind, p in ((PP.ABC, (1e4, 0.1, 2.5)), (PP.AB, (1e2, 2.0, 0.0))):
        whole, win = framed(X)
        _ops.psd_signal(win, 0.7, model=(kind,) + p + (0.1,))
        want = PP.signal(X, PP.model_psd(kind, shape, 0.1, *p, dtype=dt), 0.7)
        C.compare('model', 'signal', parts(host(win)), parts(want), dt, f'model {kind}, {cols} columns')
        assert frame_untouched(whole, win)
    again = dev(X)
    _ops.psd_signal(again, 2.5, psd=dev(psd))
    assert np.array_equal(host(again), got, equal_nan=True)      # a repeated call returns the same bits


@pytest.mark.parametrize('cols', C.COLS)
@pytest.mark.parametrize('dt', DTYPES)
def test_finish_and_scale_kernels_against_the_model(ops, dt, cols):
    _ops, L = ops
    shape = (C.COLS_ROWS, cols)
    field = C.integer_field(shape, dt, batch=3)
    mask = np.random.default_rng(5).random(shape) > 0.3
    none = np.zeros(shape, bool)
    for label, kw, mk in (('no mask', {}, dict()), ('array', dict(mask=dev(mask)), dict(mask_kind=PP.MASK_ARRAY, mask=mask)),
                          ('circle', dict(circle=(2.6, 0.1)), dict(mask_kind=PP.MASK_CIRCLE, radius=2.6, step=0.1)),
                          ('all masked', dict(mask=dev(none)), dict(mask_kind=PP.MASK_ARRAY, mask=none))):
        fw, fwin = framed(field)
        zw, zwin = framed(np.zeros((3,) + shape, dt))
        z, sums = _ops.psd_finish(fwin, out=zwin, **kw)
        wz, wsums = PP.finish(field, **mk)
        assert np.array_equal(host(z), wz, equal_nan=True), label      # the real part, NaN outside the mask
        assert np.array_equal(host(sums), wsums), label                # integer data: count and sum of squares to the bit
        assert frame_untouched(zw, zwin) and np.array_equal(host(fwin), field)
        _ops.psd_scale(zwin, sums, 3.0)
        C.compare('model', 'scale', host(zwin), PP.scale(wz, wsums, 3.0), dt, f'{label}, {cols} columns')
        assert frame_untouched(zw, zwin)
        if label == 'all masked':
            assert np.isnan(host(zwin)).all() and not host(sums).any()      # left unscaled, all NaN
        elif label == 'circle':
            assert 0 < np.isnan(wz).sum() < wz.size


@pytest.mark.parametrize('dt', DTYPES)
def test_finish_fold_on_the_second_trip(ops, dt):
    """(1024, 513): every first-stage thread makes a second trip; integer data, so the sums are exact in any order"""
    _ops, L = ops
    field = C.integer_field(C.SECOND_TRIP_SHAPE, dt, batch=2)
    f = dev(field)
    z, sums = _ops.psd_finish(f, circle=(300.0, 1.0))
    wz, wsums = PP.finish(field, PP.MASK_CIRCLE, radius=300.0, step=1.0)
    assert np.array_equal(host(z), wz, equal_nan=True) and np.array_equal(host(sums), wsums)
    z2, sums2 = _ops.psd_finish(f, circle=(300.0, 1.0))
    assert np.array_equal(host(sums2), host(sums)) and np.array_equal(host(z2), host(z), equal_nan=True)
    noisy = C.spectrum(C.SECOND_TRIP_SHAPE, dt, zeros=False)[None]
    zn, sn = _ops.psd_finish(dev(noisy))
    wn, wsn = PP.finish(noisy)
    assert host(sn)[0, 0] == wsn[0, 0]
    C.compare('model', 'sums', host(sn)[0, 1], wsn[0, 1], np.float64, 'sum of squares of 525312 values')
    _ops.psd_scale(zn, sn, 2.0)
    C.compare('model', 'scale', host(zn), PP.scale(wn, host(sn), 2.0), dt, 'second trip')
