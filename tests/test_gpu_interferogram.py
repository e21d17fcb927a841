"""GPU: prysm_amd.interferogram and prysm_amd.util on an MI355X -- every kernel of csrc/interferogram.hip against its numpy model
(prysm_amd/interferogram_plan.py) on the smallest shapes that can go wrong, and the public layer against the reference's outputs in
tests/golden/interferogram.npz.  Cases and bounds: tests/interferogram_common.py; each comparison prints measured against bound."""
import numpy as np
import pytest
import torch

import interferogram_common as C
from prysm_amd import interferogram_plan as IP

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
EXACT = (IP.N, IP.NNAN, IP.SUM, IP.SUMSQ, IP.MIN, IP.MAX, IP.ROW0, IP.ROW1, IP.COL0, IP.COL1, IP.MEAN)
SUMS = (IP.SAD, IP.M2, IP.STD, IP.RMS, IP.SA)


@pytest.fixture(scope='module')
def G():
    return C.golden()


@pytest.fixture(scope='module')
def ops(pa):
    from prysm_amd import _lib, _ops
    return _ops, _lib


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


def check_record(rec, z, label):
    """a record against the model: the selections and the counts to the bit, the sums within the model's bound"""
    want = IP.stats(z)
    assert np.array_equal(rec[[IP.N, IP.NNAN, IP.MIN, IP.MAX, IP.ROW0, IP.ROW1, IP.COL0, IP.COL1]],
                          want[[IP.N, IP.NNAN, IP.MIN, IP.MAX, IP.ROW0, IP.ROW1, IP.COL0, IP.COL1]], equal_nan=True), label
    for k in (IP.SUM, IP.SUMSQ, IP.MEAN) + SUMS:
        C.compare('model', 'stat', rec[k], want[k], np.float64, f'{label} [{k}]')


# ----------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('dt', DTYPES)
def test_stats_of_tiny_and_all_nan_maps(ops, dt):
    _ops, _ = ops
    for shape in C.TINY_SHAPES:
        z = (np.arange(shape[0] * shape[1], dtype=dt).reshape(shape) - 2) * dt(1.5)
        rec = host(_ops.ifg_stats(dev(z)))
        assert np.array_equal(rec, IP.stats(z)), shape      # a handful of exact values: to the bit
    z = np.full(C.ALL_NAN_SHAPE, np.nan, dtype=dt)
    rec = host(_ops.ifg_stats(dev(z)))
    assert rec[IP.N] == 0 and rec[IP.NNAN] == 15 and (rec[[IP.ROW0, IP.ROW1, IP.COL0, IP.COL1]] == -1).all()
    assert np.isnan(rec[[IP.MIN, IP.MAX, IP.MEAN, IP.STD, IP.RMS, IP.SA]]).all() and rec[IP.SUM] == 0
    from prysm_amd import util
    assert np.isnan(util.rms(z)) and np.isnan(util.pv(z)) and np.isnan(util.mean(z))
    # inf is in neither count and in no sum
    z = np.array([[1, np.inf, 3], [np.nan, -np.inf, 5]], dtype=dt)
    rec = host(_ops.ifg_stats(dev(z)))
    assert np.array_equal(rec, IP.stats(z)) and rec[IP.N] == 3 and rec[IP.NNAN] == 1 and rec[IP.MEAN] == 3


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('cols', C.COLS)
def test_stats_and_edits_around_a_wavefront_of_columns(ops, cols, dt):
    _ops, L = ops
    z = C.noisy_data((C.COLS_ROWS, cols), dt)
    t = dev(z)
    rec = _ops.ifg_stats(t)
    check_record(host(rec), z, f'{cols} columns')
    assert torch.equal(rec, _ops.ifg_stats(t))      # the same call twice: the same bits
    std = float(rec[IP.STD])
    keep = np.random.default_rng(cols).random(z.shape) < 0.7
    assert np.array_equal(host(_ops.ifg_edit(t.clone(), L.PM_IFG_FILL, value=-2.5)), IP.fill(z, -2.5))
    assert np.array_equal(host(_ops.ifg_edit(t.clone(), L.PM_IFG_MASK, mask=dev(keep))), IP.mask(z, keep), equal_nan=True)
    shifted = z - dt(500)
    srec = _ops.ifg_stats(dev(shifted))
    got = host(_ops.ifg_edit(dev(shifted), L.PM_IFG_CLIP, value=1.5, record=srec))
    want = IP.clip(shifted, 1.5, float(srec[IP.STD]))
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(want).sum() > np.isnan(z).sum() and std > 0


@pytest.mark.parametrize('dt', DTYPES)
def test_integer_data_is_exact_on_the_second_trip(ops, dt):
    """every first-stage thread makes a second trip of its grid-stride loop; count, sum, sum of squares, extrema and mean of small
    integers are exact in double in any order, so they equal numpy's to the bit"""
    _ops, _ = ops
    z = C.integer_data(C.SECOND_TRIP_SHAPE, dt)
    assert z.size >= IP.second_trip_elements()
    rec = host(_ops.ifg_stats(dev(z)))
    want = IP.stats(z)
    assert np.array_equal(rec[list(EXACT)], want[list(EXACT)])
    for k in SUMS:
        C.compare('model', 'stat', rec[k], want[k], np.float64, f'second trip [{k}]')
    # the fit's sums on the second trip: z = 2 x - 3 y + 7 on integer coordinates, every sum exact
    rows, cols = C.SECOND_TRIP_SHAPE
    x, y = IP.grid_xy((rows, cols), (rows // 2, cols // 2), 1.0, dt)
    zz = (2 * x - 3 * y + 7).astype(dt)
    co = _ops.ifg_coords(torch.float32 if dt == np.float32 else torch.float64, 0, origin=(rows // 2, cols // 2), dx=1.0)
    coef = host(_ops.ifg_fit(dev(zz), 7, co))
    want = IP.fit(zz, 7, x, y)
    assert np.array_equal(coef, want) and np.abs(want[:3] - (7, 2, -3)).max() < 1e-9


@pytest.mark.parametrize('dt', DTYPES)
def test_a_window_with_a_leading_dimension_inside_a_frame(ops, dt):
    """statistics of the view equal those of a contiguous copy bit for bit; in-place edits leave the frame untouched"""
    _ops, L = ops
    z = C.noisy_data((11, 29), dt)
    fr, fc = C.FRAME
    for sentinel in (np.nan, -12345.0):
        frame = np.full((z.shape[0] + 2 * fr, z.shape[1] + 2 * fc), sentinel, dtype=dt)
        frame[fr:-fr, fc:-fc] = z
        ft = dev(frame)
        view = ft[fr:-fr, fc:-fc]
        assert view.stride(0) > view.shape[1]
        assert torch.equal(_ops.ifg_stats(view), _ops.ifg_stats(dev(z)))
        tdt = ft.dtype
        co = _ops.ifg_coords(tdt, 0, origin=(5, 14), dx=0.5)
        coef = _ops.ifg_fit(view, 15, co)
        assert torch.equal(coef, _ops.ifg_fit(dev(z), 15, co))
        _ops.ifg_remove(view, 15, co, coef)
        _ops.ifg_edit(view, L.PM_IFG_CLIP, value=2.0, record=_ops.ifg_stats(view))
        _ops.ifg_edit(view, L.PM_IFG_MASK, mask=dev(np.random.default_rng(1).random(z.shape) < 0.8))
        _ops.ifg_edit(view, L.PM_IFG_FILL, value=1.0)
        after = host(ft)
        border = np.ones(frame.shape, dtype=bool)
        border[fr:-fr, fc:-fc] = False
        assert np.array_equal(after[border], frame[border], equal_nan=True)
        assert not np.isnan(after[~border]).any()
        gx, gy, gr = _ops.ifg_slope(view, 0.25)
        for got, want in zip((gx, gy, gr), _ops.ifg_slope(view.contiguous(), 0.25)):
            assert torch.equal(got, want)


# ----------------------------------------------------------------------------- fit and removal
@pytest.mark.parametrize('dt', DTYPES)
def test_fit_of_an_exact_plane_in_every_coordinate_form(ops, dt):
    _ops, L = ops
    tdt = torch.float32 if dt == np.float32 else torch.float64
    rows, cols = C.FIT_SHAPE
    x, y = IP.grid_xy(C.FIT_SHAPE, (rows // 2, cols // 2), 1.0, dt)
    z = (C.FIT_A * x + C.FIT_B * y).astype(dt) + np.zeros(C.FIT_SHAPE, dtype=dt)
    z[3, 4] = z[9, 20] = np.nan
    t = dev(z)
    xv, yv = dev(x[0].astype(dt)), dev(y[:, 0].astype(dt))
    x2, y2 = dev(np.broadcast_to(x, C.FIT_SHAPE).astype(dt)), dev(np.broadcast_to(y, C.FIT_SHAPE).astype(dt))
    forms = {
        'generated': _ops.ifg_coords(tdt, L.PM_COORDS_GRID, origin=(rows // 2, cols // 2), dx=1.0),
        'vectors': _ops.ifg_coords(tdt, L.PM_COORDS_SEPARABLE, x=xv, y=yv),
        'arrays': _ops.ifg_coords(tdt, L.PM_COORDS_POINTWISE, x=x2, y=y2),
    }
    terms = L.PM_IFG_TERM_X | L.PM_IFG_TERM_Y
    want = IP.fit(z, terms, x, y)
    G_, _ = IP.fit_sums(z, x, y)
    cond = np.linalg.cond(G_[1:3, 1:3])
    first = None
    for name, co in forms.items():
        coef = _ops.ifg_fit(t, terms, co)
        assert torch.equal(coef, _ops.ifg_fit(t, terms, co))
        c = host(coef)
        # the sums are of integers and exact multiples of 1 / 8: exact in double, so the three forms and the model agree to the bit
        assert np.array_equal(c, want), name
        first = c if first is None else first
        assert np.array_equal(c, first)
        # a 2 x 2 elimination loses at most a few eps cond(G) of the exact coefficients
        assert np.abs(c[1:3] - (C.FIT_A, C.FIT_B)).max() <= 8 * 2 * C.eps(np.float64) * cond * abs(C.FIT_B), name
        got = host(_ops.ifg_remove(t.clone(), terms, co, coef))
        assert np.array_equal(got, IP.remove(z, terms, c, x, y), equal_nan=True)
        assert np.nanmax(np.abs(got)) <= 64 * C.eps(dt) * np.nanmax(np.abs(z))


@pytest.mark.parametrize('dt', DTYPES)
def test_fit_and_removal_against_the_model(ops, dt):
    _ops, L = ops
    tdt = torch.float32 if dt == np.float32 else torch.float64
    z = C.noisy_data((C.COLS_ROWS, 65), dt)
    t = dev(z)
    x, y = IP.grid_xy(z.shape, (2, 40), 0.3, dt)
    co = _ops.ifg_coords(tdt, L.PM_COORDS_GRID, origin=(2, 40), dx=0.3)
    lx, ly = IP.linspace_xy(z.shape)
    lin = _ops.ifg_coords(tdt, L.PM_COORDS_GRID, linspace=(-1.0, IP.linspace_step(65), -1.0, IP.linspace_step(C.COLS_ROWS)))
    for terms, c, cx, cy, label in ((1, co, x, y, 'piston'), (6, co, x, y, 'plane'), (15, co, x, y, 'all four'), (9, lin, lx, ly, 'sphere')):
        coef = _ops.ifg_fit(t, terms, c)
        want = IP.fit(z, terms, cx, cy)
        C.compare('model', 'coef', host(coef), want, np.float64, label)
        got = host(_ops.ifg_remove(t.clone(), terms, c, coef))
        assert np.array_equal(got, IP.remove(z, terms, host(coef), cx, cy), equal_nan=True), label      # pointwise: the same arithmetic
    # a rank-deficient fit drops the term and adds no NaN
    zero = _ops.ifg_coords(tdt, L.PM_COORDS_GRID, origin=(0, 0), dx=0.0)
    coef = _ops.ifg_fit(t, 6, zero)
    assert np.array_equal(host(coef), np.zeros(4))
    assert np.array_equal(host(_ops.ifg_remove(t.clone(), 6, zero, coef)), z, equal_nan=True)
    allnan = dev(np.full(C.ALL_NAN_SHAPE, np.nan, dtype=dt))
    assert np.array_equal(host(_ops.ifg_fit(allnan, 15, co)), np.zeros(4))


@pytest.mark.parametrize('dt', DTYPES)
def test_fit_removal_and_edits_of_tiny_maps(ops, dt):
    _ops, L = ops
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for shape in C.TINY_SHAPES + (C.ALL_NAN_SHAPE,):
        z = (np.arange(shape[0] * shape[1], dtype=dt).reshape(shape) - 2) * dt(1.5)
        if shape == C.ALL_NAN_SHAPE:
            z[:] = np.nan
        elif z.size > 1:
            z.flat[1] = np.nan
        origin = (shape[0] // 2, shape[1] // 2)
        x, y = IP.grid_xy(shape, origin, 0.5, dt)
        co = _ops.ifg_coords(tdt, L.PM_COORDS_GRID, origin=origin, dx=0.5)
        for terms in (1, 6, 15):
            coef = host(_ops.ifg_fit(dev(z), terms, co))
            want = IP.fit(z, terms, x, y)      # a few exact values: the sums, and so the elimination, agree to the bit
            assert np.array_equal(coef, want) and np.isfinite(coef).all(), (shape, terms)
            got = host(_ops.ifg_remove(dev(z), terms, co, dev(coef)))
            assert np.array_equal(got, IP.remove(z, terms, coef, x, y), equal_nan=True), (shape, terms)
        keep = np.arange(z.size).reshape(shape) % 2 == 0
        assert np.array_equal(host(_ops.ifg_edit(dev(z), L.PM_IFG_FILL, value=9.0)), IP.fill(z, 9.0))
        assert np.array_equal(host(_ops.ifg_edit(dev(z), L.PM_IFG_MASK, mask=dev(keep))), IP.mask(z, keep), equal_nan=True)
        rec = _ops.ifg_stats(dev(z))
        got = host(_ops.ifg_edit(dev(z), L.PM_IFG_CLIP, value=1.0, record=rec))
        assert np.array_equal(got, IP.clip(z, 1.0, float(rec[IP.STD])), equal_nan=True)


def test_coordinate_arrays_that_do_not_match_are_refused(pa, ops):
    from prysm_amd import interferogram
    _ops, L = ops
    z = dev(C.noisy_data((5, 7), np.float64))
    x, y = np.arange(7.0), np.arange(5.0)
    for xs, ys in ((x[:6], y), (x, y[:4]), (x[None, :], y[:, None]), (np.zeros((6, 8)), np.zeros((6, 8)))):
        with pytest.raises(ValueError, match='data of shape'):
            interferogram.fit_plane(xs, ys, z)
    I = interferogram.Interferogram(z.clone(), dx=0.1)
    I.x = dev(np.zeros((9, 9)))      # the uncropped grid of some other map
    with pytest.raises(ValueError, match='data of shape'):
        I.remove_tiptilt()
    assert torch.equal(interferogram.fit_plane(x, y, z), interferogram.fit_plane(*np.meshgrid(x, y), z))


# ----------------------------------------------------------------------------- slope, windows, band, filter design, PSD models
@pytest.mark.parametrize('dt', DTYPES)
def test_slope_against_the_model(ops, dt):
    _ops, _ = ops
    for shape in ((2, 2), (5, 65), (C.COLS_ROWS, 64)):
        z = C.noisy_data(shape, dt, seed=shape[1])
        gx, gy, gr = (host(v) for v in _ops.ifg_slope(dev(z), 0.3))
        wx, wy, wr = IP.slope(z, 0.3)
        assert np.array_equal(gx, wx, equal_nan=True) and np.array_equal(gy, wy, equal_nan=True)      # differences and one division
        C.compare('model', 'hypot', gr, wr, dt, f'slope magnitude {shape}')


@pytest.mark.parametrize('dt', DTYPES)
def test_windows_against_the_model(ops, dt):
    _ops, L = ops
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for shape in ((1, 7), (9, 63), (8, 64), C.SQUARE_SHAPE):
        h = C.noisy_data(shape, dt, seed=5)
        h[np.isnan(h)] = 0
        for kind, kw in ((L.PM_IFG_WIN_HANN, {}), (L.PM_IFG_WIN_WELCH, dict(dx=0.1, alpha=4)), (L.PM_IFG_WIN_WELCH, dict(dx=0.1, alpha=2.5))):
            if kind == L.PM_IFG_WIN_WELCH and shape[0] == 1:
                continue      # rmax = 0: the reference divides by zero
            w = IP.window(kind, shape, kw.get('dx', 0.0), kw.get('alpha', 4), dt)
            want, s2 = IP.windowed(h, w)
            got, gs2 = _ops.ifg_window(kind, shape, tdt, height=dev(h), **kw)
            again, gs2b = _ops.ifg_window(kind, shape, tdt, height=dev(h), **kw)
            assert torch.equal(gs2, gs2b) and torch.equal(got, again)      # the same call twice: the same bits
            C.compare('model', 'window', host(got), want, dt, f'kind {kind} {shape}')
            C.compare('model', 's2', float(gs2), s2, dt, f'S2 kind {kind} {shape}')
            alone, _ = _ops.ifg_window(kind, shape, tdt, **kw)
            C.compare('model', 'window', host(alone), w.astype(dt), dt, f'window alone {kind} {shape}')
        w = np.random.default_rng(3).random(shape).astype(dt)
        got, gs2 = _ops.ifg_window(L.PM_IFG_WIN_ARRAY, shape, tdt, height=dev(h), window=dev(w))
        want, s2 = IP.windowed(h, w.astype(np.float64))
        assert np.array_equal(host(got), want)
        C.compare('model', 's2', float(gs2), s2, dt, f'S2 array {shape}')


@pytest.mark.parametrize('dt', DTYPES)
def test_band_against_the_model(ops, dt):
    _ops, _ = ops
    for shape in ((1, 5), (9, 63), C.SQUARE_SHAPE, (5, 1)):
        p = np.random.default_rng(shape[1]).random(shape).astype(dt)
        nu = IP.band_nu(shape, C.DX)
        for flow, fhigh in ((0.3, 2.0), (0.0, np.inf)):
            want = IP.band(p, nu, flow, fhigh) if shape[0] > 1 else (0.0, abs(nu[-1, shape[1] // 2] - nu[0, shape[1] // 2]))
            got = host(_ops.ifg_band(dev(p), flow, fhigh, dx=C.DX))
            assert np.array_equal(got, host(_ops.ifg_band(dev(p), flow, fhigh, dx=C.DX)))      # the same call twice: the same bits
            C.compare('model', 'band', got[0], want[0], np.float64, f'generated {shape} {flow}')
            assert got[1] == 1 / (shape[0] * C.DX) or shape[0] == 1
            got = host(_ops.ifg_band(dev(p), flow, fhigh, nu=dev(nu.astype(dt))))
            want = IP.band(p, nu.astype(dt), flow, fhigh) if shape[0] > 1 else (0.0, 0.0)
            C.compare('model', 'band', got[0], want[0], np.float64, f'read {shape} {flow}')
    p = np.random.default_rng(2).random(33).astype(dt)
    nu = (np.arange(33) * 0.25).astype(dt)
    got = host(_ops.ifg_band(dev(p), 1.0, 5.0, nu=dev(nu)))
    want = IP.band(p, nu, 1.0, 5.0)
    C.compare('model', 'band', got[0], want[0], np.float64, '1-D')
    assert got[1] == want[1] == 0.25


@pytest.mark.parametrize('dt', DTYPES)
def test_filter_design_against_the_model(ops, dt):
    _ops, L = ops
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for shape in ((9, 63), C.SQUARE_SHAPE, (33, 33)):
        x, y = IP.grid_xy(shape, (shape[0] // 2, shape[1] // 2), C.DX, dt)
        r = np.hypot(x.astype(dt), y.astype(dt))
        lo, hi = _ops.ifg_iir(shape, tdt, C.DX, 0.1, 0.4, origin=(shape[0] // 2, shape[1] // 2), r_dx=C.DX)
        C.compare('model', 'iir', host(lo), IP.iir(r, C.DX, 0.1), dt, f'generated low {shape}')
        C.compare('model', 'iir', host(hi), IP.iir(r, C.DX, 0.4), dt, f'generated high {shape}')
        lo2, none = _ops.ifg_iir(shape, tdt, C.DX, 0.1, r=dev(r))
        assert none is None
        C.compare('model', 'iir', host(lo2), IP.iir(r, C.DX, 0.1), dt, f'read low {shape}')
        w = host(_ops.ifg_iir(shape, tdt, 1.0, 0.0, parts=L.PM_IFG_IIR_HANN)[0])
        C.compare('model', 'iir', w, IP.hann2d(*shape).astype(dt), dt, f'hann2d {shape}')
        a, b = np.random.default_rng(1).random(shape).astype(dt), np.random.default_rng(2).random(shape).astype(dt)
        for typ in (L.PM_IFG_LP, L.PM_IFG_HP, L.PM_IFG_BP, L.PM_IFG_BR):
            want = IP.combine(typ, a, b)
            assert np.array_equal(host(_ops.ifg_combine(typ, dev(a), dev(b))), want)
            cplx = host(_ops.ifg_combine(typ, dev(a), dev(b), complex_out=True))
            assert np.array_equal(cplx.real, want) and not cplx.imag.any()


@pytest.mark.parametrize('dt', DTYPES)
def test_psd_models_against_the_model(pa, precision, dt):
    from prysm_amd import interferogram
    precision(dt)
    nu = np.linspace(0.05, 9, 130).astype(dt)
    C.compare('model', 'psd_model', host(interferogram.abc_psd(dev(nu), 3.0, 0.5, 2.5)), IP.psd_model(IP.PSD_ABC, nu, 3.0, 0.5, 2.5), dt, 'abc')
    C.compare('model', 'psd_model', host(interferogram.ab_psd(dev(nu), 3.0, 1.5)), IP.psd_model(IP.PSD_AB, nu, 3.0, 1.5), dt, 'ab')
    assert interferogram.abc_psd(2.0, 3.0, 0.5, 2.0) == 3.0 / 17 and interferogram.ab_psd(2.0, 3.0, 2) == 0.75


# ----------------------------------------------------------------------------- the public layer against the golden
@pytest.mark.parametrize('key,dt', [('main_f64', np.float64), ('main_f32', np.float32), ('inf', np.float64)])
def test_interferogram_pipeline_against_golden(pa, precision, G, key, dt):
    from prysm_amd import interferogram, util
    precision(dt)
    z = C.main_case(dt, inf=key == 'inf')
    I = interferogram.Interferogram(z.copy(), dx=C.DX)
    assert I.data.dtype == (torch.float32 if dt == np.float32 else torch.float64)
    assert I.dropout_percentage == G[f'{key}_dropout']
    raw = (I.pv, I.rms, I.Sa, I.std, util.mean(I.data))
    assert all(isinstance(v, float) for v in raw)
    assert raw[0] == G[f'{key}_raw'][0]      # pv: a maximum and a minimum are selections
    C.compare('golden', 'stat', raw, G[f'{key}_raw'], np.float64, f'{key} pv rms Sa std mean')
    base = I.data
    assert I.crop() is I and I.shape == tuple(G[f'{key}_shape']) == C.CROPPED
    assert I.data.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() and I.data.stride(0) == C.MAIN_SHAPE[1]      # a view
    assert I.crop() is I and I.shape == C.CROPPED
    sphere_before = None
    for stage in C.STAGES:
        if stage.startswith('piston'):
            assert I.remove_piston() is I
        elif stage == 'tilt':
            plane = host(interferogram.fit_plane(I.x, I.y, I.data))
            want = G[f'{key}_plane'][0] * host(I.x).astype(np.float64) + G[f'{key}_plane'][1] * host(I.y).astype(np.float64)
            C.compare('golden', 'coef', plane, want, dt, f'{key} fit_plane')
            assert I.remove_tiptilt() is I
        else:
            sphere_before = interferogram.fit_sphere(I.data)
            assert I.remove_power() is I
        C.compare('golden', 'removed', host(I.data), G[f'{key}_{stage}'], dt, f'{key} after {stage}')
    pts, sphere = sphere_before
    assert np.array_equal(host(pts), np.isfinite(G[f'{key}_tilt'])) and sphere.dim() == 1 and sphere.numel() == int(host(pts).sum())
    final = (I.pv, I.rms, I.Sa, I.std, I.strehl)
    C.compare('golden', 'stat', final[:4], G[f'{key}_final'][:4], dt, f'{key} cleaned pv rms Sa std')
    C.compare('golden', 'stat', final[4], G[f'{key}_final'][4], dt, f'{key} strehl')
    J = I.copy().fill(0)
    for name, rd in zip(('gx', 'gy', 'gr'), J.slope()):
        C.compare('golden', 'slope', host(rd.data), G[f'{key}_{name}'], dt, f'{key} {name}')
    valid = int(np.isfinite(host(I.data)).sum())
    assert I.spike_clip(C.NSIGMA) is I
    got = host(I.data)
    assert np.array_equal(np.isnan(got), np.isnan(G[f'{key}_clipped']))      # the clipped set, exactly
    assert valid - int(np.isfinite(got).sum()) == 5
    frame = host(base)
    outside = np.ones(C.MAIN_SHAPE, dtype=bool)
    r0, r1, c0, c1 = G[f'{key}_box']
    outside[r0:r1 + 1, c0:c1 + 1] = False
    assert np.isnan(frame[outside]).all()      # what lies around the cropped view is untouched


def test_edits_pad_and_coordinates_against_golden(pa, precision, G):
    from prysm_amd import interferogram
    precision(np.float64)
    z = C.main_case()
    new = lambda: interferogram.Interferogram(z.copy(), dx=C.DX)      # noqa: E731
    assert np.array_equal(host(new().mask(C.user_mask()).data), G['main_f64_masked'], equal_nan=True)
    assert np.array_equal(host(new().mask(dev(C.user_mask())).data), G['main_f64_masked'], equal_nan=True)
    assert np.array_equal(host(new().fill(-7.5).data), G['main_f64_filled'])
    I = new()
    with pytest.raises(ValueError, match='Neither'):
        I.pad()
    with pytest.raises(ValueError, match='only one'):
        I.pad(samples=2, shape=(50, 60))
    assert np.array_equal(host(I.pad(samples=C.PAD_SAMPLES).data), G['main_f64_padded'], equal_nan=True)
    want = np.full(G['main_f64_padded'].shape, 0.5)
    off = tuple(-(-p // 2) for p in C.PAD_SAMPLES)      # pad2d puts the data at ceil(d / 2)
    want[off[0]:off[0] + z.shape[0], off[1]:off[1] + z.shape[1]] = z
    assert np.array_equal(host(new().pad(0.5, shape=want.shape).data), want, equal_nan=True)
    inf = interferogram.Interferogram(C.main_case(inf=True), dx=C.DX).fill(0)
    assert np.isinf(host(inf.data)[C.INF_AT]) and not np.isnan(host(inf.data)).any()

    def xy(I):
        return host(I.x)[0], host(I.y)[:, 0]

    def same(I, name, exact=True):
        gx, gy = xy(I)
        if exact:
            assert np.array_equal(gx, G[f'coord_{name}_x']) and np.array_equal(gy, G[f'coord_{name}_y']), name
        else:
            for g, w in ((gx, G[f'coord_{name}_x']), (gy, G[f'coord_{name}_y'])):
                assert g.shape == w.shape and np.abs(g - w).max() <= 2 * C.eps(np.float64) * max(1.0, np.abs(w).max()), name
    same(new().crop(), 'unseen_crop')
    I = new()
    I.x
    same(I.crop(), 'seen_crop')
    assert tuple(I.r.shape) == C.CROPPED
    C.compare('model', 'hypot', host(I.r), np.hypot(host(I.x), host(I.y)), np.float64, 'Interferogram.r')
    same(I.recenter(), 'recenter', exact=False)
    same(new().remove_tiptilt().crop(), 'tilt_crop')      # remove_tiptilt reads x and y, so the crop carries them
    same(new().remove_piston().crop(), 'unseen_crop')     # ... a piston reads none
    I = new()
    I.x
    same(I.crop().pad(samples=C.PAD_SAMPLES), 'pad')
    same(I.crop(), 'pad_crop')
    same(I.latcal(0.25), 'latcal')
    assert I.dx == 0.25
    same(I.strip_latcal(), 'strip')
    assert I.dx == 1.0
    # assigning .x switches the object to arrays, which the fit then reads
    I = new().crop()
    a = new().crop()
    a.x = a.x * 1
    assert a.grid is None and I.grid is not None
    assert torch.equal(I.remove_piston().remove_tiptilt().data.nan_to_num(), a.remove_piston().remove_tiptilt().data.nan_to_num())


@pytest.mark.parametrize('dt', DTYPES)
def test_spectra_and_filters_against_golden(pa, precision, G, dt):
    from prysm_amd import interferogram
    from prysm_amd._richdata import RichData
    precision(dt)
    z = C.square_case(dt)
    I = interferogram.Interferogram(z.copy(), dx=C.DX)
    p = I.psd()
    assert isinstance(p, RichData) and tuple(p.x.shape) == C.SQUARE_SHAPE
    C.compare('golden', 'psd', host(p.data), G['sq_psd'], dt, 'psd, Hann by the corner test')
    ux, uy, pw = interferogram.psd(dev(z), C.DX, 'welch')
    C.compare('golden', 'psd', host(pw), G['sq_psd_welch'], dt, 'psd, Welch')
    assert np.array_equal(host(ux)[0], np.fft.fftshift(np.fft.fftfreq(48, C.DX)).astype(dt))
    w = interferogram.make_window(dev(z), C.DX)
    C.compare('model', 'window', host(w), IP.window(IP.WIN_HANN, z.shape).astype(dt), dt, 'make_window(None)')
    _, _, pa_ = interferogram.psd(dev(z), C.DX, w)
    C.compare('golden', 'psd', host(pa_), G['sq_psd'], dt, 'psd, window given as an array')
    for name, kw in C.BANDS:
        got = I.bandlimited_rms(**kw)
        assert isinstance(got, float)
        C.compare('golden', 'band', got, G[f'sq_band_{name}'], dt, f'bandlimited_rms {name}')
        got = interferogram.bandlimited_rms(dev(IP.band_nu(z.shape, C.DX).astype(dt)), p.data, **kw)
        C.compare('golden', 'band', got, G[f'sq_band_{name}'], dt, f'bandlimited_rms function {name}')
    C.compare('golden', 'band', I.total_integrated_scatter(C.TIS_WVL), G['sq_tis'], dt, 'total_integrated_scatter')
    with pytest.raises(ValueError):
        I.bandlimited_rms()
    for typ, fc in C.FILTERS:
        J = interferogram.Interferogram(z.copy(), dx=C.DX)
        H = interferogram.designfilt2d(J.r, C.DX, fc, typ)
        C.compare('golden', 'H', host(H), G[f'sq_H_{typ}'], dt, f'designfilt2d {typ}')
        assert J.filter(fc, typ) is J
        C.compare('golden', 'filtered', host(J.data), G[f'sq_filtered_{typ}'], dt, f'filter {typ}')
    for name, rd in zip(('gx', 'gy', 'gr'), I.slope()):
        C.compare('golden', 'slope', host(rd.data), G[f'sq_{name}'], dt, f'square {name}')
    rr = np.hypot(*C.grid(C.SQUARE_SHAPE)).astype(dt)
    welch = host(interferogram.window_2d_welch(dev(rr), alpha=4))
    want = 1 - np.abs(rr / rr[C.SQUARE_SHAPE[0] - 1, C.SQUARE_SHAPE[1] // 2]) ** 4      # the reference's expression, in dt
    C.compare('model', 'window', welch, want, dt, 'window_2d_welch')
    h2 = host(interferogram.hann2d(*C.SQUARE_SHAPE))
    C.compare('model', 'iir', h2, IP.hann2d(*C.SQUARE_SHAPE).astype(dt), dt, 'hann2d')
    r = np.hypot(*C.grid(C.SQUARE_SHAPE)).astype(dt)
    lpf = host(interferogram.ideal_lpf_iir2d(dev(r), C.DX, 0.2))
    want = IP.jinc(r.astype(np.float64) * (np.pi * 0.2 / C.DX)) * (0.2 ** 2 * np.pi / 2)
    C.compare('model', 'iir', lpf, want.astype(dt), dt, 'ideal_lpf_iir2d')


@pytest.mark.parametrize('dt', DTYPES)
def test_psd_of_an_odd_shape_against_the_model(pa, precision, dt):
    """a cropped map: odd rows and columns, the rotations n - n // 2, the real array through the complex transform"""
    from prysm_amd import interferogram
    precision(dt)
    z = C.noisy_data(C.CROPPED, dt, seed=9)
    z[np.isnan(z)] = 0
    for which, kind in (('hann', IP.WIN_HANN), ('welch', IP.WIN_WELCH)):
        _, _, p = interferogram.psd(dev(z), C.DX, which)
        want = IP.psd(z, C.DX, IP.window(kind, z.shape, C.DX, 4, dt))
        C.compare('model', 'psd', host(p), want, dt, f'odd shape {which}')
