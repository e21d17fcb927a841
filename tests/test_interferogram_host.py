"""CPU: the host side of prysm_amd.interferogram and prysm_amd.util -- the argument checks of every entry point of csrc/interferogram.hip
(refused before anything is launched, so no device is needed), the workspace queries, the numpy model of every kernel against the
reference's outputs in tests/golden/interferogram.npz, the coordinate bookkeeping against the reference's .x and .y, and the
reference's ValueErrors.  Cases and bounds: tests/interferogram_common.py."""
import ctypes

import numpy as np
import pytest

import interferogram_common as C
from prysm_amd import _lib as L
from prysm_amd import interferogram_plan as IP

P = ctypes.c_void_p(16)         # never dereferenced
ARG, WS = L.PM_ERR_ARG, L.PM_ERR_WORKSPACE
F32, F64 = L.PM_F32, L.PM_F64
BIG = 1 << 40
R, CO = 4, 6                    # rows and columns of every shape here


@pytest.fixture(scope='module')
def lib():
    return L.load()


@pytest.fixture(scope='module')
def G():
    return C.golden()


def grid_coords():
    co = L.pm_ifg_coords()
    co.mode, co.dx, co.dy = L.PM_COORDS_GRID, 0.1, 0.1
    return co


def array_coords(mode, ldx=CO, ldy=CO, x=16, y=16):
    co = L.pm_ifg_coords()
    co.mode, co.x, co.y, co.ldx, co.ldy = mode, x, y, ldx, ldy
    return co


# name: call(lib, dt, p, ld, ws) -> rc, with p the data pointer, ld the data's leading dimension and ws the workspace bytes
CALLS = {
    'pm_ifg_stats': lambda lib, dt, p, ld, ws: lib.pm_ifg_stats(dt, R, CO, p, ld, P, P, ws, None),
    'pm_ifg_fit': lambda lib, dt, p, ld, ws: lib.pm_ifg_fit(dt, 6, R, CO, p, ld, ctypes.byref(grid_coords()), P, P, ws, None),
    'pm_ifg_remove': lambda lib, dt, p, ld, ws: lib.pm_ifg_remove(dt, 6, R, CO, p, ld, ctypes.byref(grid_coords()), P, None),
    'pm_ifg_edit': lambda lib, dt, p, ld, ws: lib.pm_ifg_edit(dt, L.PM_IFG_FILL, R, CO, p, ld, 0.0, None, 0, None, None),
    'pm_ifg_slope': lambda lib, dt, p, ld, ws: lib.pm_ifg_slope(dt, R, CO, p, ld, 0.1, P, P, P, CO, None),
    'pm_ifg_window': lambda lib, dt, p, ld, ws: lib.pm_ifg_window(dt, L.PM_IFG_WIN_HANN, R, CO, P, ld, 0.1, 4.0, None, 0, p, CO, P, P, ws, None),
    'pm_ifg_psd_scale': lambda lib, dt, p, ld, ws: lib.pm_ifg_psd_scale(dt, R, CO, p, ld, P, 10.0, None),
    'pm_ifg_band': lambda lib, dt, p, ld, ws: lib.pm_ifg_band(dt, L.PM_COORDS_GRID, 2, R, CO, p, ld, None, 0, 0.1, 0.0, 1.0, P, P, ws, None),
    'pm_ifg_iir': lambda lib, dt, p, ld, ws: lib.pm_ifg_iir(dt, 3, L.PM_COORDS_GRID, R, CO, None, 0, 2, 3, 0.1, 0.1, 0.2, 0.4, p, P, ld, None),
    'pm_ifg_combine': lambda lib, dt, p, ld, ws: lib.pm_ifg_combine(dt, L.PM_IFG_BP, 0, R, CO, p, ld, P, CO, P, CO, None),
    'pm_ifg_psd_model': lambda lib, dt, p, ld, ws: lib.pm_ifg_psd_model(dt, L.PM_IFG_PSD_ABC, 8, p, 1.0, 2.0, 3.0, P, None),
}
WITH_WORKSPACE = ('pm_ifg_stats', 'pm_ifg_fit', 'pm_ifg_window', 'pm_ifg_band')
WITHOUT_LD = ('pm_ifg_psd_model',)


def refused(lib, rc, code, word):
    assert rc == code, (rc, lib.pm_last_error())
    assert word.encode() in lib.pm_last_error(), lib.pm_last_error()
    with pytest.raises(ValueError):
        L.check(rc)


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_point_refusals(lib, name):
    call = CALLS[name]
    for dt in (L.PM_C64, 99):
        refused(lib, call(lib, dt, P, CO, BIG), ARG, 'dtype')
        refused(lib, call(lib, dt, None, CO - 1, 0), ARG, 'dtype')      # the dtype is looked at first
    for dt in (F32, F64):
        refused(lib, call(lib, dt, None, CO, BIG), ARG, 'null pointer')
        if name not in WITHOUT_LD:
            refused(lib, call(lib, dt, P, CO - 1, BIG), ARG, 'leading dimension')
        if name in WITH_WORKSPACE:
            refused(lib, call(lib, dt, P, CO, 7), WS, 'workspace')      # the smallest of these workspaces is one double
            refused(lib, call(lib, dt, P, CO - 1, 7), ARG, 'leading dimension')      # ... and the shape before the workspace


def test_refusals_of_modes_and_coordinates(lib):
    co = grid_coords()
    refused(lib, lib.pm_ifg_fit(F64, 0, R, CO, P, CO, ctypes.byref(co), P, P, BIG, None), ARG, 'terms')
    refused(lib, lib.pm_ifg_fit(F64, 16, R, CO, P, CO, ctypes.byref(co), P, P, BIG, None), ARG, 'terms')
    refused(lib, lib.pm_ifg_remove(F64, 0, R, CO, P, CO, ctypes.byref(co), P, None), ARG, 'terms')
    refused(lib, lib.pm_ifg_fit(F64, 6, R, CO, P, CO, None, P, P, BIG, None), ARG, 'coordinates')
    bad = grid_coords()
    bad.mode = 7
    refused(lib, lib.pm_ifg_fit(F64, 6, R, CO, P, CO, ctypes.byref(bad), P, P, BIG, None), ARG, 'coords')
    bad = grid_coords()
    bad.dx = float('nan')
    refused(lib, lib.pm_ifg_remove(F64, 6, R, CO, P, CO, ctypes.byref(bad), P, None), ARG, 'finite')
    refused(lib, lib.pm_ifg_fit(F64, 6, R, CO, P, CO, ctypes.byref(array_coords(L.PM_COORDS_SEPARABLE, x=None)), P, P, BIG, None), ARG, 'coordinate arrays')
    refused(lib, lib.pm_ifg_fit(F64, 6, R, CO, P, CO, ctypes.byref(array_coords(L.PM_COORDS_POINTWISE, ldy=CO - 1)), P, P, BIG, None), ARG,
            'leading dimension')
    # a piston alone reads no coordinate array
    assert lib.pm_ifg_remove(F64, 1, 0, CO, P, CO, ctypes.byref(array_coords(L.PM_COORDS_SEPARABLE, x=None, y=None)), P, None) == 0
    refused(lib, lib.pm_ifg_edit(F32, 3, R, CO, P, CO, 0.0, None, 0, None, None), ARG, 'op')
    refused(lib, lib.pm_ifg_edit(F32, L.PM_IFG_MASK, R, CO, P, CO, 0.0, None, CO, None, None), ARG, 'mask')
    refused(lib, lib.pm_ifg_edit(F32, L.PM_IFG_MASK, R, CO, P, CO, 0.0, P, CO - 1, None, None), ARG, 'leading dimension')
    refused(lib, lib.pm_ifg_edit(F32, L.PM_IFG_CLIP, R, CO, P, CO, 3.0, None, 0, None, None), ARG, 'record')
    refused(lib, lib.pm_ifg_slope(F64, 1, CO, P, CO, 0.1, P, P, P, CO, None), ARG, '2 samples')
    refused(lib, lib.pm_ifg_slope(F64, R, CO, P, CO, 0.1, None, None, None, CO, None), ARG, 'no output')
    refused(lib, lib.pm_ifg_slope(F64, R, CO, P, CO, 0.1, P, P, P, CO - 1, None), ARG, 'leading dimension')
    refused(lib, lib.pm_ifg_window(F64, 5, R, CO, P, CO, 0.1, 4.0, None, 0, P, CO, P, P, BIG, None), ARG, 'kind')
    refused(lib, lib.pm_ifg_window(F64, L.PM_IFG_WIN_ARRAY, R, CO, P, CO, 0.1, 4.0, None, CO, P, CO, P, P, BIG, None), ARG, 'window array')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_SEPARABLE, 2, R, CO, P, CO, None, 0, 0.1, 0.0, 1.0, P, P, BIG, None), ARG, 'coords')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_GRID, 3, R, CO, P, CO, None, 0, 0.1, 0.0, 1.0, P, P, BIG, None), ARG, 'ndim')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_GRID, 1, R, CO, P, CO, None, 0, 0.1, 0.0, 1.0, P, P, BIG, None), ARG, '1-D')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_POINTWISE, 2, R, CO, P, CO, None, CO, 0.1, 0.0, 1.0, P, P, BIG, None), ARG, 'frequencies')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_GRID, 2, R, CO, P, CO, None, 0, 0.0, 0.0, 1.0, P, P, BIG, None), ARG, 'spacing')
    refused(lib, lib.pm_ifg_band(F64, L.PM_COORDS_GRID, 2, R, CO, P, CO, None, 0, 0.1, float('nan'), 1.0, P, P, BIG, None), ARG, 'NaN')
    refused(lib, lib.pm_ifg_iir(F64, 0, L.PM_COORDS_GRID, R, CO, None, 0, 2, 3, 0.1, 0.1, 0.2, 0.4, P, P, CO, None), ARG, 'parts')
    refused(lib, lib.pm_ifg_iir(F64, 3, L.PM_COORDS_POINTWISE, R, CO, None, CO, 2, 3, 0.1, 0.1, 0.2, 0.4, P, P, CO, None), ARG, 'radial')
    refused(lib, lib.pm_ifg_iir(F64, 3, L.PM_COORDS_GRID, R, CO, None, 0, 2, 3, 0.1, 0.0, 0.2, 0.4, P, P, CO, None), ARG, 'spacing')
    refused(lib, lib.pm_ifg_combine(F64, 4, 0, R, CO, P, CO, P, CO, P, CO, None), ARG, 'typ')
    refused(lib, lib.pm_ifg_combine(F64, L.PM_IFG_BR, 0, R, CO, P, CO, None, CO, P, CO, None), ARG, 'null pointer')
    refused(lib, lib.pm_ifg_psd_model(F64, 2, 8, P, 1.0, 2.0, 3.0, P, None), ARG, 'kind')


def test_empty_shapes_and_workspace_queries(lib):
    co = grid_coords()
    assert lib.pm_ifg_remove(F64, 6, 0, CO, P, CO, ctypes.byref(co), P, None) == 0
    assert lib.pm_ifg_edit(F32, L.PM_IFG_FILL, R, 0, P, CO, 0.0, None, 0, None, None) == 0
    assert lib.pm_ifg_psd_scale(F32, 0, 0, P, 0, P, 1.0, None) == 0
    assert lib.pm_ifg_psd_model(F32, 0, 0, P, 1.0, 1.0, 1.0, P, None) == 0
    refused(lib, lib.pm_ifg_stats(F64, 0, CO, P, CO, P, P, BIG, None), ARG, 'empty')
    wgs = lambda n: min(IP.WGS, -(-n // IP.THREADS))      # noqa: E731
    for shape in (C.MAIN_SHAPE, C.SECOND_TRIP_SHAPE, (1, 1)):
        n = shape[0] * shape[1]
        assert lib.pm_ifg_stats_workspace(*shape) == wgs(n) * 12 * 8
        assert lib.pm_ifg_fit_workspace(*shape) == wgs(n) * 14 * 8
        assert lib.pm_ifg_window_workspace(*shape) == lib.pm_ifg_band_workspace(*shape) == wgs(n) * 8
    assert lib.pm_ifg_stats_workspace(0, 5) == 0 and lib.pm_ifg_fit_workspace(5, -1) == 0
    # the shape of the second-trip test is one on which every first-stage thread makes a second trip, within 2^22 elements
    n = C.SECOND_TRIP_SHAPE[0] * C.SECOND_TRIP_SHAPE[1]
    assert IP.second_trip_elements() <= n <= 1 << 22


def test_no_compute_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    from prysm_amd import interferogram, util
    with pytest.raises(RuntimeError):
        util.rms(np.ones((4, 4)))
    with pytest.raises(RuntimeError):
        interferogram.Interferogram(np.ones((4, 4)), dx=0.1)


# ----------------------------------------------------------------------------- the numpy model against the golden
def host_compare(key, got, want, dtype, label):
    """against C.HOST: four times the float64 model's deviation from the reference as make_golden_interferogram.py prints it"""
    f64, f32 = C.HOST[key]
    bound = f32 if np.dtype(dtype) == np.float32 else f64
    dev = C.deviation(got, want, dtype)
    print(f'host   {key:10s} {C.tag(dtype)} {label:28s} measured {dev:10.3f} eps   bound {bound:8.2f} eps')
    assert dev <= bound, (key, label, dev, bound)


@pytest.mark.parametrize('key,dt', [('main_f64', np.float64), ('main_f32', np.float32), ('inf', np.float64)])
def test_model_pipeline_against_golden(G, key, dt):
    z = C.main_case(dt, inf=key == 'inf')
    rec = IP.stats(z)
    assert rec[IP.NNAN] / z.size * 100 == G[f'{key}_dropout']
    assert np.array_equal(rec[[IP.ROW0, IP.ROW1, IP.COL0, IP.COL1]], G[f'{key}_box'])
    raw = (rec[IP.MAX] - rec[IP.MIN], rec[IP.RMS], rec[IP.SA], rec[IP.STD], rec[IP.MEAN])
    assert raw[0] == G[f'{key}_raw'][0]      # pv: two selections
    host_compare('stat', raw, G[f'{key}_raw'], np.float64, 'pv rms Sa std mean')
    r0, r1, c0, c1 = IP.crop_box(rec, z.shape)
    m = z[r0:r1, c0:c1]
    assert m.shape == tuple(G[f'{key}_shape']) == C.CROPPED
    gx, gy = IP.grid_xy(m.shape, (m.shape[0] // 2, m.shape[1] // 2), C.DX, dt)
    lx, ly = IP.linspace_xy(m.shape)
    for stage in C.STAGES:
        if stage.startswith('piston'):
            m = IP.remove(m, IP.TERM_PISTON, IP.fit(m, IP.TERM_PISTON, gx, gy), gx, gy)
        elif stage == 'tilt':
            coef = IP.fit(m, IP.TERM_X | IP.TERM_Y, gx, gy)
            host_compare('coef', coef[1:3], G[f'{key}_plane'], dt, 'plane')
            m = IP.remove(m, IP.TERM_X | IP.TERM_Y, coef, gx, gy)
        else:
            coef = IP.fit(m, IP.TERM_R2 | IP.TERM_PISTON, lx, ly)
            host_compare('coef', coef[[3, 0]], G[f'{key}_sphere'], dt, 'sphere')
            m = IP.remove(m, IP.TERM_R2, coef, lx, ly)
        assert m.dtype == dt
        host_compare('removed', m, G[f'{key}_{stage}'], dt, stage)
    rec = IP.stats(m)
    fin = (rec[IP.MAX] - rec[IP.MIN], rec[IP.RMS], rec[IP.SA], rec[IP.STD])
    host_compare('stat_final', fin, G[f'{key}_final'][:4], dt, 'pv rms Sa std, cleaned')
    filled = IP.fill(m, 0)
    for name, a in zip(('gx', 'gy', 'gr'), IP.slope(filled, C.DX)):
        host_compare('slope', a, G[f'{key}_{name}'], dt, name)
    clipped = IP.clip(m, C.NSIGMA, rec[IP.STD])
    assert np.array_equal(np.isnan(clipped), np.isnan(G[f'{key}_clipped']))      # the clipped set, exactly
    assert np.isfinite(m).sum() - np.isfinite(clipped).sum() == 5


def test_model_edits_against_golden(G):
    z = C.main_case()
    assert np.array_equal(IP.mask(z, C.user_mask()), G['main_f64_masked'], equal_nan=True)
    assert np.array_equal(IP.fill(z, -7.5), G['main_f64_filled'])
    shape = IP.pad_shape(z.shape, C.PAD_SAMPLES, None)
    assert shape == G['main_f64_padded'].shape
    inf = C.main_case(inf=True)
    assert np.isinf(IP.fill(inf, 0)[C.INF_AT])      # fill uses isnan: the inf stays


def test_all_nan_and_tiny_maps_in_the_model():
    rec = IP.stats(np.full(C.ALL_NAN_SHAPE, np.nan))
    assert rec[IP.N] == 0 and rec[IP.NNAN] == 15 and np.isnan(rec[[IP.MIN, IP.MAX, IP.MEAN, IP.STD, IP.RMS, IP.SA]]).all()
    assert (rec[[IP.ROW0, IP.ROW1, IP.COL0, IP.COL1]] == -1).all() and IP.crop_box(rec, C.ALL_NAN_SHAPE) is None
    rec = IP.stats(np.array([[3.0]]))
    assert rec[IP.MEAN] == 3 and rec[IP.STD] == 0 and rec[IP.RMS] == 3 and IP.crop_box(rec, (1, 1)) is None
    # a rank-deficient fit drops the term: coordinates that are all zero
    z = C.noisy_data((5, 7), np.float64)
    coef = IP.fit(z, IP.TERM_X | IP.TERM_Y, np.zeros((1, 7)), np.zeros((5, 1)))
    assert np.array_equal(coef, np.zeros(4))
    assert np.array_equal(IP.remove(z, IP.TERM_X | IP.TERM_Y, coef, np.zeros((1, 7)), np.zeros((5, 1))), z, equal_nan=True)


def test_model_spectra_against_golden(G):
    z = C.square_case()
    host_compare('psd', IP.psd(z, C.DX, IP.window(IP.WIN_HANN, z.shape)), G['sq_psd'], np.float64, 'hann')
    host_compare('psd', IP.psd(z, C.DX, IP.window(IP.WIN_WELCH, z.shape, C.DX, 4)), G['sq_psd_welch'], np.float64, 'welch')
    nu = IP.band_nu(z.shape, C.DX)
    for name, kw in C.BANDS:
        lim = IP.band_limits(kw.get('wllow'), kw.get('wlhigh'), kw.get('flow'), kw.get('fhigh'))
        integral, spacing = IP.band(G['sq_psd'], nu, *lim)
        assert spacing == abs(nu[31, 24] - nu[32, 24]) == 1 / (64 * C.DX)
        host_compare('band', np.sqrt(integral), G[f'sq_band_{name}'], np.float64, name)
    integral, _ = IP.band(G['sq_psd'], nu, *IP.band_limits(None, None, None, 1000 / C.TIS_WVL))
    tis = 1 - np.exp(-(4 * np.pi * np.sqrt(integral) / C.TIS_WVL) ** 2)
    host_compare('band', tis, G['sq_tis'], np.float64, 'tis')
    x, y = C.grid(C.SQUARE_SHAPE)
    r = np.hypot(x, y)
    for typ, fc in C.FILTERS:
        t = IP.filter_type(typ)
        lo, hi = IP.corner_frequencies(fc, t, C.DX)
        Hl = np.abs(np.fft.fft2(IP.iir(r, C.DX, lo)))
        Hh = np.abs(np.fft.fft2(IP.iir(r, C.DX, hi))) if hi is not None else None
        H = IP.combine(t, Hl, Hh)
        host_compare('H', H, G[f'sq_H_{typ}'], np.float64, typ)
        host_compare('filtered', np.fft.ifft2(np.fft.fft2(z) * H).real, G[f'sq_filtered_{typ}'], np.float64, typ)
    for name, a in zip(('gx', 'gy', 'gr'), IP.slope(z, C.DX)):
        host_compare('slope', a, G[f'sq_{name}'], np.float64, 'square ' + name)


def test_model_pieces():
    assert np.array_equal(IP.hanning(7), np.hanning(7)) and np.array_equal(IP.hanning(64), np.hanning(64)) and np.array_equal(IP.hanning(1), np.hanning(1))
    # 1-D spectra: np.trapezoid of the masked samples
    p = np.random.default_rng(2).random(33)
    nu = np.arange(33) * 0.25
    integral, d = IP.band(p, nu, 1.0, 5.0)
    work = p.copy()
    work[(nu < 1.0) | (nu > 5.0)] = 0
    assert d == 0.25 and abs(integral - np.trapezoid(work, dx=0.25)) <= 33 * C.eps(np.float64) * np.abs(work).sum() * 0.25
    # a single row or column integrates to 0, as np.trapezoid over one sample does
    assert IP.band(np.ones((1, 5)), np.ones((1, 5)), 0, 2)[0] == 0
    nu = np.linspace(0.1, 4, 9)
    assert np.allclose(IP.psd_model(IP.PSD_ABC, nu, 3.0, 0.5, 2.5), 3.0 / (1 + (nu / 0.5) ** 2.5), rtol=4 * C.eps(np.float64), atol=0)
    assert np.allclose(IP.psd_model(IP.PSD_AB, nu, 3.0, 1.5), 3.0 * nu ** -1.5, rtol=4 * C.eps(np.float64), atol=0)
    assert IP.psd_shifts((64, 48)) == (32, 24) and IP.psd_shifts((33, 7)) == (17, 4)
    x = np.arange(7.0)
    assert np.array_equal(np.roll(x, -IP.psd_shifts((7,))[0]), np.fft.fftshift(x))      # logical i reads memory (i + shift) mod n


# ----------------------------------------------------------------------------- coordinates
def coords(state, shape, dx):
    oy, ox, step = IP.grid_current(state, shape, dx)
    x, y = IP.grid_xy(shape, (oy, ox), step, np.float64)
    return x[0], y[:, 0]


def close(got, want):
    """coordinates kept as (origin index, step): equal but for the rounding of (a step - b step) against (a - b) step"""
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.abs(g - w).max() <= 2 * C.eps(np.float64) * max(1.0, np.abs(w).max())


def test_coordinate_bookkeeping_against_the_reference(G):
    rec = IP.stats(C.main_case())
    r0, r1, c0, c1 = IP.crop_box(rec, C.MAIN_SHAPE)
    shape = (r1 - r0, c1 - c0)
    # coordinates never looked at: re-centred on the cropped shape
    state = IP.grid_crop(None, r0, c0)
    assert state is None
    got = coords(state, shape, C.DX)
    assert np.array_equal(got[0], G['coord_unseen_crop_x']) and np.array_equal(got[1], G['coord_unseen_crop_y'])
    # looked at first: carried through the crop, to the bit
    state = IP.grid_crop(IP.grid_default(C.MAIN_SHAPE, C.DX), r0, c0)
    got = coords(state, shape, C.DX)
    assert np.array_equal(got[0], G['coord_seen_crop_x']) and np.array_equal(got[1], G['coord_seen_crop_y'])
    assert np.array_equal(got[0], G['coord_tilt_crop_x']) and np.array_equal(got[1], G['coord_tilt_crop_y'])      # read by remove_tiptilt
    close(coords(IP.grid_recenter(state, shape, C.DX), shape, C.DX), (G['coord_recenter_x'], G['coord_recenter_y']))
    # pad: a new shape forgets the grid, then latcal(dx) centres it
    padded = IP.pad_shape(shape, C.PAD_SAMPLES, None)
    assert padded == (shape[0] + C.PAD_SAMPLES[0], shape[1] + C.PAD_SAMPLES[1])
    state = IP.grid_default(padded, C.DX)
    got = coords(state, padded, C.DX)
    assert np.array_equal(got[0], G['coord_pad_x']) and np.array_equal(got[1], G['coord_pad_y'])
    off = tuple(-(-p // 2) for p in C.PAD_SAMPLES)      # pad2d puts the data at ceil(d / 2)
    state = IP.grid_crop(state, *off)
    got = coords(state, shape, C.DX)
    assert np.array_equal(got[0], G['coord_pad_crop_x']) and np.array_equal(got[1], G['coord_pad_crop_y'])
    got = coords(IP.grid_default(shape, 0.25), shape, 0.25)
    assert np.array_equal(got[0], G['coord_latcal_x']) and np.array_equal(got[1], G['coord_latcal_y'])
    got = coords(IP.grid_default(shape, 1.0), shape, 1.0)
    assert np.array_equal(got[0], G['coord_strip_x']) and np.array_equal(got[1], G['coord_strip_y'])


def test_coordinate_arrays_must_match_the_data(lib):
    """the kernels read x[c], y[r] or x[r, c] for every pixel: a shorter, longer or broadcast-shaped array is refused on the host"""
    IP.check_coord_shapes((6,), (4,), (4, 6))
    IP.check_coord_shapes((4, 6), (4, 6), (4, 6))
    for xs, ys in (((5,), (4,)), ((6,), (3,)), ((7,), (4,)), ((4,), (6,)), ((1, 6), (4, 1)), ((4, 6), (4, 1)), ((5, 6), (5, 6)), ((4, 7), (4, 7)),
                   ((6,), (4, 6)), ((24,), (24,))):
        with pytest.raises(ValueError, match='data of shape'):
            IP.check_coord_shapes(xs, ys, (4, 6))
    sep = array_coords(L.PM_COORDS_SEPARABLE, ldy=0)
    refused(lib, lib.pm_ifg_fit(F64, 6, R, CO, P, CO, ctypes.byref(sep), P, P, BIG, None), ARG, 'one element apart')
    refused(lib, lib.pm_ifg_remove(F64, 6, R, CO, P, CO, ctypes.byref(sep), P, None), ARG, 'one element apart')


# ----------------------------------------------------------------------------- the reference's ValueErrors
def test_value_errors_of_the_reference():
    from prysm_amd import interferogram
    with pytest.raises(ValueError, match='Neither samples nor shape'):
        IP.pad_shape((4, 4), None, None)
    with pytest.raises(ValueError, match='only one can be given'):
        IP.pad_shape((4, 4), 2, (8, 8))
    assert IP.pad_shape((4, 5), 2, None) == (6, 7) and IP.pad_shape((4, 5), None, 9) == (9, 9) and IP.pad_shape((4, 5), None, (8, 9)) == (8, 9)
    with pytest.raises(ValueError, match='unknown window type'):
        interferogram.make_window(np.ones((8, 8)), 0.1, 'blackman')
    with pytest.raises(ValueError, match='unknown window type'):
        interferogram.psd(np.ones((8, 8)), 0.1, 'blackman')
    with pytest.raises(ValueError, match='period .* or frequency'):
        interferogram.bandlimited_rms(np.ones((8, 8)), np.ones((8, 8)))
    with pytest.raises(ValueError, match='unknown filter type'):
        IP.filter_type('notch')
    # as the reference: a short period alone is overwritten by the open long one, so wllow without wlhigh keeps every frequency
    assert IP.band_limits(0.5, None, None, None) == (0.0, float('inf')) and IP.band_limits(0.5, 4.0, None, None) == (0.25, 2.0)
    assert IP.band_limits(None, 4.0, None, None) == (0.25, float('inf'))
    assert IP.band_limits(None, None, None, 3.0) == (0.0, 3.0) and IP.band_limits(None, None, 0.3, None) == (0.3, float('inf'))
    assert interferogram.HeNe == 0.6328
