"""CPU: the numpy model of the image-chain unit (prysm_amd/imagechain_plan.py) against the reference's outputs in
tests/golden/imagechain.npz, the records and specs, argument errors, and the C ABI's refusals and workspace queries (no device)."""
import ctypes

import numpy as np
import pytest

import imagechain_common as C
from prysm_amd import _lib as L
from prysm_amd import imagechain_plan as IP

F32, F64 = L.PM_F32, L.PM_F64
P = ctypes.c_void_p(64)
DTS = [np.float64, np.float32]


@pytest.fixture(scope='module')
def lib():
    return L.load()


def specs():
    return {'smear': IP.smear_spec(*C.SMEAR), 'smear_x': IP.smear_spec(C.SMEAR[0], 0), 'jitter': IP.jitter_spec(C.JITTER),
            'pinhole_ft': IP.pinhole_spec(C.PINHOLE_R), 'slit_ft': IP.slit_spec(*C.SLITW), 'slit_ft_x': IP.slit_spec(C.SLITW[0], None),
            'slit_ft_y': IP.slit_spec(None, C.SLITW[1]), 'airydisk_ft': IP.airydisk_ft_spec(C.AIRY_FNO, C.AIRY_WVL),
            'pixel': IP.pixel_spec(*C.PIXEL), 'olpf': IP.olpf_spec(*C.OLPF)}


target_model, compare_target = C.target_model, C.compare_target


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('name', list(C.TARGETS))
def test_targets_against_the_reference(name, tag, dt):
    g = C.golden()
    for form in ('arrays', 'cart'):
        got, margin = target_model(name, tag, dt, form)
        assert got.dtype == (bool if name in ('pinhole', 'slit') else dt)
        compare_target(got, g[f'{tag}_{name}' + ('_f32' if dt == np.float32 else '')], margin, dt)


@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('name', list(C.EXTRA_TARGETS))
def test_more_target_behaviour_against_the_reference(name, tag):
    got, margin = target_model(name, tag, np.float64)
    ref = C.golden()[f'{tag}_{name}']
    if name == 'siemens_sin_white':       # a cosine, not a decision: compared by value off the radius thresholds
        params, a, b, polar = margin
        near = IP.decision_margin(params[0], 0, params[2], a, b, np.float64, polar=polar)
        assert near.mean() <= C.EXCLUDE_CAP and np.abs(got - ref)[~near].max() <= 16 * C.eps(np.float64) * (1 + 18 * np.pi)
    else:
        compare_target(got, ref, margin, np.float64)


def test_siemensstar_background_goes_through_the_binarisation():
    x, y = C.grid_xy('a')
    r, t = C.polar_of(x, y)
    black = IP.object_render(*IP.object_params(IP.SIEMENSSTAR, spokes=36, oradius=0.8, iradius=0.1, background='black', contrast=0.9,
                                               sinusoidal=False), r, t, np.float64, polar=True)
    white = IP.object_render(*IP.object_params(IP.SIEMENSSTAR, spokes=36, oradius=0.8, iradius=0.1, background='White', contrast=0.9,
                                               sinusoidal=False), r, t, np.float64, polar=True)
    outside = r > 0.8
    assert np.all(black[outside] == (1 - 0.9) / 2) and np.all(white[outside] == 1 - (1 - 0.9) / 2)
    # a cosine of exactly 0 gives 0.5, which neither comparison moves
    half = IP.object_render(*IP.object_params(IP.SIEMENSSTAR, spokes=2, oradius=9, iradius=0, background='black', contrast=0.0,
                                              sinusoidal=False), np.ones((1, 3)), np.array([[0.1, 1.0, 2.0]]), np.float64, polar=True)
    assert np.all(half == 0.5)


@pytest.mark.parametrize('dt', DTS)
def test_crossed_edge_against_the_reference(dt):
    x, y = C.grid_xy('c', dt)
    params = IP.object_params(IP.SLANTEDEDGE, angle=4, contrast=0.9, crossed=True)
    got = IP.object_render(*params, x, y, dt)
    compare_target(got, C.golden()['c_crossed' + ('_f32' if dt == np.float32 else '')], (params, x, y, False), dt)
    # the four positions of the kernel: upperright[i, j] = m[i, j] & m[j, N-1-i], lowerleft[i, j] = upperright[N-1-i, N-1-j]
    m = x * params[2][0] - y * params[2][1] > 0
    N = m.shape[0]
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    four = (m[i, j] & m[j, N - 1 - i]) | (m[N - 1 - i, N - 1 - j] & m[N - 1 - j, i])
    assert np.array_equal(four, got == got.min())
    with pytest.raises(ValueError, match='square'):
        IP.object_render(*params, *C.grid_xy('a'), np.float64)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_transfer_functions_against_the_reference(tag, dt):
    g = C.golden()
    idx = g[f'{tag}_idx']
    fx, fy = C.freq_vectors(tag, dt)
    sp = specs()
    for name in list(C.TFS) + ['product']:
        factors = [sp[n] for n in C.PRODUCT] if name == 'product' else [sp[name]]
        got = IP.tf_product(C.SHAPES[tag], factors, dt, fx=fx, fy=fy, out_complex=False)
        assert got.dtype == dt
        dev = np.abs(got.reshape(-1)[idx].astype(np.float64) - g[f'{tag}_tf_{name}']).max()
        assert dev <= C.tf_bound(name, tag, dt), (name, dev, C.tf_bound(name, tag, dt))
    rad = C.airy_radius(tag).astype(dt)
    for name, ef in (('airydisk', False), ('airydisk_efield', True)):
        got = IP.tf_product(C.SHAPES[tag], [IP.airydisk_spec(C.AIRY_FNO, C.AIRY_WVL, efield=ef)], dt, fr=rad, out_complex=False)
        dev = np.abs(got.reshape(-1)[idx].astype(np.float64) - g[f'{tag}_{name}']).max()
        assert dev <= C.airy_bound(tag, dt, ef), (name, dev)


def test_jinc_branches_and_the_value_at_zero():
    for dt in DTS:
        x = np.array([0.0, 1e-9, 7.999, 8.0, 8.001, -3.0, 3.0], dt)
        j = IP.jinc(x)
        assert j.dtype == dt and j[0] == dt(0.5) and j[5] == j[6]
        assert abs(float(j[3]) - float(j[4])) < 1e-4 and abs(float(j[6]) - 0.11301963) < 1e-6      # J1(3) / 3


@pytest.mark.parametrize('n', [64, 65])
@pytest.mark.parametrize('shift', [False, True])
def test_generated_frequencies_are_forward_ft_unit(n, shift):
    """fttools.forward_ft_unit(dx, n, shift) is numpy's fftfreq(n, dx) in config.precision, rolled by n // 2 when shift"""
    for dx in (0.5, 0.37, 3.0):
        for dt in DTS:
            unit = np.fft.fftfreq(n, dx).astype(dt)
            ref = np.roll(unit, n // 2) if shift else unit
            assert np.array_equal(IP.gen_axis(dx, n, shift, dt), ref)
    if shift:
        assert np.array_equal(IP.gen_axis(0.5, n, True, np.float64), np.fft.fftshift(np.fft.fftfreq(n, 0.5)))


def test_product_rotation_and_maps():
    """shift: frequencies and maps are centred, the result never is; the rotation is np.fft.ifftshift"""
    rng = np.random.default_rng(3)
    for m, n in ((6, 7), (8, 8), (5, 4)):
        a = rng.standard_normal((m, n))
        c = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
        sp = [IP.pixel_spec(0.9, 1.1), IP.jitter_spec(0.4)]
        centred = IP.tf_product((m, n), sp + [a, c], np.float64, dx=0.5, shift=True)
        plain = IP.tf_product((m, n), sp + [np.fft.ifftshift(a), np.fft.ifftshift(c)], np.float64, dx=0.5, shift=False)
        assert np.array_equal(centred, plain)
        H = IP.tf_product((m, n), sp, np.float64, dx=0.5, shift=False, out_complex=False)
        fx, fy = np.fft.fftfreq(n, 0.5)[None, :], np.fft.fftfreq(m, 0.5)[:, None]
        ref = np.sinc(fx * 0.9) * np.sinc(fy * 1.1) * np.exp(-2 * (np.pi * 0.4 * np.hypot(fx, fy)) ** 2)
        assert np.abs(H - ref).max() < 1e-15
    assert IP.tf_product((3, 4), [], np.float32, dx=1.0).dtype == np.complex64


def test_specs_round_trip_and_pack():
    assert ctypes.sizeof(L.pm_tf_record) == IP.RECORD_DTYPE.itemsize == 56
    for f in ('kind', 'flags', 'ld', 'ptr', 'p'):
        assert getattr(L.pm_tf_record, f).offset == IP.RECORD_DTYPE.fields[f][1]
    assert ctypes.sizeof(L.pm_object) == 72 and ctypes.sizeof(L.pm_tf_freq) == 64
    sp = specs()
    assert sp['smear'].records == (IP.Record(IP.SINC_X, 0, (1.3, 0, 0, 0)), IP.Record(IP.SINC_Y, 0, (0.7, 0, 0, 0)))
    assert sp['smear_x'].records == (IP.Record(IP.SINC_X, 0, (1.3, 0, 0, 0)),) and sp['smear'].needs == 'xy'
    assert sp['jitter'].records[0].p[0] == np.pi * 0.9 and sp['jitter'].needs == 'r'
    assert sp['pinhole_ft'].records[0] == IP.Record(IP.JINC_R, 0, (1.1 * 2 * np.pi, 0, 0, 0))
    assert sp['olpf'].records[1] == IP.Record(IP.COS_Y, 0, (0.9, 0, 0, 0))
    assert sp['slit_ft'].records[0].flags == 3 and sp['slit_ft_x'].records[0].flags == 1 and sp['slit_ft_y'].records[0].flags == 2
    assert sp['airydisk_ft'].records[0].p[0] == 1 / (0.55 * 4.0)
    table = IP.pack_records(list(sp['smear'].records) + [(IP.MAP_COMPLEX, 48, 4096)] + list(sp['slit_ft'].records))
    rec = ctypes.cast(table.ctypes.data, ctypes.POINTER(L.pm_tf_record))
    assert [rec[i].kind for i in range(4)] == [IP.SINC_X, IP.SINC_Y, IP.MAP_COMPLEX, IP.SLIT_FT]
    assert rec[2].ld == 48 and rec[2].ptr == 4096 and rec[3].flags == 3 and list(rec[3].p) == [0.8, 0.6, 0, 0] and rec[0].p[0] == 1.3
    assert IP.flatten([sp['smear'], np.ones((2, 2)), sp['jitter']])[2].shape == (2, 2)
    with pytest.raises(ValueError, match='at most 16'):
        IP.flatten([sp['smear']] * 9)
    with pytest.raises(ValueError):
        IP.pack_records([(IP.SINC_X, 1, 2)])


def test_public_specs_are_the_plan_records():
    from prysm_amd import degradations, detector, objects, psf
    assert detector.pixel_ft.spec(0.9, 1.1) == IP.pixel_spec(0.9, 1.1) and detector.olpf_ft.spec(1, 2) == IP.olpf_spec(1, 2)
    assert degradations.smear_ft.spec(1.3, 0.7) == IP.smear_spec(1.3, 0.7) and degradations.jitter_ft.spec(0.9) == IP.jitter_spec(0.9)
    assert objects.pinhole_ft.spec(1.1) == IP.pinhole_spec(1.1) and objects.slit_ft.spec(0.8, None) == IP.slit_spec(0.8, 0)
    assert psf.airydisk_ft.spec(4, 0.55) == IP.airydisk_ft_spec(4, 0.55)
    assert (psf.FIRST_AIRY_ZERO, psf.SECOND_AIRY_ZERO, psf.THIRD_AIRY_ZERO) == (1.220, 2.233, 3.238)
    assert psf.AIRYDATA[2] == (2.233, 0.9099305350850819) and psf.FIRST_AIRY_ENCIRCLED == 0.8377850436212378


def test_argument_errors_raise_before_any_launch():
    """no device here: anything that reached a launch would raise RuntimeError instead"""
    from prysm_amd import convolution, degradations, objects, psf
    x, y = C.grid_xy('a')
    r, t = C.polar_of(x, y)
    with pytest.raises(ValueError, match='invalid background'):
        objects.siemensstar(r, t, 36, background='green')
    with pytest.raises(ValueError, match='square'):
        objects.slantededge(x, y, crossed=True)
    with pytest.raises(ValueError, match='square'):
        objects.slantededge(shape=(4, 5), dx=1.0, crossed=True)
    with pytest.raises(ValueError, match='nonzero'):
        objects.slit_ft(None, 0, x, y)
    with pytest.raises(ValueError, match='nonzero'):
        degradations.smear_ft(x, y, 0, 0)
    with pytest.raises(ValueError, match='either shape'):
        objects.tiltedsquare(x, y, shape=(4, 4), dx=1.0)
    with pytest.raises(ValueError, match='either shape'):
        objects.tiltedsquare()
    with pytest.raises(ValueError, match='unknown metric'):
        psf.estimate_size(np.ones((4, 4)), 'fwtm', dx=1.0)
    with pytest.raises(ValueError, match='unknown metric'):
        psf.estimate_size(np.ones((4, 4)), None, dx=1.0)
    with pytest.raises(ValueError, match='unknown criteria'):
        psf.fwhm(np.ones((4, 4)), dx=1.0, criteria='middle')
    with pytest.raises(TypeError):
        objects.tiltedsquare(x + 0j, y)
    with pytest.raises(TypeError, match='plain callable'):
        convolution.transfer_function((4, 4), 1.0, [lambda fx: fx])
    with pytest.raises(RuntimeError):          # a valid call does reach the device
        objects.tiltedsquare(x, y)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_polar_resample_against_the_reference(tag, dt):
    g = C.golden()
    x, y = C.grid_vectors(tag, dt)
    data = C.smooth_data(tag, dt)
    rho, phi, pol = IP.polar_resample(x, y, data, dt)
    assert pol.dtype == dt and pol.shape == data.shape and rho.shape == x.shape and phi.shape == y.shape
    x64, y64 = C.grid_vectors(tag)
    dev = np.abs(pol.reshape(-1)[g[f'{tag}_idx']].astype(np.float64) - g[f'{tag}_polar'])
    near = C.polar_excluded(x64, y64, dt).reshape(-1)[g[f'{tag}_idx']]
    if dt == np.float64:
        near[:] = False              # the model meets the bound with none excluded on the fixture's smooth data
    assert near.mean() <= C.POLAR_EXCLUDE_CAP
    assert dev[~near].max() <= C.polar_bound(x64, y64, C.smooth_data(tag), dt)


def test_polar_resample_boundary_and_fill():
    x, y = np.linspace(-1, 1, 5), np.linspace(-1, 1, 5)
    rho, phi, pol = IP.polar_resample(x, y, np.ones((5, 5)), np.float64)
    assert rho[-1] == 1 and phi[-1] == 2 * np.pi
    assert pol[0, -1] == 1.0                # (1, 0): on the boundary, inside
    assert pol[1, -1] == 1.0 and np.all(pol[:, 0] == 1.0)
    big = IP.polar_resample(np.linspace(-2, 2, 5), y, np.ones((5, 5)), np.float64)[2]
    assert big[0, -1] == 1.0 and big[0, 2] == 1.0      # (2, 0): on x's boundary, inside
    assert big[1, -1] == 0.0                # (0, 2): y outside -> fill value


def test_centroid_crossings_and_sizes_against_the_reference():
    g = C.golden()
    d = C.gaussian_psf()
    com = IP.centroid(d)
    assert np.abs(np.array(com) - g['psf_centroid_px']).max() < 1e-12
    assert abs(com[0] - 30.4) < 1e-3 and abs(com[1] - 35.2) < 1e-3
    dx = C.psf_dx()
    assert np.abs(np.array([dx * (c - n // 2) for c, n in zip(com, d.shape)]) - g['psf_centroid_spatial']).max() < 1e-13
    x, y = C.psf_grid()
    rho, phi, pol = IP.polar_resample(x, y, d, np.float64)
    assert np.abs(pol - g['psf_polar']).max() <= C.polar_bound(x, y, d, np.float64)
    metrics = ['fwhm', '1/e', '1/e^2', 0.3]
    got = np.array([IP.estimate_size(pol, rho, m)[0] * (1 if m == 0.3 else 2) for m in metrics])
    assert np.abs(got - g['psf_sizes']).max() < 1e-13
    x32, y32 = C.psf_grid(np.float32)
    r32, _, p32 = IP.polar_resample(x32, y32, d.astype(np.float32), np.float32)
    got32 = np.array([IP.estimate_size(p32, r32, m)[0] * (1 if m == 0.3 else 2) for m in metrics])
    assert np.array_equal(np.abs(got32 - g['psf_sizes']), g['size_dev32']) and g['size_dev32'].max() < 1e-6
    pa = IP.polar_resample(x, y, C.airy_psf(), np.float64)[2]
    first, last = IP.estimate_size(pa, rho, C.AIRY_LEVEL, 'first'), IP.estimate_size(pa, rho, C.AIRY_LEVEL, 'LAST')
    assert abs(first[0] - g['psf_airy_first']) < 1e-13 and abs(last[0] - g['psf_airy_last']) < 1e-13 and last[0] > first[0] + 0.05
    assert first[1] == last[1] == d.shape[0]
    assert IP.estimate_size(pol, rho, 2.0) == (0.0, 0.0)                 # never crossed: count 0
    flat = np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    rc, has = IP.crossings(flat, np.arange(4.0), 0.5, 1)
    assert list(has) == [1.0, 0.0] and rc[0] == 1.5
    rc, _ = IP.crossings(np.array([[1.0, 0.5, 0.5, 0.0]]), np.arange(4.0), 0.5, 0)       # 0.5 > 0.5 is false: the change is at index 0
    assert rc[0] == 1.0


def test_autocrop_window_arithmetic():
    """the window the one launch writes: row i of the output is row cy - px // 2 + i of data, zero outside"""
    g = C.golden()
    d = C.gaussian_psf()
    cy, cx = (int(c) for c in IP.centroid(d))
    for px, key in ((100, 'psf_autocrop100'), (20, 'psf_autocrop20')):
        w = px // 2
        out = np.zeros((px, px))
        for i in range(px):
            for j in range(px):
                r, c = cy - w + i, cx - w + j
                if 0 <= r < d.shape[0] and 0 <= c < d.shape[1]:
                    out[i, j] = d[r, c]
        assert np.array_equal(out, g[key])
    assert np.all(g['psf_autocrop100'][[0, -1], :] == 0) and np.all(g['psf_autocrop100'][:, [0, -1]] == 0)


def test_symbols_and_signatures(lib):
    for name in ('pm_object_render', 'pm_tf_product', 'pm_polar_resample', 'pm_centroid_workspace', 'pm_centroid', 'pm_psf_size_workspace',
                 'pm_psf_size_groups', 'pm_psf_size'):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.pm_version() == 107


def test_workspace_queries(lib):
    assert lib.pm_centroid_workspace(1, 256) == 24 and lib.pm_centroid_workspace(16, 16 + 1) == 2 * 24
    assert lib.pm_centroid_workspace(4096, 4096) == 1024 * 24 and lib.pm_centroid_workspace(0, 5) == 0
    assert lib.pm_psf_size_workspace(10) == 8 * (1 + 1024 + 20) and lib.pm_psf_size_workspace(0) == 0
    assert lib.pm_psf_size_groups(4) == 1 and lib.pm_psf_size_groups(5) == 2 and lib.pm_psf_size_groups(10 ** 6) == 1024


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    ARG, WS = L.PM_ERR_ARG, L.PM_ERR_WORKSPACE
    obj = L.pm_object()
    obj.kind = IP.SLANTEDEDGE

    def render(dt=F32, coords=L.PM_COORDS_POINTWISE, polar=0, ny=4, nx=4, a=P, lda=4, b=P, ldb=4, o=obj, out=P, ld=4):
        return lib.pm_object_render(dt, coords, polar, ny, nx, a, lda, b, ldb, 1.0, ctypes.byref(o), out, ld, None)

    assert render(dt=L.PM_C64) == ARG and b'dtype' in lib.pm_last_error()
    assert render(coords=7) == ARG and render(ny=-1) == ARG and render(out=None) == ARG and render(a=None) == ARG
    assert render(lda=3) == ARG and render(ld=3) == ARG and b'leading dimension' in lib.pm_last_error()
    assert render(polar=1) == ARG and b'pinhole' in lib.pm_last_error()
    obj.flags = IP.CROSSED
    assert render(ny=4, nx=5, lda=5, ldb=5, ld=5) == ARG and b'square' in lib.pm_last_error()
    bad = L.pm_object()
    bad.kind = 9
    assert render(o=bad) == ARG and b'kind' in lib.pm_last_error()
    obj.flags = 0
    assert render(ny=0) == 0

    fq = L.pm_tf_freq()
    fq.mode, fq.dx = L.PM_FREQ_GRID, 0.5
    recs = (L.pm_tf_record * 17)()

    def product(dt=F32, m=4, n=4, f=fq, nrec=1, cplx=1, out=P, ld=4):
        return lib.pm_tf_product(dt, m, n, ctypes.byref(f), recs, nrec, cplx, out, ld, None)

    assert product(dt=99) == ARG and product(nrec=17) == ARG and b'at most 16' in lib.pm_last_error()
    assert product(out=None) == ARG and product(ld=3) == ARG and product(m=-1) == ARG
    recs[0].kind = 44
    assert product() == ARG and b'unknown kind' in lib.pm_last_error()
    recs[0].kind = IP.MAP_COMPLEX
    assert product() == ARG and b'null' in lib.pm_last_error()
    recs[0].ptr, recs[0].ld = 64, 4
    assert product(cplx=0) == ARG and b'complex' in lib.pm_last_error()
    recs[0].ld = 3
    assert product() == ARG
    recs[0].kind, recs[0].flags = IP.SLIT_FT, 0
    assert product() == ARG and b'slit' in lib.pm_last_error()
    recs[0].flags = 3
    assert product(m=1, ld=4) == ARG and b'two frequencies' in lib.pm_last_error()
    recs[0].kind = IP.SINC_X
    vec = L.pm_tf_freq()
    vec.mode = L.PM_FREQ_VECTORS
    assert product(f=vec) == ARG and b'missing' in lib.pm_last_error()
    zero = L.pm_tf_freq()
    assert product(f=zero) == ARG and b'spacing' in lib.pm_last_error()
    zero.mode = 5
    assert product(f=zero) == ARG
    assert product(m=0) == 0

    def resample(dt=F32, ny=4, nx=4, x=P, xs=1.0, ys=1.0, dld=4, ld=4):
        return lib.pm_polar_resample(dt, ny, nx, x, P, xs, ys, P, P, P, dld, P, ld, None)

    assert resample(dt=L.PM_C128) == ARG and resample(x=None) == ARG and resample(ny=1) == ARG and resample(xs=0.0) == ARG
    assert resample(ys=float('nan')) == ARG and resample(dld=3) == ARG and resample(ld=2) == ARG and resample(ny=0) == 0

    def cen(dt=F64, m=4, n=4, d=P, ld=4, out=P, ws=P, wsb=1 << 20):
        return lib.pm_centroid(dt, m, n, d, ld, out, ws, wsb, None)

    assert cen(dt=1) == ARG and cen(m=0) == ARG and cen(d=None) == ARG and cen(ld=3) == ARG and cen(ws=None) == ARG
    assert cen(wsb=8) == WS and cen(out=ctypes.c_void_p(12)) == ARG

    def size(dt=F64, rows=4, cols=4, p=P, ld=4, r=P, out=P, ws=P, wsb=1 << 20):
        return lib.pm_psf_size(dt, rows, cols, p, ld, r, 1, 0.5, 1, out, ws, wsb, None)

    assert size(dt=0) == ARG and size(rows=0) == ARG and size(r=None) == ARG and size(ld=1) == ARG and size(wsb=64) == WS
    assert size(ws=ctypes.c_void_p(4)) == ARG


def test_neither_the_plan_nor_the_modules_import_scipy_or_the_reference():
    import subprocess
    import sys
    from conftest import ROOT
    code = ('import sys\n'
            'import prysm_amd.objects, prysm_amd.degradations, prysm_amd.psf, prysm_amd.imagechain_plan\n'
            'bad = [m for m in sys.modules if m.split(".")[0] in ("scipy", "oracle", "mpmath", "prysm")]\n'
            'assert not bad, bad\n')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=ROOT)
