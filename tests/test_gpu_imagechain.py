"""GPU: the image-chain unit (csrc/imagechain.hip) behind prysm_amd.objects, degradations, psf, coordinates.uniform_cart_to_polar and
the fused transfer-function product of prysm_amd.convolution, against the reference's outputs in tests/golden/imagechain.npz and against
the numpy model.  Bounds and cases: tests/imagechain_common.py."""
import functools

import numpy as np
import pytest
import torch

import imagechain_common as C
from conftest import rel_max
from gpu_common import TOL32, TOL64, tonp

pytestmark = pytest.mark.gpu

DTS = [np.float64, np.float32]
TDT = {np.float64: torch.float64, np.float32: torch.float32}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(a, pad=5):
    """the same values as a view of a wider device buffer: rows lie a.shape[1] + pad elements apart"""
    buf = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=TDT[a.dtype.type], device='cuda')
    view = buf[:, :a.shape[1]]
    view.copy_(dev(a))
    assert view.stride(0) == a.shape[1] + pad
    return view


@pytest.fixture(scope='module')
def mods():
    from prysm_amd import degradations, detector, objects, psf
    return {'objects': objects, 'degradations': degradations, 'psf': psf, 'detector': detector}


def IP():
    from prysm_amd import imagechain_plan
    return imagechain_plan


def specs(mods):
    o, d, p, det = mods['objects'], mods['degradations'], mods['psf'], mods['detector']
    return {'smear': d.smear_ft.spec(*C.SMEAR), 'jitter': d.jitter_ft.spec(C.JITTER), 'pinhole_ft': o.pinhole_ft.spec(C.PINHOLE_R),
            'pixel': det.pixel_ft.spec(*C.PIXEL), 'airydisk_ft': p.airydisk_ft.spec(C.AIRY_FNO, C.AIRY_WVL), 'olpf': det.olpf_ft.spec(*C.OLPF),
            'slit_ft': o.slit_ft.spec(*C.SLITW)}


# ----------------------------------------------------------------------------- 1. parity: targets

def gpu_target(objects, name, tag, dt, form):
    """a target of TARGETS on one of its coordinate forms"""
    from prysm_amd import coordinates
    fn, kind, args, kw = {**C.TARGETS, **C.EXTRA_TARGETS}[name]
    f = getattr(objects, fn)
    x, y = C.grid_xy(tag, dt)
    if form in ('arrays', 'strided'):
        put = strided if form == 'strided' else dev
        if kind == 'polar':
            r, t = C.polar_of(x, y)
            return f(put(r), put(t), *args, **kw)
        if kind == 'rho':
            return f(args[0], put(np.hypot(x, y)))
        return f(put(x), put(y), *args, **kw)
    if form == 'vectors':
        xv, yv = (dev(v) for v in C.grid_vectors(tag, dt))
        coords = dict(x=xv, y=yv)
    elif form == 'device_arrays':      # meshgrids made on the device, and their polar form from cart_to_polar
        x2, y2 = coordinates.make_xy_grid(C.SHAPES[tag], dx=C.grid_dx(tag))
        if kind == 'polar':
            r, t = coordinates.cart_to_polar(x2, y2)
            return f(r, t, *args, **kw)
        if kind == 'rho':
            return f(args[0], coordinates.cart_to_polar(x2, y2)[0])
        return f(x2, y2, *args, **kw)
    else:
        coords = dict(shape=C.SHAPES[tag], dx=C.grid_dx(tag))
    if kind == 'rho':
        return f(args[0], **coords)
    if kind == 'polar':
        return f(None, None, *args, **kw, **coords)
    if form == 'vectors':
        return f(coords['x'], coords['y'], *args, **kw)
    return f(None, None, *args, **kw, **coords)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('name', list(C.TARGETS))
def test_targets_against_the_reference(mods, name, tag, dt):
    g = C.golden()
    ref = g[f'{tag}_{name}' + ('_f32' if dt == np.float32 else '')]
    for form in ('arrays', 'strided', 'vectors'):
        got = gpu_target(mods['objects'], name, tag, dt, form)
        assert got.dtype == (torch.bool if name in ('pinhole', 'slit') else TDT[dt]) and tuple(got.shape) == C.SHAPES[tag]
        C.compare_target(tonp(got), ref, C.target_margin(name, tag, dt, form), dt)


@pytest.mark.parametrize('tag', ['a', 'b'])
@pytest.mark.parametrize('name', list(C.TARGETS) + list(C.EXTRA_TARGETS))
def test_the_three_coordinate_forms_agree_bit_for_bit(mods, name, tag):
    """float64 (config.precision): arrays made on the device, 1-D vectors, and shape= / dx= give the same bits"""
    forms = [gpu_target(mods['objects'], name, tag, np.float64, form) for form in ('device_arrays', 'vectors', 'grid')]
    assert torch.equal(forms[0], forms[1]) and torch.equal(forms[1], forms[2])
    if name == 'siemens_sin_white':       # a cosine, not a decision: compared by value off the radius thresholds
        params, a, b, polar = C.target_margin(name, tag, np.float64, 'grid')
        near = IP().decision_margin(params[0], 0, params[2], a, b, np.float64, polar=polar)
        dev_ = np.abs(tonp(forms[2]) - C.golden()[f'{tag}_{name}'])
        assert near.mean() <= C.EXCLUDE_CAP and dev_[~near].max() <= 16 * C.eps(np.float64) * (1 + 18 * np.pi)
    elif name in C.EXTRA_TARGETS:
        C.compare_target(tonp(forms[2]), C.golden()[f'{tag}_{name}'], C.target_margin(name, tag, np.float64, 'grid'), np.float64)


@pytest.mark.parametrize('dt', DTS)
def test_crossed_edge(mods, dt):
    objects = mods['objects']
    x, y = C.grid_xy('c', dt)
    params = IP().object_params(IP().SLANTEDEDGE, angle=4, contrast=0.9, crossed=True)
    ref = C.golden()['c_crossed' + ('_f32' if dt == np.float32 else '')]
    outs = [objects.slantededge(dev(x), dev(y), crossed=True), objects.slantededge(strided(x), strided(y), crossed=True),
            objects.slantededge(*(dev(v) for v in C.grid_vectors('c', dt)), crossed=True)]
    for got in outs:
        C.compare_target(tonp(got), ref, (params, x, y, False), dt)
    if dt == np.float64:
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[0], objects.slantededge(shape=64, dx=C.grid_dx('c'), crossed=True))
    with pytest.raises(ValueError, match='square'):
        objects.slantededge(*(dev(v) for v in C.grid_xy('a')), crossed=True)


# ----------------------------------------------------------------------------- 1. parity: transfer functions

def centred(H):
    return np.fft.fftshift(tonp(H))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_transfer_functions_against_the_reference(mods, tag, dt):
    from prysm_amd import convolution, coordinates
    g = C.golden()
    idx = g[f'{tag}_idx']
    fxv, fyv = C.freq_vectors(tag, dt)
    fx, fy = np.meshgrid(fxv, fyv)
    fr = tonp(coordinates.cart_to_polar(dev(fx), dev(fy))[0])     # the device's hypot, which the generated form uses too
    assert np.abs(fr - np.hypot(fx, fy)).max() <= 2 * C.eps(dt)
    sp = specs(mods)
    for name in C.TFS:
        ref, bound = g[f'{tag}_tf_{name}'], C.tf_bound(name, tag, dt)
        outs = [C.call_tf(mods, name, dev(fx), dev(fy), dev(fr)), C.call_tf(mods, name, strided(fx), strided(fy), strided(fr))]
        if C.TFS[name][0] == 'detector':       # the torch calls broadcast: a row and a column
            outs.append(C.call_tf(mods, name, dev(fxv.reshape(1, -1)), dev(fyv.reshape(-1, 1)), None))
        elif 'r' not in C.TFS[name][2]:        # 1-D vectors give (ny, nx)
            outs.append(C.call_tf(mods, name, dev(fxv), dev(fyv), None))
        for got in outs:
            assert got.dtype == TDT[dt] and tuple(got.shape) == C.SHAPES[tag]
            dev_ = np.abs(tonp(got).reshape(-1)[idx].astype(np.float64) - ref).max()
            print(f'{name} {tag} {dt.__name__}: {dev_:.3e} (bound {bound:.3e})')
            assert dev_ <= bound, (name, dev_, bound)
        if dt == np.float64:
            assert all(torch.equal(outs[0], o) for o in outs[1:])
            if name in sp:        # the third form: frequencies generated in the kernel
                gen = centred(convolution.transfer_function(C.SHAPES[tag], C.DX, [sp[name]], shift=True, dtype=torch.float64))
                if C.TFS[name][0] == 'detector':      # pixel_ft and olpf_ft themselves are torch calls: equal to the bound, not to the bit
                    assert np.abs(gen.reshape(-1)[idx] - ref).max() <= bound
                else:
                    assert np.array_equal(gen, tonp(outs[0]))
    rad = C.airy_radius(tag).astype(dt)
    for name, fn, ef in (('airydisk', mods['psf'].airydisk, False), ('airydisk_efield', mods['psf'].airydisk_efield, True)):
        a, b = fn(dev(rad), C.AIRY_FNO, C.AIRY_WVL), fn(strided(rad), C.AIRY_FNO, C.AIRY_WVL)
        dev_ = np.abs(tonp(a).reshape(-1)[idx].astype(np.float64) - g[f'{tag}_{name}']).max()
        print(f'{name} {tag} {dt.__name__}: {dev_:.3e} (bound {C.airy_bound(tag, dt, ef):.3e})')
        assert torch.equal(a, b) and a.dtype == TDT[dt] and dev_ <= C.airy_bound(tag, dt, ef)


def test_airydisk_ft_leaves_its_argument_alone(mods):
    fr = dev(np.linspace(0, 3, 50).reshape(5, 10))
    keep = fr.clone()
    out = mods['psf'].airydisk_ft(fr, C.AIRY_FNO, C.AIRY_WVL)
    assert torch.equal(fr, keep) and float(out[-1, -1]) == 0.0 and float(out[0, 0]) == 1.0


# ----------------------------------------------------------------------------- 3. the fused product

@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('tag', ['a', 'b'])
def test_fused_product_equals_the_product_of_the_eager_maps(mods, tag, dt):
    from prysm_amd import convolution
    g = C.golden()
    fxv, fyv = C.freq_vectors(tag, dt)
    fx, fy = np.meshgrid(fxv, fyv)
    fr = np.hypot(fx, fy)
    sp = specs(mods)
    cdt = torch.complex128 if dt == np.float64 else torch.complex64
    H = convolution.transfer_function(C.SHAPES[tag], C.DX, [sp[n] for n in C.PRODUCT], shift=True, dtype=cdt)
    assert H.dtype == cdt and not tonp(H).imag.any()
    eager = functools.reduce(lambda a, b: a * b, [tonp(C.call_tf(mods, n, dev(fx), dev(fy), dev(fr))).astype(np.float64) for n in C.PRODUCT])
    bound = C.tf_bound('product', tag, dt)
    got = centred(H).real.astype(np.float64)
    print(f'product {tag} {dt.__name__}: against eager {np.abs(got - eager).max():.3e}, against the reference '
          f"{np.abs(got.reshape(-1)[g[f'{tag}_idx']] - g[f'{tag}_tf_product']).max():.3e} (bound {bound:.3e})")
    assert np.abs(got - eager).max() <= bound
    assert np.abs(got.reshape(-1)[g[f'{tag}_idx']] - g[f'{tag}_tf_product']).max() <= bound
    # real on request, frequencies from vectors, and user maps (real and complex) multiplied in
    rdt = TDT[dt]
    Hr = convolution.transfer_function(C.SHAPES[tag], C.DX, [sp[n] for n in C.PRODUCT], shift=True, dtype=rdt)
    assert Hr.dtype == rdt and torch.equal(Hr, H.real)
    Hv = convolution.transfer_function(C.SHAPES[tag], C.DX, [sp[n] for n in C.PRODUCT], shift=True, dtype=cdt, fx=dev(fxv), fy=dev(fyv))
    assert torch.equal(Hv, H) if dt == np.float64 else rel_max(tonp(Hv), tonp(H)) <= bound
    rng = np.random.default_rng(5)
    a = rng.standard_normal(C.SHAPES[tag]).astype(dt)
    c = (rng.standard_normal(C.SHAPES[tag]) + 1j * rng.standard_normal(C.SHAPES[tag])).astype(np.complex128 if dt == np.float64 else np.complex64)
    for shift in (False, True):
        Hm = convolution.transfer_function(C.SHAPES[tag], C.DX, [sp['pixel'], dev(a), sp['jitter'], strided(a), dev(c)], shift=shift, dtype=cdt)
        model = IP().tf_product(C.SHAPES[tag], [sp['pixel'], a, sp['jitter'], a, c], dt, dx=C.DX, shift=shift)
        assert np.abs(tonp(Hm) - model).max() <= (C.tf_bound('pixel', tag, dt) + C.tf_bound('jitter', tag, dt)) * np.abs(a * a * c).max()


def callables(mods):
    o, d, p, det = mods['objects'], mods['degradations'], mods['psf'], mods['detector']
    return [lambda fx, fy: d.smear_ft(fx, fy, *C.SMEAR), lambda fr: d.jitter_ft(fr, C.JITTER), lambda fr: o.pinhole_ft(C.PINHOLE_R, fr),
            lambda fx, fy: det.pixel_ft(fx, fy, *C.PIXEL), lambda fr: p.airydisk_ft(fr, C.AIRY_FNO, C.AIRY_WVL)]


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('shape', [(64, 65), (128, 128)])
def test_apply_transfer_functions_with_specs_equals_callables(mods, shape, precision):
    from prysm_amd import convolution
    from prysm_amd.conf import config
    rng = np.random.default_rng(11)
    sp = [specs(mods)[n] for n in C.PRODUCT]
    fns = callables(mods)
    rdt, cdt = (np.float32, np.complex64) if precision == 32 else (np.float64, np.complex128)
    tol = TOL32 if precision == 32 else TOL64
    extra = rng.random(shape).astype(rdt)
    config.precision = precision
    try:
        for obj in (rng.random(shape).astype(rdt), (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt)):
            for shift in (False, True):
                fused = convolution.apply_transfer_functions(dev(obj), 0.5, sp, shift=shift)
                plain = convolution.apply_transfer_functions(dev(obj), 0.5, fns, shift=shift)
                assert fused.dtype == plain.dtype and fused.shape == plain.shape
                err = rel_max(tonp(fused), tonp(plain))
                print(f'{shape} precision {precision} complex {np.iscomplexobj(obj)} shift {shift}: {err:.3e} (tol {tol:.1e})')
                assert err <= tol
                fused = convolution.apply_transfer_functions(dev(obj), 0.5, sp[:2] + [dev(extra)], shift=shift)
                plain = convolution.apply_transfer_functions(dev(obj), 0.5, fns[:2] + [dev(extra)], shift=shift)
                assert rel_max(tonp(fused), tonp(plain)) <= tol
                # a record next to a plain callable: the map-by-map path, with the record's map from the same frequencies
                mixed = convolution.apply_transfer_functions(dev(obj), 0.5, [sp[0], fns[1], dev(extra)], shift=shift)
                assert rel_max(tonp(mixed), tonp(plain)) <= tol
    finally:
        config.precision = 64


def test_the_product_is_one_capturable_launch_in_front_of_the_chain(mods):
    """nothing but the one kernel: no uploads, no host reads -- so the build of H records into a graph and replays to the same bits"""
    from prysm_amd import convolution, graph
    sp = [specs(mods)[n] for n in C.PRODUCT]
    a = dev(np.random.default_rng(2).random((128, 128)).astype(np.float32))
    eager = convolution.transfer_function((128, 128), 0.5, sp + [a], shift=True, dtype=torch.complex64)
    model = graph.capture(lambda m: convolution.transfer_function((128, 128), 0.5, sp + [m], shift=True, dtype=torch.complex64), a)
    assert torch.equal(model(a), eager)
    assert torch.equal(model(a * 2), eager * 2)
    # the whole call: H in the precision apply_transfer_functions chooses (config.precision for generated frequencies)
    obj = dev(np.random.default_rng(3).random((128, 128)).astype(np.float32))
    whole = graph.capture(lambda o: convolution.apply_transfer_functions(o, 0.5, sp + [a], shift=True), obj)
    H = convolution.transfer_function((128, 128), 0.5, sp + [a], shift=True)
    assert H.dtype == torch.complex128 and torch.equal(whole(obj), convolution.apply_transfer_functions(obj, 0.5, [H]))


# ----------------------------------------------------------------------------- 2. the second trip of the grid-stride loops

ROWS = 4 * 65535 + 5      # pm_sweep.h: 4 rows per workgroup, at most 65535 workgroups down the rows


def test_object_render_on_the_second_trip(mods):
    objects = mods['objects']
    x = np.array([-0.3, 0.01, 0.5])
    y = (np.arange(ROWS) - ROWS // 2) * (0.7 / ROWS)
    params = IP().object_params(IP().TILTEDSQUARE, angle=4, radius=0.37, contrast=0.9, background='white')
    got = tonp(objects.tiltedsquare(dev(x), dev(y), angle=4, radius=0.37))
    xx, yy = np.meshgrid(x, y)
    C.compare_target(got, IP().object_render(*params, xx, yy, np.float64), (params, xx, yy, False), np.float64)
    assert got.shape == (ROWS, 3) and len(np.unique(got[4 * 65535:])) == 2       # both values on the second trip's rows
    from prysm_amd.conf import config
    config.precision = 32
    try:
        edge = tonp(objects.slantededge(shape=(ROWS, 3), dx=0.01, angle=40))
    finally:
        config.precision = 64
    p2 = IP().object_params(IP().SLANTEDEDGE, angle=40, contrast=0.9, crossed=False)
    gx, gy = IP().grid_axes((ROWS, 3), 0.01, np.float32)
    xx, yy = np.meshgrid(gx, gy)
    assert edge.dtype == np.float32
    C.compare_target(edge, IP().object_render(*p2, xx, yy, np.float32), (p2, xx, yy, False), np.float32)


@pytest.mark.parametrize('dt', DTS)
def test_tf_product_on_the_second_trip(mods, dt):
    from prysm_amd import convolution
    sp = [specs(mods)['pixel'], specs(mods)['jitter']]
    cdt = torch.complex128 if dt == np.float64 else torch.complex64
    got = tonp(convolution.transfer_function((ROWS, 3), C.DX, sp, shift=True, dtype=cdt))
    model = IP().tf_product((ROWS, 3), sp, dt, dx=C.DX, shift=True)
    fmax = 1 / (2 * C.DX)
    bound = sum(16 * C.eps(dt) * (1 + a) for a in (np.pi * fmax * C.PIXEL[0], np.pi * fmax * C.PIXEL[1], 2 * (np.pi * C.JITTER * fmax * 2 ** 0.5) ** 2))
    assert got.shape == (ROWS, 3) and np.abs(got - model).max() <= bound


def test_polar_resample_on_the_second_trip():
    from prysm_amd import coordinates
    x = np.array([-1.0, 0.0, 1.0])
    y = np.linspace(-1, 1, ROWS)
    data = np.exp(-(x[None, :] ** 2 + (y[:, None] - 0.2) ** 2) / 0.3)
    rho, phi, pol = coordinates.uniform_cart_to_polar(x, y, dev(data))
    mr, mp, model = IP().polar_resample(x, y, data, np.float64)
    assert np.array_equal(tonp(rho), mr) and np.array_equal(tonp(phi), mp) and pol.shape == (ROWS, 3)
    near = C.polar_excluded(x, y, np.float64)
    assert near.mean() <= C.POLAR_EXCLUDE_CAP
    assert np.abs(tonp(pol) - model)[~near].max() <= C.polar_bound(x, y, data, np.float64)


@functools.lru_cache(None)
def centroid_cap():
    """the most workgroups pm_centroid launches, read from its workspace query (24 bytes per workgroup)"""
    from prysm_amd import _lib as L
    lib = L.load()
    g = 1
    while g <= 1 << 22:
        got = lib.pm_centroid_workspace(256, g) // 24
        if got < g:
            assert lib.pm_centroid_workspace(256, got) // 24 == got == lib.pm_centroid_workspace(256 * got + 1, 1) // 24
            return int(got)
        g *= 2
    raise AssertionError('the workgroup count of pm_centroid never stops growing')


@pytest.mark.parametrize('dt', DTS)
def test_centroid_past_one_trip_is_exact_on_integers(mods, dt):
    """cap * 256 samples are one trip; small integers sum exactly in double in any order, so one sample dropped or doubled shows"""
    n = centroid_cap() * 256
    cols = 512
    rows = n // cols + 3
    rng = np.random.default_rng(8)
    d = rng.integers(0, 4, (rows, cols)).astype(dt)
    got = tonp(mods['psf'].centroid_device(strided(d)))
    s = d.astype(np.float64)
    ref = np.array([(np.arange(rows)[:, None] * s).sum() / s.sum(), (np.arange(cols)[None, :] * s).sum() / s.sum()])
    assert rows * cols > n and np.array_equal(got, ref)


@pytest.mark.parametrize('dt', DTS)
def test_crossing_mean_past_one_trip(dt):
    from prysm_amd import _lib as L
    from prysm_amd import _ops
    lib = L.load()
    cap = 1
    while lib.pm_psf_size_groups(4 * cap * 2) > cap:
        cap *= 2
    rows, cols = 4 * cap + 7, 70          # four rows per workgroup and trip; 70 columns: a lane's second column
    rng = np.random.default_rng(9)
    r = np.linspace(0, 1, cols).astype(dt)
    width = rng.uniform(0.1, 0.9, rows)
    polar = np.exp(-(r[None, :].astype(np.float64) / width[:, None]) ** 2).astype(dt)
    polar[5] = 0.0                        # rows that never cross
    polar[-1] = 0.0
    for metric, last in (('fwhm', 1), ('1/e', 0), (0.25, 1)):
        relative, value = IP().size_threshold(metric)
        got = tonp(_ops.psf_size(dev(polar), dev(r), relative, value, last))
        mean, count = IP().estimate_size(polar, r, metric, 'last' if last else 'first')
        hm = value * polar.max() if relative else value
        crossed = int(np.sum((polar[:, 0] > hm) & ~(polar[:, -1] > hm)))      # monotonic rows: they cross iff their ends straddle hm
        assert got[1] == count == crossed and rows - 300 < crossed <= rows - 2
        assert abs(got[0] - mean) <= C.eps(np.float64) * rows       # the rows' radii are the model's bits; only the order of the sum differs


# ----------------------------------------------------------------------------- 4., 5. centroid, autocrop, sizes

@pytest.mark.parametrize('dt', DTS)
def test_centroid_and_autocrop_of_a_displaced_gaussian(mods, dt):
    psf = mods['psf']
    g = C.golden()
    d = C.gaussian_psf(dt)
    data = dev(d)
    a, b = psf.centroid_device(data), psf.centroid_device(data)
    assert a.dtype == torch.float64 and torch.equal(a, b) and torch.equal(a, psf.centroid_device(strided(d)))
    px = psf.centroid(data, unit='pixels')
    tol = 1e-12 if dt == np.float64 else C.eps(np.float32) * 65
    assert isinstance(px[0], float) and np.abs(np.array(px) - g['psf_centroid_px']).max() <= tol
    assert abs(px[0] - 30.4) < 1e-3 and abs(px[1] - 35.2) < 1e-3
    sp = psf.centroid(data, dx=C.psf_dx())
    assert np.abs(np.array(sp) - g['psf_centroid_spatial']).max() <= tol * C.psf_dx()
    for n, key in ((100, 'psf_autocrop100'), (20, 'psf_autocrop20')):
        crop = psf.autocrop(data, n)
        assert crop.dtype == TDT[dt] and np.array_equal(tonp(crop), g[key].astype(dt))
        assert torch.equal(crop, psf.autocrop(strided(d), n))
    assert not tonp(psf.autocrop(data, 100))[[0, -1]].any()


@pytest.mark.parametrize('dt', DTS)
def test_sizes_of_a_displaced_gaussian(mods, dt):
    from prysm_amd import coordinates
    psf = mods['psf']
    g = C.golden()
    d = C.gaussian_psf(dt)
    data = dev(d)
    x, y = C.psf_grid()
    rho, phi, pol = coordinates.uniform_cart_to_polar(*C.psf_grid(dt), data)
    near = C.polar_excluded(x, y, dt)
    dev_ = np.abs(tonp(pol).astype(np.float64) - g['psf_polar'])[~near].max()
    print(f'polar {dt.__name__}: {dev_:.3e} (bound {C.polar_bound(x, y, C.gaussian_psf(), dt):.3e})')
    assert near.mean() <= C.POLAR_EXCLUDE_CAP and dev_ <= C.polar_bound(x, y, C.gaussian_psf(), dt)
    fns = [(psf.fwhm, 'fwhm', 2), (psf.one_over_e, '1/e', 2), (psf.one_over_e_sq, '1/e^2', 2),
           (lambda *a, **k: psf.estimate_size(a[0], 0.3, **k), 0.3, 1)]
    for i, (fn, metric, mult) in enumerate(fns):
        got = fn(data, dx=C.psf_dx())
        assert isinstance(got, float) and got == fn(data, dx=C.psf_dx()) == fn(strided(d), dx=C.psf_dx())
        assert got == fn(data, x=C.psf_grid(dt)[0], y=C.psf_grid(dt)[1])
        bound = mult * C.size_bound64(C.gaussian_psf(), g['psf_polar'], rho_of(), metric) if dt == np.float64 else 4 * g['size_dev32'][i]
        print(f'size {metric} {dt.__name__}: got {got!r} reference {g["psf_sizes"][i]!r} deviation {abs(got - g["psf_sizes"][i]):.3e} (bound {bound:.3e})')
        assert abs(got - g['psf_sizes'][i]) <= bound
    with pytest.raises(ValueError, match='does not cross'):
        psf.estimate_size(data, 2.0, dx=C.psf_dx())


def rho_of():
    x, y = C.psf_grid()
    return IP().polar_axes(x, y)[0]


@pytest.mark.parametrize('dt', DTS)
def test_first_and_last_crossing_of_an_airy_pattern(mods, dt):
    psf = mods['psf']
    g = C.golden()
    airy = C.airy_psf(dt)
    # the pattern itself, from the kernel: the Airy function over the grid's radii
    x, y = C.psf_grid(dt)
    rad = (np.hypot(*np.meshgrid(x, y)) * dt(C.AIRY_SCALE)).astype(dt)
    made = tonp(psf.airydisk(dev(rad), C.AIRY_FNO, C.AIRY_WVL))
    assert np.abs(made.astype(np.float64) - C.airy_psf()).max() <= 2 * 16 * C.eps(dt) * (1 + np.pi * rad.max() / C.AIRY_WVL / C.AIRY_FNO)
    first = psf.estimate_size(dev(airy), C.AIRY_LEVEL, dx=C.psf_dx(), criteria='first')
    last = psf.estimate_size(dev(airy), C.AIRY_LEVEL, dx=C.psf_dx(), criteria='last')
    assert last > first + 0.05 and first == psf.estimate_size(dev(airy), C.AIRY_LEVEL, dx=C.psf_dx(), criteria='First')
    pa = IP().polar_resample(*C.psf_grid(), C.airy_psf(), np.float64)[2]
    for got, crit, key, k in ((first, 'first', 'psf_airy_first', 0), (last, 'last', 'psf_airy_last', 1)):
        bound = C.size_bound64(C.airy_psf(), pa, rho_of(), C.AIRY_LEVEL, crit) if dt == np.float64 else 4 * g['airy_dev32'][k]
        print(f'airy {crit} {dt.__name__}: got {got!r} reference {float(g[key])!r} deviation {abs(got - g[key]):.3e} (bound {bound:.3e})')
        assert abs(got - g[key]) <= bound


def test_smoke_sized_polar_maps_against_the_reference():
    """uniform_cart_to_polar on grids a and b, both precisions, contiguous and strided"""
    from prysm_amd import coordinates
    g = C.golden()
    for tag in ('a', 'b'):
        for dt in DTS:
            x, y = C.grid_vectors(tag, dt)
            data = C.smooth_data(tag, dt)
            rho, phi, pol = coordinates.uniform_cart_to_polar(x, y, dev(data))
            assert pol.dtype == TDT[dt] and torch.equal(pol, coordinates.uniform_cart_to_polar(dev(x), dev(y), strided(data))[2])
            x64, y64 = C.grid_vectors(tag)
            idx = g[f'{tag}_idx']
            near = C.polar_excluded(x64, y64, dt).reshape(-1)[idx]
            dev_ = np.abs(tonp(pol).reshape(-1)[idx].astype(np.float64) - g[f'{tag}_polar'])
            bound = C.polar_bound(x64, y64, C.smooth_data(tag), dt)
            print(f'polar {tag} {dt.__name__}: {dev_[~near].max():.3e} (bound {bound:.3e}), excluded {near.mean():.4f}')
            assert near.mean() <= C.POLAR_EXCLUDE_CAP and dev_[~near].max() <= bound
            assert np.array_equal(tonp(rho).astype(np.float64), IP().polar_axes(x, y)[0].astype(dt).astype(np.float64))
