"""GPU: the detector kernels (csrc/detector.hip) against their numpy model (prysm_amd/detector_plan.py), the reference's recorded
exposures (tests/golden/detector.npz) and the statistics of tests/detector_common.py.

The Philox words are read through the small entry point pm_detector_words (cleaner than an exposure configured to leak them).
No test provokes a fault: bad values are data, never addresses."""
import json

import numpy as np
import pytest
import torch

from detector_common import MEANS, assert_poisson, corr, detector_kwargs, exposure_cases, ks_normal
from prysm_amd import detector_plan as DP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g(golden):
    return golden('detector')


@pytest.fixture(scope='module')
def det(pa):
    from prysm_amd import detector
    return detector


def tonp(t):
    return t.cpu().numpy()


def same(a, b):
    """bitwise equality of two device tensors, judged on the host (torch's comparisons do not cover every unsigned dtype)"""
    a, b = tonp(a), tonp(b)
    return a.dtype == b.dtype and np.array_equal(a, b)


def counting(det, seed, read_noise=0.0, bias=0.0):
    """a detector whose DN is the electron count itself: gain 1, 32 bits, a full well out of reach"""
    return det.Detector(0.0, read_noise, bias, 1e18, 1.0, 32, 1.0, seed=seed)


def test_philox_words_equal_the_model(pa):
    from prysm_amd import _lib as L
    for seed, pixel0, frame, block in ((0, 0, 0, 0), (0x123456789abcdef, 5, 3, 1), (2 ** 64 - 1, 2 ** 32 - 10, 2 ** 31 + 7, 200)):
        n = 1000
        out = torch.empty((n, 4), dtype=torch.int32, device='cuda')
        sseed = seed - (1 << 64) if seed >= (1 << 63) else seed
        L.check(L.load().pm_detector_words(sseed, pixel0, n, frame, block, L.ptr(out), L.stream_ptr()))
        got = tonp(out).view(np.uint32)
        want = np.stack(DP.sample_words(seed, frame, 0, pixel0 + np.arange(n, dtype=np.int64), block), axis=1)
        assert np.array_equal(got, want)
    # the published vector, through the kernel: counter (pixel = 0, frame = 0, block = 0), key 0
    out = torch.empty((1, 4), dtype=torch.int32, device='cuda')
    L.check(L.load().pm_detector_words(0, 0, 1, 0, 0, L.ptr(out), L.stream_ptr()))
    assert ' '.join('%08x' % int(x) for x in tonp(out).view(np.uint32)[0]) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_digitize_equals_the_reference_on_recorded_draws(det, g, dtype):
    """fp64 electrons: the reference's DN exactly.  fp32 electrons: the model on the same rounded electrons (the tail widens them
    to fp64), and the reference wherever rounding the electrons to fp32 did not move them across a DN."""
    for name, (c, a) in exposure_cases(g).items():
        d = det.Detector(**detector_kwargs(c, a), seed=1)
        el = (a['shot'] + a['read']).astype(dtype)
        want = DP.digitize(el, c['bias'], c['fwc'], c['conversion_gain'], c['bits'], a['lut'])
        if dtype == np.float64:
            assert np.array_equal(want, a['dn'].reshape(el.shape))
        got = d.digitize(el)
        assert tonp(got).dtype == want.dtype and got.shape == el.shape
        assert np.array_equal(tonp(got), want), name
        # a stack with strided rows and members: the same samples
        big = torch.zeros((el.shape[0] + 1, el.shape[1] + 3, el.shape[2] + 5), dtype=torch.from_numpy(el).dtype, device='cuda')
        view = big[:el.shape[0], 2:2 + el.shape[1], 1:1 + el.shape[2]]
        view.copy_(torch.from_numpy(el))
        assert not view.is_contiguous() and np.array_equal(tonp(d.digitize(view)), want), name
        assert np.array_equal(tonp(d.digitize(el[0])), want[0])


def test_mean_electrons(det, g):
    for name, (c, a) in exposure_cases(g).items():
        d = det.Detector(**detector_kwargs(c, a), seed=1)
        np.testing.assert_allclose(tonp(d.mean_electrons(a['img'])), a['mean'], rtol=4e-16, atol=0)


def _ramp_image(n=256):
    """means 0 ... 1e5 at exposure time 1: a quadratic ramp through every regime of the sampler, exact zeros included"""
    i = np.arange(n * n, dtype=np.float64).reshape(n, n)
    img = 1e5 * (i / (n * n - 1)) ** 3
    img[0, :16] = 0.0
    return img


@pytest.mark.parametrize('bits', [8, 12, 16, 24])
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_expose_equals_the_model(det, bits, dtype):
    """256 x 256, means 0 ... 1e5, 8 frames, maps (and a LUT up to 16 bits): equality on EVERY sample.  The integer stream is exact; a
    transcendental may round differently on the device and flip a sample only when a uniform falls within an ulp of a threshold
    (about once in 1e13 samples), so a difference is printed with its pixel and mean, not tolerated."""
    rng = np.random.default_rng(bits)
    img = _ramp_image().astype(dtype)
    prnu = 1 + 0.02 * rng.standard_normal(img.shape)
    dcnu = np.abs(1 + 0.3 * rng.standard_normal(img.shape))
    lut = np.round(np.arange(2 ** bits, dtype=np.float64) ** 0.99 + 2).astype(np.uint16 if bits < 16 else np.uint32) if bits <= 16 else None
    cap_e = 0.8e5                                              # the ADC cap sits at 80 % of the brightest mean, the full well at 90 %
    kw = dict(dark_current=3.0, read_noise=4.5, bias=-6.0, fwc=0.9e5, conversion_gain=cap_e / (2 ** bits - 1), bits=bits, exposure_time=1.0,
              prnu=prnu, dcnu=dcnu, lut=lut)
    d = det.Detector(**kw, seed=0xfeedbeef12345)
    d.expose(img, frames=3)                                    # the exposure index is 3 when the frames under test start
    got = tonp(d.expose(img, frames=8))
    want, shot, read, mean = DP.expose_walk(img, seed=0xfeedbeef12345, exposure=3, frames=8, parts=True, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape == (8, 256, 256)
    assert d.exposure_index == 11
    bad = np.argwhere(got != want)
    for f, r, c in bad[:20]:
        print(f'frame {f} pixel ({r}, {c}) mean {mean[r, c]!r} shot {shot[f, r, c]} read {read[f, r, c]!r}: kernel {got[f, r, c]} model {want[f, r, c]}')
    assert len(bad) == 0, f'{len(bad)} of {got.size} samples differ'
    # every branch was visited
    assert (mean == 3.0 * dcnu)[0, :16].all() and (mean < DP.PTRS_MIN).any() and (mean > 5e4).any()
    assert (got == got.max()).sum() > 100 and (got == got.min()).sum() > 10


def test_device_samples_are_poisson_and_normal(det):
    """the statistics of the CPU tests on device output at 1024 x 1024"""
    n = 1024
    pix = np.arange(n * n)
    for lam in MEANS:
        img = torch.full((n, n), lam, dtype=torch.float64, device='cuda')
        d = counting(det, seed=17)
        x = tonp(d.expose(img))
        assert x.dtype == np.uint32
        assert_poisson(x, lam, 'kernel')
        if lam in (4.0, 37.0):
            assert np.array_equal(x.ravel()[:4096], DP.poisson_walk(lam, 17, 0, 0, pix[:4096]).astype(np.uint32))
    # read noise alone: mean 0, sigma 1e6 electrons about a bias of 2^31, so the truncation to a DN moves the KS statistic by < 1e-6
    d = counting(det, seed=17, read_noise=1e6, bias=2.0 ** 31)
    zero = torch.zeros((n, n), dtype=torch.float32, device='cuda')
    r2 = tonp(d.expose(zero, frames=2)).astype(np.float64)
    z = (r2 - 2.0 ** 31) / 1e6
    ks, bound = ks_normal(z[0])
    print(f'kernel KS {ks:.5f} / {bound:.5f}')
    assert ks < bound
    # independence: frames k and k + 1, neighbouring pixels, and the shot and the read draw of the SAME sample (same seed, exposure
    # index, frame and pixel: one exposure with the read noise alone, one with the shot noise alone)
    cb = 6 / np.sqrt(n * n)
    assert corr(z[0], z[1]) < cb and corr(z[0].ravel()[:-1], z[0].ravel()[1:]) < cb
    for lam in (4.0, 37.0):
        d = counting(det, seed=17)
        s2 = tonp(d.expose(torch.full((n, n), lam, dtype=torch.float64, device='cuda'), frames=2)).astype(np.float64)
        assert corr(s2[0], s2[1]) < cb and corr(s2[0].ravel()[:-1], s2[0].ravel()[1:]) < cb
        assert corr(s2[0], z[0]) < cb and corr(s2[1], z[1]) < cb
    assert np.all(tonp(counting(det, seed=3).expose(zero)) == 0)


def test_same_seed_same_frames(det, g):
    c, a = exposure_cases(g)['b16']
    kw = detector_kwargs(c, a)
    img = np.tile(a['img'], (4, 5))
    d1, d2 = det.Detector(**{**kw, 'prnu': None, 'dcnu': None}, seed=2026), det.Detector(**{**kw, 'prnu': None, 'dcnu': None}, seed=2026)
    many = d1.expose(img, frames=5)
    assert many.shape == (5,) + img.shape and many.dtype == torch.uint16
    loop = [d2.expose(img) for _ in range(5)]
    assert loop[0].shape == img.shape and all(same(many[f], loop[f]) for f in range(5))
    assert d1.exposure_index == d2.exposure_index == 5
    # repeat runs: bitwise equal; validate on / off: the same frames
    d1.seed(2026)
    again = d1.expose(img, frames=5, validate=False)
    assert same(again, many)
    # another seed: other frames
    assert np.mean(tonp(det.Detector(**{**kw, 'prnu': None, 'dcnu': None}, seed=2027).expose(img, frames=5)) != tonp(many)) > 0.5
    # a stack against its members at the documented pixel offsets (pixel_offset = b * m * n, same exposure index)
    stack = np.stack([img, 0.5 * img, 0.25 * img])
    d1.seed(5)
    st = d1.expose(stack, frames=2)
    assert st.shape == (2, 3) + img.shape
    for b in range(3):
        d2.seed(5)
        assert same(d2.expose(stack[b], frames=2, pixel_offset=b * img.size), st[:, b])
    # launch geometry: a strided view and fp32 / fp64 copies of an image that is exact in fp32 give the same frames
    img32 = img.astype(np.float32)
    d1.seed(8)
    ref = d1.expose(img32, frames=3)
    big = torch.zeros((img.shape[0] + 2, img.shape[1] + 7), dtype=torch.float32, device='cuda')
    big[1:-1, 3:-4] = torch.from_numpy(img32)
    d1.seed(8)
    assert same(d1.expose(big[1:-1, 3:-4], frames=3), ref)
    d1.seed(8)
    assert same(d1.expose(img32.astype(np.float64), frames=3), ref)


def test_graph_replays_draw_fresh_frames(det, g):
    """capture() runs fn twice to warm up (warmup=2) and those runs advance the exposure index like any other call: the replays are
    the eager sequence counted from there.  One stream, no queue or graph setting changed."""
    from prysm_amd import graph
    c, a = exposure_cases(g)['b12']
    kw = detector_kwargs(c, a)
    img = torch.from_numpy(np.tile(a['img'], (2, 2))).cuda()
    kw['prnu'], kw['dcnu'] = np.tile(a['prnu'], (2, 2)), None
    dg, de = det.Detector(**kw, seed=31337), det.Detector(**kw, seed=31337)
    model = graph.capture(lambda x: dg.expose(x, frames=2), img)
    replays = [model(img).clone() for _ in range(3)]
    for _ in range(2):
        de.expose(img, frames=2)                 # what the two warm-up runs consumed
    eager = [de.expose(img, frames=2) for _ in range(3)]
    for r, e in zip(replays, eager):
        assert r.dtype == torch.uint16 and same(r, e)
    assert not same(replays[0], replays[1]) and not same(replays[1], replays[2])
    assert dg.exposure_index == de.exposure_index == 10


def _bin_cases(g, which):
    for c in json.loads(str(g[which])):
        f = c['factor']
        yield c, (tuple(f) if isinstance(f, list) else f)


def test_bindown_and_tile_against_the_fixture(det, g):
    eps = np.finfo(np.float64).eps
    for c, f in _bin_cases(g, 'bins'):
        a, want = g[f"bin_{c['name']}_in"], g[f"bin_{c['name']}_out"]
        fy, fx = DP.factors_of(a.shape, f)
        np.testing.assert_allclose(tonp(det.bindown(a, f, c['mode'])), want, rtol=2 * fy * fx * eps, atol=0)
    for c, f in _bin_cases(g, 'tiles'):
        a, want = g[f"tile_{c['name']}_in"], g[f"tile_{c['name']}_out"]
        np.testing.assert_allclose(tonp(det.tile(a, f, c['scaling'])), want, rtol=2 * eps, atol=0)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bindown_and_tile_equal_the_model_bitwise(det, dtype):
    rng = np.random.default_rng(12)
    cases = [((1024, 1536), 2), ((1024, 1536), 4), ((1024, 1536), 8), ((90, 105), 3), ((90, 105), (3, 5)), ((96, 120), (2, 4)), ((96, 120), (4, 2)),
             ((33, 57), 1), ((3, 96, 120), (1, 4, 2)), ((2, 90, 105), (1, 3, 1)), ((1021, 771), (1, 3))]
    for shape, f in cases:
        fy, fx = DP.factors_of(shape, f)
        a = rng.random(shape).astype(dtype)
        small = rng.random(shape[:-2] + (shape[-2] // fy, shape[-1] // fx)).astype(dtype)
        for mode in ('avg', 'sum'):
            got = det.bindown(a, f, mode)
            assert got.dtype == torch.from_numpy(a).dtype and np.array_equal(tonp(got), DP.bindown(a, f, mode)), (shape, f, mode)
            assert np.array_equal(tonp(det.tile(small, f, mode)), DP.tile(small, f, mode)), (shape, f, mode)
        assert same(det.bindown(a, f), det.bindown(a, f))
        # strided input: rows and members of a larger tensor, at an odd element offset (no 16-byte alignment)
        big = torch.zeros(shape[:-2] + (shape[-2] + 1, shape[-1] + 3), dtype=torch.from_numpy(a).dtype, device='cuda')
        view = big[..., 1:, 3:]
        view.copy_(torch.from_numpy(a))
        assert np.array_equal(tonp(det.bindown(view, f, 'sum')), DP.bindown(a, f, 'sum')), (shape, f)
        sbig = torch.zeros(small.shape[:-1] + (small.shape[-1] + 5,), dtype=big.dtype, device='cuda')
        sbig[..., 2:-3] = torch.from_numpy(small)
        assert np.array_equal(tonp(det.tile(sbig[..., 2:-3], f, 'sum')), DP.tile(small, f, 'sum')), (shape, f)
        # the adjoint identity, on device results
        eps = np.finfo(dtype).eps
        for bmode, tmode in (('avg', 'sum'), ('sum', 'avg')):
            lhs = float(np.sum(tonp(det.bindown(a, f, bmode)).astype(np.float64) * small))
            rhs = float(np.sum(a.astype(np.float64) * tonp(det.tile(small, f, tmode))))
            assert abs(lhs - rhs) <= 2 * fy * fx * eps * max(abs(lhs), abs(rhs))
    with pytest.raises(ValueError):
        det.bindown(torch.zeros((5, 6), device='cuda'), 2)


def test_thin_functions_against_the_fixture(det, g):
    pa_ = json.loads(str(g['pixel_args']))
    x, y = g['pix_x'], g['pix_y']
    got = det.pixel(x, y, **pa_)
    assert got.dtype == torch.bool and np.array_equal(tonp(got), g['pixel'])
    np.testing.assert_allclose(tonp(det.pixel_ft(x * 0.1, y * 0.1, **pa_)), g['pixel_ft'], rtol=0, atol=4 * np.finfo(np.float64).eps)
    np.testing.assert_allclose(tonp(det.olpf_ft(x * 0.1, y * 0.1, **pa_)), g['olpf_ft'], rtol=0, atol=4 * np.finfo(np.float64).eps)
    lut = np.arange(256, dtype=np.float32)[::-1].copy()
    img = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(tonp(det.apply_lut(img, lut)), lut[img])


def test_pupil_to_exposure_end_to_end(det):
    """focus(...).intensity -> bindown -> expose on a seeded circular pupil with a little defocus.  Read noise 0, gain 1 and an integer
    bias, so a DN is the shot count plus the bias and its expectation is the model's mean exactly; every mean is >= 1000 electrons,
    so the 64-frame average is normal to well within the bound.  Per pixel: |average - mean| < 6 sigma / sqrt(64).  The normal tail
    puts 2e-9 of the pixels outside (1.3e-4 expected among 65536): none is allowed; and the noise must be there: the share beyond 3
    sigma / sqrt(64) (expected 0.27 %) lies in [0.1 %, 0.6 %]."""
    from prysm_amd import propagation as P
    n = 256
    yy, xx = np.mgrid[-n // 2:n // 2, -n // 2:n // 2] / (n / 2)
    r2 = xx * xx + yy * yy
    pupil = ((r2 <= 1) * np.exp(2j * np.pi * 0.35 * r2)).astype(np.complex64)
    psf = P.focus_intensity(pupil, 2)                                   # (512, 512) on the device
    psf = psf * (3e5 / float(psf.max()))
    binned = det.bindown(psf, 2, 'sum')
    assert binned.shape == (256, 256)
    assert np.array_equal(tonp(binned), DP.bindown(tonp(psf), 2, 'sum'))
    d = det.Detector(dark_current=2000.0, read_noise=0.0, bias=100.0, fwc=1e9, conversion_gain=1.0, bits=32, exposure_time=0.5, seed=64)
    frames = tonp(d.expose(binned, frames=64)).astype(np.float64)
    mean = DP.mean_electrons(tonp(binned), 0.5, 2000.0)
    assert mean.min() >= 1000
    want = DP.digitize(mean, 100.0, 1e9, 1.0, 32).astype(np.float64)                  # the noise-free DN: floor(mean) + bias
    z = (frames.mean(0) - (mean + 100.0)) / (np.sqrt(mean) / 8)
    print(f'max |z| {np.abs(z).max():.2f}, share beyond 3 sigma {np.mean(np.abs(z) > 3):.4f}')
    assert np.abs(want - (mean + 100.0)).max() <= 1
    assert (np.abs(z) >= 6).sum() == 0
    assert 0.001 <= np.mean(np.abs(z) > 3) <= 0.006


def test_validate_raises_on_a_negative_pixel(det):
    img = np.full((64, 64), 50.0)
    img[10, 20] = -1.0
    img[11, 21] = np.nan
    d = counting(det, seed=5)
    with pytest.raises(ValueError):
        d.expose(img)
    quiet = tonp(d.expose(img, validate=False))
    assert quiet[10, 20] == 0 and quiet[11, 21] == 0 and (quiet > 0).sum() == 64 * 64 - 2
    # the flag of an unvalidated call does not stick: a clean image after it passes
    img[10, 20] = img[11, 21] = 50.0
    assert tonp(d.expose(img)).mean() > 40
    d2 = counting(det, seed=5)
    with pytest.raises(ValueError):
        d2.expose(-img)
    assert tonp(d2.expose(img)).mean() > 40
    with pytest.raises(ValueError):
        det.Detector(0, 0, 0, 1, 1, 33, 1).expose(img)
