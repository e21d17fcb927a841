"""CPU: the detector's model (prysm_amd/detector_plan.py, the numpy restatement of csrc/detector.hip) against published vectors, the
reference's recorded exposures (tests/golden/detector.npz) and theory; and the argument checks of the C entry points."""
import ctypes
import json

import numpy as np
import pytest

from detector_common import MEANS, assert_poisson, chi_square_poisson, corr, detector_kwargs, exposure_cases, ks_normal
from prysm_amd import detector_plan as DP

N = 1 << 20


@pytest.fixture(scope='module')
def g(golden):
    return golden('detector')


def _hex(words):
    return ' '.join('%08x' % int(w) for w in words)


def test_philox_known_answers():
    """the published vectors of Philox4x32-10 (Random123's kat_vectors)"""
    assert _hex(DP.philox4x32((0, 0, 0, 0), (0, 0))) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert _hex(DP.philox4x32((0xffffffff,) * 4, (0xffffffff,) * 2)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert _hex(DP.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'
    # arrays broadcast: element i equals the scalar call
    c0 = np.arange(5)
    w = DP.philox4x32((c0, 7, 9, 1), (3, 4))
    for i in range(5):
        assert [int(x[i]) for x in w] == [int(x) for x in DP.philox4x32((i, 7, 9, 1), (3, 4))]


def test_uniform53_is_exact_and_half_open():
    assert DP.uniform53(0, 0) == 0.0
    top = DP.uniform53(0xffffffff, 0xffffffff)
    assert top == 1.0 - 2.0 ** -53 and top < 1.0
    assert DP.uniform53(1 << 5, 0) == 2.0 ** -27 and DP.uniform53(0, 1 << 6) == 2.0 ** -53


def test_digitize_equals_the_reference_on_recorded_draws(g):
    """exact integer equality on every pixel of every case; the fixture's generator asserts that each case clips at the full well,
    at the ADC cap and at 0"""
    for name, (c, a) in exposure_cases(g).items():
        dn = DP.digitize(a['shot'] + a['read'], c['bias'], c['fwc'], c['conversion_gain'], c['bits'], a['lut'])
        want = a['dn'].reshape(a['shot'].shape)
        assert dn.dtype == a['dn'].dtype, name
        assert np.array_equal(dn, want), f'{name}: {np.count_nonzero(dn != want)} samples differ'


def test_mean_electrons_matches_the_recorded_poisson_mean(g):
    for name, (c, a) in exposure_cases(g).items():
        m = DP.mean_electrons(a['img'], c['exposure_time'], c['dark_current'], a['prnu'], a['dcnu'])
        np.testing.assert_allclose(m, a['mean'], rtol=4e-16, atol=0, err_msg=name)


def test_container_dtypes_and_the_32_bit_limit():
    assert DP.container(8) == np.uint8 and DP.container(9) == np.uint16 and DP.container(16) == np.uint16
    assert DP.container(17) == np.uint32 and DP.container(32) == np.uint32
    assert DP.container(12, np.zeros(4096, dtype=np.float32)) == np.float32
    with pytest.raises(ValueError):
        DP.container(33)
    with pytest.raises(ValueError):
        DP.digitize(np.zeros(3), 0, 1, 1, 40)


def _bin_cases(g, which):
    for c in json.loads(str(g[which])):
        f = c['factor']
        yield c, (tuple(f) if isinstance(f, list) else f)


def test_bindown_and_tile_model_against_the_reference(g):
    """a bin of f non-negative terms summed in any order has relative error at most f eps: 2 f eps of the dtype"""
    eps = np.finfo(np.float64).eps
    for c, f in _bin_cases(g, 'bins'):
        a, want = g[f"bin_{c['name']}_in"], g[f"bin_{c['name']}_out"]
        fy, fx = DP.factors_of(a.shape, f)
        got = DP.bindown(a, f, c['mode'])
        assert got.shape == want.shape and got.dtype == want.dtype
        np.testing.assert_allclose(got, want, rtol=2 * fy * fx * eps, atol=0, err_msg=c['name'])
    for c, f in _bin_cases(g, 'tiles'):
        a, want = g[f"tile_{c['name']}_in"], g[f"tile_{c['name']}_out"]
        got = DP.tile(a, f, c['scaling'])
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=2 * eps, atol=0, err_msg=c['name'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_tile_is_the_adjoint_of_bindown_in_the_model(dtype):
    rng = np.random.default_rng(3)
    eps = np.finfo(dtype).eps
    for shape, f in (((24, 36), 3), ((24, 36), (2, 4)), ((3, 16, 20), (1, 4, 2))):
        fy, fx = DP.factors_of(shape, f)
        a = rng.random(shape).astype(dtype)
        b = rng.random(shape[:-2] + (shape[-2] // fy, shape[-1] // fx)).astype(dtype)
        for bmode, tmode in (('avg', 'sum'), ('sum', 'avg')):
            lhs = np.sum(DP.bindown(a, f, bmode).astype(np.float64) * b)
            rhs = np.sum(a.astype(np.float64) * DP.tile(b, f, tmode))
            assert abs(lhs - rhs) <= 2 * fy * fx * eps * max(abs(lhs), abs(rhs)), (shape, f, bmode)


def test_bin_arguments():
    with pytest.raises(ValueError):
        DP.bindown(np.zeros((5, 6)), 2)
    with pytest.raises(ValueError):
        DP.bindown(np.zeros((4, 6)), 2, 'median')
    with pytest.raises(ValueError):
        DP.tile(np.zeros((4, 6)), 2, 'median')
    with pytest.raises(ValueError):
        DP.bindown(np.zeros((4, 6)), (2, 2, 2))
    from prysm_amd import detector
    with pytest.raises(ValueError):      # before any launch: no device is needed to be told so
        detector.bindown(np.zeros((5, 6)), 2)
    with pytest.raises(ValueError):
        detector.bindown(np.zeros((4, 6)), 2, 'median')
    with pytest.raises(ValueError):
        detector.tile(np.zeros((4, 6)), 2, 'median')


def test_the_yardstick_on_numpys_own_generators():
    """the statistics themselves, applied to numpy's samplers: they sit far inside the thresholds"""
    for lam in MEANS:
        assert_poisson(np.random.RandomState(3).poisson(lam, N), lam, 'numpy')
    ks, bound = ks_normal(np.random.RandomState(5).normal(0, 3.7, N) / 3.7)
    assert ks < bound
    # and they do reject a wrong sampler: a Gaussian approximation at mean 4, a mean off by 1 %
    bad = np.maximum(np.rint(np.random.RandomState(3).normal(4.0, 2.0, N)), 0)
    chi, dof = chi_square_poisson(bad, 4.0)
    assert chi > 100 * dof
    chi, dof = chi_square_poisson(np.random.RandomState(3).poisson(37.0 * 1.01, N), 37.0)
    assert chi > 10 * dof


@pytest.mark.parametrize('lam', MEANS)
def test_poisson_walk_is_poisson(lam):
    assert_poisson(DP.poisson_walk(lam, 11, 0, 0, np.arange(N)), lam, 'model')


def test_poisson_walk_over_frames_is_poisson():
    """the frame word of the counter, not only the pixel word"""
    fr = np.arange(1 << 10).reshape(-1, 1)
    assert_poisson(DP.poisson_walk(4.0, 5, 3, fr, np.arange(1 << 10).reshape(1, -1)), 4.0, 'model frames')
    assert_poisson(DP.poisson_walk(37.0, 5, 3, fr, np.arange(1 << 10).reshape(1, -1)), 37.0, 'model frames')


def test_normal_walk_is_normal():
    z = DP.normal_walk(11, 0, 0, np.arange(N))
    ks, bound = ks_normal(z)
    print(f'KS {ks:.5f} / {bound:.5f}')
    assert ks < bound
    assert abs(z.mean()) < 6 / np.sqrt(N) and abs(z.var() - 1) < 6 * np.sqrt(2 / N)


def test_independence_across_the_counter_layout():
    n = 1 << 18
    pix = np.arange(n)
    bound = 6 / np.sqrt(n)
    for lam in (4.0, 37.0):
        s0, s1 = DP.poisson_walk(lam, 9, 0, 0, pix), DP.poisson_walk(lam, 9, 0, 1, pix)
        assert corr(s0, s1) < bound                       # frames k and k + 1
        assert corr(s0[:-1], s0[1:]) < bound              # neighbouring pixels
        assert corr(s0, DP.normal_walk(9, 0, 0, pix)) < bound     # shot and read draw of one sample
    z0, z1 = DP.normal_walk(9, 0, 0, pix), DP.normal_walk(9, 0, 1, pix)
    assert corr(z0, z1) < bound and corr(z0[:-1], z0[1:]) < bound


def test_poisson_walk_edge_cases():
    assert np.all(DP.poisson_walk(0.0, 1, 0, 0, np.arange(1000)) == 0)
    big = DP.poisson_walk(2.0 ** 31 - 1, 1, 0, 0, np.arange(4096))        # the largest mean promised exact: PTRS, no approximation
    assert np.all(big == np.floor(big)) and abs(big.mean() - (2.0 ** 31 - 1)) < 6 * np.sqrt(2.0 ** 31 / 4096)
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError):
            DP.poisson_walk(np.array([1.0, bad]), 1, 0, 0, np.arange(2))
        z = DP.poisson_walk(np.array([1.0, bad]), 1, 0, 0, np.arange(2), invalid='zero')
        assert z[1] == 0


def test_log_factorial():
    """against math.lgamma.  The series' largest term is x log x (x = k + 1), rounded twice (the logarithm, the product) before the
    sums: 4 eps of that term bounds the model's error plus lgamma's own; the truncation of the series is below eps from x = 33 on."""
    import math
    eps = np.finfo(np.float64).eps
    for k in list(range(0, 200)) + [1000, 12345, 10 ** 6, 10 ** 9]:
        want = math.lgamma(k + 1)
        assert abs(float(DP.log_factorial(float(k))) - want) <= 4 * eps * max(1.0, (k + 1) * math.log(k + 1)), k


def test_frames_equal_successive_single_frames_and_seeds_differ(g):
    c, a = exposure_cases(g)['b12']
    kw = detector_kwargs(c, a)
    img = a['img']
    many = DP.expose_walk(img, seed=42, exposure=5, frames=4, **kw)
    assert many.shape == (4,) + img.shape and many.dtype == np.uint16
    for f in range(4):
        one = DP.expose_walk(img, seed=42, exposure=5 + f, frames=1, **kw)
        assert np.array_equal(one[0], many[f])
    other = DP.expose_walk(img, seed=43, exposure=5, frames=4, **kw)
    assert np.mean(other != many) > 0.5
    # a stack counts its pixels through: member b is the image at pixel_offset b * m * n
    st = DP.expose_walk(np.stack([img, img * 0.5]), seed=42, exposure=5, frames=2, **kw)
    assert np.array_equal(st[:, 0], many[:2])
    assert np.array_equal(st[:, 1], DP.expose_walk(img * 0.5, seed=42, exposure=5, frames=2, pixel_offset=img.size, **kw))


def test_expose_walk_statistics_match_the_recorded_reference(g):
    """the model's exposure and the reference's, same parameters: the mean DN over the unclipped pixels agrees within 6 sigma of the
    frame average (different generators, so only in distribution)"""
    c, a = exposure_cases(g)['b16']
    kw = detector_kwargs(c, a)
    dn, shot, read, mean = DP.expose_walk(a['img'], seed=1, frames=3, parts=True, **kw)
    np.testing.assert_allclose(mean, a['mean'], rtol=4e-16)
    ref = a['dn'].astype(np.float64)
    mid = (ref.min(0) > 0) & (ref.max(0) < 2 ** 16 - 1) & (a['mean'] + 6 * np.sqrt(a['mean'] + 10) < c['fwc'])
    sigma = np.sqrt(a['mean'] + c['read_noise'] ** 2) / c['conversion_gain']
    z = (dn.astype(np.float64).mean(0) - ref.mean(0))[mid] / (sigma[mid] * np.sqrt(2 / 3) + 1)
    assert mid.sum() > 300 and np.abs(z).max() < 6


def test_c_entry_points_report_argument_errors_without_a_gpu():
    from prysm_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(256)

    def err(rc, word):
        assert rc == L.PM_ERR_ARG
        assert word.encode() in lib.pm_last_error(), lib.pm_last_error()
        with pytest.raises(ValueError):
            L.check(rc)
    # pm_bindown / pm_tile
    err(lib.pm_bindown(L.PM_C64, 1, 4, 4, 2, 2, L.PM_BIN_AVG, p, 8, 64, p, 4, 16, None), 'dtype')
    err(lib.pm_bindown(L.PM_F32, 1, 4, 4, 2, 2, 7, p, 8, 64, p, 4, 16, None), 'mode')
    err(lib.pm_bindown(L.PM_F32, 1, 4, 4, 0, 2, L.PM_BIN_SUM, p, 8, 64, p, 4, 16, None), 'factors')
    err(lib.pm_bindown(L.PM_F32, 1, 4, 4, 2, 2, L.PM_BIN_SUM, None, 8, 64, p, 4, 16, None), 'null')
    err(lib.pm_bindown(L.PM_F32, 1, 4, 4, 2, 2, L.PM_BIN_SUM, p, 7, 64, p, 4, 16, None), 'leading dimension')
    err(lib.pm_bindown(L.PM_F32, 2, 4, 4, 2, 2, L.PM_BIN_SUM, p, 8, 63, p, 4, 16, None), 'bstride')
    err(lib.pm_tile(L.PM_BOOL, 1, 4, 4, 2, 2, 1.0, p, 4, 16, p, 8, 64, None), 'dtype')
    err(lib.pm_tile(L.PM_F64, 1, 4, 4, 2, -1, 1.0, p, 4, 16, p, 8, 64, None), 'factors')
    err(lib.pm_tile(L.PM_F64, 1, 4, 4, 2, 2, float('nan'), p, 4, 16, p, 8, 64, None), 'scale')
    err(lib.pm_tile(L.PM_F64, 1, 4, 4, 2, 2, 1.0, p, 4, 16, None, 8, 64, None), 'null')
    err(lib.pm_tile(L.PM_F64, 1, 4, 4, 2, 2, 1.0, p, 4, 16, p, 7, 64, None), 'leading dimension')
    # pm_detector_digitize
    dig = lib.pm_detector_digitize
    err(dig(L.PM_C128, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 8, None, 0, 1, p, None), 'dtype')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 33, None, 0, 4, p, None), 'bits')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 0, None, 0, 4, p, None), 'bits')
    err(dig(L.PM_F64, 1, 4, 4, None, 4, 16, 0.0, 100.0, 1.0, 8, None, 0, 1, p, None), 'null')
    err(dig(L.PM_F64, 1, 4, 4, p, 3, 16, 0.0, 100.0, 1.0, 8, None, 0, 1, p, None), 'ld')
    err(dig(L.PM_F64, 2, 4, 4, p, 4, 15, 0.0, 100.0, 1.0, 8, None, 0, 1, p, None), 'bstride')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 0.0, 8, None, 0, 1, p, None), 'conversion_gain')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 8, None, 0, 3, p, None), 'out_bytes')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 12, None, 0, 1, p, None), 'do not fit')
    err(dig(L.PM_F64, 1, 4, 4, p, 4, 16, 0.0, 100.0, 1.0, 12, p, 4095, 2, p, None), 'look-up table')
    # pm_detector_expose
    def expose(dtype=L.PM_F32, img=p, ld=4, bits=8, lut=None, lut_len=0, obytes=1, frames=1, offset=0, state=p, out=p, rn=1.0):
        return lib.pm_detector_expose(dtype, 1, 4, 4, img, ld, 16, None, None, 1.0, 0.0, rn, 0.0, 100.0, 1.0, bits, lut, lut_len, obytes,
                                      frames, 1, offset, state, out, None)
    err(expose(dtype=L.PM_C64), 'dtype')
    err(expose(bits=40, obytes=4), 'bits')
    err(expose(img=None), 'null')
    err(expose(out=None), 'null')
    err(expose(ld=2), 'ld')
    err(expose(state=None), 'state')
    err(expose(frames=-1), 'frames')
    err(expose(offset=-4), 'pixel_offset')
    err(expose(rn=float('inf')), 'finite')
    err(expose(bits=16, obytes=1), 'do not fit')
    err(expose(bits=8, lut=p, lut_len=100, obytes=2), 'look-up table')
    # pm_detector_words
    err(lib.pm_detector_words(1, 0, 16, 0, 0, None, None), 'null')
    err(lib.pm_detector_words(1, -1, 16, 0, 0, p, None), 'negative')
    # empty work is no error and touches no device
    assert lib.pm_bindown(L.PM_F32, 0, 4, 4, 2, 2, L.PM_BIN_SUM, p, 8, 64, p, 4, 16, None) == 0
    assert expose(frames=0) == 0


def test_symbols_are_declared_exported_and_signed():
    from prysm_amd import _lib as L
    lib = L.load()
    hdr = open(__import__('os').path.join(__import__('conftest').ROOT, 'include', 'prysm_amd.h')).read()
    for s in ('pm_bindown', 'pm_tile', 'pm_detector_digitize', 'pm_detector_expose', 'pm_detector_words'):
        assert s + '(' in hdr and hasattr(lib, s) and s in L.SIGNATURES
    assert lib.pm_version() == 107


def test_detector_object_without_a_device():
    """construction, seeding and the checks that come before any device work"""
    from prysm_amd.detector import Detector
    d = Detector(1.0, 2.0, 3.0, 4.0, 5.0, 12, 0.5, seed=99)
    assert (d.dark_current, d.read_noise, d.bias, d.fwc, d.conversion_gain, d.bits, d.exposure_time) == (1.0, 2.0, 3.0, 4.0, 5.0, 12, 0.5)
    assert d.prnu is None and d.dcnu is None and d.lut is None and d.seed_value == 99 and d.exposure_index == 0
    a, b = Detector(1, 2, 3, 4, 5, 12, 0.5), Detector(1, 2, 3, 4, 5, 12, 0.5)
    assert a.seed_value != b.seed_value and 0 <= a.seed_value < 2 ** 64          # host entropy, readable
    assert d.seed(7) is d and d.seed_value == 7
    with pytest.raises(TypeError):
        d.seed(1.5)
    with pytest.raises(ValueError):
        Detector(1, 2, 3, 4, 5, 40, 0.5).expose(np.zeros((4, 4)))
    with pytest.raises(ValueError):
        Detector(1, 2, 3, 4, 5, 40, 0.5).digitize(np.zeros((4, 4)))
