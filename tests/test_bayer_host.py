"""CPU: the Bayer model (prysm_amd/bayer_plan.py, the numpy restatement of csrc/bayer.hip) against the reference's results
(tests/golden/bayer.npz), the argument checks of prysm_amd.bayer that need no device, and those of the C entry points."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from prysm_amd import bayer_plan as BP

CFAS = ('rggb', 'bggr')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pm_bayer_demosaic', 'pm_bayer_weave', 'pm_bayer_deinterlace', 'pm_bayer_assemble', 'pm_bayer_class_max_workspace',
           'pm_bayer_class_max', 'pm_bayer_scale')


@pytest.fixture(scope='module')
def g(golden):
    return golden('bayer')


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as gr
        gr.build()
    return _lib.load()


def demosaic_bound(img, dtype):
    """32 eps max|img|: at most 11 products per sum, sum |w| <= 2.5, and a summation order (and, in float32, a precision of the
    running sum) that differs from scipy's"""
    return 32 * np.finfo(dtype).eps * float(np.max(np.abs(img)))


def test_reflect_rule():
    assert [int(BP.reflect_index(i, 4)) for i in (-2, -1, 0, 3, 4, 5)] == [1, 0, 0, 3, 3, 2]
    assert [int(BP.reflect_index(i, 1)) for i in (-2, -1, 0, 1, 2)] == [0, 0, 0, 0, 0]
    pad = np.pad(np.arange(5), 7, mode='symmetric')
    assert np.array_equal(BP.reflect_index(np.arange(-7, 12), 5), pad)


def test_weights_are_sixteenths_that_sum_to_one():
    for t in (BP.kernel_G_at_R_or_B, BP.kernel_R_at_G_in_RB, BP.kernel_R_at_G_in_BR, BP.kernel_R_at_B_in_BB):
        w = np.array(t) / 8.
        assert np.array_equal(w * 16, np.round(w * 16)) and w.sum() == 1.0 and np.abs(w).sum() <= 2.5
        yy, xx = np.indices((5, 5)) - 2
        assert np.all(w[np.abs(yy) + np.abs(xx) > 2] == 0) and np.count_nonzero(w) <= 11


def test_demosaic_model_equals_the_reference(g):
    cases = json.loads(str(g['demosaic']))
    assert len(cases) == 18
    for c in cases:
        img = g[c['key'] + '_in']
        for cfa in CFAS:
            want = g[f"{c['key']}_{cfa}"]
            got = BP.demosaic_malvar(img, cfa)
            assert got.dtype == want.dtype and got.shape == want.shape
            if c['dtype'] == 'float64':
                assert np.array_equal(got, want), (c['key'], cfa, np.abs(got - want).max())
            else:
                err = np.abs(got.astype(np.float64) - want).max()
                assert err <= demosaic_bound(img, np.float32), (c['key'], cfa, err)
    for cfa in CFAS:
        assert np.array_equal(BP.demosaic_malvar(g['dem_u16_in'], cfa), g[f'dem_u16_{cfa}'])
        assert BP.demosaic_malvar(g['dem_u16_in'], cfa, precision=np.float32).dtype == np.float32


def test_native_sites_of_the_model_are_copies(g):
    img = g['dem_37x70_float32_in']
    for cfa in CFAS:
        out = BP.demosaic_malvar(img, cfa)
        r, b = (0, 2) if cfa == 'rggb' else (2, 0)
        assert np.array_equal(out[0::2, 0::2, r], img[0::2, 0::2]) and np.array_equal(out[1::2, 1::2, b], img[1::2, 1::2])
        assert np.array_equal(out[0::2, 1::2, 1], img[0::2, 1::2]) and np.array_equal(out[1::2, 0::2, 1], img[1::2, 0::2])


def test_plane_functions_of_the_model_equal_the_reference(g):
    for m, n in ((6, 8), (24, 32)):
        planes = [g[f'pl_{m}x{n}_{k}'] for k in ('r', 'g1', 'g2', 'b')]
        mos = g[f'mos_{m}x{n}']
        for cfa in CFAS:
            assert np.array_equal(BP.composite(*planes, cfa=cfa), g[f'comp_{m}x{n}_{cfa}'])
            dec = BP.decomposite(mos, cfa)
            assert np.array_equal(np.stack(dec), g[f'dec_{m}x{n}_{cfa}'])
            assert all(np.shares_memory(p, mos) for p in dec)
            assert np.array_equal(BP.recomposite(*dec, cfa=cfa), g[f'recomp_{m}x{n}_{cfa}'])
            assert np.array_equal(BP.deinterlace(mos, cfa), g[f'deint_{m}x{n}_{cfa}'])


def test_white_balance_model_equals_the_reference(g):
    cases = json.loads(str(g['wb']))
    assert {(c['kind'], c.get('regime')) for c in cases if c['safe']} == {(k, r) for k in ('pre', 'post') for r in ('scalar', 'planes', 'one')}
    assert sum(not c['safe'] for c in cases) == 3
    for c in cases:
        for dt, suffix in ((np.float64, '_out'), (np.float32, '_out32')):
            src = g['wb_mosaic' if c['kind'] == 'pre' else 'wb_rgb'].astype(dt)
            if c['kind'] == 'pre':
                got = BP.wb_prescale(src, *c['gains'], cfa=c['cfa'], safe=c['safe'], saturation=c['saturation'])
            else:
                got = BP.wb_postscale(src, *c['gains'], safe=c['safe'], saturation=c['saturation'])
            want = g[f"wb_{c['name']}{suffix}"]
            assert got.dtype == want.dtype and np.array_equal(got, want), (c['name'], dt)


def test_superresolved_model_equals_the_reference(g):
    """the model composes the same transforms (pocketfft) with the separable multiplier: what is left is the rounding of the
    multiplier's product, a few eps"""
    for c in json.loads(str(g['superres'])):
        m, n = c['shape']
        planes = [g[f'sr_{m}x{n}_{k}'] for k in ('r', 'g1', 'g2', 'b')]
        want = g[f"sr_{m}x{n}_z{c['zoomfactor']}"]
        got = BP.assemble_superresolved(*planes, c['zoomfactor'])
        assert got.shape == want.shape == (m, n, 3)
        assert np.abs(got - want).max() <= 64 * np.finfo(np.float64).eps * np.abs(want).max()


def test_argument_checks_raise_the_references_errors():
    from prysm_amd import bayer
    x = np.ones((4, 4))
    with pytest.raises(ValueError):
        bayer.wb_prescale(x, 1, 1, 1, 1, safe=True)
    with pytest.raises(ValueError):
        bayer.wb_prescale(x, 1, 1, 1, 1, safe=True, saturation=[1, 2, 3])
    with pytest.raises(ValueError):
        bayer.wb_prescale(x, 1, 1, 1, 1, safe=True, saturation=[1, 2, 3, 0])
    with pytest.raises(ValueError):
        bayer.wb_prescale(x, 1, 1, 1, 1, safe=True, saturation=-1.0)
    with pytest.raises(ValueError):
        bayer.wb_postscale(np.ones((4, 4, 3)), 1, 1, 1, safe=True)
    with pytest.raises(ValueError):
        bayer.wb_postscale(np.ones((4, 4, 3)), 1, 1, 1, safe=True, saturation=[1, 2, 3, 4])
    with pytest.raises(ValueError):
        bayer.wb_postscale(np.ones((4, 4, 3)), 1, 1, 1, safe=True, saturation=[1, 0, 3])
    for call in (lambda: bayer.wb_prescale(x, 1, 1, 1, 1, cfa='grbg'), lambda: bayer.composite_bayer(x, x, x, x, cfa='grbg'),
                 lambda: bayer.decomposite_bayer(x, cfa='gbrg'), lambda: bayer.recomposite_bayer(x, x, x, x, cfa='xxxx'),
                 lambda: bayer.demosaic_deinterlace(x, cfa='grbg'), lambda: bayer.demosaic_malvar(x, cfa='grbg')):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert e.value is bayer.ErrBadCFA
    with pytest.raises(NotImplementedError):
        bayer.assemble_superresolved(x, x, x, x, 3, cfa='bggr')
    assert isinstance(bayer.ErrBadCFA, NotImplementedError)
    assert bayer.top_left == (slice(0, None, 2), slice(0, None, 2)) and bayer.bottom_right == (slice(1, None, 2), slice(1, None, 2))
    assert bayer.top_right == (slice(0, None, 2), slice(1, None, 2)) and bayer.bottom_left == (slice(1, None, 2), slice(0, None, 2))
    assert bayer.kernel_R_at_B_in_BB[2][2] == 6 and bayer.kernel_G_at_R_or_B[2][2] == 4
    assert bayer.kernel_R_at_G_in_RB[0][2] == .5 and bayer.kernel_R_at_G_in_BR[2][0] == .5


def test_the_model_imports_neither_oracle_nor_reference():
    src = open(os.path.join(ROOT, 'prysm_amd', 'bayer_plan.py')).read()
    assert not re.search(r'^\s*(from|import)\s+(oracle|prysm)\b', src, flags=re.M)


def test_symbols_are_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'prysm_amd.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert hasattr(lib, s) and s in L.SIGNATURES
        assert getattr(lib, s).argtypes == L.SIGNATURES[s][1]
    assert lib.pm_version() == 107
    assert lib.pm_bayer_class_max_workspace() > 0


def test_argument_errors_before_any_device_work(lib):
    from prysm_amd import _lib as L
    p = ctypes.c_void_p(16)
    four = (ctypes.c_double * 4)(1, 1, 1, 1)
    ws = lib.pm_bayer_class_max_workspace()

    def planes(rs):
        return [p, rs, 1, 0] * 4

    def demosaic(idt=L.PM_F32, odt=L.PM_F32, cfa=0, m=8, n=8, ld=8):
        return lib.pm_bayer_demosaic(idt, odt, cfa, 0, 1, m, n, p, ld, m * ld, p, None)

    def weave(dt=L.PM_F32, mode=1, cfa=0, m=8, n=8, ld=8):
        return lib.pm_bayer_weave(dt, mode, cfa, 1, m, n, *planes(4), p, ld, m * ld, None)

    def deinterlace(dt=L.PM_F32, cfa=0, m=8, n=8, ld=8):
        return lib.pm_bayer_deinterlace(dt, cfa, 1, m, n, p, ld, m * ld, p, None)

    def class_max(dt=L.PM_F32, classes=0, m=8, n=8, ld=8, wsb=ws):
        return lib.pm_bayer_class_max(dt, classes, 1, m, n, p, ld, m * ld, p, p, wsb, None)

    def scale(dt=L.PM_F32, classes=0, cfa=0, m=8, n=8, ld=8, safe=0, sat=four):
        return lib.pm_bayer_scale(dt, classes, cfa, 1, m, n, p, ld, m * ld, four, safe, sat, p, None)

    def refused(rc, word):
        assert rc == L.PM_ERR_ARG and word in lib.pm_last_error(), (rc, lib.pm_last_error())
        with pytest.raises(ValueError):
            L.check(rc)

    for fn in (demosaic, weave, deinterlace, class_max, scale):
        name = ('pm_bayer_' + fn.__name__).encode()
        refused(fn(ld=7), b'row stride')
        refused(fn(m=0), b'at least 1')
        assert name in lib.pm_last_error()
    for fn in (demosaic, weave, deinterlace, scale):
        refused(fn(cfa=2), b'cfa')
    refused(demosaic(odt=L.PM_C64), b'dtype')
    refused(demosaic(idt=L.PM_F64, odt=L.PM_F32), b'dtype')
    refused(demosaic(idt=L.PM_BOOL), b'dtype')
    for fn in (weave, deinterlace, class_max, scale):
        refused(fn(dt=L.PM_C64), b'dtype')
        refused(fn(dt=L.PM_U16), b'dtype')
    refused(weave(m=7), b'even')
    refused(weave(mode=2), b'mode')
    refused(deinterlace(n=6, ld=5), b'row stride')
    refused(deinterlace(m=7), b'even')
    refused(class_max(classes=2), b'classes')
    refused(class_max(classes=1, ld=23), b'row stride')          # an RGB row holds 3 n values
    assert class_max(wsb=16) == L.PM_ERR_WORKSPACE
    refused(scale(classes=5), b'classes')
    refused(scale(safe=1, sat=(ctypes.c_double * 4)(1, 0, 1, 1)), b'saturation')
    refused(scale(safe=1, sat=None), b'safe')
    assert lib.pm_bayer_assemble(L.PM_C128, 1, 4, 4, *planes(4), p, None) == L.PM_ERR_ARG and b'dtype' in lib.pm_last_error()
    assert lib.pm_bayer_assemble(L.PM_F64, 1, 0, 4, *planes(4), p, None) == L.PM_ERR_ARG
