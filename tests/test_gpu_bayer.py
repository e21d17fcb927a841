"""GPU: the Bayer kernels (csrc/bayer.hip) against their numpy model (prysm_amd/bayer_plan.py) and the reference's results
(tests/golden/bayer.npz).  Every shape is the fixture's.  No test provokes a fault: bad values are data, never addresses."""
import json

import numpy as np
import pytest
import torch

from conftest import rel_max
from prysm_amd import bayer_plan as BP

pytestmark = pytest.mark.gpu

CFAS = ('rggb', 'bggr')
NAMES = ('r', 'g1', 'g2', 'b')


@pytest.fixture(scope='module')
def g(golden):
    return golden('bayer')


@pytest.fixture(scope='module')
def bayer(pa):
    from prysm_amd import bayer
    return bayer


def tonp(t):
    return t.cpu().numpy()


def same(a, b):
    a, b = tonp(a), tonp(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def demosaic_bound(img, dtype):
    """32 eps max|img|: at most 11 products per sum, sum |w| <= 2.5, and a summation order (and, in float32, a precision of the
    running sum) that differs from scipy's"""
    return 32 * np.finfo(dtype).eps * float(np.max(np.abs(img)))


def ulps(got, want):
    return np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64))


def test_demosaic_equals_the_model_and_the_reference(bayer, g):
    for c in json.loads(str(g['demosaic'])):
        img = g[c['key'] + '_in']
        for cfa in CFAS:
            got = tonp(bayer.demosaic_malvar(img, cfa))
            want = g[f"{c['key']}_{cfa}"]
            assert got.dtype == want.dtype == img.dtype and got.shape == want.shape, (c['key'], cfa)
            assert np.array_equal(got, BP.demosaic_malvar(img, cfa)), (c['key'], cfa)
            err = np.abs(got.astype(np.float64) - want).max()
            assert err <= demosaic_bound(img, img.dtype), (c['key'], cfa, err)


def test_demosaic_of_detector_dn(bayer, g):
    from prysm_amd.conf import config
    dn = g['dem_u16_in']
    for cfa in CFAS:
        got = bayer.demosaic_malvar(dev(dn), cfa)
        assert got.dtype == torch.float64 and np.array_equal(tonp(got), g[f'dem_u16_{cfa}'])
        for idt in (np.uint8, np.uint32):
            x = (dn >> 4).astype(idt)
            assert np.array_equal(tonp(bayer.demosaic_malvar(x, cfa)), BP.demosaic_malvar(x, cfa))
    config.precision = 32
    try:
        got = bayer.demosaic_malvar(dn, 'rggb')
    finally:
        config.precision = 64
    assert got.dtype == torch.float32 and np.array_equal(tonp(got), BP.demosaic_malvar(dn, 'rggb', precision=np.float32))


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_demosaic_stack_layout_and_strides(bayer, g, dtype):
    img = g[f'dem_37x70_{dtype}_in']
    stack = np.stack([img, -0.5 * img, img[::-1].copy()])
    for cfa in CFAS:
        st = bayer.demosaic_malvar(stack, cfa)
        assert st.shape == (3, 37, 70, 3)
        for b in range(3):
            assert same(st[b], bayer.demosaic_malvar(stack[b], cfa))
        chw = bayer.demosaic_malvar(stack, cfa, layout='chw')
        assert chw.shape == (3, 3, 37, 70) and same(chw, st.permute(0, 3, 1, 2).contiguous())
        assert same(bayer.demosaic_malvar(img, cfa, layout='chw'), st[0].permute(2, 0, 1).contiguous())
        # a column slice of a wider tensor (and of a wider stack): the rows are strided
        wide = torch.zeros((3, 40, 81), dtype=st.dtype, device='cuda')
        view = wide[:, 2:39, 5:75]
        view.copy_(dev(stack))
        assert not view.is_contiguous() and same(bayer.demosaic_malvar(view, cfa), st)
        assert same(bayer.demosaic_malvar(view[1], cfa), st[1])


def test_native_sites_are_copies(bayer, g):
    for key in ('dem_37x70_float32_in', 'dem_5x8_float64_in'):
        img = g[key]
        for cfa in CFAS:
            out = tonp(bayer.demosaic_malvar(img, cfa))
            r, b = (0, 2) if cfa == 'rggb' else (2, 0)
            assert np.array_equal(out[0::2, 0::2, r], img[0::2, 0::2]) and np.array_equal(out[1::2, 1::2, b], img[1::2, 1::2])
            assert np.array_equal(out[0::2, 1::2, 1], img[0::2, 1::2]) and np.array_equal(out[1::2, 0::2, 1], img[1::2, 0::2])


def test_plane_functions_against_the_fixture(bayer, g):
    for m, n in ((6, 8), (24, 32)):
        planes = [g[f'pl_{m}x{n}_{k}'] for k in NAMES]
        mos = g[f'mos_{m}x{n}']
        for cfa in CFAS:
            assert np.array_equal(tonp(bayer.composite_bayer(*planes, cfa=cfa)), g[f'comp_{m}x{n}_{cfa}'])
            x = dev(mos)
            dec = bayer.decomposite_bayer(x, cfa)
            assert all(p.data_ptr() >= x.data_ptr() and p._base is not None and p.stride() == (2 * n, 2) for p in dec)
            assert np.array_equal(np.stack([tonp(p) for p in dec]), g[f'dec_{m}x{n}_{cfa}'])
            rec = bayer.recomposite_bayer(*dec, cfa=cfa)          # the views straight through
            assert same(rec, x) and np.array_equal(tonp(rec), g[f'recomp_{m}x{n}_{cfa}'])
            assert np.array_equal(tonp(bayer.demosaic_deinterlace(mos, cfa)), g[f'deint_{m}x{n}_{cfa}'])
            x32 = dev(mos.astype(np.float32))
            assert same(bayer.recomposite_bayer(*bayer.decomposite_bayer(x32, cfa), cfa=cfa), x32)
            assert np.array_equal(tonp(bayer.demosaic_deinterlace(x32, cfa)), BP.deinterlace(mos.astype(np.float32), cfa))
            outbuf = torch.zeros((m, n), dtype=torch.float64, device='cuda')
            assert bayer.composite_bayer(*planes, cfa=cfa, output=outbuf) is outbuf and np.array_equal(tonp(outbuf), g[f'comp_{m}x{n}_{cfa}'])
        # stacks in one launch
        st = np.stack([mos, 2 * mos])
        assert np.array_equal(tonp(bayer.demosaic_deinterlace(st)), np.stack([BP.deinterlace(s) for s in st]))
        assert same(bayer.recomposite_bayer(*bayer.decomposite_bayer(dev(st))), dev(st))
    with pytest.raises(ValueError):
        bayer.demosaic_deinterlace(np.ones((5, 6)))


def test_white_balance_against_the_fixture(bayer, g):
    for c in json.loads(str(g['wb'])):
        for dt, suffix in ((np.float64, '_out'), (np.float32, '_out32')):
            src = g['wb_mosaic' if c['kind'] == 'pre' else 'wb_rgb'].astype(dt)
            x = dev(src)
            if c['kind'] == 'pre':
                got = bayer.wb_prescale(x, *c['gains'], cfa=c['cfa'], safe=c['safe'], saturation=c['saturation'])
                model = BP.wb_prescale(src, *c['gains'], cfa=c['cfa'], safe=c['safe'], saturation=c['saturation'])
                again = bayer.wb_prescale(src, *c['gains'], cfa=c['cfa'], safe=c['safe'], saturation=c['saturation'])
            else:
                got = bayer.wb_postscale(x, *c['gains'], safe=c['safe'], saturation=c['saturation'])
                model = BP.wb_postscale(src, *c['gains'], safe=c['safe'], saturation=c['saturation'])
                again = bayer.wb_postscale(src, *c['gains'], safe=c['safe'], saturation=c['saturation'])
            assert got is x and got.data_ptr() == x.data_ptr()          # in place: the argument comes back
            want = g[f"wb_{c['name']}{suffix}"]
            u = ulps(tonp(got), want)
            print(c['name'], np.dtype(dt).name, 'ulp', u, 'equals the model:', np.array_equal(tonp(got), model))
            assert tonp(got).dtype == want.dtype and u <= 2, (c['name'], dt, u)
            assert same(again, got)                                     # a numpy argument: a scaled device copy


def test_white_balance_of_views_and_stacks(bayer, g):
    src = g['wb_mosaic']
    wide = torch.zeros((26, 40), dtype=torch.float64, device='cuda')
    view = wide[1:25, 3:35]
    view.copy_(dev(src))
    out = bayer.wb_prescale(view, 1.9, 1.0, 1.02, 1.6, safe=True, saturation=1200.0)
    assert out.data_ptr() == view.data_ptr() and np.array_equal(tonp(view), BP.wb_prescale(src, 1.9, 1.0, 1.02, 1.6, safe=True, saturation=1200.0))
    assert float(wide[0].abs().max()) == 0 and float(wide[:, :3].abs().max()) == 0 and float(wide[:, 35:].abs().max()) == 0
    st = np.stack([src, 0.5 * src])
    got = bayer.wb_prescale(dev(st), 1.9, 1.0, 1.02, 1.6, cfa='bggr', safe=True, saturation=1200.0)
    # the maxima of a stack are taken over all its members: the first member holds them here
    ratio = BP.safe_gains([p.max() for p in BP.decomposite(src, 'bggr')], (1.9, 1.0, 1.02, 1.6), [1200.0] * 4, np.float64)[1]
    assert ratio > 1
    want = np.stack([BP.wb_prescale(s, 1.9 / ratio, 1.0 / ratio, 1.02 / ratio, 1.6 / ratio, cfa='bggr') for s in st])
    assert np.array_equal(tonp(got), want)


def _class_maxima(bayer, t):
    """pm_bayer_class_max of one contiguous mosaic, called as bayer._scale calls it; class 2 * (r & 1) + (c & 1)"""
    from prysm_amd import _lib as L
    lib = L.load()
    v, ld, bs = bayer._mosaic_view(t, 'mosaic')
    B, m, n = v.shape
    maxima = torch.empty(4, dtype=torch.float64, device=t.device)
    ws = L.workspace(int(lib.pm_bayer_class_max_workspace()))
    L.check(lib.pm_bayer_class_max(bayer._code(t.dtype), L.PM_BAYER_MOSAIC, B, m, n, L.ptr(v), ld, bs, L.ptr(maxima), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return tonp(maxima)


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_class_maxima_where_the_second_stage_loops_and_ends_ragged(bayer, dtype):
    """362 x 130: the first stage runs 3 x 91 workgroups (64 columns by 4 rows each, at most kMaxPartials = 4096 of them), so the
    second stage folds 273 partials: more than its 256 threads and no multiple of them.  The last workgroup, and the last partial,
    holds rows 360, 361 of columns 128, 129: one sample of each class.  The maxima are put there, so a second stage that stops at
    256 partials or drops the ragged end misses all four.  Comparisons only: the result equals numpy's, NaN included."""
    m, n = 362, 130
    assert ((n + 63) // 64, min((m + 3) // 4, 4096 // ((n + 63) // 64))) == (3, 91)
    src = np.random.default_rng(273).random((m, n)).astype(dtype)
    src[360:, 128:] = np.array([[2.5, 3.5], [4.5, 5.5]], dtype=dtype)
    want = np.array([src[i::2, j::2].max() for i in (0, 1) for j in (0, 1)], dtype=np.float64)
    assert list(want) == [2.5, 3.5, 4.5, 5.5]
    got = _class_maxima(bayer, dev(src))
    print(dtype, 'maxima', got)
    assert np.array_equal(got, want)
    # a NaN in one class, seen by the last workgroup only: that class is NaN (numpy's max), the other three are unchanged
    src[361, 128] = np.nan
    want_nan = np.array([src[i::2, j::2].max() for i in (0, 1) for j in (0, 1)], dtype=np.float64)
    assert np.isnan(want_nan[2]) and np.array_equal(np.delete(want_nan, 2), np.delete(want, 2))
    got = _class_maxima(bayer, dev(src))
    print(dtype, 'maxima with a NaN', got)
    assert np.array_equal(got, want_nan, equal_nan=True)


def test_assemble_superresolved_against_the_fixture(bayer, g):
    """rel_max against the reference.  Observed for the reference-vs-model pair (the same transforms in numpy with the separable
    multiplier): 5.7e-16 and 5.1e-16 in float64; the same cases computed in float32: 1.7e-7 and 1.5e-7, the floor of that precision.
    The tolerance is 8 times the larger observed value of each precision."""
    for c in json.loads(str(g['superres'])):
        m, n = c['shape']
        planes = [g[f'sr_{m}x{n}_{k}'] for k in NAMES]
        want = g[f"sr_{m}x{n}_z{c['zoomfactor']}"]
        got = bayer.assemble_superresolved(*planes, c['zoomfactor'])
        e64 = rel_max(tonp(got), want)
        got32 = bayer.assemble_superresolved(*[p.astype(np.float32) for p in planes], c['zoomfactor'])
        e32 = rel_max(tonp(got32).astype(np.float64), want)
        print(c, 'rel_max float64', e64, 'float32', e32)
        assert got.shape == (m, n, 3) and got.dtype == torch.float64 and got32.dtype == torch.float32
        assert e64 <= 8 * 5.7e-16      # observed reference-vs-model 5.7e-16
        assert e32 <= 8 * 1.7e-7       # observed reference-vs-model in float32 1.7e-7
    with pytest.raises(NotImplementedError):
        bayer.assemble_superresolved(*planes, 3, cfa='bggr')


def test_graph_of_safe_prescale_and_demosaic(bayer, g):
    """wb_prescale(safe=True) keeps the maxima and the ratio on the device, so the pair is capturable; replayed on new data it equals
    the eager pair"""
    from prysm_amd import graph
    src = g['dem_24x32_float32_in']

    def fn(x):
        return bayer.demosaic_malvar(bayer.wb_prescale(x, 1.9, 1.0, 1.02, 1.6, safe=True, saturation=150.0))
    model = graph.capture(fn, dev(src))
    for k in (1.0, 0.125, 3.0):
        new = (src * k + 1).astype(np.float32)
        replay = model(dev(new)).clone()
        assert same(replay, fn(dev(new)))
        assert np.array_equal(tonp(replay), BP.demosaic_malvar(BP.wb_prescale(new, 1.9, 1.0, 1.02, 1.6, safe=True, saturation=150.0)))
    ratios = [BP.safe_gains([p.max() for p in BP.decomposite((src * k + 1).astype(np.float32))], (1.9, 1.0, 1.02, 1.6), [150.0] * 4, np.float32)[1]
              for k in (0.125, 3.0)]
    assert ratios[0] == 1 and ratios[1] > 1          # the replays cover both regimes
