"""CPU: the deformable-mirror entry points (pm_lattice, pm_warp) and the host logic of prysm_amd.x.dm without a GPU --
declared / exported / bound symbols, argument errors, lattice geometry and homographies against the reference fixture, and a numpy
model of the kernels' formulation (separable FIR prefilter + 4 x 4 taps, constant mode) against scipy and the fixture."""
import ctypes
import json
import os

import numpy as np
import pytest
from scipy import ndimage

from conftest import GOLDEN
import dm_common as DC
from dm_common import model_sample

SYMS = ('pm_lattice', 'pm_warp', 'pm_warp_workspace')


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope='module')
def fx():
    d = np.load(os.path.join(GOLDEN, 'dm.npz'))
    return d, json.loads(bytes(d['meta']).decode())


def test_symbols_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'prysm_amd.h')).read()
    for s in SYMS:
        assert s + '(' in hdr
        assert hasattr(lib, s)
        assert s in L.SIGNATURES


def _lattice(lib, **kw):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, op=L.PM_LATTICE_SCATTER, batch=1, rows=64, cols=64, ny=8, nx=8, y0=4, x0=4, sy=6, sx=6, scale=1.0,
             inp=ctypes.c_void_p(256), in_ld=8, in_bs=64, out=ctypes.c_void_p(256), out_ld=64, out_bs=4096)
    a.update(kw)
    return lib.pm_lattice(a['dtype'], a['op'], a['batch'], a['rows'], a['cols'], a['ny'], a['nx'], a['y0'], a['x0'], a['sy'], a['sx'],
                          a['scale'], a['inp'], a['in_ld'], a['in_bs'], a['out'], a['out_ld'], a['out_bs'], None)


def _warp(lib, **kw):
    from prysm_amd import _lib as L
    a = dict(dtype=L.PM_F64, order=3, batch=1, rows=32, cols=32, inp=ctypes.c_void_p(256), in_ld=32, in_bs=1024, orows=32, ocols=32,
             oy=0, ox=0, out=ctypes.c_void_p(256), out_ld=32, out_bs=1024, ws=ctypes.c_void_p(256), wsb=1 << 20)
    a.update(kw)
    H = (L.c_f64 * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    return lib.pm_warp(a['dtype'], a['order'], a['batch'], a['rows'], a['cols'], a['inp'], a['in_ld'], a['in_bs'], H, 1.0, a['orows'],
                       a['ocols'], a['oy'], a['ox'], a['out'], a['out_ld'], a['out_bs'], a['ws'], a['wsb'], None)


@pytest.mark.parametrize('kw, code, word', [
    (dict(dtype=7), -1, b'dtype'),
    (dict(dtype=0), -1, b'dtype'),                       # SCATTER writes a real grid
    (dict(op=5), -1, b'op'),
    (dict(y0=23), -1, b'does not fit'),                  # 23 + 7 * 6 = 65 > 63
    (dict(x0=-1), -1, b'does not fit'),
    (dict(sy=0), -1, b'separation'),
    (dict(out_ld=32), -1, b'overlap'),
    (dict(batch=2, out_bs=64 * 63), -1, b'overlap'),
])
def test_lattice_argument_errors(lib, kw, code, word):
    # every call here fails validation before anything is launched (the pointers are not real)
    rc = _lattice(lib, **kw)
    assert rc == code
    assert word in lib.pm_last_error()


def test_lattice_gather_reads_complex(lib):
    from prysm_amd import _lib as L
    # GATHER accepts the real part of a complex field; bad pointers / overlap are still argument errors
    assert _lattice(lib, op=L.PM_LATTICE_GATHER, dtype=L.PM_C128, in_ld=64, out_ld=4) == L.PM_ERR_ARG
    assert b'overlap' in lib.pm_last_error()


@pytest.mark.parametrize('kw, code, word', [
    (dict(dtype=9), -1, b'dtype'),
    (dict(order=1), -2, b'order'),
    (dict(order=5), -2, b'order'),
    (dict(in_ld=16), -1, b'in_ld'),
    (dict(out_ld=16), -1, b'overlap'),
    (dict(batch=2, out_bs=100), -1, b'overlap'),
    (dict(wsb=16), -3, b'workspace'),
])
def test_warp_argument_errors(lib, kw, code, word):
    assert _warp(lib, **kw) == code
    assert word in lib.pm_last_error()


def test_warp_workspace(lib):
    from prysm_amd import _lib as L
    assert lib.pm_warp_workspace(L.PM_F64, 3, 100, 120) == 3 * 100 * 120 * 8
    assert lib.pm_warp_workspace(L.PM_C64, 2, 64, 64) == 2 * 64 * 64 * 4
    assert lib.pm_warp_workspace(11, 1, 8, 8) == 0


# ----------------------------------------------------------------------------- geometry

def test_lattice_geometry_matches_fixture(fx):
    from prysm_amd.x.dm import prepare_actuator_lattice
    _, meta = fx
    for name, m in meta.items():
        Nact, sep = m['Nact'], m['sep']
        Nact = (Nact, Nact) if isinstance(Nact, int) else tuple(Nact)
        sep = (sep, sep) if isinstance(sep, int) else tuple(sep)
        assert list(prepare_actuator_lattice(tuple(m['shape']), Nact, sep)) == m['lattice'], name


def test_homographies_match_fixture(fx):
    from prysm_amd.x.dm import projection_homographies, apply_homography, make_rotation_matrix
    d, meta = fx
    for name, m in meta.items():
        rot = m.get('rot', (0, 0, 0))
        assert float(make_rotation_matrix(rot)[2, 2]) == m['obliquity'], name
        if f'{name}_projx' not in d:
            continue
        Mfwd, Mifwd = projection_homographies(tuple(m['shape']), rot)
        ps = m['proj_step']         # the fixture holds every ps-th row and column
        x, y = np.meshgrid(*[np.arange(0, n, ps, dtype=np.float64) for n in reversed(m['shape'])])
        px, py = apply_homography(Mifwd, x, y)
        ix, iy = apply_homography(Mfwd, x, y)
        for got, key in ((px, 'projx'), (py, 'projy'), (ix, 'invprojx'), (iy, 'invprojy')):
            ref = d[f'{name}_{key}']
            assert np.max(np.abs(got.astype(np.float32) - ref)) <= 1e-4, (name, key)


# ----------------------------------------------------------------------------- the kernels' formulation in numpy

@pytest.mark.parametrize('shape', [(5, 7), (1, 6), (2, 3), (40, 33)])
def test_model_matches_map_coordinates(shape):
    rng = np.random.default_rng(sum(shape))
    m, n = shape
    img = rng.standard_normal(shape)
    yy = rng.uniform(-1.5, m + 0.5, 3000)
    xx = rng.uniform(-1.5, n + 0.5, 3000)
    edge_y = np.array([0, -1e-12, m - 1, m - 1 + 1e-12, 0.5 * (m - 1), m - 1, 0, 0, -1e-300])
    edge_x = np.array([0, 0.25 * (n - 1), n - 1, 0.5 * (n - 1), -1e-12, n - 1 + 1e-12, n - 1 - 1e-12, 1e-12, 0])
    yy, xx = np.r_[yy, edge_y], np.r_[xx, edge_x]
    ref = ndimage.map_coordinates(img, (yy, xx), order=3, mode='constant', cval=0)
    got = model_sample(img, yy, xx)
    assert np.max(np.abs(got - ref)) <= 1e-14 * np.max(np.abs(ref))
    assert np.all(got[ref == 0] == 0)
    # the fp32 tap count (K = 14) is good to ~1e-8
    assert np.max(np.abs(model_sample(img, yy, xx, K=14) - ref)) <= 3e-8 * np.max(np.abs(ref))


def _model_render(d, m, name, wfe=True):
    """DM.render as the device runs it: scatter, real part of ifft2(fft2(poke) * tf), warp through Mifwd, window."""
    from prysm_amd.x.dm import prepare_actuator_lattice, projection_homographies, apply_homography, _window, _pair
    ifn = d[f"ifn_{m['ifn']}"].astype(m['dtype']).astype(np.float64)
    acts = d[f'{name}_acts'].astype(np.float64)
    s = ifn.shape
    y0, x0, sy, sx, ny, nx = prepare_actuator_lattice(s, _pair(m['Nact']), _pair(m['sep']))
    poke = np.zeros(s)
    poke[y0:y0 + ny * sy:sy, x0:x0 + nx * sx:sx] = acts
    tf = np.fft.fft2(ifn)
    sh = m.get('shift', (0, 0))
    tf = tf * np.exp(np.fft.fftfreq(s[1]) * (-2j * np.pi * sh[0]))[None, :] * np.exp(np.fft.fftfreq(s[0]) * (-2j * np.pi * sh[1]))[:, None]
    sfe = np.fft.ifft2(np.fft.fft2(poke) * tf).real
    scale = 2 * m['obliquity'] if wfe else 1.0
    win = _window(s, _pair(m['Nout']))
    (orows, ocols), (oy, ox) = win if win is not None else (s, (0, 0))
    R, C = np.meshgrid(np.arange(orows) + oy, np.arange(ocols) + ox, indexing='ij')
    dom = (R >= 0) & (R < s[0]) & (C >= 0) & (C < s[1])
    rot = m.get('rot', (0, 0, 0))
    if np.allclose(rot, 0):
        out = np.zeros((orows, ocols))
        out[dom] = scale * sfe[R[dom], C[dom]]
        return out, np.ones((orows, ocols), bool)
    _, Mifwd = projection_homographies(s, rot)
    xx, yy = apply_homography(Mifwd, C.astype(float), R.astype(float))
    out = np.where(dom, scale * model_sample(sfe, np.where(dom, yy, -1), np.where(dom, xx, -1)), 0.0)
    edge = np.zeros_like(dom)
    for v, n in ((xx, s[1]), (yy, s[0])):
        edge |= (np.abs(v) < 1e-9) | (np.abs(v - (n - 1)) < 1e-9)
    return out, ~(edge & dom)


@pytest.mark.parametrize('name', ['plain', 'shift', 'clock', 'tilt', 'rot3', 'small', 'large', 'odd'])
def test_model_render_matches_fixture(fx, name):
    d, meta = fx
    m = meta[name]
    got, keep = _model_render(d, m, name)
    st = m['render_step']           # the fixture holds every st-th row and column
    got, keep = got[::st, ::st], keep[::st, ::st]
    ref = d[f'{name}_wfe']
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)[keep]) <= 1e-12 * np.max(np.abs(ref))


# ----------------------------------------------------------------------------- the references of tests/test_gpu_dm_kernels.py

WARP_CASES = DC.warp_cases()


def _case_id(c):
    (m, n), name, (om, on), off = c
    return f'{m}x{n} {name} {om}x{on}@{off[0]},{off[1]}'


@pytest.mark.parametrize('case', WARP_CASES, ids=_case_id)
def test_warp_reference_is_model_through_window(case):
    """the scipy reference of the entry point against the kernels' arithmetic composed with the window rule, to 1e-14 of
    max|img| |scale| (the scale of the GPU bounds), on white noise, at every case of the GPU file; an exact zero of one is one of the other"""
    shape, name, out_shape, off = case
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.standard_normal(shape)
    H = DC.homography(name, shape)
    ref = DC.warp_reference(img, H, out_shape, off, -0.5)
    got = DC.model_warp(img, H, out_shape, off, -0.5)
    assert ref.shape == got.shape == tuple(out_shape)
    assert np.max(np.abs(got - ref), initial=0) <= 1e-14 * 0.5 * np.max(np.abs(img))
    assert np.array_equal(got == 0, ref == 0)
    # outside the rows x cols grid the window rule gives 0 whatever the homography
    R, C, _, _ = DC.pull_coordinates(H, out_shape, off)
    assert not ref[(R < 0) | (R >= shape[0]) | (C < 0) | (C >= shape[1])].any()


@pytest.mark.parametrize('case', WARP_CASES, ids=_case_id)
def test_near_cutoff_share(case):
    shape, name, out_shape, off = case
    exact, make = DC.HOMOGRAPHIES[name]
    H = make(shape)
    out = DC.left_out(shape, name, out_shape, off)
    assert out.shape == tuple(out_shape)
    if not exact:
        assert np.array_equal(out, DC.near_cutoff(shape, H, out_shape, off))
        assert out.sum() <= 1e-3 * out.size
        return
    # an exact homography leaves nothing out, because float64 holds every coordinate it gives: H is affine with entries that are
    # multiples of 2^-40, so 2^40 (x, y) is an integer that int64 arithmetic gives without rounding
    assert not out.any()
    assert np.array_equal(H[2], [0, 0, 1])
    Hi = np.rint(H * 2.0 ** 40).astype(np.int64)
    assert np.array_equal(Hi.astype(np.float64) * 2.0 ** -40, H)
    R, C, xx, yy = DC.pull_coordinates(H, out_shape, off)
    for v, row in ((xx, Hi[0]), (yy, Hi[1])):
        want = row[0] * C + row[1] * R + row[2]
        scaled = v * 2.0 ** 40
        assert np.array_equal(scaled, np.floor(scaled)) and np.array_equal(scaled.astype(np.int64), want)


def test_exact_homographies_reach_the_cutoff():
    """what the cutoff cases of the GPU file rely on: a translation by 2^-40 puts exactly one column or row outside, and the identity none"""
    for shape in DC.CUTOFF_SHAPES:
        m, n = shape
        for name, lost in (('identity', 0), ('x-2^-40', m), ('x+2^-40', m), ('y-2^-40', n), ('y+2^-40', n)):
            _, _, xx, yy = DC.pull_coordinates(DC.homography(name, shape), shape, (0, 0))
            outside = (xx < 0) | (xx > n - 1) | (yy < 0) | (yy > m - 1)
            assert outside.sum() == lost, (shape, name)


def test_lattice_reference_against_loops():
    from prysm_amd import _lib as L
    rng = np.random.default_rng(4)
    for rows, cols, ny, nx, y0, x0, sy, sx in ((7, 9, 2, 3, 1, 2, 4, 3), (4, 4, 2, 2, 0, 1, 3, 2)):
        a = rng.integers(-9, 10, (2, ny, nx)).astype(np.float64)
        want = np.zeros((2, rows, cols))
        for b in range(2):
            for i in range(ny):
                for j in range(nx):
                    want[b, y0 + i * sy, x0 + j * sx] = -2 * a[b, i, j]
        got = DC.lattice_reference(L.PM_LATTICE_SCATTER, a, rows, cols, ny, nx, y0, x0, sy, sx, -2)
        assert np.array_equal(got, want)
        f = rng.integers(-9, 10, (2, rows, cols)).astype(np.float64)
        want = np.empty((2, ny, nx))
        for b in range(2):
            for i in range(ny):
                for j in range(nx):
                    want[b, i, j] = 0.5 * f[b, y0 + i * sy, x0 + j * sx]
        assert np.array_equal(DC.lattice_reference(L.PM_LATTICE_GATHER, f, rows, cols, ny, nx, y0, x0, sy, sx, 0.5), want)


def test_lattice_geometries_fit():
    for name, (rows, cols, ny, nx, y0, x0, sy, sx, _) in DC.LATTICES.items():
        assert 0 <= y0 and y0 + (ny - 1) * sy < rows and 0 <= x0 and x0 + (nx - 1) * sx < cols, name
