"""CPU: the deformable-mirror entry points (pm_lattice, pm_warp) and the host logic of prysm_amd.x.dm without a GPU --
declared / exported / bound symbols, argument errors, lattice geometry and homographies against the reference fixture, and a numpy
model of the kernels' formulation (separable FIR prefilter + 4 x 4 taps, constant mode) against scipy and the fixture."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
from scipy import ndimage

from conftest import GOLDEN

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

Z = math.sqrt(3) - 2


def _mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i > n - 1, p - i, i)


def _fir(a, axis, K):
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k in range(-K, K + 1):
        out += math.sqrt(3) * Z ** abs(k) * np.take(a, _mirror(np.arange(n) + k, n), axis=axis)
    return out


def _weights(t):
    u = 1 - t
    return [u ** 3 / 6, 2 / 3 - t * t + t ** 3 / 2, 2 / 3 - u * u + u ** 3 / 2, t ** 3 / 6]


def model_sample(img, yy, xx, K=30):
    """pm_warp's arithmetic: FIR prefilter (2K + 1 taps, mirror), 4 x 4 taps with mirrored indices, exact 0 outside [0, n - 1]."""
    c = _fir(_fir(img, 0, K), 1, K)
    m, n = img.shape
    inside = (yy >= 0) & (yy <= m - 1) & (xx >= 0) & (xx <= n - 1)
    fy, fx = np.floor(yy), np.floor(xx)
    wy, wx = _weights(yy - fy), _weights(xx - fx)
    out = np.zeros(yy.shape)
    for a in range(4):
        iy = _mirror(fy.astype(int) - 1 + a, m)
        for b in range(4):
            ix = _mirror(fx.astype(int) - 1 + b, n)
            out += wy[a] * wx[b] * c[iy, ix]
    return np.where(inside, out, 0.0)


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
