"""GPU: the deformable-mirror kernels (csrc/dm.hip) at the C ABI -- pm_warp against scipy.ndimage.map_coordinates and pm_lattice
against numpy slicing, at the smallest shapes where the kernels can go wrong.  References, homographies, cases, bounds, NaN frames and
the two call helpers are tests/dm_common.py's; tests/test_dm_host.py pins the references on the CPU at every case used here.

pm_warp, on white noise, float64 and float32 in every case: axes shorter than the prefilter's K (the mirror wraps several periods,
n = 1 and n = 2 included), one tile and one element past it, ragged tiles, the constant-mode cutoff to the bit (identity and
translations by 2^-40), crop / pad / corner / empty output windows with scale -0.5, pitched inputs and outputs inside NaN frames, the
real part of a complex field whose imaginary parts are NaN, stacks (distinct, shared, and 65535 + 3 members: the second trip of the
blockIdx.z loop) and grids of 4 x 65535 + 5 and 16 x 65535 + 5 rows (the second trip down the rows of the sample kernel and of the
prefilter).  pm_lattice, on integers with np.array_equal: scatter as the memset of its grid, gather from real and complex fields,
scatter-then-gather, the same stacks and tall grids.

Largest |got - ref| / bound of pm_warp over all cases as printed on an MI355X (the bound is 1; it is derived in tests/dm_common.py):
  float64   2.7e-2   |got - ref| = 1.0e-13 at (130, 70) under the perspective map (bound 1e-12 max|img|)
  float32   1.2e-2   |got - ref| = 1.9e-6 at (29, 61) under the identity (bound 4.3e-5 max|img|), a fortieth of the worst case and below
                     the tenth of the bound past which a cause would have to be looked for
RECORDED below holds the same figures; test_warp_recorded_figures prints those of the session.
"""
import numpy as np
import pytest
import torch

import dm_common as DC
from prysm_amd import _lib as L

pytestmark = pytest.mark.gpu

REAL = [L.PM_F64, L.PM_F32]
CX = [L.PM_C128, L.PM_C64]
SC, GA = L.PM_LATTICE_SCATTER, L.PM_LATTICE_GATHER

# largest |got - ref| / bound per dtype as measured on an MI355X; a record, not a bound
RECORDED = {'float64': 2.715e-2, 'float32': 1.240e-2}

_worst = {}


def _noise(shape, code, seed, B=None):
    """white noise rounded to the dtype's real type (the reference then reads the same numbers)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape if B is None else (B,) + tuple(shape)).astype(DC.REAL_NP[code])


def _check(what, code, got, img, name, out_shape=None, off=(0, 0), scale=1.0):
    """one member against warp_reference under the derived bound; prints the ratio, returns the reference"""
    shape = img.shape
    out_shape = shape if out_shape is None else out_shape
    ref = DC.warp_reference(img, DC.homography(name, shape), out_shape, off, scale)
    assert got.shape == ref.shape and got.dtype == DC.REAL_NP[code]
    assert np.isfinite(got).all()
    keep = ~DC.left_out(shape, name, out_shape, off)
    dev = float(np.max(np.abs(got.astype(np.float64) - ref)[keep], initial=0))
    ratio = dev / DC.warp_bound(code, img, scale)
    key = DC.NAME[DC.REAL_CODE.get(code, code)]
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f'{what} {DC.NAME[code]} {shape} {name}: max|got - ref| {dev:.3e} = {ratio:.3e} of the bound (worst so far {_worst[key]:.3e})')
    assert ratio <= 1.0
    return ref


def _bit_equal(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


# ----------------------------------------------------------------------------- pm_warp

@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
@pytest.mark.parametrize('shape', DC.SHAPES, ids=str)
def test_warp_shapes(shape, code):
    img = _noise(shape, code, shape[0] * 1000 + shape[1])
    homs = DC.SHAPE_HOMS + (DC.EXTRA_HOMS if shape in DC.EXTRA_SHAPES else [])
    for name in homs:
        got = DC.run_warp(code, img[None], DC.homography(name, shape))[0]
        ref = _check('shapes', code, got, img, name)
        assert np.array_equal(got == 0, ref == 0) or not DC.HOMOGRAPHIES[name][0]      # exact coordinates: the same pixels are outside


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
@pytest.mark.parametrize('shape', DC.CUTOFF_SHAPES, ids=str)
def test_warp_cutoff_is_exact(shape, code):
    """a coordinate exactly at 0 or n - 1 is inside, one 2^-40 outside gives exactly 0.0; on a unit axis the only coordinate inside is 0"""
    m, n = shape
    rng = np.random.default_rng(m * 100 + n)
    img = rng.uniform(1, 2, shape).astype(DC.REAL_NP[code])       # no zero by coincidence
    got = DC.run_warp(code, img[None], DC.homography('identity', shape))[0]
    _check('cutoff', code, got, img, 'identity')
    assert np.max(np.abs(got.astype(np.float64) - img)) <= DC.warp_bound(code, img, 1.0)
    assert (got != 0).all()
    lost = {'x-2^-40': np.s_[:, 0], 'x+2^-40': np.s_[:, n - 1], 'y-2^-40': np.s_[0, :], 'y+2^-40': np.s_[m - 1, :]}
    for name in DC.CUTOFF_SHIFTS:
        got = DC.run_warp(code, img[None], DC.homography(name, shape))[0]
        outside = np.zeros(shape, bool)
        outside[lost[name]] = True
        if (n == 1 and name[0] == 'x') or (m == 1 and name[0] == 'y'):
            outside[:] = True           # the unit axis: every coordinate left 0
        assert np.array_equal(got[outside], np.zeros(outside.sum(), got.dtype)), name
        assert (got[~outside] != 0).all(), name
        _check('cutoff', code, got, img, name)


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
@pytest.mark.parametrize('name', DC.WINDOW_HOMS)
@pytest.mark.parametrize('shape', DC.WINDOW_SHAPES, ids=str)
def test_warp_windows(shape, name, code):
    img = _noise(shape, code, shape[0] + 7)
    H = DC.homography(name, shape)
    for wname, (oshape, off) in DC.windows(shape).items():
        got = DC.run_warp(code, img[None], H, oshape, off, scale=-0.5, out_pad=2)[0]
        assert got.shape == tuple(oshape)
        if wname == 'empty':
            continue                    # run_warp has asserted the return code 0 and that the frame is all NaN still
        ref = _check('window ' + wname, code, got, img, name, oshape, off, -0.5)
        R, C, _, _ = DC.pull_coordinates(H, oshape, off)
        beyond = (R < 0) | (R >= shape[0]) | (C < 0) | (C >= shape[1])
        assert np.array_equal(got[beyond], np.zeros(beyond.sum(), got.dtype))
        assert beyond.any() == (wname != 'crop') and (ref != 0).any()


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
def test_warp_pitches_and_frames(code):
    """out_ld = out_cols + 5, out_bstride = out_rows * out_ld + 11, in_ld = cols + 3 with NaN in every gap and margin, B = 3"""
    shape = (20, 37)
    imgs = _noise(shape, code, 5, B=3)
    got = DC.run_warp(code, imgs, DC.homography('rotation', shape), in_pad=3, in_gap=4, out_pad=5, out_gap=11)
    packed = DC.run_warp(code, imgs, DC.homography('rotation', shape))
    for b in range(3):
        _check(f'pitched member {b}', code, got[b], imgs[b], 'rotation')
    assert _bit_equal(got, packed)


@pytest.mark.parametrize('code', CX, ids=DC.NAME.get)
def test_warp_reads_the_real_part(code):
    """complex input, every imaginary part NaN, in_ld and in_bstride in complex elements: bitwise the result of the real parts"""
    real = DC.REAL_CODE[code]
    for shape, name, kw in (((9, 12), 'shift+half', dict()), ((20, 37), 'rotation', dict(in_pad=3, in_gap=4)),
                            ((48, 100), 'perspective', dict(in_pad=1))):
        imgs = _noise(shape, code, 17, B=2)
        H = DC.homography(name, shape)
        got = DC.run_warp(code, imgs, H, **kw)
        assert np.isfinite(got).all()
        assert _bit_equal(got, DC.run_warp(real, imgs, H))
        shared = DC.run_warp(code, imgs[:1], H, batch=3, shared=True, **kw)
        assert all(_bit_equal(shared[b], got[0]) for b in range(3))


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
def test_warp_stacks(code):
    shape = DC.STACK_SHAPE
    big = (13, 29)
    imgs = _noise(big, code, 23, B=5)
    got = DC.run_warp(code, imgs, DC.homography('rotation', big))
    for b in range(5):
        _check(f'stack member {b}', code, got[b], imgs[b], 'rotation')
    shared = DC.run_warp(code, imgs[:1], DC.homography('rotation', big), batch=5, shared=True)
    assert shared.shape == got.shape and all(_bit_equal(shared[b], got[0]) for b in range(5))
    # 65535 + 3 members, member b = base[b % 7]: the second trip of the blockIdx.z loop of both kernels
    B = DC.MAX_GRID + 3
    base = _noise(shape, code, 29, B=7)
    for name in ('shift+half', 'rotation'):
        got = DC.run_warp(code, base[np.arange(B) % 7], DC.homography(name, shape))
        assert got.shape == (B,) + shape
        for b in range(7):
            _check(f'long stack member {b}', code, got[b], base[b], name)
        assert (got[:7] != 0).any()
        assert _bit_equal(got, got[np.arange(B) % 7])


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
@pytest.mark.parametrize('rows', DC.TALL_ROWS)
def test_warp_tall_grid(rows, code):
    """more rows than 65535 workgroups of the sample kernel (4 rows each) and of the prefilter (16 rows each) cover in one trip"""
    shape = (rows, DC.TALL_COLS)
    img = _noise(shape, code, 31)
    got = DC.run_warp(code, img[None], DC.homography('shift+half', shape))[0]
    ref = _check('tall', code, got, img, 'shift+half')
    last = got[-5:]
    assert (last[:-1, :2] != 0).all() and not last[-1].any() and not last[:, 2].any()
    assert np.max(np.abs(last - ref[-5:])) <= DC.warp_bound(code, img, 1.0)


def test_warp_recorded_figures():
    """runs last: the worst ratios of this session, for the record in this file's docstring"""
    for k, v in sorted(_worst.items()):
        print(f'pm_warp {k}: worst |got - ref| / bound over all cases {v:.3e} (recorded {RECORDED[k]})')
    assert all(v <= 1.0 for v in _worst.values())


# ----------------------------------------------------------------------------- pm_lattice

def _ints(shape, code, seed):
    return np.random.default_rng(seed).integers(-9, 10, shape).astype(DC.REAL_NP[code])


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
@pytest.mark.parametrize('geom', DC.LATTICES.values(), ids=DC.LATTICES.keys())
def test_lattice_scatter(geom, code):
    """the kernel is the memset: the NaN-filled grid holds scale * a at the lattice points and exact zeros elsewhere, the frame NaN"""
    *g, pad = geom
    rows, cols, ny, nx = g[:4]
    a = _ints((2, ny, nx), code, rows + nx)
    a[a == 0] = 5                       # a lattice point is then never 0
    got = DC.run_lattice(code, SC, a, g, scale=-2.0, in_pad=pad, in_gap=pad)
    ref = DC.lattice_reference(SC, a, *g, -2.0)
    assert got.dtype == DC.REAL_NP[code] and not np.isnan(got).any()
    assert np.array_equal(got, ref)
    assert (got != 0).sum() == 2 * ny * nx


@pytest.mark.parametrize('code', REAL + CX, ids=DC.NAME.get)
@pytest.mark.parametrize('geom', DC.LATTICES.values(), ids=DC.LATTICES.keys())
def test_lattice_gather(geom, code):
    """from real fields and from the real parts of complex ones (imaginary parts NaN), in_ld = cols + 3 with NaN in the gap"""
    *g, _ = geom
    rows, cols, ny, nx = g[:4]
    f = _ints((2, rows, cols), code, rows + ny)
    got = DC.run_lattice(code, GA, f, g, scale=-2.0, in_pad=3, in_gap=5)
    assert got.shape == (2, ny, nx) and np.isfinite(got).all()
    assert np.array_equal(got, DC.lattice_reference(GA, f, *g, -2.0))
    if code in DC.REAL_CODE:
        assert _bit_equal(got, DC.run_lattice(DC.REAL_CODE[code], GA, f, g, scale=-2.0, in_pad=3, in_gap=5))


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
def test_lattice_scatter_then_gather(code):
    *g, _ = DC.LATTICES['37x70 sy != sx, y0 != x0']
    a = _noise(g[2:4], code, 41, B=2)
    grid = DC.run_lattice(code, SC, a, g, scale=4.0)
    assert _bit_equal(DC.run_lattice(code, GA, grid, g, scale=0.25), a)
    # one row down no lattice point is hit: the gather of the zero fill
    off = DC.run_lattice(code, GA, grid, g, scale=0.25, y0=g[4] + 1)
    assert np.array_equal(off, np.zeros_like(a))


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
def test_lattice_stacks(code):
    *g, _ = DC.LATTICES['4x4 2x2 to the last row and column']
    B = DC.MAX_GRID + 3
    which = np.arange(B) % 7
    a = _ints((7, 2, 2), code, 43)
    a[a == 0] = 3
    got = DC.run_lattice(code, SC, a[which], g, scale=-2.0, out_pad=0, out_gap=0)
    assert np.array_equal(got, DC.lattice_reference(SC, a, *g, -2.0)[which])
    f = _ints((7, 4, 4), code, 47)
    got = DC.run_lattice(code, GA, f[which], g, scale=-2.0, out_pad=0, out_gap=0)
    assert np.array_equal(got, DC.lattice_reference(GA, f, *g, -2.0)[which])
    for cx in (code, {L.PM_F32: L.PM_C64, L.PM_F64: L.PM_C128}[code]):
        got = DC.run_lattice(cx, GA, f[:1], g, scale=-2.0, batch=4, shared=True)
        assert np.array_equal(got, np.repeat(DC.lattice_reference(GA, f[:1], *g, -2.0), 4, axis=0))
    got = DC.run_lattice(code, SC, a[:1], g, scale=-2.0, batch=4, shared=True)
    assert np.array_equal(got, np.repeat(DC.lattice_reference(SC, a[:1], *g, -2.0), 4, axis=0))


@pytest.mark.parametrize('code', REAL, ids=DC.NAME.get)
def test_lattice_tall_grid(code):
    """4 x 65535 + 5 rows: the last five are the second trip down the rows; the lattice's last row is the grid's"""
    rows = DC.TALL_ROWS[0]
    g = (rows, DC.TALL_COLS, (rows - 1) // 4 + 1, 2, 0, 0, 4, 2)
    a = _ints((1, g[2], 2), code, 53)
    a[a == 0] = 7
    got = DC.run_lattice(code, SC, a, g, scale=-2.0)
    assert np.array_equal(got, DC.lattice_reference(SC, a, *g, -2.0))
    assert np.array_equal(got[0, -1], [-2.0 * a[0, -1, 0], 0, -2.0 * a[0, -1, 1]]) and not got[0, -4:-1].any()
    # every pixel a lattice point: the gather's second trip
    g = (rows, DC.TALL_COLS, rows, DC.TALL_COLS, 0, 0, 1, 1)
    f = _ints((1, rows, DC.TALL_COLS), code, 59)
    got = DC.run_lattice(code, GA, f, g, scale=-2.0, in_pad=1)
    assert np.array_equal(got, -2.0 * f)
