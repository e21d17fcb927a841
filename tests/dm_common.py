"""What tests/test_dm_host.py and tests/test_gpu_dm_kernels.py share: the numpy model of pm_warp's arithmetic, the float64 references of
the two entry points (pm_warp by scipy, pm_lattice by numpy slicing), the homographies and cases, the bounds, NaN frames and one call of
each entry point with everything around it asserted.  Imports without a GPU.

Frames.  A stack of B windows of rows x cols lies inside ONE flat buffer filled with NaN (complex: both parts): LEAD elements, then member
b's element (r, c) at b * bstride + r * ld + c with ld = cols + pad and bstride = rows * ld + gap, then TAIL elements.  An input read
past a row, an image or a stack member multiplies a NaN in; after a call every element of an output buffer outside the windows must
still be NaN (Frame.read).  A complex input carries NaN in every imaginary part, so a real part read one float off is noticed as well.

Homographies.  Row-major 3 x 3 acting on (c, r, 1), as prysm_amd/x/dm.py passes them: (x', y', w) = H (c, r, 1), the pull coordinate is
(y'/w, x'/w).  HOMOGRAPHIES maps a name to (exact, f(shape) -> H).  The exact ones give integers or multiples of 2^-40 that float64
holds, so numpy, scipy and the kernel see the same coordinate to the bit, the constant-mode cutoff included, and NO pixel is left out
of a comparison (tests/test_dm_host.py shows the exactness in integer arithmetic).  For the others a coordinate within 1e-9 of 0 or
n - 1 may fall on either side of the cutoff in the last bit: near_cutoff() is that mask (the rule of tests/test_gpu_dm.py's _keep),
left_out() applies it to the inexact homographies only, and tests/test_dm_host.py asserts that it never takes more than 0.1 % of a
case's pixels.  That is why the rotation, the anisotropic scale and the perspective map act about the grid centre or carry an offset:
about the origin they would put row 0 and column 0 exactly on the cutoff.

Bounds of pm_warp (derived, not measured; the kernels only multiply and add).  The separable prefilter has absolute gain
sqrt(3) (1 + 2 |z| / (1 - |z|)) = 3 per axis, an output is 16 taps over coefficients that are each (2K + 1) + (2K + 1) products:
  float64   |got - ref| <= 1e-12 max|img| |scale|                              (about 140 eps * 9 = 1.4e-13 at the worst)
  float32   |got - ref| <= (80 * 2^-24 * 9 + 3e-8) max|img| |scale| = 4.3e-5   (3e-8: the K = 14 truncation of the prefilter)
Everything else is compared bit for bit, or is an exact zero or NaN check.
"""
import ctypes
import math

import numpy as np
from scipy import ndimage

from prysm_amd import _lib as L

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


# ----------------------------------------------------------------------------- homographies

def _translation(tx, ty):
    return lambda shape: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype=np.float64)


def _about_centre(A, shape):
    """the 2 x 2 map A about the grid centre ((cols - 1) / 2, (rows - 1) / 2)"""
    ctr = np.array([(shape[1] - 1) / 2, (shape[0] - 1) / 2])
    H = np.eye(3)
    H[:2, :2] = A
    H[:2, 2] = ctr - np.asarray(A) @ ctr
    return H


def _rotation(shape):
    t = math.radians(7)
    return _about_centre([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]], shape)


def _anisotropic(shape):
    return _about_centre([[1.25, 0.1], [0.0, 0.8]], shape)


def _perspective(shape):
    # w = 1 + 1e-3 c - 5e-4 r is positive on every grid here (rows <= 130 in the cases that use it)
    return np.array([[1.02, 0.03, 0.37], [-0.02, 0.97, 0.31], [1e-3, -5e-4, 1.0]])


HOMOGRAPHIES = {
    'identity': (True, _translation(0, 0)),
    'shift+3-2': (True, _translation(3, -2)),
    'shift+half': (True, _translation(0.5, 0.25)),
    'shift-half': (True, _translation(-0.5, -0.25)),
    'x-2^-40': (True, _translation(-2.0 ** -40, 0)),
    'x+2^-40': (True, _translation(2.0 ** -40, 0)),
    'y-2^-40': (True, _translation(0, -2.0 ** -40)),
    'y+2^-40': (True, _translation(0, 2.0 ** -40)),
    'half scale': (True, lambda shape: np.diag([0.5, 0.5, 1.0])),
    'rotation': (False, _rotation),
    'anisotropic': (False, _anisotropic),
    'perspective': (False, _perspective),
}
CUTOFF_SHIFTS = ('x-2^-40', 'x+2^-40', 'y-2^-40', 'y+2^-40')


def homography(name, shape):
    return HOMOGRAPHIES[name][1](shape)


def pull_coordinates(H, out_shape, off):
    """(R, C, xx, yy): the input pixel (R, C) = (r + off_y, c + off_x) of every output pixel and its pull coordinate, in the order of
    operations of the kernel (and of apply_homography): H[0] C + H[1] R + H[2], divided by w"""
    H = np.asarray(H, dtype=np.float64).ravel()
    R, C = np.meshgrid(np.arange(out_shape[0], dtype=np.int64) + off[0], np.arange(out_shape[1], dtype=np.int64) + off[1], indexing='ij')
    xc, yr = C.astype(np.float64), R.astype(np.float64)
    w = H[6] * xc + H[7] * yr + H[8]
    return R, C, (H[0] * xc + H[1] * yr + H[2]) / w, (H[3] * xc + H[4] * yr + H[5]) / w


def _domain(R, C, shape):
    return (R >= 0) & (R < shape[0]) & (C >= 0) & (C < shape[1])


def warp_reference(img, H, out_shape, off, scale):
    """float64 reference of pm_warp by scipy: output pixel (r, c) takes (R, C) = (r + off_y, c + off_x); outside the rows x cols grid
    it is 0, else scale * map_coordinates(img, (y'/w, x'/w), order=3, mode='constant', cval=0) with (x', y', w) = H (C, R, 1)"""
    img = np.asarray(img, dtype=np.float64)
    R, C, xx, yy = pull_coordinates(H, out_shape, off)
    dom = _domain(R, C, img.shape)
    out = np.zeros(tuple(out_shape))
    if dom.any():
        out[dom] = scale * ndimage.map_coordinates(img, (yy[dom], xx[dom]), order=3, mode='constant', cval=0)
    return out


def model_warp(img, H, out_shape, off, scale, K=30):
    """the same through model_sample: the kernels' arithmetic composed with the window rule"""
    img = np.asarray(img, dtype=np.float64)
    R, C, xx, yy = pull_coordinates(H, out_shape, off)
    dom = _domain(R, C, img.shape)
    return np.where(dom, scale * model_sample(img, np.where(dom, yy, -1.0), np.where(dom, xx, -1.0), K), 0.0)


def near_cutoff(img_shape, H, out_shape, off):
    """the output pixels whose pull coordinate lies within 1e-9 of 0 or n - 1 on either axis"""
    _, _, xx, yy = pull_coordinates(H, out_shape, off)
    edge = np.zeros(tuple(out_shape), bool)
    for v, n in ((xx, img_shape[1]), (yy, img_shape[0])):
        edge |= (np.abs(v) < 1e-9) | (np.abs(v - (n - 1)) < 1e-9)
    return edge


def left_out(img_shape, name, out_shape, off):
    """the pixels a comparison under homography `name` leaves out: none for an exact one, near_cutoff for the others"""
    if HOMOGRAPHIES[name][0]:
        return np.zeros(tuple(out_shape), bool)
    return near_cutoff(img_shape, homography(name, img_shape), out_shape, off)


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_dm_kernels.py

# every axis below the K of float32 | one tile and one past it | between the two K and above 30 | several ragged tiles
SHAPES = [(1, 6), (6, 1), (2, 3), (5, 7), (13, 29), (16, 32), (17, 33), (29, 61), (31, 95), (48, 100), (130, 70)]
SHAPE_HOMS = ['identity', 'shift+3-2', 'shift+half', 'shift-half', 'rotation', 'perspective']
# the two members of the list that no other case uses, where both axes are long enough for an inexact map to stay off the cutoff
EXTRA_SHAPES = [(5, 7), (17, 33), (48, 100), (130, 70)]
EXTRA_HOMS = ['half scale', 'anisotropic']
CUTOFF_SHAPES = [(1, 6), (6, 1), (5, 7), (17, 33)]
WINDOW_SHAPES = [(48, 100), (31, 95)]
WINDOW_HOMS = ['rotation', 'perspective']
STACK_SHAPE = (3, 5)
MAX_GRID = 65535
TALL_ROWS = [4 * MAX_GRID + 5, 16 * MAX_GRID + 5]      # past the sample kernel's 4 rows x 65535 workgroups; past the prefilter's 16 x 65535
TALL_COLS = 3


def windows(shape):
    """name -> (out_shape, off): a crop, a pad on all sides, a window over one corner of the grid only, an empty one"""
    m, n = shape
    return {
        'crop': ((m - 12, n - 21), (5, 9)),
        'pad': ((m + 16, n + 10), (-7, -3)),
        'corner': ((9, 14), (-5, n - 6)),           # rows -5 .. 3, the last 6 columns and 8 past them: pad above, crop on the left
        'empty': ((0, n), (0, 0)),
    }


def warp_cases():
    """every (shape, homography name, out_shape, off) that tests/test_gpu_dm_kernels.py runs pm_warp at"""
    out = [(s, h, s, (0, 0)) for s in SHAPES for h in SHAPE_HOMS]
    out += [(s, h, s, (0, 0)) for s in EXTRA_SHAPES for h in EXTRA_HOMS]
    out += [(s, h, s, (0, 0)) for s in CUTOFF_SHAPES for h in ('identity',) + CUTOFF_SHIFTS]
    out += [(s, h, o, off) for s in WINDOW_SHAPES for h in WINDOW_HOMS for o, off in windows(s).values()]
    out += [((20, 37), 'rotation', (20, 37), (0, 0)), ((9, 12), 'shift+half', (9, 12), (0, 0))]      # pitches, complex input
    out += [(STACK_SHAPE, h, STACK_SHAPE, (0, 0)) for h in ('rotation', 'shift+half')]
    out += [((r, TALL_COLS), 'shift+half', (r, TALL_COLS), (0, 0)) for r in TALL_ROWS]
    return out


# ----------------------------------------------------------------------------- bounds

REAL_NP = {L.PM_F32: np.float32, L.PM_F64: np.float64, L.PM_C64: np.float32, L.PM_C128: np.float64}
CX_NP = {L.PM_C64: np.complex64, L.PM_C128: np.complex128}
REAL_CODE = {L.PM_C64: L.PM_F32, L.PM_C128: L.PM_F64}
NAME = {L.PM_F32: 'float32', L.PM_F64: 'float64', L.PM_C64: 'complex64', L.PM_C128: 'complex128'}


def warp_bound(code, img, scale):
    amp = float(np.max(np.abs(img))) * abs(scale)
    if REAL_NP[code] == np.float64:
        return 1e-12 * amp
    return (80 * 2.0 ** -24 * 9 + 3e-8) * amp


# ----------------------------------------------------------------------------- lattice

def lattice_reference(op, a, rows, cols, ny, nx, y0, x0, sy, sx, scale):
    """float64 reference of pm_lattice on (B, ., .) stacks.  SCATTER: a is (B, ny, nx), the result (B, rows, cols) with scale * a at
    (y0 + i sy, x0 + j sx) and zeros elsewhere.  GATHER: a is (B, rows, cols), the result scale * a at the lattice points."""
    a = np.asarray(a, dtype=np.float64)
    ys, xs = slice(y0, y0 + (ny - 1) * sy + 1, sy), slice(x0, x0 + (nx - 1) * sx + 1, sx)
    if op == L.PM_LATTICE_SCATTER:
        assert a.shape[1:] == (ny, nx)
        out = np.zeros((a.shape[0], rows, cols))
        out[:, ys, xs] = scale * a
        return out
    assert a.shape[1:] == (rows, cols)
    return scale * a[:, ys, xs]


# (rows, cols, ny, nx, y0, x0, sy, sx, pad of the commands' rows)
LATTICES = {
    '4x4 2x2 to the last row and column': (4, 4, 2, 2, 0, 1, 3, 2, 0),
    '4x4 one point': (4, 4, 1, 1, 2, 3, 1, 1, 0),
    '37x70 sy != sx, y0 != x0': (37, 70, 12, 13, 2, 4, 3, 5, 0),
    '37x70 to the last row and column': (37, 70, 10, 12, 0, 3, 4, 6, 2),
    '37x70 every pixel': (37, 70, 37, 70, 0, 0, 1, 1, 0),
    '37x70 one point': (37, 70, 1, 1, 20, 69, 1, 1, 0),
    '66x130 sy != sx, commands pitched': (66, 130, 33, 43, 1, 2, 2, 3, 3),
    '66x130 every pixel': (66, 130, 66, 130, 0, 0, 1, 1, 0),
}


# ----------------------------------------------------------------------------- frames

LEAD, TAIL = 7, 13


class Frame:
    """B windows of rows x cols inside one NaN-filled flat buffer (see the module docstring); shared: ONE window that every member of
    the stack reads (bstride 0)"""

    def __init__(self, B, rows, cols, np_dtype, pad=0, gap=0, shared=False):
        self.shape = (1 if shared else B, rows, cols)
        self.ld = cols + pad
        self.bstride = 0 if shared else rows * self.ld + gap
        nb = self.shape[0]
        b, r, c = np.ogrid[:nb, :rows, :cols]
        self.index = LEAD + b * (rows * self.ld + gap) + r * self.ld + c
        span = int(self.index.max()) + 1 - LEAD if self.index.size else 0
        self.host = np.full(LEAD + span + TAIL, np.nan, dtype=np_dtype)
        if np.iscomplexobj(self.host):
            self.host.imag = np.nan
        self.dev = None

    def fill(self, values):
        self.host[self.index] = values
        return self

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host).cuda()
        return self

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + LEAD * self.host.dtype.itemsize)

    def read(self):
        """the windows after a call; asserts that every element outside them is still NaN"""
        h = self.dev.cpu().numpy()
        outside = np.ones(h.shape, bool)
        outside[self.index] = False
        nan = np.isnan(h.real) & np.isnan(h.imag) if np.iscomplexobj(h) else np.isnan(h)
        bad = np.flatnonzero(outside & ~nan)
        assert bad.size == 0, f'{bad.size} elements outside the windows were written, first at buffer element {bad[0]} (window starts at {LEAD})'
        return h[self.index]

    def unchanged(self):
        """an input: not a bit of its buffer may change"""
        item = self.host.dtype.itemsize
        return np.array_equal(self.dev.cpu().numpy().view(np.uint8).reshape(-1, item), self.host.view(np.uint8).reshape(-1, item))


def input_frame(code, values, pad=0, gap=0, shared=False):
    """real values (B, rows, cols) as the input of dtype `code`: real, or complex with NaN in every imaginary part"""
    values = np.asarray(values)
    B, rows, cols = values.shape
    if code in CX_NP:
        cx = np.empty(values.shape, dtype=CX_NP[code])
        cx.real = values
        cx.imag = np.nan
        values = cx
    else:
        values = values.astype(REAL_NP[code])
    return Frame(B, rows, cols, values.dtype, pad, gap, shared).fill(values).upload()


# ----------------------------------------------------------------------------- calls (GPU)

def run_warp(code, imgs, H, out_shape=None, off=(0, 0), scale=1.0, batch=None, in_pad=0, in_gap=0, out_pad=0, out_gap=0, shared=False):
    """one pm_warp call: imgs (B, rows, cols) real values (a complex `code` reads them as real parts), or ONE image shared by `batch`
    members (in_bstride 0).  Returns the (batch, out_rows, out_cols) result; asserts the return code, the output frame and that the
    input was not written."""
    lib = L.load()
    imgs = np.asarray(imgs)
    B = batch if shared else imgs.shape[0]
    rows, cols = imgs.shape[1:]
    orows, ocols = out_shape if out_shape is not None else (rows, cols)
    fin = input_frame(code, imgs, in_pad, in_gap, shared)
    fout = Frame(B, orows, ocols, REAL_NP[code], out_pad, out_gap).upload()
    nbytes = lib.pm_warp_workspace(code, B, rows, cols)
    assert nbytes == B * rows * cols * np.dtype(REAL_NP[code]).itemsize
    ws = L.workspace(nbytes)
    Hc = (L.c_f64 * 9)(*[float(v) for v in np.asarray(H, dtype=np.float64).ravel()])
    L.check(lib.pm_warp(code, 3, B, rows, cols, fin.ptr, fin.ld, fin.bstride if B > 1 else rows * fin.ld, Hc, float(scale), orows, ocols,
                        off[0], off[1], fout.ptr, fout.ld, fout.bstride, L.ptr(ws), nbytes, L.stream_ptr()))
    got = fout.read()
    assert fin.unchanged()
    return got


def run_lattice(code, op, a, geom, scale=1.0, batch=None, in_pad=0, in_gap=0, out_pad=4, out_gap=9, shared=False, y0=None):
    """one pm_lattice call on geom = (rows, cols, ny, nx, y0, x0, sy, sx): SCATTER of commands a (B, ny, nx) or GATHER from fields
    a (B, rows, cols), the output NaN-filled inside a NaN frame.  Returns the (batch, ., .) result."""
    lib = L.load()
    rows, cols, ny, nx, gy0, x0, sy, sx = geom
    y0 = gy0 if y0 is None else y0
    a = np.asarray(a)
    B = batch if shared else a.shape[0]
    oshape = (rows, cols) if op == L.PM_LATTICE_SCATTER else (ny, nx)
    assert a.shape[1:] == ((ny, nx) if op == L.PM_LATTICE_SCATTER else (rows, cols))
    fin = input_frame(code, a, in_pad, in_gap, shared)
    fout = Frame(B, oshape[0], oshape[1], REAL_NP[code], out_pad, out_gap).upload()
    L.check(lib.pm_lattice(code, op, B, rows, cols, ny, nx, y0, x0, sy, sx, float(scale), fin.ptr, fin.ld,
                           fin.bstride if B > 1 else a.shape[1] * fin.ld, fout.ptr, fout.ld, fout.bstride, L.stream_ptr()))
    got = fout.read()
    assert fin.unchanged()
    return got
