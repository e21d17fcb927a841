"""Helpers of the C-ABI tests of the pointwise, synthesis and resampling kernels (tests/test_gpu_pointwise.py): guarded device
windows with a leading dimension and an offset base, an exact reference for exp(2 pi i t), and plain numpy / longdouble restatements
of the arithmetic kernels.  Nothing here needs a GPU until `window()` is asked for a device buffer."""
import ctypes
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import torch

LD = np.longdouble
REAL_OF = {np.dtype('complex64'): np.dtype('float32'), np.dtype('complex128'): np.dtype('float64')}
COMPLEX_OF = {v: k for k, v in REAL_OF.items()}
# the byte pattern outside every window: a quiet NaN with a payload for float types (no kernel produces it), 0xA5 for bytes
_SENTINEL_WORD = {4: np.uint32(0x7FC5A5A5), 8: np.uint64(0x7FF8A5A5A5A5A5A5)}

LAYOUT_SHAPES = [(1, 1), (1, 65), (5, 63), (4, 64), (3, 129)]
TALL_SHAPE = (262145, 3)       # (rows + 3) / 4 > 65535 blocks: the grid-stride step of the row loop runs
LD_PADS = (0, 1, 7)
BASE_OFFS = (0, 1)


def layouts():
    """(shape, ld_pad, base_off) of the layout sweep: every small shape with every padding and offset, the tall shape once"""
    out = [(s, p, o) for s in LAYOUT_SHAPES for p in LD_PADS for o in BASE_OFFS]
    out.append((TALL_SHAPE, 1, 1))
    return out


def other_layout(ld_pad, base_off, k=1):
    """an independent (ld_pad, base_off) for another array of the same call"""
    return LD_PADS[(LD_PADS.index(ld_pad) + k) % len(LD_PADS)], (base_off + k) % 2


def sentinel_bytes(dtype, count):
    """`count` elements of `dtype` filled with the sentinel, as a uint8 array"""
    dtype = np.dtype(dtype)
    if dtype.kind in 'fc':
        word = 4 if dtype in (np.dtype('float32'), np.dtype('complex64')) else 8
        return np.full(count * dtype.itemsize // word, _SENTINEL_WORD[word]).view(np.uint8)
    return np.full(count * dtype.itemsize, 0xA5, dtype=np.uint8)


class Window:
    """A rows x cols window with leading dimension `ld` inside one larger allocation that is otherwise all sentinel.

    buf  : the whole allocation (a uint8 torch tensor)
    ptr  : ctypes pointer to element [0][0] of the window (`base_off` elements past an aligned position)
    ld   : cols + ld_pad
    """

    def __init__(self, shape, dtype, ld_pad=0, base_off=0, rng=None, data=None, device='cuda'):
        self.rows, self.cols = (int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        if ld_pad < 0 or base_off < 0 or self.rows < 1 or self.cols < 1:
            raise ValueError('window: a leading dimension below cols or a negative offset would leave the allocation')
        self.ld = self.cols + int(ld_pad)
        guard = -(-(self.ld + 64) // 16) * 16          # >= ld + 64 elements, and a multiple of 16 so that base_off alone sets the alignment
        self.start = guard + int(base_off)
        self.total = self.start + self.rows * self.ld + guard
        host = sentinel_bytes(self.dtype, self.total).view(self.dtype).copy()
        if data is None and rng is not None:
            data = random_values(rng, (self.rows, self.cols), self.dtype)
        self._view(host)[...] = 0 if data is None else np.asarray(data).astype(self.dtype, copy=False).reshape(self.rows, self.cols)
        self.initial = host
        self.buf = torch.from_numpy(host.view(np.uint8).copy()).to(device)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.start * self.dtype.itemsize)
        self._mask = np.ones(self.total, dtype=bool)
        self._view(self._mask)[...] = False

    def _view(self, flat):
        """the rows x cols window of a flat array of `total` elements (a strided view)"""
        return np.lib.stride_tricks.as_strided(flat[self.start:], (self.rows, self.cols), (self.ld * flat.itemsize, flat.itemsize))

    def host(self):
        return self.buf.cpu().numpy().view(self.dtype)

    def data(self):
        """what the window holds now, as a contiguous rows x cols array"""
        return np.ascontiguousarray(self._view(self.host()))

    def set(self, values):
        flat = self.host().copy()
        self._view(flat)[...] = values
        self.buf.copy_(torch.from_numpy(flat.view(np.uint8)))

    def check_guards(self):
        """every element outside [0:rows, 0:cols] -- the ld padding and both guard bands -- is still the sentinel, bit for bit"""
        size = self.dtype.itemsize
        now, was = self.host().view(np.uint8).reshape(-1, size), self.initial.view(np.uint8).reshape(-1, size)
        bad = np.flatnonzero((now != was).any(axis=1) & self._mask)
        assert bad.size == 0, (f'{bad.size} elements outside the {self.rows} x {self.cols} window (ld {self.ld}) were written; first at '
                               f'window offset {int(bad[0]) - self.start}')


def window(shape, dtype, ld_pad=0, base_off=0, rng=None, data=None, device='cuda'):
    return Window(shape, dtype, ld_pad, base_off, rng, data, device)


def random_values(rng, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == 'c':
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    if dtype.kind == 'f':
        return rng.standard_normal(shape).astype(dtype)
    return rng.integers(0, 256, size=shape + (dtype.itemsize,), dtype=np.uint8).view(dtype).reshape(shape)


# --------------------------------------------------------------------------- exact phases
def exact_unit_phase(turns_fraction):
    """(cos, sin) of 2 pi t for an exact rational t, as mpmath numbers at 40 digits: t is reduced mod 1 as a Fraction, so no
    floating-point rounding happens before the reduction, however many turns t holds."""
    t = Fraction(turns_fraction)
    r = t - math.floor(t)                       # exact, in [0, 1)
    if r >= Fraction(1, 2):
        r -= 1                                  # [-1/2, 1/2): the small argument keeps the series short
    with mpmath.workdps(40):
        x = mpmath.mpf(2 * r.numerator) / mpmath.mpf(r.denominator)
        return mpmath.cospi(x), mpmath.sinpi(x)


def phase_errors(got, turns, amp=None):
    """max over the samples of |got - amp exp(2 pi i t)| per component, and the same for each sample, as floats; `turns` exact
    Fractions, `got` complex values as stored by the kernel, amp exact floats (default 1)"""
    err = np.zeros(len(turns))
    with mpmath.workdps(40):
        for i, t in enumerate(turns):
            c, s = exact_unit_phase(t)
            a = mpmath.mpf(1.0 if amp is None else float(amp[i]))
            g = complex(got[i])
            err[i] = float(max(abs(mpmath.mpf(g.real) - a * c), abs(mpmath.mpf(g.imag) - a * s)))
    return err


def phase_bound(rdtype, turns, amp=None, product_roundings=2, extra_rel=0.0):
    """Per-component bound of a kernel that forms t in fp64, reduces it to one turn exactly, calls sincospi and rounds to T:

        |err| <= |amp| * (eps_T / 2  +  2 pi |t| * product_roundings * 2^-53  +  2 pi |t| * extra_rel)  +  tiny

    - eps_T / 2: the one rounding of amp * cos (or sin) to T;
    - every fp64 rounding on the way to t moves the phase by at most 2 pi |t| 2^-53 rad, and a unit-modulus value by as much.
      The default of two (2 pi |t| 2^-52) is the allowance the kernels are specified to: the fp64 product and the host's division of
      k by 2 pi.  The tests repeat that division themselves and take t from its result, so of the two only the product is in the
      measured error.  Counted in the source, t carries: pm_pupil_synth and pm_mdft_basis one rounding (the product);
      pm_as_tf_vectors two in fp64 (k * k, times the coefficient), one in fp32 (k * k is exact); pm_quadratic_phase two in fp32 (the
      squares of float32 numbers are exact: the sum and the product by c / 2 pi) but THREE in fp64 (y * y, the fused x * x + y * y,
      the product).  For pm_quadratic_phase in complex128 the allowance of two is therefore not a proven bound: the worst case is
      1.5 times it, reached only if all three roundings are near half an ulp with one sign at a mantissa near 1.  The test holds the
      kernel to the specified figure all the same (largest seen: 0.8 of it at 1e6 rad) and would show a fourth rounding creeping in;
    - tiny = |amp| * 2^-51: the device sincospi (2 ulp of a value of at most 1 in the ROCm device-library tables: 2^-52) and the
      fp64 product amp * cos before the rounding to T (2^-53), 1.5 * 2^-52 together.  Against eps_32 / 2 = 6e-8 it is nothing; for
      T = double it is four times the rounding term beside it and is what bounds the result at small phases.
    """
    eps = float(np.finfo(rdtype).eps)
    t = np.abs(turns.astype(np.float64)) if isinstance(turns, np.ndarray) else np.array([abs(float(x)) for x in turns])
    a = np.ones(len(t)) if amp is None else np.abs(np.asarray(amp, dtype=np.float64))
    return a * (eps / 2 + 2 * math.pi * t * (product_roundings * 2.0 ** -53 + extra_rel)) + a * 2.0 ** -51 + 1e-300


def sample_indices(rng, shape, limit=4096):
    n = shape[0] * shape[1]
    if n <= limit:
        return np.arange(n)
    return np.sort(rng.choice(n, size=limit, replace=False))


# --------------------------------------------------------------------------- arithmetic references (longdouble, same stored inputs)
def _parts(z):
    z = np.asarray(z)
    return z.real.astype(LD), z.imag.astype(LD)


def ref_cmul(a, b, conj_b=False):
    """(real, imag, S_real, S_imag): a * b or a * conj(b) in longdouble, with the sums of the absolute terms of each component"""
    ar, ai = _parts(a)
    br, bi = _parts(b)
    if conj_b:
        bi = -bi
    return ar * br - ai * bi, ar * bi + ai * br, np.abs(ar * br) + np.abs(ai * bi), np.abs(ar * bi) + np.abs(ai * br)


def ref_cmul_parts(ar, ai, sa_r, sa_i, b, conj_b=False):
    """the product of an already-accumulated (ar + i ai), whose terms sum to (sa_r, sa_i) in absolute value, with b"""
    br, bi = _parts(b)
    if conj_b:
        bi = -bi
    return (ar * br - ai * bi, ar * bi + ai * br, sa_r * np.abs(br) + sa_i * np.abs(bi), sa_r * np.abs(bi) + sa_i * np.abs(br))


def ref_abs2(x):
    xr, xi = _parts(x)
    return xr * xr + xi * xi


def ref_sum_modes(modes, weights, out0=None):
    """(sum, S): sum_b w_b modes[b] (+ out0) in longdouble and the sum of the absolute terms; the weights as the kernel holds them"""
    shape = modes.shape[1:]
    acc = np.zeros(shape, LD) if out0 is None else out0.astype(LD)
    S = np.abs(acc)
    for b in range(modes.shape[0]):
        term = LD(weights[b]) * modes[b].astype(LD)
        acc = acc + term
        S = S + np.abs(term)
    return acc, S


# --------------------------------------------------------------------------- embed / pad references
def ref_embed(x, out_shape, off, fill):
    """out = fill; x placed with its [0][0] at `off` of out, whatever falls outside dropped (negative offsets crop)"""
    out = np.empty(out_shape, dtype=x.dtype)
    out[...] = fill
    oy, ox = off
    r0, r1 = max(oy, 0), min(oy + x.shape[0], out_shape[0])
    c0, c1 = max(ox, 0), min(ox + x.shape[1], out_shape[1])
    if r1 > r0 and c1 > c0:
        out[r0:r1, c0:c1] = x[r0 - oy:r1 - oy, c0 - ox:c1 - ox]
    return out


PAD_MODES = {1: 'edge', 2: 'reflect', 3: 'symmetric', 4: 'wrap'}


def pad_source_index(r, n, mode):
    """np.pad's index maps restated one index at a time (r relative to the first input sample): which input sample lands there"""
    if 0 <= r < n:
        return r
    if n == 1:
        return 0
    if mode == 1:
        return 0 if r < 0 else n - 1
    if mode == 4:
        return r % n
    period = 2 * n - 2 if mode == 2 else 2 * n
    r %= period
    if r < n:
        return r
    return period - r if mode == 2 else period - 1 - r


def ref_pad_index(x, before, after, mode):
    """np.pad(x, (before, after), mode) by explicit index maps: before / after are (rows, cols) pad widths"""
    m, n = x.shape
    ri = [pad_source_index(r - before[0], m, mode) for r in range(m + before[0] + after[0])]
    ci = [pad_source_index(c - before[1], n, mode) for c in range(n + before[1] + after[1])]
    return x[np.ix_(ri, ci)]


# --------------------------------------------------------------------------- encircled energy
def ee_grid(shape, df):
    """the radial frequency of every bin, as fp64 coordinates (fftrange * df, the products the kernel forms) -> exact hypot in mpmath"""
    rows, cols = shape
    y = (np.arange(rows) - rows // 2) * float(df)
    x = (np.arange(cols) - cols // 2) * float(df)
    return x, y


@functools.lru_cache(maxsize=None)
def _ee_kernel_terms(shape, df, radii, support):
    """J1(2 pi r nu) / nu at 30 digits for every radius and every bin of `support` (flat indices), as mpmath numbers"""
    x, y = ee_grid(shape, df)
    out = []
    with mpmath.workdps(30):
        for g in support:
            i, j = divmod(g, shape[1])
            nu = mpmath.sqrt(mpmath.mpf(float(x[j])) ** 2 + mpmath.mpf(float(y[i])) ** 2)
            if nu == 0:
                nu = mpmath.mpf(1e-16)
            out.append([mpmath.besselj(1, 2 * mpmath.pi * mpmath.mpf(float(r)) * nu) / nu for r in radii])
    return out


def ref_encircled_energy(mtf, df, radii_mm, support=None):
    """EE(r) = r df^2 sum_ij mtf_ij J1(2 pi r nu_ij) / nu_ij: the terms from mpmath, rounded to fp64 one by one, summed with
    math.fsum.  `support`: the flat indices where mtf is non-zero (default: all)."""
    mtf = np.asarray(mtf)
    flat = mtf.ravel()
    support = tuple(range(flat.size)) if support is None else tuple(int(g) for g in support)
    radii = tuple(float(r) for r in radii_mm)
    K = _ee_kernel_terms(tuple(mtf.shape), float(df), radii, support)
    out = np.zeros(len(radii))
    with mpmath.workdps(30):
        for k, r in enumerate(radii):
            s = math.fsum(float(mpmath.mpf(float(flat[g])) * K[n][k]) for n, g in enumerate(support))
            out[k] = float(mpmath.mpf(r) * mpmath.mpf(s) * mpmath.mpf(float(df)) ** 2)
    return out


def ref_encircled_energy_adjoint(shape, df, radii_mm, ee_bar):
    """mtf_bar_ij = sum_r ee_bar_r r J1(2 pi r nu_ij) / nu_ij df^2 for every bin, from mpmath, rounded once to fp64"""
    radii = tuple(float(r) for r in radii_mm)
    n = shape[0] * shape[1]
    K = _ee_kernel_terms(tuple(shape), float(df), radii, tuple(range(n)))
    out = np.zeros(n)
    with mpmath.workdps(30):
        for g in range(n):
            out[g] = float(sum((mpmath.mpf(float(w)) * mpmath.mpf(r) * K[g][k] for k, (r, w) in enumerate(zip(radii, ee_bar))),
                               mpmath.mpf(0)) * mpmath.mpf(float(df)) ** 2)
    return out.reshape(shape)


def ulps(got, want_mp, dtype):
    """|got - want| in units in the last place of `dtype` at want (want an mpmath number)"""
    w = float(want_mp)
    if w == 0.0:
        return 0.0 if got == 0.0 else math.inf
    spacing = float(np.spacing(np.dtype(dtype).type(abs(w))))
    with mpmath.workdps(40):
        return float(abs(mpmath.mpf(float(got)) - want_mp) / spacing)
