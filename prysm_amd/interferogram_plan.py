"""Host side of prysm_amd.interferogram and prysm_amd.util: a numpy model of every kernel of csrc/interferogram.hip, and the host logic
of the public layer (argument errors, the band limits, the crop box, the coordinate bookkeeping).  Imports without a device.

The models do the kernels' arithmetic -- the same operations in the same precision, every product and sum rounded by itself -- except
for the ORDER of the long sums: a kernel adds per thread, per workgroup and over the partials, numpy adds pairwise.  Sums of values
that are exact in double in any order (counts, small integers) agree to the bit; the rest agree within n eps of the sum of the
magnitudes.

  grid_default .. grid_recenter, crop_box, pad_shape, band_limits, window_kind     host logic of the Interferogram
  stats                pm_ifg_stats: the record of RECORD doubles
  grid_xy, linspace_xy the generated coordinates of pm_ifg_coords, as doubles
  fit, solve           pm_ifg_fit: the 14 sums and the elimination with diagonal pivoting
  remove, fill, mask, clip, slope     pm_ifg_remove, pm_ifg_edit, pm_ifg_slope
  window, windowed     pm_ifg_window: the window in double, S2, the product
  band_nu, band        pm_ifg_band
  hann2d, iir, combine, psd_model     pm_ifg_iir, pm_ifg_combine, pm_ifg_psd_model
"""
import math

import numpy as np

from .imagechain_plan import jinc

(N, NNAN, SUM, SUMSQ, MIN, MAX, ROW0, ROW1, COL0, COL1, MEAN, SAD, M2, STD, RMS, SA, RECORD) = range(17)
TERM_PISTON, TERM_X, TERM_Y, TERM_R2 = 1, 2, 4, 8
FILL, MASK, CLIP = 0, 1, 2
WIN_WELCH, WIN_HANN, WIN_ARRAY = 0, 1, 2
LP, HP, BP, BR = 0, 1, 2, 3
PSD_ABC, PSD_AB = 0, 1
THREADS, WGS = 256, 1024        # kIfgThreads, kIfgWgs: a first stage runs min(WGS, ceil(n / THREADS)) workgroups

FILTER_TYPES = {'lp': LP, 'lowpass': LP, 'hp': HP, 'highpass': HP, 'bp': BP, 'bandpass': BP, 'br': BR, 'bandreject': BR}


def second_trip_elements():
    """the smallest element count at which every first-stage thread makes a second trip of its grid-stride loop"""
    return 2 * THREADS * WGS


# --------------------------------------------------------------------------- statistics
def stats(z):
    """pm_ifg_stats of a 2-D float32 / float64 array: the record as RECORD float64 values"""
    z = np.asarray(z)
    rec = np.zeros(RECORD)
    fin = np.isfinite(z)
    v = z[fin].astype(np.float64)
    n = v.size
    rec[N], rec[NNAN] = n, np.count_nonzero(np.isnan(z))
    rec[SUM], rec[SUMSQ] = v.sum(), (v * v).sum()
    if n:
        rows, cols = np.nonzero(fin.any(axis=1))[0], np.nonzero(fin.any(axis=0))[0]
        rec[MIN], rec[MAX] = v.min(), v.max()
        rec[ROW0], rec[ROW1], rec[COL0], rec[COL1] = rows[0], rows[-1], cols[0], cols[-1]
        rec[MEAN] = rec[SUM] / n
        e = v - rec[MEAN]
        rec[SAD], rec[M2] = np.abs(e).sum(), (e * e).sum()
        rec[STD], rec[RMS], rec[SA] = math.sqrt(rec[M2] / n), math.sqrt(rec[SUMSQ] / n), rec[SAD] / n
    else:
        rec[[MIN, MAX, MEAN, STD, RMS, SA]] = np.nan
        rec[[ROW0, ROW1, COL0, COL1]] = -1
    return rec


# --------------------------------------------------------------------------- coordinates
def grid_xy(shape, origin, dx, dtype):
    """PM_COORDS_GRID: x = T(c - ox) * T(dx), y = T(r - oy) * T(dx) -- make_xy_grid's elements shifted to an origin index -- as float64
    row and column vectors"""
    T = np.dtype(dtype).type
    oy, ox = origin
    x = (np.arange(shape[1]) - ox).astype(T) * T(dx)
    y = (np.arange(shape[0]) - oy).astype(T) * T(dx)
    return x.astype(np.float64)[None, :], y.astype(np.float64)[:, None]


def linspace_step(n):
    return 2.0 / (n - 1) if n > 1 else 0.0


def linspace_xy(shape):
    """the linspace form: -1 + j * (2 / (n - 1)) in double along each axis (np.linspace(-1, 1, n) but for its last sample, which numpy
    sets to 1 exactly)"""
    x = -1.0 + np.arange(shape[1], dtype=np.float64) * linspace_step(shape[1])
    y = -1.0 + np.arange(shape[0], dtype=np.float64) * linspace_step(shape[0])
    return x[None, :], y[:, None]


# --------------------------------------------------------------------------- fit and removal
def fit_sums(z, x, y):
    """the 14 sums of pm_ifg_fit over the finite pixels: the Gram matrix of (1, x, y, q = x^2 + y^2) and the right-hand sides"""
    z = np.asarray(z)
    fin = np.isfinite(z)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), z.shape)[fin]
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), z.shape)[fin]
    v = z[fin].astype(np.float64)
    q = x * x + y * y
    b = [np.ones_like(v), x, y, q]
    G = np.array([[(b[i] * b[j]).sum() for j in range(4)] for i in range(4)])
    rhs = np.array([(b[i] * v).sum() for i in range(4)])
    return G, rhs


def solve(G, rhs, terms):
    """fit_solve_kernel: elimination with diagonal pivoting on the chosen subsystem; a pivot that is not above eps times the first ends
    it and the terms left get 0"""
    A = np.array(G, dtype=np.float64)
    b = np.array(rhs, dtype=np.float64)
    left = [bool((terms >> i) & 1) for i in range(4)]
    m = sum(left)
    perm, first = [], 0.0
    for step in range(m):
        p = -1
        for i in range(4):
            if left[i] and (p < 0 or A[i, i] > A[p, p]):
                p = i
        if step == 0:
            first = A[p, p]
        if not (A[p, p] > np.finfo(np.float64).eps * first) or not (A[p, p] > 0.0):
            break
        left[p] = False
        perm.append(p)
        for i in range(4):
            if not left[i]:
                continue
            f = A[i, p] / A[p, p]
            for j in range(4):
                if left[j]:
                    A[i, j] = A[i, j] - f * A[p, j]
            b[i] = b[i] - f * b[p]
    x = np.zeros(4)
    for k in range(len(perm) - 1, -1, -1):
        p = perm[k]
        acc = b[p]
        for t in range(k + 1, len(perm)):
            acc = acc - A[p, perm[t]] * x[perm[t]]
        x[p] = acc / A[p, p]
    return x


def fit(z, terms, x, y):
    return solve(*fit_sums(z, x, y), terms)


def remove(z, terms, coef, x, y):
    """pm_ifg_remove: a copy of z with the chosen terms taken off its finite pixels, the sum in double, the result rounded once"""
    z = np.asarray(z)
    fin = np.isfinite(z)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), z.shape)
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), z.shape)
    p = np.zeros(z.shape)
    if terms & TERM_X:
        p = p + coef[1] * x
    if terms & TERM_Y:
        p = p + coef[2] * y
    if terms & TERM_R2:
        p = p + coef[3] * (x * x + y * y)
    if terms & TERM_PISTON:
        p = p + coef[0]
    out = z.copy()
    out[fin] = (z.astype(np.float64) - p)[fin].astype(z.dtype)
    return out


# --------------------------------------------------------------------------- edits and slope
def fill(z, value):
    out = np.array(z)
    out[np.isnan(out)] = value
    return out


def mask(z, keep):
    out = np.array(z)
    out[~np.asarray(keep, dtype=bool)] = np.nan
    return out


def clip(z, nsigma, std):
    out = np.array(z)
    with np.errstate(invalid='ignore'):
        out[np.abs(out).astype(np.float64) > nsigma * std] = np.nan
    return out


def slope(z, dx):
    """pm_ifg_slope: (gx, gy, gr) -- np.gradient's arithmetic written out, every operation in z's type"""
    z = np.asarray(z)
    T = z.dtype.type
    d1, d2 = T(dx), T(2.0 * dx)

    def along(a):      # differences along axis 0
        g = np.empty_like(a)
        g[1:-1] = (a[2:] - a[:-2]) / d2
        g[0] = (a[1] - a[0]) / d1
        g[-1] = (a[-1] - a[-2]) / d1
        return g
    with np.errstate(invalid='ignore'):
        gy = along(z)
        gx = along(z.T).T
        return gx, gy, np.hypot(gx, gy)


# --------------------------------------------------------------------------- window and PSD
def hanning(n):
    """np.hanning's formula, [1] for one sample"""
    if n == 1:
        return np.ones(1)
    j = np.arange(n)
    return 0.5 + 0.5 * np.cos(np.pi * (1 - n + 2 * j).astype(np.float64) / float(n - 1))


def window(kind, shape, dx=0.0, alpha=4, dtype=np.float64, array=None):
    """the window of pm_ifg_window in double"""
    rows, cols = shape
    T = np.dtype(dtype).type
    if kind == WIN_HANN:
        return np.outer(hanning(rows), hanning(cols))
    if kind == WIN_ARRAY:
        return np.asarray(array).astype(np.float64)
    x = (np.arange(cols) - cols // 2).astype(T) * T(dx)
    y = (np.arange(rows) - rows // 2).astype(T) * T(dx)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.hypot(x[None, :], y[:, None]).astype(np.float64)
        rmax = float(np.hypot(T(0) * T(dx), y[-1]))
        return 1.0 - np.abs(r / rmax) ** float(alpha)


def windowed(height, w):
    """(height x window rounded once to height's type, S2)"""
    height = np.asarray(height)
    return (height.astype(np.float64) * w).astype(height.dtype), float((w * w).sum())


def psd_shifts(shape):
    """the rotation that is fftshift on the transform's input and ifftshift on its output, per axis: n - n // 2"""
    return tuple(n - n // 2 for n in shape)


def psd(height, dx, w):
    """the model of the whole of psd(): window, transform, |.|^2 and the division by S2 fs^2"""
    hw, s2 = windowed(height, w)
    ft = np.fft.ifftshift(np.fft.fft2(np.fft.fftshift(hw.astype(np.float64))))
    fs = 1.0 / dx
    return (np.abs(ft) ** 2 / (s2 * fs * fs)).astype(np.asarray(height).dtype)


# --------------------------------------------------------------------------- band-limited integral
def band_nu(shape, dx):
    """the generated frequency of pm_ifg_band in double: the radius of fftshift(fftfreq(n, dx)) along each axis"""
    rows, cols = shape
    ux, uy = 1.0 / (cols * dx), 1.0 / (rows * dx)
    return np.hypot((np.arange(cols) - cols // 2) * ux, ((np.arange(rows) - rows // 2) * uy)[:, None])


def _trapezoid_weights(n):
    i = np.arange(n)
    return 0.5 * ((i > 0).astype(np.float64) + (i < n - 1).astype(np.float64))


def band(psd_, nu, flow, fhigh):
    """pm_ifg_band: (integral, spacing) of a 2-D spectrum with 2-D frequencies, or of 1-D ones"""
    p = np.asarray(psd_).astype(np.float64)
    nu = np.asarray(nu).astype(np.float64)
    keep = ~((nu < flow) | (nu > fhigh))
    if p.ndim == 1:
        c = p.size // 2
        d = abs(nu[c - 1] - nu[c])
        return float((_trapezoid_weights(p.size) * p * keep).sum() * d), float(d)
    rows, cols = p.shape
    d = abs(nu[rows // 2 - 1, cols // 2] - nu[rows // 2, cols // 2])
    w = np.outer(_trapezoid_weights(rows), _trapezoid_weights(cols))
    return float((w * p * keep).sum() * d * d), float(d)


def band_limits(wllow, wlhigh, flow, fhigh):
    """the limits of bandlimited_rms from periods or frequencies (prysm/interferogram.py:214-241); an open upper limit is +inf, which
    keeps what the reference's r.max() keeps"""
    if wllow is not None or wlhigh is not None:
        if wllow is None:
            flow = 0
        else:
            fhigh = 1 / wllow
        if wlhigh is None:
            fhigh = math.inf
        else:
            flow = 1 / wlhigh
    elif flow is not None or fhigh is not None:
        if flow is None:
            flow = 0
        if fhigh is None:
            fhigh = math.inf
    else:
        raise ValueError('must specify either period (wavelength) or frequency')
    if flow is None:
        flow = 0
    if fhigh is None:
        fhigh = math.inf
    return float(flow), float(fhigh)


# --------------------------------------------------------------------------- filter design
def hann2d(M, N):
    """prysm/interferogram.py:547-558 in double"""
    n = (np.arange(N) - N // 2).astype(np.float64)[None, :]
    m = (np.arange(M) - M // 2).astype(np.float64)[:, None]
    nn = np.hypot(n, m)
    k = min(N, M)
    cw = np.cos(np.pi / float(k) * nn)
    w = cw * cw
    w[nn > float(k // 2)] = 0
    return w


def iir(r, dx, fcn, dtype=None):
    """pm_ifg_iir for one corner frequency: hann2d x jinc(r c) (fcn^2 pi / 2), c = pi fcn / dx, in double, rounded once"""
    r = np.asarray(r)
    dtype = r.dtype if dtype is None else dtype
    rho = r.astype(np.float64)
    cc = np.pi * fcn / dx
    h = jinc(rho * cc) * (fcn * fcn * np.pi / 2.0)
    return (hann2d(*r.shape) * h).astype(dtype)


def combine(typ, Hl, Hh=None):
    Hl = np.asarray(Hl)
    T = Hl.dtype.type
    if typ == LP:
        return Hl.copy()
    if typ == HP:
        return T(1) - Hl
    b = (T(1) - np.asarray(Hh)) + Hl
    return T(1) - b if typ == BP else b


def filter_type(typ):
    try:
        return FILTER_TYPES[typ.lower()]
    except KeyError:
        raise ValueError(f'unknown filter type {typ!r}') from None


def corner_frequencies(fc, typ, dx):
    """(fcn_low, fcn_high or None): the corner frequencies over Nyquist"""
    nyq = 1 / (2 * dx)
    if typ in (LP, HP):
        return float(fc) / nyq, None
    return float(fc[0]) / nyq, float(fc[1]) / nyq


def psd_model(kind, nu, a, b, c=0.0):
    nu = np.asarray(nu)
    T = nu.dtype.type
    with np.errstate(invalid='ignore', divide='ignore'):
        if kind == PSD_ABC:
            return T(a) / (T(1) + np.power((nu / T(b)).astype(np.float64), float(T(c))).astype(T))
        return T(a) * np.power(nu.astype(np.float64), float(-T(b))).astype(T)


# --------------------------------------------------------------------------- host logic of the Interferogram
def crop_box(rec, shape):
    """(row0, row1 + 1, col0, col1 + 1) of the bounding box in a record, or None when the reference's crop returns without cropping:
    the box is the whole array, or there is no finite value"""
    if rec[N] == 0:
        return None
    r0, r1, c0, c1 = (int(rec[k]) for k in (ROW0, ROW1, COL0, COL1))
    if r0 == 0 and c0 == 0 and r1 == shape[0] - 1 and c1 == shape[1] - 1:
        return None
    return r0, r1 + 1, c0, c1 + 1


def grid_default(shape, dx):
    """(origin row, origin column, step) of make_xy_grid(shape, dx=dx)"""
    return (shape[0] // 2, shape[1] // 2, dx)


def grid_current(explicit, shape, dx):
    """the grid in force: the explicit one, or -- coordinates never looked at -- make_xy_grid's on the current shape"""
    return explicit if explicit is not None else grid_default(shape, dx)


def grid_crop(explicit, r0, c0):
    """after a crop that starts at (r0, c0): an explicit grid keeps its origin, now r0 rows and c0 columns nearer; a grid never looked
    at stays unset and re-centres on the new shape, as the reference's does"""
    return None if explicit is None else (explicit[0] - r0, explicit[1] - c0, explicit[2])


def grid_recenter(explicit, shape, dx):
    return grid_default(shape, grid_current(explicit, shape, dx)[2])


def check_coord_shapes(xshape, yshape, shape):
    """coordinate arrays against the data's shape (rows, cols): vectors of cols and rows values, or two arrays of the data's shape.
    Anything else is a ValueError -- the kernels read x[c], y[r] or x[r, c] for every pixel and never broadcast"""
    rows, cols = shape
    xshape, yshape = tuple(xshape), tuple(yshape)
    if len(xshape) == 1 and len(yshape) == 1:
        if xshape != (cols,) or yshape != (rows,):
            raise ValueError(f'coordinate vectors of {xshape[0]} and {yshape[0]} values do not describe data of shape {(rows, cols)}')
    elif xshape != (rows, cols) or yshape != (rows, cols):
        raise ValueError(f'coordinate arrays of shapes {xshape} and {yshape} do not match data of shape {(rows, cols)}')


def pad_shape(shape, samples, out_shape):
    """the target shape of Interferogram.pad and the reference's two refusals (prysm/interferogram.py:951-960)"""
    if samples is None and out_shape is None:
        raise ValueError('Neither samples nor shape specified')
    if samples is not None and out_shape is not None:
        raise ValueError('Both samples and shape provided: only one can be given')
    if samples is not None:
        if isinstance(samples, int):
            samples = (samples, samples)
        return tuple(s + p for s, p in zip(shape, samples))
    if isinstance(out_shape, int):
        return (out_shape, out_shape)
    return tuple(out_shape)


def window_kind(which):
    """the kind of a named window, the reference's ValueError for an unknown name"""
    wl = which.lower()
    if wl == 'welch':
        return WIN_WELCH
    if wl in ('hann', 'hanning'):
        return WIN_HANN
    raise ValueError('unknown window type')


def corner_samples(shape):
    """rows and columns of the four corner blocks make_window(which=None) tests for zeros: round(2 %) of each axis"""
    return int(round(shape[0] * 0.02, 0)), int(round(shape[1] * 0.02, 0))
