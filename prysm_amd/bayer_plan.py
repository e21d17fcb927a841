"""csrc/bayer.hip in numpy: the CPU-checkable statement of what the Bayer kernels compute (prysm/bayer.py).

The same weights (the reference's tables divided by 8), the same reflect rule, the same order of every sum and the same `ratio` rule.
Plain numpy slices and loops; every product and sum is rounded by itself in the array's precision, as in the kernels (their unit is
compiled without multiply-add contraction), so results are bit-equal.
"""
import numpy as np

CFAS = ('rggb', 'bggr')

kernel_G_at_R_or_B = [
    [0, 0, -1, 0, 0],
    [0, 0, 2, 0, 0],
    [-1, 2, 4, 2, -1],
    [0, 0, 2, 0, 0],
    [0, 0, -1, 0, 0],
]
kernel_R_at_G_in_RB = [
    [0, 0, .5, 0, 0],
    [0, -1, 0, -1, 0],
    [-1, 4, 5, 4, -1],
    [0, -1, 0, -1, 0],
    [0, 0, .5, 0, 0],
]
kernel_R_at_G_in_BR = [
    [0, 0, -1, 0, 0],
    [0, -1, 4, -1, 0],
    [.5, 0, 5, 0, .5],
    [0, -1, 4, -1, 0],
    [0, 0, -1, 0, 0],
]
kernel_R_at_B_in_BB = [
    [0, 0, -3 / 2, 0, 0],
    [0, 2, 0, 2, 0],
    [-3 / 2, 0, 6, 0, -3 / 2],
    [0, 2, 0, 2, 0],
    [0, 0, -3 / 2, 0, 0],
]


def cfa_code(cfa):
    """0 for 'rggb', 1 for 'bggr' (any case); None for anything else"""
    cfa = cfa.lower() if isinstance(cfa, str) else cfa
    return CFAS.index(cfa) if cfa in CFAS else None


def reflect_index(i, n):
    """scipy's mode='reflect' on an axis of length n: j = i mod 2n; j >= n ? 2n - 1 - j : j (the edge sample is repeated)"""
    j = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(j >= n, 2 * n - 1 - j, j)


def _filter(pad, table, m, n):
    """One running sum that starts at 0 over the non-zero taps of `table` / 8 in row-major order, on a 2-sample reflect-padded image"""
    dt = pad.dtype.type
    acc = np.zeros((m, n), dtype=pad.dtype)
    for dy in range(5):
        for dx in range(5):
            w = table[dy][dx] / 8.
            if w != 0:
                acc = acc + dt(w) * pad[dy:dy + m, dx:dx + n]
    return acc


def demosaic_malvar(img, cfa='rggb', precision=np.float64):
    """(m, n) -> (m, n, 3) R, G, B.  A float mosaic keeps its dtype, an integer one is converted to `precision` first."""
    code = cfa_code(cfa)
    if code is None:
        raise NotImplementedError('only rggb, bggr bayer patterns currently implemented')
    img = np.asarray(img)
    if img.dtype.kind != 'f':
        img = img.astype(precision)
    m, n = img.shape
    pad = img[reflect_index(np.arange(-2, m + 2), m)][:, reflect_index(np.arange(-2, n + 2), n)]
    g = _filter(pad, kernel_G_at_R_or_B, m, n)
    h = _filter(pad, kernel_R_at_G_in_RB, m, n)      # the like colour left and right
    v = _filter(pad, kernel_R_at_G_in_BR, m, n)      # above and below
    d = _filter(pad, kernel_R_at_B_in_BB, m, n)
    py, px = np.indices((m, n)) & 1
    site = py == px
    first = np.where(site, np.where(py == 0, img, d), np.where(py == 0, h, v))      # the colour of the (even, even) sites
    second = np.where(site, np.where(py == 0, d, img), np.where(py == 0, v, h))
    green = np.where(site, g, img)
    red, blue = (first, second) if code == 0 else (second, first)
    return np.stack((red, green, blue), axis=2)


def _parity_planes(r, g1, g2, b, cfa):
    code = cfa_code(cfa)
    if code is None:
        raise NotImplementedError('only rggb, bggr bayer patterns currently implemented')
    return (r, g1, g2, b) if code == 0 else (b, g1, g2, r)


def composite(r, g1, g2, b, cfa='rggb'):
    """out[r][c] = plane(parity)[r][c]"""
    planes = _parity_planes(r, g1, g2, b, cfa)
    out = np.empty_like(np.asarray(r))
    for k, p in enumerate(planes):
        out[k // 2::2, k % 2::2] = np.asarray(p)[k // 2::2, k % 2::2]
    return out


def recomposite(r, g1, g2, b, cfa='rggb'):
    """out[2i + py][2j + px] = plane(parity)[i][j]"""
    planes = _parity_planes(r, g1, g2, b, cfa)
    m, n = np.asarray(r).shape
    out = np.empty((2 * m, 2 * n), dtype=np.asarray(r).dtype)
    for k, p in enumerate(planes):
        out[k // 2::2, k % 2::2] = p
    return out


def decomposite(img, cfa='rggb'):
    """the four stride-2 views r, g1, g2, b"""
    code = cfa_code(cfa)
    if code is None:
        raise NotImplementedError('only rggb, bggr bayer patterns currently implemented')
    a, g1, g2, d = img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2]
    return (a, g1, g2, d) if code == 0 else (d, g1, g2, a)


def deinterlace(img, cfa='rggb'):
    r, g1, g2, b = decomposite(np.asarray(img), cfa)
    return np.stack([r, (g1 + g2) / img.dtype.type(2), b], axis=2)


def assemble(r, g1, g2, b):
    """the last sweep of assemble_superresolved: r, (g2 + g1) / 2, b"""
    r = np.asarray(r)
    return np.stack([r, (np.asarray(g2) + np.asarray(g1)) / r.dtype.type(2), np.asarray(b)], axis=2)


def safe_gains(maxima, gains, saturation, dtype):
    """The gains divided by the reference's ratio, every operation in `dtype`: ratio = 1; per class, in order, rat = max * gain / sat,
    taken when rat > 1 and rat > ratio."""
    dt = np.dtype(dtype).type
    w = [dt(g) for g in gains]
    ratio = dt(1)
    for mx, g, s in zip(maxima, w, saturation):
        rat = dt(mx) * g / dt(s)
        if rat > 1 and rat > ratio:
            ratio = rat
    return [g / ratio for g in w], ratio


def check_saturation(safe, saturation, count):
    """the reference's checks (bayer.py:37-49, 98-110); returns the list of `count` saturations, or None when not safe"""
    if not safe:
        return None
    if saturation is None:
        raise ValueError('When doing safe WB prescaling, saturation must be not-none')
    if not hasattr(saturation, '__iter__'):
        saturation = [saturation] * count
    else:
        saturation = list(saturation)
        if len(saturation) != count:
            raise ValueError('saturation must be scalar or contain %s values' % ('four' if count == 4 else 'three'))
    if any(s <= 0 for s in saturation):
        raise ValueError('saturation must be positive')
    return [float(s) for s in saturation]


def wb_prescale(mosaic, wr, wg1, wg2, wb, cfa='rggb', safe=False, saturation=None):
    """a scaled COPY of the mosaic (the reference scales in place)"""
    saturation = check_saturation(safe, saturation, 4)
    out = np.array(mosaic, copy=True)
    dt = out.dtype.type
    planes = decomposite(out, cfa)
    w = [dt(x) for x in (wr, wg1, wg2, wb)]
    if safe:
        w, _ = safe_gains([p.max() for p in planes], w, saturation, out.dtype)
    for p, g in zip(planes, w):
        p *= g
    return out


def wb_postscale(rgb, wr, wg, wb, safe=False, saturation=None):
    """a scaled COPY of the (..., 3) image"""
    saturation = check_saturation(safe, saturation, 3)
    out = np.array(rgb, copy=True)
    dt = out.dtype.type
    w = [dt(x) for x in (wr, wg, wb)]
    if safe:
        w, _ = safe_gains([out[..., i].max() for i in range(3)], w, saturation, out.dtype)
    for i in range(3):
        out[..., i] *= w[i]
    return out


def fourier_shift_vectors(shape, shift, dtype=np.float64):
    """ndimage.fourier_shift's multiplier as its two separable factors: exp(-2 pi i shift f), f = fftfreq(N), per axis"""
    cdt = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    return tuple(np.exp(-2j * np.pi * float(s) * np.fft.fftfreq(n)).astype(cdt) for n, s in zip(shape, shift))


# the shifts of assemble_superresolved for 'rggb' (bayer.py:312-315), as (rows, cols)
def superres_shifts(zoomfactor):
    return dict(r=(-zoomfactor, 0), b=(0, zoomfactor), g2=(-zoomfactor, zoomfactor))


def assemble_superresolved(r, g1, g2, b, zoomfactor):
    r = np.asarray(r)
    sh = superres_shifts(zoomfactor)
    moved = {}
    for name, p in (('r', r), ('b', b), ('g2', g2)):
        hy, hx = fourier_shift_vectors(r.shape, sh[name], r.dtype)
        moved[name] = np.fft.ifft2(np.fft.fft2(np.asarray(p)) * (hy[:, None] * hx[None, :])).real.astype(r.dtype)
    return assemble(moved['r'], g1, moved['g2'], moved['b'])
