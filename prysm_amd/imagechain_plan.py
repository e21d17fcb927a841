"""Host side of the image-chain unit (csrc/imagechain.hip), numpy only: the records its kernels walk, the deferred `spec` forms of the
analytic transfer functions, and every kernel restated in numpy -- operation by operation, in the precision of the launch, with the
unit's own jinc (the Chebyshev series of x/fibers_plan.py; for x <= 8 the series J1S is J1(x) / x itself, 0.5 at 0).

  Record / Spec        one factor of a transfer-function product / what `<function>.spec(...)` returns: a tuple of Records, no device work
  pack_records         Records and user maps -> the table pm_tf_product reads (RECORD_DTYPE, the layout of pm_tf_record)
  frequencies          the frequency of every input sample: generated from (dx, n, shift) as fttools.forward_ft_unit makes it -- the
                       bin's integer times 1 / (n dx) in double, rounded once -- or taken from vectors or arrays
  tf_product           pm_tf_product: the product in input order, then the index rotation that puts the origin at [0, 0]
  object_params        a target's kind, flags and parameters from the reference's arguments (argument errors raise here)
  object_render        pm_object_render
  polar_axes, polar_resample   uniform_cart_to_polar's axes and pm_polar_resample
  centroid, crossings, estimate_size   pm_centroid and the passes of pm_psf_size
"""
from collections import namedtuple

import numpy as np

from .x.fibers_plan import _cheb

(SINC_X, SINC_Y, COS_X, COS_Y, GAUSS_R, JINC_R, AIRY_FT_R, SLIT_FT, MAP_REAL, MAP_COMPLEX, AIRY_R, AIRY_EFIELD_R) = range(12)
FREQ_GRID, FREQ_VECTORS, FREQ_POINTWISE = 0, 1, 2
MAX_RECORDS = 16
SLIT, PINHOLE, SIEMENSSTAR, TILTEDSQUARE, SLANTEDEDGE = range(5)
SLIT_X, SLIT_Y, BINARY, CROSSED = 1, 2, 4, 8
COORDS_GRID, COORDS_SEPARABLE, COORDS_POINTWISE = 0, 1, 2

# pm_tf_record: int32 kind, flags; int64 ld; pointer; double p[4]
RECORD_DTYPE = np.dtype([('kind', '<i4'), ('flags', '<i4'), ('ld', '<i8'), ('ptr', '<u8'), ('p', '<f8', (4,))])
_NEEDS = {SINC_X: 'x', SINC_Y: 'y', COS_X: 'x', COS_Y: 'y', GAUSS_R: 'r', JINC_R: 'r', AIRY_FT_R: 'r', AIRY_R: 'r', AIRY_EFIELD_R: 'r',
          SLIT_FT: 'xy'}

Record = namedtuple('Record', 'kind flags p')


class Spec(namedtuple('Spec', 'name records')):
    """The deferred form of an analytic transfer function: its name and its factors.  Holds numbers only."""
    __slots__ = ()

    @property
    def needs(self):
        """which of the frequencies 'x', 'y', 'r' the factors read"""
        return ''.join(sorted(set(''.join(_NEEDS[r.kind] for r in self.records))))


def _rec(kind, *p, flags=0):
    p = tuple(float(v) for v in p)
    return Record(int(kind), int(flags), p + (0.0,) * (4 - len(p)))


# --------------------------------------------------------------------------- the spec of every analytic transfer function
def pixel_spec(width_x, width_y):
    return Spec('pixel_ft', (_rec(SINC_X, width_x), _rec(SINC_Y, width_y)))


def olpf_spec(width_x, width_y):
    return Spec('olpf_ft', (_rec(COS_X, 2 * width_x), _rec(COS_Y, 2 * width_y)))


def smear_spec(width, height):
    if width == 0 and height == 0:
        raise ValueError('one of width or height must be nonzero')
    recs = ([_rec(SINC_X, width)] if width != 0 else []) + ([_rec(SINC_Y, height)] if height != 0 else [])
    return Spec('smear_ft', tuple(recs))


def jitter_spec(scale):
    return Spec('jitter_ft', (_rec(GAUSS_R, np.pi * scale),))


def pinhole_spec(radius):
    return Spec('pinhole_ft', (_rec(JINC_R, radius * 2 * np.pi),))


def slit_spec(width_x, width_y):
    width_x, width_y = width_x or None, width_y or None
    if width_x is None and width_y is None:
        raise ValueError('slit_ft: at least one of width_x, width_y must be nonzero')
    flags = (SLIT_X if width_x is not None else 0) | (SLIT_Y if width_y is not None else 0)
    return Spec('slit_ft', (_rec(SLIT_FT, width_x or 0.0, width_y or 0.0, flags=flags),))


def airydisk_ft_spec(fno, wavelength):
    return Spec('airydisk_ft', (_rec(AIRY_FT_R, 1 / (wavelength * fno)),))


def airydisk_spec(fno, wavelength, efield=False):
    return Spec('airydisk_efield' if efield else 'airydisk', (_rec(AIRY_EFIELD_R if efield else AIRY_R, wavelength, fno),))


def flatten(tfs):
    """Specs and arrays -> a list of Records and arrays in order; more than MAX_RECORDS factors is a ValueError"""
    out = []
    for tf in tfs:
        if isinstance(tf, Spec):
            out.extend(tf.records)
        elif isinstance(tf, Record):
            out.append(tf)
        else:
            out.append(tf)
    if len(out) > MAX_RECORDS:
        raise ValueError(f'a transfer-function product takes at most {MAX_RECORDS} factors, got {len(out)}')
    return out


def pack_records(factors, maps=()):
    """The table of a product.  factors: Records, and for each user map a (kind, ld, address) triple with kind MAP_REAL / MAP_COMPLEX"""
    t = np.zeros(len(factors), RECORD_DTYPE)
    for i, f in enumerate(factors):
        if isinstance(f, Record):
            t[i]['kind'], t[i]['flags'], t[i]['p'] = f.kind, f.flags, f.p
        else:
            kind, ld, address = f
            if kind not in (MAP_REAL, MAP_COMPLEX):
                raise ValueError('a map factor is (MAP_REAL or MAP_COMPLEX, ld, address)')
            t[i]['kind'], t[i]['ld'], t[i]['ptr'] = kind, ld, address
    return t


# --------------------------------------------------------------------------- special functions
def jinc(x):
    """J1(x) / x in x's precision (float32 or float64), 0.5 at 0, even"""
    x = np.asarray(x)
    T = x.dtype.type
    ax = np.abs(x).reshape(-1)
    out = np.empty_like(ax)
    small = ax <= T(8)
    if small.any():
        xs = ax[small]
        out[small] = _cheb('J1S', xs * xs * T(0.03125) - T(1))
    if (~small).any():
        xl = ax[~small]
        z = T(8) / xl
        t = T(2) * (z * z) - T(1)
        s, c = np.sin(xl), np.cos(xl)
        amp = np.sqrt(T(0.6366197723675814) / xl)
        c0, s0 = (c + s) * T(0.7071067811865476), (s - c) * T(0.7071067811865476)
        out[~small] = amp * (_cheb('P1', t) * s0 + z * _cheb('Q1', t) * c0) / xl
    out[ax < T(1e-8)] = T(0.5)        # as the reference sets it; the series gives 0.5 there to within one rounding
    return out.reshape(x.shape)


def _sinc(a):
    T = a.dtype.type
    y = T(np.pi) * np.where(a == 0, T(1), a)
    return np.where(a == 0, T(1), np.sin(y) / y)


# --------------------------------------------------------------------------- frequencies and the product
def gen_axis(dx, n, shift, dtype):
    """forward_ft_unit(dx, n, shift) in dtype: element i of the INPUT order"""
    s = n // 2 if shift else 0
    o = (np.arange(n) - s) % n
    k = np.where(o < (n + 1) // 2, o, o - n)
    return (k.astype(np.float64) * (1.0 / (float(n) * dx))).astype(dtype)


def frequencies(shape, dtype, *, dx=None, shift=False, fx=None, fy=None, fr=None):
    """(FX, FY, FR) of every input sample, broadcastable to shape; FR is None until a factor needs it"""
    m, n = shape
    if dx is not None:
        return gen_axis(dx, n, shift, dtype).reshape(1, n), gen_axis(dx, m, shift, dtype).reshape(m, 1), None
    conv = lambda a: None if a is None else np.asarray(a, dtype)       # noqa: E731
    fx, fy, fr = conv(fx), conv(fy), conv(fr)
    if fx is not None and fx.ndim == 1:
        fx = fx.reshape(1, n)
    if fy is not None and fy.ndim == 1:
        fy = fy.reshape(m, 1)
    return fx, fy, fr


def _factor(rec, T, FX, FY, FRf):
    p = [T(v) for v in rec.p]
    k = rec.kind
    if k == SINC_X:
        return _sinc(FX * p[0])
    if k == SINC_Y:
        return _sinc(FY * p[0])
    if k == COS_X:
        return np.cos(p[0] * FX)
    if k == COS_Y:
        return np.cos(p[0] * FY)
    if k == GAUSS_R:
        core = p[0] * FRf()
        return np.exp(T(-2) * core * core)
    if k == JINC_R:
        return jinc(FRf() * p[0])
    if k == AIRY_FT_R:
        s = np.minimum(np.abs(FRf()) / p[0], T(1))
        return T(2 / np.pi) * (np.arccos(s) - s * np.sqrt(T(1) - s * s))
    if k in (AIRY_R, AIRY_EFIELD_R):
        e = T(2) * jinc(FRf() * T(np.pi) / p[0] / p[1])
        return np.abs(e) * np.abs(e) if k == AIRY_R else e
    if k == SLIT_FT:
        wx, wy = p[0], p[1]
        if rec.flags == (SLIT_X | SLIT_Y):
            fx0, fy0 = np.broadcast_to(FX, FRf().shape), np.broadcast_to(FY, FRf().shape)
            Lx, Ly = T(1) / (fx0[0, 1] - fx0[0, 0]), T(1) / (fy0[1, 0] - fy0[0, 0])
            sx, sy = _sinc(FX * wx), _sinc(FY * wy)
            bx, by = (wx * Ly) * sx * (FY == 0).astype(T), (wy * Lx) * sy * (FX == 0).astype(T)
            ov = T(rec.p[0] * rec.p[1]) * sx * sy
            area = wx * Ly + wy * Lx - T(rec.p[0] * rec.p[1])
            return (bx + by - ov) / area
        if rec.flags == SLIT_X:
            return _sinc(FX * wx) * (FY == 0).astype(T)
        return _sinc(FY * wy) * (FX == 0).astype(T)
    raise ValueError(f'unknown record kind {k}')


def tf_product(shape, factors, dtype, *, dx=None, shift=False, fx=None, fy=None, fr=None, out_complex=True):
    """pm_tf_product in numpy.  factors: Records and arrays (in input order, like the frequencies); the result has its origin at [0, 0]"""
    m, n = shape
    T = np.dtype(dtype).type
    FX, FY, FR = frequencies(shape, dtype, dx=dx, shift=shift, fx=fx, fy=fy, fr=fr)
    cache = {}

    def FRf():
        if 'r' not in cache:
            cache['r'] = np.broadcast_to(FR if FR is not None else np.hypot(FX, FY), (m, n))
        return cache['r']

    re, im = np.ones((m, n), T), np.zeros((m, n), T)
    for f in flatten(factors):
        if isinstance(f, Record):
            v = np.broadcast_to(_factor(f, T, FX, FY, FRf), (m, n)).astype(T)
            re, im = re * v, im * v
            continue
        a = np.asarray(f)
        if np.iscomplexobj(a):
            wr, wi = a.real.astype(T), a.imag.astype(T)
            re, im = re * wr - im * wi, re * wi + im * wr
        else:
            v = a.astype(T)
            re, im = re * v, im * v
    if shift:
        re, im = np.roll(re, (-(m // 2), -(n // 2)), (0, 1)), np.roll(im, (-(m // 2), -(n // 2)), (0, 1))
    return re + 1j * im if out_complex else re


# --------------------------------------------------------------------------- targets
def _background(background):
    b = background.lower()
    if b in ('b', 'black'):
        return 0.0
    if b in ('w', 'white'):
        return 1.0
    raise ValueError('invalid background color')


def object_params(kind, **kw):
    """(kind, flags, p) of a target from the reference's arguments; the argument errors of the reference raise here, before any launch"""
    if kind == SLIT:
        wx, wy = kw['width_x'], kw['width_y']
        flags = (SLIT_X if wx is not None else 0) | (SLIT_Y if wy is not None else 0)
        return kind, flags, (0.0 if wx is None else wx / 2, 0.0 if wy is None else wy / 2)
    if kind == PINHOLE:
        return kind, 0, (float(kw['radius']),)
    if kind == SIEMENSSTAR:
        bg = _background(kw['background'])
        contrast = kw['contrast']
        delta = (1 - contrast) / 2
        return kind, (0 if kw['sinusoidal'] else BINARY), (kw['spokes'] / 2, contrast, kw['oradius'], kw['iradius'], bg, delta, 1 - delta)
    if kind == TILTEDSQUARE:
        background = kw['background'].lower()
        delta = (1 - kw['contrast']) / 2
        a = np.radians(kw['angle'])
        inside, outside = (delta, 1 - delta) if background in ('w', 'white') else (1 - delta, delta)
        return kind, 0, (float(np.cos(a)), float(np.sin(a)), kw['radius'], inside, outside)
    if kind == SLANTEDEDGE:
        diff = (1 - kw['contrast']) / 2
        a = np.radians(kw['angle'])
        return kind, (CROSSED if kw['crossed'] else 0), (float(np.cos(a)), float(np.sin(a)), diff, 1 - diff)
    raise ValueError(f'unknown target kind {kind}')


def grid_axes(shape, dx, dtype):
    """the coordinates PM_COORDS_GRID generates: make_xy_grid's vectors"""
    ny, nx = shape
    T = np.dtype(dtype).type
    return (np.arange(nx) - nx // 2).astype(T) * T(dx), (np.arange(ny) - ny // 2).astype(T) * T(dx)


def _star(r, t, p, flags, C):
    """the Siemens star at (r, t), computed in C with the parameters p as the launch rounded them"""
    p = [C(v) for v in p]
    arr = p[1] * np.cos(p[0] * t)
    arr = (arr + C(1)) / C(2)
    arr = np.where((r > p[2]) | (r < p[3]), p[4], arr)
    if flags & BINARY:
        arr = np.where(arr < C(0.5), p[5], arr)
        arr = np.where(arr > C(0.5), p[6], arr)
    return arr


def object_render(kind, flags, p, a, b, dtype, polar=False):
    """pm_object_render in numpy.  a, b: 2-D arrays (or broadcastable row / column) of x, y -- or of r, t when polar"""
    T = np.dtype(dtype).type
    p = [T(v) for v in p]
    a = None if a is None else np.asarray(a, T)
    b = None if b is None else np.asarray(b, T)
    if kind == SLIT:
        shape = np.broadcast_shapes(a.shape, b.shape)
        m = np.zeros(shape, bool)
        if flags & SLIT_X:
            m = m | (np.abs(a) <= p[0])
        if flags & SLIT_Y:
            m = m | (np.abs(b) <= p[1])
        return m
    if kind == PINHOLE:
        # polar coordinates formed in registers are formed, and used, in double whatever the working precision
        return a <= p[0] if polar else np.hypot(a.astype(np.float64), b.astype(np.float64)) <= np.float64(p[0])
    if kind == SIEMENSSTAR:
        if polar:
            return _star(a, b, p, flags, T).astype(T)
        a64, b64 = np.broadcast_arrays(a.astype(np.float64), b.astype(np.float64))
        return _star(np.hypot(a64, b64), np.arctan2(b64, a64), p, flags, np.float64).astype(T)
    a, b = np.broadcast_arrays(a, b)
    if kind == TILTEDSQUARE:
        xp, yp = a * p[0] - b * p[1], a * p[1] + b * p[0]
        return np.where((np.abs(xp) <= p[2]) & (np.abs(yp) <= p[2]), p[3], p[4]).astype(T)
    m = a * p[0] - b * p[1] > 0
    if flags & CROSSED:
        if m.shape[0] != m.shape[1]:
            raise ValueError('crossed edges need a square grid')
        ur = m & np.rot90(m)
        m = ur | np.rot90(ur, 2)
    return np.where(m, p[2], p[3]).astype(T)


def decision_margin(kind, flags, p, a, b, dtype, polar=False):
    """|decision variable - threshold| and its 8 eps (1 + |variable|) band per sample, the smallest over the target's decisions: where the
    first is below the second a comparison may exclude the sample"""
    T = np.float64
    eps = float(np.finfo(dtype).eps)
    a = None if a is None else np.asarray(a, T)
    b = None if b is None else np.asarray(b, T)
    near = None

    def add(var, thr):
        nonlocal near
        n = np.abs(var - thr) <= 8 * eps * (1 + np.abs(var))
        near = n if near is None else (near | n)

    if kind == SLIT:
        if flags & SLIT_X:
            add(np.abs(a) + 0 * b, p[0])
        if flags & SLIT_Y:
            add(np.abs(b) + 0 * a, p[1])
    elif kind == PINHOLE:
        add(a if polar else np.hypot(a, b), p[0])
    elif kind == SIEMENSSTAR:
        r, t = (a, b) if polar else (np.hypot(a, b), np.arctan2(b + 0 * a, a + 0 * b))
        add(r, p[2])
        add(r, p[3])
        if flags & BINARY:
            add(np.cos(p[0] * t), 0.0)
    else:
        a, b = np.broadcast_arrays(a, b)
        xp, yp = a * p[0] - b * p[1], a * p[1] + b * p[0]
        if kind == TILTEDSQUARE:
            add(np.abs(xp), p[2])
            add(np.abs(yp), p[2])
        else:
            add(xp, 0.0)
            if flags & CROSSED:
                near = near | np.rot90(near)
                near = near | np.rot90(near, 2)
    return near


# --------------------------------------------------------------------------- uniform_cart_to_polar
def polar_axes(x, y):
    """(rho, phi, _max): linspace(0, max|extremes|, len(x)) and linspace(0, 2 pi, len(y)) in float64, as the reference builds them"""
    x, y = np.asarray(x), np.asarray(y)
    _max = max(abs(np.asarray([x.min(), x.max(), y.min(), y.max()])))
    return np.linspace(0, _max, len(x)), np.linspace(0, 2 * np.pi, len(y)), float(_max)


def _cell(g, q):
    return np.clip(np.searchsorted(g, q, side='right') - 1, 0, len(g) - 2)


def polar_resample(x, y, data, dtype):
    """pm_polar_resample in numpy: (rho, phi, polar) with the axes rounded to dtype"""
    T = np.dtype(dtype).type
    x, y, data = np.asarray(x, T).reshape(-1), np.asarray(y, T).reshape(-1), np.asarray(data, T)
    rho, phi, _ = polar_axes(x, y)
    rho, phi = rho.astype(T), phi.astype(T)
    rv, pv = rho.reshape(1, -1), phi.reshape(-1, 1)
    xq, yq = rv * np.cos(pv), rv * np.sin(pv)
    inside = (xq >= x[0]) & (xq <= x[-1]) & (yq >= y[0]) & (yq <= y[-1])
    ix, iy = _cell(x, xq), _cell(y, yq)
    tx, ty = (xq - x[ix]) / (x[ix + 1] - x[ix]), (yq - y[iy]) / (y[iy + 1] - y[iy])
    ux, uy = T(1) - tx, T(1) - ty
    v = data[iy, ix] * (uy * ux)
    v = v + data[iy, ix + 1] * (uy * tx)
    v = v + data[iy + 1, ix] * (ty * ux)
    v = v + data[iy + 1, ix + 1] * (ty * tx)
    return rho, phi, np.where(inside, v, T(0)).astype(T)


# --------------------------------------------------------------------------- centroid and sizes
def centroid(data):
    """pm_centroid: (sum row d / sum d, sum col d / sum d) in double"""
    d = np.asarray(data, np.float64)
    s = d.sum()
    return float((np.arange(d.shape[0])[:, None] * d).sum() / s), float((np.arange(d.shape[1])[None, :] * d).sum() / s)


METRICS = {'fwhm': 0.5, '1/e': 1 / np.e, '1/e^2': 1 / (np.e ** 2)}


def size_threshold(metric):
    """(relative, value) of a metric name or number; ValueError for anything else"""
    import numbers
    if isinstance(metric, str):
        if metric.lower() not in METRICS:
            raise ValueError('unknown metric, use fwhm, 1/e, or 1/e^2')
        return 1, METRICS[metric.lower()]
    if isinstance(metric, numbers.Number):
        return 0, float(metric)
    raise ValueError('unknown metric, use fwhm, 1/e, or 1/e^2')


def size_criteria(criteria):
    criteria = criteria.lower()
    if criteria not in ('first', 'last'):
        raise ValueError('unknown criteria, use first or last')
    return int(criteria == 'last')


def crossings(polar, r, hm, last):
    """the crossing pass of pm_psf_size: (radius per row, 1.0 where the row crosses)"""
    p = np.asarray(polar)
    T = p.dtype.type
    hm = T(hm)
    change = (p[:, :-1] > hm) != (p[:, 1:] > hm)
    has = change.any(axis=1)
    i = (change.shape[1] - 1 - np.argmax(change[:, ::-1], axis=1)) if last else np.argmax(change, axis=1)
    rows = np.arange(p.shape[0])
    y0, y1 = p[rows, i], p[rows, i + 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(y1 == y0, T(0), (hm - y0) / (y1 - y0))
    r = np.asarray(r, T).astype(np.float64)
    rc = r[i] + frac.astype(np.float64) * (r[i + 1] - r[i])
    return np.where(has, rc, 0.0), has.astype(np.float64)


def estimate_size(polar, r, metric, criteria='last'):
    """pm_psf_size: (mean crossing radius, count)"""
    relative, value = size_threshold(metric)
    last = size_criteria(criteria)
    p = np.asarray(polar)
    T = p.dtype.type
    hm = T(value) * T(p.max()) if relative else T(value)
    rc, has = crossings(p, r, hm, last)
    n = has.sum()
    return (float(rc.sum() / n) if n else 0.0), float(n)
