"""What tests/test_imagechain_host.py, tests/test_gpu_imagechain.py and tests/golden/make_golden_imagechain.py share: the grids, the
cases, access to tests/golden/imagechain.npz and the bounds.  Imports without a GPU.

Grids.  SHAPES 'a' = (33, 47) and 'b' = (130, 257): odd and even sizes, non-square, columns no multiple of 64; 'c' = (64, 64) for the
crossed edge.  x = (arange(nx) - nx // 2) (2 / nx), y = (arange(ny) - ny // 2) (2 / nx); frequencies are forward_ft_unit(DX, n) with
DX = 0.5.  Maps of grid 'b' are stored at the flat indices `b_idx` (every 11th sample plus the rows and columns through zero
frequency): whole maps would be 2.7 MB.

Targets.  TARGETS are the five inputs for which the reference on float32 and on float64 coordinates agrees on every sample of grids 'a'
and 'b' (the generator prints the counts), so no sample needs excluding from the reference's side.  A comparison may still exclude a
sample whose decision variable lies within 8 eps (1 + |variable|) of its threshold (imagechain_plan.decision_margin); the samples so
excused -- those that differ -- are at most 0.5 % of the map (EXCLUDE_CAP).  The band itself is wider on these grids: the star's cosine
is zero along the diagonals (2 % of grid 'a'), where the reference's two precisions nevertheless agree.

Bounds, absolute, eps that of the precision under test (every factor is at most 1 in magnitude):
  analytic factor      16 eps (1 + max|argument|), the argument that of its transcendental function: pi f w for a sinc, 2 w f for the
                       filter's cosine, 2 (pi scale fr)^2 for the Gaussian, 2 pi radius fr for jinc, pi r / (wavelength fno) for the
                       Airy pattern, s <= 1 for the Airy transform.  Bounds sum over the factors of a product (tf_bound).
  airydisk             two factors (the square of 2 jinc <= 1); slit_ft with both widths four (two sincs in each of its band and overlap
                       terms, normalised by the area).
  The generator measures the float64 model against the reference and prints measured / bound per function; every function meets the
  form, none took the four-times-measured route (see its printout, copied to DESIGN.md).
  uniform_cart_to_polar   per sample max|grad data| dx 16 eps n + 16 eps max|data| (polar_bound); samples within 8 eps _max of the
                       grid's outer boundary may be excluded, at most 1 % of the map.
  sizes                the float32 model's deviation from the float64 reference, times four (stored by the generator as size_dev32);
                       float64: the resample bound over the slope at the crossing (size_bound64).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'imagechain.npz')
SHAPES = {'a': (33, 47), 'b': (130, 257), 'c': (64, 64)}
DX = 0.5
EXCLUDE_CAP = 0.005
POLAR_EXCLUDE_CAP = 0.01
PSF_SHAPE = (65, 64)
PSF_CENTRE = (0.1, -0.05)
PSF_SIGMA = 0.2
AIRY_FNO, AIRY_WVL, AIRY_SCALE = 4.0, 0.55, 14.0
AIRY_LEVEL = 0.01
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def eps(dt):
    return float(np.finfo(dt).eps)


def grid_vectors(tag, dtype=np.float64):
    ny, nx = SHAPES[tag]
    x = (np.arange(nx) - nx // 2) * (2 / nx)
    y = (np.arange(ny) - ny // 2) * (2 / nx)
    return x.astype(dtype), y.astype(dtype)


def grid_dx(tag):
    return 2 / SHAPES[tag][1]


def grid_xy(tag, dtype=np.float64):
    x, y = grid_vectors(tag, dtype)
    return np.meshgrid(x, y)


def polar_of(x, y):
    return np.hypot(x, y), np.arctan2(y, x)


def freq_vectors(tag, dtype=np.float64):
    ny, nx = SHAPES[tag]
    fx = np.fft.fftshift(np.fft.fftfreq(nx, DX))
    fy = np.fft.fftshift(np.fft.fftfreq(ny, DX))
    return fx.astype(dtype), fy.astype(dtype)


def sub_index(tag):
    """flat indices of the samples stored for a grid: all of 'a' and 'c'; of 'b' every 11th plus the zero-frequency row and column"""
    ny, nx = SHAPES[tag]
    if tag != 'b':
        return np.arange(ny * nx)
    idx = set(range(0, ny * nx, 11))
    idx |= {(ny // 2) * nx + j for j in range(nx)} | {i * nx + nx // 2 for i in range(ny)}
    return np.array(sorted(idx))


# ---------------------------------------------------------------------------- targets
# name -> (function, coordinates 'polar' / 'cart' / 'rho', positional arguments after the coordinates, keywords)
TARGETS = {
    'siemensstar': ('siemensstar', 'polar', (36,), dict(oradius=0.8, iradius=0.1)),
    'tiltedsquare': ('tiltedsquare', 'cart', (), dict(angle=4, radius=0.37)),
    'slantededge': ('slantededge', 'cart', (), dict(angle=4)),
    'pinhole': ('pinhole', 'rho', (0.33,), {}),
    'slit': ('slit', 'cart', (0.21, 0.4), {}),
}
# more of the reference's behaviour, float64 only: the sinusoidal star on a white background, a white binary star, a black square
EXTRA_TARGETS = {
    'siemens_sin_white': ('siemensstar', 'polar', (36,), dict(oradius=0.8, iradius=0.1, background='white', sinusoidal=True)),
    'siemens_white': ('siemensstar', 'polar', (36,), dict(oradius=0.8, iradius=0.1, background='w', contrast=0.7)),
    'tiltedsquare_black': ('tiltedsquare', 'cart', (), dict(angle=-11, radius=0.37, background='black')),
    'slit_x': ('slit', 'cart', (0.21, None), {}),
}


def call_target(mod, name, x, y, spec=None):
    """the target `name` from module `mod` (the reference's objects or prysm_amd.objects) on meshgrids x, y"""
    fn, kind, args, kw = spec or {**TARGETS, **EXTRA_TARGETS}[name]
    f = getattr(mod, fn)
    if kind == 'polar':
        r, t = polar_of(x, y)
        return f(r, t, *args, **kw)
    if kind == 'rho':
        return f(args[0], np.hypot(x, y))
    return f(x, y, *args, **kw)


def target_params(name):
    """(kind, flags, p) of a target of TARGETS / EXTRA_TARGETS, through imagechain_plan.object_params with the reference's defaults"""
    from prysm_amd import imagechain_plan as IP
    fn, kind, args, kw = {**TARGETS, **EXTRA_TARGETS}[name]
    k = {'siemensstar': IP.SIEMENSSTAR, 'tiltedsquare': IP.TILTEDSQUARE, 'slantededge': IP.SLANTEDEDGE, 'pinhole': IP.PINHOLE,
         'slit': IP.SLIT}[fn]
    defaults = {IP.SIEMENSSTAR: dict(oradius=0.9, iradius=0, background='black', contrast=0.9, sinusoidal=False),
                IP.TILTEDSQUARE: dict(angle=4, radius=0.5, contrast=0.9, background='white'),
                IP.SLANTEDEDGE: dict(angle=4, contrast=0.9, crossed=False), IP.PINHOLE: {}, IP.SLIT: {}}[k]
    named = {IP.SIEMENSSTAR: ('spokes',), IP.PINHOLE: ('radius',), IP.SLIT: ('width_x', 'width_y')}.get(k, ())
    return IP.object_params(k, **{**defaults, **dict(zip(named, args)), **kw})


def target_margin(name, tag, dt, form='arrays'):
    """what compare_target needs for a target on a grid: (params, a, b, polar), the coordinates as the form hands them over"""
    kind = {**TARGETS, **EXTRA_TARGETS}[name][1]
    x, y = grid_xy(tag, dt)
    if kind == 'cart' or form != 'arrays':
        return target_params(name), x, y, False
    r, t = polar_of(x, y)
    return target_params(name), r, t, True


def target_model(name, tag, dt, form='arrays'):
    """the numpy model of a target on one of the coordinate forms, and its target_margin"""
    from prysm_amd import imagechain_plan as IP
    params, a, b, polar = margin = target_margin(name, tag, dt, form)
    return IP.object_render(*params, a, b, dt, polar=polar), margin


def compare_target(got, ref, margin_args, dt):
    """got == ref on every sample, except that a sample whose decision variable sits within 8 eps (1 + |variable|) of its threshold may
    differ; the samples so excused are at most 0.5 % of the map"""
    from prysm_amd import imagechain_plan as IP
    params, a, b, polar = margin_args
    near = IP.decision_margin(*params, a, b, dt, polar=polar)
    near = np.zeros(got.shape, bool) if near is None else np.broadcast_to(near, got.shape)
    bad = (got != ref) if got.dtype == bool else (np.abs(got.astype(np.float64) - ref) > 4 * eps(dt))
    assert not (bad & ~near).any(), int((bad & ~near).sum())
    assert bad.mean() <= EXCLUDE_CAP, bad.mean()


# ---------------------------------------------------------------------------- transfer functions
# name -> (module, function, which frequencies in call order, arguments, [(argument scale of a factor, axis)], factors counted)
SMEAR, JITTER, PINHOLE_R, PIXEL, OLPF, SLITW = (1.3, 0.7), 0.9, 1.1, (0.9, 1.1), (0.35, 0.45), (0.8, 0.6)
TFS = {
    'smear': ('degradations', 'smear_ft', 'xy>', SMEAR),
    'smear_x': ('degradations', 'smear_ft', 'xy>', (SMEAR[0], 0)),
    'jitter': ('degradations', 'jitter_ft', 'r>', (JITTER,)),
    'pinhole_ft': ('objects', 'pinhole_ft', '<r', (PINHOLE_R,)),
    'slit_ft': ('objects', 'slit_ft', '<xy', SLITW),
    'slit_ft_x': ('objects', 'slit_ft', '<xy', (SLITW[0], None)),
    'slit_ft_y': ('objects', 'slit_ft', '<xy', (None, SLITW[1])),
    'airydisk_ft': ('psf', 'airydisk_ft', 'r>', (AIRY_FNO, AIRY_WVL)),
    'pixel': ('detector', 'pixel_ft', 'xy>', PIXEL),
    'olpf': ('detector', 'olpf_ft', 'xy>', OLPF),
}
PRODUCT = ('smear', 'jitter', 'pinhole_ft', 'pixel', 'airydisk_ft')


def call_tf(mods, name, fx, fy, fr):
    """the transfer function `name` from the modules in `mods` (name -> module) on frequencies fx, fy, fr"""
    mod, fn, order, args = TFS[name]
    f = getattr(mods[mod], fn)
    if fn == 'slit_ft' and fx.ndim == 2:        # the reference's two-band branch indexes fx[0, 1]: it takes 1-D vectors only
        fx, fy = fx[0, :], fy[:, 0]
    freqs = [{'x': fx, 'y': fy, 'r': fr}[c] for c in order if c in 'xyr']
    return f(*args, *freqs) if order[0] == '<' else f(*freqs, *args)


def tf_arguments(name, fxmax, fymax):
    """max|argument| of every factor of a transfer function on frequencies up to fxmax, fymax"""
    frmax = float(np.hypot(fxmax, fymax))
    if name == 'smear':
        return [np.pi * fxmax * SMEAR[0], np.pi * fymax * SMEAR[1]]
    if name == 'smear_x':
        return [np.pi * fxmax * SMEAR[0]]
    if name == 'jitter':
        return [2 * (np.pi * JITTER * frmax) ** 2]
    if name == 'pinhole_ft':
        return [2 * np.pi * PINHOLE_R * frmax]
    if name == 'slit_ft':
        return [np.pi * fxmax * SLITW[0], np.pi * fymax * SLITW[1]] * 2
    if name == 'slit_ft_x':
        return [np.pi * fxmax * SLITW[0]]
    if name == 'slit_ft_y':
        return [np.pi * fymax * SLITW[1]]
    if name == 'airydisk_ft':
        return [1.0]
    if name == 'pixel':
        return [np.pi * fxmax * PIXEL[0], np.pi * fymax * PIXEL[1]]
    if name == 'olpf':
        return [2 * OLPF[0] * fxmax, 2 * OLPF[1] * fymax]
    if name in ('airydisk', 'airydisk_efield'):
        raise ValueError('spatial functions: see airy_bound')
    if name == 'product':
        return [a for n in PRODUCT for a in tf_arguments(n, fxmax, fymax)]
    raise KeyError(name)


def tf_bound(name, tag, dt):
    """sum over the factors of 16 eps (1 + max|argument|)"""
    fx, fy = freq_vectors(tag)
    return sum(16 * eps(dt) * (1 + a) for a in tf_arguments(name, np.abs(fx).max(), np.abs(fy).max()))


def airy_radius(tag):
    x, y = grid_xy(tag)
    return np.hypot(x, y) * AIRY_SCALE


def airy_bound(tag, dt, efield):
    u = np.pi * airy_radius(tag).max() / AIRY_WVL / AIRY_FNO
    return (1 if efield else 2) * 16 * eps(dt) * (1 + u)


# ---------------------------------------------------------------------------- PSF metrics
def smooth_data(tag, dtype=np.float64):
    """smooth data for the resample: two displaced Gaussians on the grid"""
    x, y = grid_xy(tag)
    d = np.exp(-((x - 0.2) ** 2 + (y + 0.1) ** 2) / 0.18) + 0.5 * np.exp(-((x + 0.3) ** 2 + (y - 0.25) ** 2) / 0.08)
    return d.astype(dtype)


def polar_bound(x, y, data, dt):
    d = np.asarray(data, np.float64)
    gy, gx = np.gradient(d, np.asarray(y, np.float64), np.asarray(x, np.float64))
    dx = max(x[1] - x[0], y[1] - y[0])
    n = max(len(x), len(y))
    return float(np.hypot(gx, gy).max() * dx * 16 * eps(dt) * n + 16 * eps(dt) * np.abs(d).max())


def polar_excluded(x, y, dt):
    """samples whose query point lies within 8 eps _max of the outer boundary of the grid"""
    from prysm_amd import imagechain_plan as IP
    rho, phi, _max = IP.polar_axes(np.asarray(x, np.float64), np.asarray(y, np.float64))
    xq, yq = rho[None, :] * np.cos(phi[:, None]), rho[None, :] * np.sin(phi[:, None])
    band = 8 * eps(dt) * _max
    near = np.zeros(xq.shape, bool)
    for q, lo, hi in ((xq, x[0], x[-1]), (yq, y[0], y[-1])):
        near |= (np.abs(q - lo) <= band) | (np.abs(q - hi) <= band)
    return near


def psf_grid(dtype=np.float64):
    ny, nx = PSF_SHAPE
    x = (np.arange(nx) - nx // 2) * 2 / nx
    y = (np.arange(ny) - ny // 2) * 2 / nx
    return x.astype(dtype), y.astype(dtype)


def psf_dx():
    return 2 / PSF_SHAPE[1]


def gaussian_psf(dtype=np.float64):
    x, y = psf_grid()
    xx, yy = np.meshgrid(x, y)
    return np.exp(-((xx - PSF_CENTRE[0]) ** 2 + (yy - PSF_CENTRE[1]) ** 2) / (2 * PSF_SIGMA ** 2)).astype(dtype)


def airy_psf(dtype=np.float64):
    """an Airy pattern with several rings on the PSF grid: AIRY_LEVEL is crossed in the main lobe and again in the rings.  Built from
    scipy-free arithmetic: the unit's own float64 jinc model (checked against the reference in the host tests)"""
    from prysm_amd import imagechain_plan as IP
    x, y = psf_grid()
    xx, yy = np.meshgrid(x, y)
    u = np.hypot(xx, yy) * AIRY_SCALE * np.pi / AIRY_WVL / AIRY_FNO
    return (np.abs(2 * IP.jinc(u)) ** 2).astype(dtype)


def size_bound64(data, polar, r, metric, criteria='last'):
    """the float64 bound of a size metric (a radius): the resample bound of the PSF grid over the smallest slope |dp/dr| at a row's
    crossing, plus 16 eps of the radius"""
    from prysm_amd import imagechain_plan as IP
    relative, value = IP.size_threshold(metric)
    last = IP.size_criteria(criteria)
    p = np.asarray(polar, np.float64)
    hm = value * p.max() if relative else value
    change = (p[:, :-1] > hm) != (p[:, 1:] > hm)
    rows = np.flatnonzero(change.any(axis=1))
    i = (change.shape[1] - 1 - np.argmax(change[:, ::-1], axis=1))[rows] if last else np.argmax(change, axis=1)[rows]
    slope = np.abs((p[rows, i + 1] - p[rows, i]) / (r[i + 1] - r[i])).min()
    x, y = psf_grid()
    return polar_bound(x, y, data, np.float64) / slope + 16 * eps(np.float64) * r[-1]
