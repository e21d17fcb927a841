"""Host side of the wavefront-sensor unit (csrc/sensors.hip), numpy only: the parameter records of its entry points and every kernel
restated in numpy -- operation by operation, in the precision of the launch, usable without a GPU.

  psi                  pm_psi: the weighted sums over the frames in double, k ascending, rounded once; atan2 of the rounded pair
  out_dtype_of         the dtype pm_psi's outputs take for a frame dtype
  lenslet_params       pm_lenslets from shack_hartmann's arguments (the pairing of n[0] with xc and n[1] with yc kept as it stands)
  lenslet_centres      the centres as the reference rounds them: make_xy_grid(n, dx=pitch, grid=False), then the += pitch / 2
  lenslet_screen       pm_lenslet_screen: the windowless sum over the lenslets, rows of lenslets outermost; also the count map
  pulse_params, sin_amp_params, grating     pm_grating: rectangle_pulse with numpy's mod and its eps midpoint rule; the sine grating
  beam_combine         pm_beam_combine
  fiber_scale          pm_fiber_scale
"""
import math

import numpy as np

MAX_FRAMES = 32
LENSLET_RECTANGLE, LENSLET_CIRCLE = 0, 1
GRATING_SIN_AMP, GRATING_PULSE = 0, 1
FRAME_DTYPES = (np.dtype('float32'), np.dtype('float64'), np.dtype('uint8'), np.dtype('uint16'))


def out_dtype_of(frame_dtype, precision):
    """float frames keep their dtype; integer frames give `precision` (config.compute_precision)"""
    frame_dtype = np.dtype(frame_dtype)
    if frame_dtype not in FRAME_DTYPES:
        raise TypeError(f'frames must be float32, float64, uint8 or uint16, got {frame_dtype}')
    return frame_dtype if frame_dtype.kind == 'f' else np.dtype(precision)


def check_scheme(K, s, c):
    s, c = [float(v) for v in np.asarray(s).reshape(-1)], [float(v) for v in np.asarray(c).reshape(-1)]
    if not 1 <= K <= MAX_FRAMES:
        raise ValueError(f'{K} frames: between 1 and {MAX_FRAMES} are taken')
    if len(s) != K or len(c) != K:
        raise ValueError(f'{K} frames, but the scheme has {len(s)} sine and {len(c)} cosine weights')
    return s, c


def psi(frames, s, c, out_dtype):
    """(num, den, phase) of pm_psi"""
    s, c = check_scheme(len(frames), s, c)
    out_dtype = np.dtype(out_dtype)
    num = np.zeros(np.shape(frames[0]), dtype=np.float64)
    den = np.zeros_like(num)
    for g, sk, ck in zip(frames, s, c):
        g = np.asarray(g).astype(np.float64)
        num = num + sk * g
        den = den + ck * g
    num, den = num.astype(out_dtype), den.astype(out_dtype)
    return num, den, np.arctan2(num, den)


# ---------------------------------------------------------------- Shack-Hartmann
def lenslet_params(pitch, n, efl, wavelength, kind, aperture_kwargs=None, shift=False):
    """the fields of pm_lenslets as a dict.  xc has n[1] values and yc n[0] (make_xy_grid's (rows, cols) order), while the half-pitch
    shift of xc is decided by n[0] and that of yc by n[1]: the reference's pairing, kept"""
    if not hasattr(n, '__iter__'):
        n = (n, n)
    n = tuple(int(v) for v in n)
    if len(n) != 2 or min(n) < 1:
        raise ValueError(f'n must be a positive int or a pair of them, got {n}')
    kw = dict(aperture_kwargs or {})
    pitch = float(pitch)
    if kind == LENSLET_RECTANGLE:
        height = kw.pop('height', None)
        angle = kw.pop('angle', 0)
        if kw or angle != 0:
            return None
        hw = pitch / 2
        hh = hw if height is None else float(height)
        if not (0 <= hh <= pitch):
            return None
    else:
        if kw:
            return None
        hw = hh = (pitch / 2) ** 2
    return dict(kind=kind, nx=n[1], ny=n[0], pitch=pitch,
                shift_x=pitch / 2 if (shift and n[0] % 2 == 0) else 0.0, shift_y=pitch / 2 if (shift and n[1] % 2 == 0) else 0.0,
                half_width=hw, half_height=hh, efl=float(efl), k=-(2 * math.pi) / (wavelength / 1e3))


def lenslet_centres(par, dtype):
    T = np.dtype(dtype).type

    def axis(n, sh):
        v = np.arange(-(n // 2), -(n // 2) + n).astype(T) * T(par['pitch'])
        return v + T(sh)
    return axis(par['nx'], par['shift_x']), axis(par['ny'], par['shift_y'])


def lenslet_screen(x, y, par, dtype):
    """(field, count): pm_lenslet_screen on 2-D coordinate arrays, and the number of lenslets each sample lies in"""
    T = np.dtype(dtype).type
    x, y = np.asarray(x, dtype=T), np.asarray(y, dtype=T)
    xc, yc = lenslet_centres(par, T)
    total = np.zeros(x.shape, dtype=T)
    count = np.zeros(x.shape, dtype=np.int32)
    hw, hh, two_efl = T(par['half_width']), T(par['half_height']), T(2 * par['efl'])
    for yy in yc:
        ly = y - yy
        for xx in xc:
            lx = x - xx
            rsq = lx * lx + ly * ly
            if par['kind'] == LENSLET_CIRCLE:
                inside = rsq - hw <= 0
            else:
                inside = (np.abs(lx) - hw <= 0) & (np.abs(ly) - hh <= 0)
            total = np.where(inside, total + rsq / two_efl, total)
            count += inside
    arg = T(par['k']) * total
    return (np.cos(arg) + 1j * np.sin(arg)).astype(np.result_type(T, 1j)), count


def grid_coords(shape, dx, dtype):
    """x, y of PM_COORDS_GRID as 2-D arrays"""
    T = np.dtype(dtype).type
    ny, nx = shape
    xv = np.arange(-(nx // 2), -(nx // 2) + nx).astype(T) * T(dx)
    yv = np.arange(-(ny // 2), -(ny // 2) + ny).astype(T) * T(dx)
    return np.meshgrid(xv, yv)


# ---------------------------------------------------------------- gratings
def pulse_params(duty=0.5, amplitude=0.5, offset=0.5, period=2 * math.pi):
    period = float(period)
    if not (math.isfinite(period) and period != 0):
        raise ValueError('the period must be finite and nonzero')
    return (period, duty * period, offset + amplitude, offset - amplitude, float(offset))


def sin_amp_params(rulings, epd):
    return (rulings * math.pi / (epd / 2), 0.0, 0.0, 0.0, 0.0)


def grating(kind, x, p, dtype, shift=0.0, field=None):
    """pm_grating: the grating at x + shift, or field times it"""
    T = np.dtype(dtype).type
    xs = np.asarray(x, dtype=T)
    if shift != 0:
        xs = xs + T(shift)
    p = [T(v) for v in p]
    if kind == GRATING_SIN_AMP:
        g = T(1) - ((np.sin(p[0] * xs) + T(1)) / T(2)) * T(0.1)
    else:
        xw = np.mod(xs, p[0])
        g = np.where(xw < p[1], p[2], p[3]).astype(T)
        g = np.where(np.abs(xw) < np.finfo(T).eps, p[4], g).astype(T)
    if field is None:
        return g
    f = np.asarray(field).astype(np.result_type(T, 1j))
    return (f.real * g + 1j * (f.imag * g)).astype(f.dtype)


def beam_combine(a, ca, b, cb):
    """(intensity, total) of pm_beam_combine"""
    a = np.asarray(a)
    T = a.real.dtype.type
    b = np.asarray(b).astype(a.dtype)
    re = a.real * T(ca) + b.real * T(cb)
    im = a.imag * T(ca) + b.imag * T(cb)
    return re * re + im * im, (re + 1j * im).astype(a.dtype)


def fiber_scale(efib, power, eta, phase_shift=0.0):
    """pm_fiber_scale"""
    efib = np.asarray(efib)
    T = efib.dtype.type
    e = efib * np.sqrt(T(power) * T(eta))
    return (e * T(math.cos(phase_shift)) + 1j * (e * T(math.sin(phase_shift)))).astype(np.result_type(T, 1j))
