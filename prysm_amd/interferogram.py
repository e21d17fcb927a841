"""Tools to analyse interferometric data (prysm/interferogram.py) on the device: from a measured map with invalid pixels to a cleaned
surface, its PSD and a band-limited RMS without leaving HBM.

Data is a real 2-D device tensor, float32 or float64 by config.precision (arrays passed in keep float32 / float64); NaN marks an invalid
pixel.  The kernels are those of csrc/interferogram.hip; prysm_amd/interferogram_plan.py restates each in numpy.  Launches and host
reads per public call:

  pv, rms, Sa, std, strehl, dropout_percentage     4 launches (pm_ifg_stats), 1 host read of the record
  crop                  4 launches, 1 host read of the bounding box, then a view: nothing is copied, every kernel takes the view's
                        leading dimension
  remove_piston / remove_tiptilt / remove_power     3 launches each (pm_ifg_fit: sums and solve; pm_ifg_remove), no host read
  fill, mask            1 launch, no host read
  spike_clip            5 launches (the record, then pm_ifg_edit reading std from it), no host read
  pad                   1 launch (pm_embed through fttools.pad2d)
  psd                   window x data and S2 (2 launches), the real-input transform with its shifts and |.|^2 epilogue, the division
                        by S2 fs^2 with S2 read on the device (1 launch); no host read with a named window, 1 for which=None
  bandlimited_rms       psd, then 2 launches (pm_ifg_band) and 1 host read; total_integrated_scatter the same
  filter                1 launch for the windowed impulse responses, one transform with the |.| epilogue per corner frequency,
                        1 launch for the 1 - H combination, then the fft2 x H ifft2 real chain
  slope                 1 launch
  pvr                   the 37 fringe Zernike planes (1 launch), polynomials.lstsq (4 launches), the projection from coefficients that
                        stay on the device (pm_zernike_sum, 1 launch), pv and rms (4 launches and 1 host read each): 2 host reads
  render_synthetic_surface    with abc_psd / ab_psd, a seed, 'circle' and rms: 5 launches of csrc/psdsynth.hip (uniform numbers, the
                        signal in place on their spectrum, the real part with the mask and the partial sums, their fold, the scale)
                        and the two transforms' own launches; no host read.  Stored: the random numbers, their spectrum, the inverse
                        transform's complex output and z -- no nu_r, psd, phase or mask map.  An array mask is read in the third
                        launch; another callable costs 3 more launches (the frequencies, nu_r, the callable's own) and a psd array
  synthesize_surface_from_psd    4 launches of the unit (3 with randnums) and the transforms; 1 host read of nu_y[0] when nu_y is on
                        the device
  fit_psd               1 host read of f and psd, then numpy (and scipy.optimize.least_squares but for ab_psd)
  make_random_subaperture_mask    a slice assignment

Coordinates.  The object keeps x and y as (origin index, step) and hands that to the kernels, which generate the coordinates; .x, .y,
.r and .t materialise arrays on demand (make_xy_grid, cart_to_polar).  As in the reference, coordinates that were never looked at are
those of make_xy_grid on the CURRENT shape -- a crop re-centres them -- while coordinates that were looked at, or set by strip_latcal,
latcal or pad, are carried through crop.  Assigning .x or .y switches the object to arrays, which the fits then read.

Reference behaviour that is kept: the statistics and crop use isfinite (+-inf is left out), dropout_percentage and fill use isnan;
fit_plane fits {x, y} without a piston term; fit_sphere fits {rho^2, 1} on linspace(-1, 1, n) grids and only its rho^2 term is removed;
spike_clip compares |data|, not |data - mean|, with nsigma std; bandlimited_rms takes the spacing from two samples along axis 0 and uses
it for both axes; filter transforms unshifted data and returns the real part; synthesize_surface_from_psd multiplies the UNSHIFTED
spectrum's phase with the centred psd element by element, takes dx = dy = -1 / (2 nu_y[0]) whatever the parity of the lengths, and
returns the real part of a complex inverse transform (the signal is Hermitian only on even lengths with a symmetric psd, so no
half-spectrum inverse is used); render_synthetic_surface spaces the grid by size / (samples - 1) but masks on make_xy_grid(samples,
diameter=size), and replaces the centre frequency by a tenth of the next one.

Random numbers.  The device generator is Philox4x32-10 keyed by `seed` (csrc/psdsynth.hip); without a seed one is drawn from Python's
random, so random.seed() makes a session reproducible.  randnums= replaces the generator (the reference's np.random.rand values, for
parity).  batch=B or a (B, m, n) randnums gives a stack, surface b drawn with surface index b and scaled to rms on its own.

Not here: the Zygo readers and writers and save_*, the interferogram() fringe picture and all plotting.
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import _ops
from . import interferogram_plan as IP
from . import psdsynth_plan as PP
from ._richdata import RichData
from .conf import config
from .coordinates import broadcast_1d_to_2d, cart_to_polar, make_xy_grid
from .fttools import forward_ft_unit, pad2d
from .util import Sa, as_map, mean, pv, record, rms, std  # noqa: F401

HeNe = 0.6328

__all__ = ['HeNe', 'fit_plane', 'fit_sphere', 'make_window', 'window_2d_welch', 'hann2d', 'psd', 'bandlimited_rms', 'abc_psd', 'ab_psd',
           'ideal_lpf_iir2d', 'designfilt2d', 'Interferogram', 'mean', 'rms', 'pv', 'Sa', 'std', 'synthesize_surface_from_psd',
           'render_synthetic_surface', 'fit_psd', 'make_random_subaperture_mask']

_TILT = L.PM_IFG_TERM_X | L.PM_IFG_TERM_Y
_POWER = L.PM_IFG_TERM_R2 | L.PM_IFG_TERM_PISTON


def _rdtype():
    return L.torch_dtype(config.compute_precision)


def _real(array):
    """an array as a real device tensor: float32 and float64 stay, anything else becomes config.precision"""
    dt = array.dtype if isinstance(array, torch.Tensor) else L._NP2TORCH.get(np.asarray(array).dtype)
    return L.as_device(array, dt if dt in (torch.float32, torch.float64) else _rdtype())


def _array_coords(x, y, dtype):
    x, y = L.as_device(x, dtype), L.as_device(y, dtype)
    if x.dim() == 1 and y.dim() == 1:
        return _ops.ifg_coords(dtype, L.PM_COORDS_SEPARABLE, x=x, y=y)
    return _ops.ifg_coords(dtype, L.PM_COORDS_POINTWISE, x=x, y=y)


def _linspace_coords(shape, dtype):
    return _ops.ifg_coords(dtype, L.PM_COORDS_GRID, linspace=(-1.0, IP.linspace_step(shape[1]), -1.0, IP.linspace_step(shape[0])))


def _evaluate(terms, co, coef, shape, dtype):
    """the sum of the chosen terms as an array: pm_ifg_remove on zeros with the coefficients negated, 0 - (-p) = p exactly"""
    out = torch.zeros(shape, dtype=dtype, device=coef.device)
    return _ops.ifg_remove(out, terms, co, -coef)


def fit_plane(x, y, z):
    """The plane c0 x + c1 y of the least-squares fit of {x, y} -- no piston term -- to the finite pixels of z (interferogram.py:35-55).
    Three launches, nothing is read back."""
    z = as_map(z)
    co = _array_coords(x, y, z.dtype)
    coef = _ops.ifg_fit(z, _TILT, co)
    return _evaluate(_TILT, co, coef, tuple(z.shape), z.dtype)


def fit_sphere(z):
    """(mask of the finite pixels, c rho^2 at those pixels as a 1-D tensor) of the fit of {rho^2, 1} on linspace(-1, 1, n) grids
    (interferogram.py:58-82)."""
    z = as_map(z)
    co = _linspace_coords(tuple(z.shape), z.dtype)
    coef = _ops.ifg_fit(z, _POWER, co)
    pts = torch.isfinite(z)
    return pts, _evaluate(L.PM_IFG_TERM_R2, co, coef, tuple(z.shape), z.dtype)[pts]


def window_2d_welch(r, alpha=8):
    """1 - |r / rmax|^alpha with rmax = r[rows - 1, cols // 2] (interferogram.py:268-286), for a radius array of any origin.  Three
    tensor operations on the device, not a kernel of the unit: the named window of make_window and psd, which is the hot path, is
    generated inside pm_ifg_window from make_xy_grid's radius instead."""
    r = _real(r)
    rmax = r[r.shape[0] - 1, r.shape[1] // 2]
    return 1 - (r / rmax).abs() ** alpha


def make_window(signal, dx, which=None, alpha=4):
    """The window of a PSD analysis (interferogram.py:85-145): 'welch', 'hann' / 'hanning', an array (returned as it is), or None: Welch
    when the four corner blocks of the signal (2 % of each axis) are zero, Hann otherwise -- one host read."""
    if which is not None and not isinstance(which, str):
        return which
    kind = _window_kind(signal, which)
    shape = tuple(signal.shape)
    dt = signal.dtype if isinstance(signal, torch.Tensor) and signal.dtype in (torch.float32, torch.float64) else _rdtype()
    return _ops.ifg_window(kind, shape, dt, dx=dx, alpha=alpha)[0]


def _window_kind(signal, which):
    if which is not None:
        return IP.window_kind(which)
    ys, xs = IP.corner_samples(tuple(signal.shape))
    s = signal if isinstance(signal, torch.Tensor) else torch.from_numpy(np.asarray(signal))
    blocks = (s[:ys, :xs], s[-ys:, :xs], s[:ys, -xs:], s[-ys:, -xs:])      # the reference's slices, -0 included
    dark = torch.stack([(b == 0).all() for b in blocks]).all()
    return L.PM_IFG_WIN_WELCH if bool(dark) else L.PM_IFG_WIN_HANN


def _psd(height, dx, window=None, alpha=4):
    if isinstance(window, str):
        IP.window_kind(window)      # an unknown name is refused before anything is moved to the device
    height = as_map(height)
    shape = tuple(height.shape)
    if window is None or isinstance(window, str):
        hw, s2 = _ops.ifg_window(_window_kind(height, window), shape, height.dtype, height=height, dx=dx, alpha=alpha)
    else:
        hw, s2 = _ops.ifg_window(L.PM_IFG_WIN_ARRAY, shape, height.dtype, height=height, window=window)
    shift = IP.psd_shifts(shape)
    if _ops.real_pairs_ok(hw) and not _pow2(shape):
        p = _ops.fft2_real(hw, in_shift=shift, out_shift=shift, epilogue=L.PM_EPI_ABS2)
    else:      # powers of two: the library's Hermitian path; an odd width: the real array through the complex transform
        p = _ops.fft2(hw, direction=-1, scale=1.0, in_shift=shift, out_shift=shift, epilogue=L.PM_EPI_ABS2)
    return _ops.ifg_psd_scale(p, s2, 1 / dx)


def _pow2(shape):
    return all(_ops._is_pow2_engine(n) for n in shape)


def psd(height, dx, window=None):
    """(ux, uy, psd) of a height map (interferogram.py:148-187): |ifftshift(fft2(fftshift(height x window)))|^2 / (S2 fs^2)."""
    p = _psd(height, dx, window)
    ux, uy = broadcast_1d_to_2d(forward_ft_unit(dx, p.shape[1]), forward_ft_unit(dx, p.shape[0]))
    return ux, uy, p


def bandlimited_rms(r, psd, wllow=None, wlhigh=None, flow=None, fhigh=None):
    """Band-limited RMS from a PSD and its radial frequencies, 1-D or 2-D (interferogram.py:190-265).  Two launches, one host read."""
    flow, fhigh = IP.band_limits(wllow, wlhigh, flow, fhigh)
    p = _real(psd)
    out = _ops.ifg_band(p, flow, fhigh, nu=L.as_device(r, p.dtype))
    return math.sqrt(float(out[0]))


def abc_psd(nu, a, b, c):
    """Lorentzian PSD model a / (1 + (nu / b)^c) (interferogram.py:289-309)."""
    if not hasattr(nu, 'shape') or not tuple(np.shape(nu)):
        return a / (1 + (nu / b) ** c)
    return _ops.ifg_psd_model(L.PM_IFG_PSD_ABC, _real(nu), a, b, c)


def ab_psd(nu, a, b):
    """Inverse-power PSD model a nu^(-b) (interferogram.py:312-330)."""
    if not hasattr(nu, 'shape') or not tuple(np.shape(nu)):
        return a * nu ** (-b)
    return _ops.ifg_psd_model(L.PM_IFG_PSD_AB, _real(nu), a, b)


def _forward_spectrum(u):
    """fft2 of the real stack u with PM_EPI_NONE, on the route PP.route names (the routes of _psd)"""
    shape = tuple(u.shape[-2:])
    way = PP.route(shape, stacked=u.shape[0] > 1)
    if way == 'hermitian':
        try:
            return _ops.fft2(u, direction=-1, scale=1.0)
        except NotImplementedError:      # a power of two outside the Hermitian path (a very small or very long row)
            way = PP.route((0, shape[1]), stacked=u.shape[0] > 1)
    if way == 'real_pairs' and _ops.real_pairs_ok(u[0]):
        return _ops.fft2_real(u[0]).unsqueeze(0)
    return _ops.fft2(u, direction=-1, scale=1.0)


def _synthesize(shape, dtype, nu_y0, *, psd=None, model=None, randnums=None, seed=None, batch=None, mask=None, circle=None, rms=None):
    """(dx, z): the chain of synthesize_surface_from_psd on a stack, with render_synthetic_surface's mask and scale in its last passes"""
    lead = PP.check_random(shape, None if randnums is None else tuple(np.shape(randnums)), seed, batch)
    dx, area, scale = PP.window(nu_y0, shape)
    if randnums is not None:
        u = L.as_device(randnums, dtype)
        u = u if u.dim() == 3 else u.unsqueeze(0)
    else:
        u = _ops.psd_uniform((lead or 1,) + tuple(shape), dtype, PP.draw_seed() if seed is None else seed)
    spectrum = _forward_spectrum(u)
    _ops.psd_signal(spectrum, area, psd=psd, model=model)
    shift = PP.shifts(shape)
    field = _ops.fft2(spectrum, direction=1, scale=scale, in_shift=shift, out_shift=shift)
    z, sums = _ops.psd_finish(field, mask=mask, circle=circle)
    if rms is not None:
        _ops.psd_scale(z, sums, rms)
    return dx, (z if lead is not None else z[0])


def _axes(shape, dx, dtype):
    dev = L.device()
    return torch.arange(shape[1], dtype=dtype, device=dev) * dx, torch.arange(shape[0], dtype=dtype, device=dev) * dx


def synthesize_surface_from_psd(psd, nu_x, nu_y, *, randnums=None, seed=None):
    """(x, y, z): a surface with the given 2-D PSD and a random phase (interferogram.py:333-368).  randnums, (m, n) or (B, m, n),
    replaces the device generator, which seed keys; z takes the leading dimension of randnums."""
    if randnums is not None and seed is not None:
        raise ValueError('randnums replaces the generator: give randnums or seed, not both')
    PP.check_shape(tuple(np.shape(psd)))
    psd = _real(psd)
    shape = tuple(psd.shape)
    dx, z = _synthesize(shape, psd.dtype, float(nu_y[0]), psd=psd, randnums=randnums, seed=seed)
    x, y = _axes(shape, dx, psd.dtype)
    return x, y, z


def render_synthetic_surface(size, samples, rms=None, mask=None, psd_fcn=abc_psd, *, seed=None, randnums=None, batch=None, **psd_fcn_kwargs):
    """(x, y, z): a synthetic surface of `samples` x `samples` points over `size`, from a PSD function, NaN outside the mask (None, an
    array, or 'circle'), scaled to `rms` if given (interferogram.py:371-432).  abc_psd and ab_psd are evaluated inside the signal kernel;
    any other callable is called with the radial frequencies as a device tensor.  batch=B: z is (B, samples, samples), each surface
    scaled on its own."""
    PP.check_mask_name(mask)
    samples = PP.check_samples(samples)
    shape, dtype = (samples, samples), _rdtype()
    PP.check_random(shape, None if randnums is None else tuple(np.shape(randnums)), seed, batch)
    dxg = size / (samples - 1)
    nu = PP.freq_vector(samples, dxg)
    source = {}
    if psd_fcn is abc_psd or psd_fcn is ab_psd:
        source['model'] = PP.model_record(PP.ABC if psd_fcn is abc_psd else PP.AB, psd_fcn_kwargs) + (dxg,)
    else:
        nu_r, _ = cart_to_polar(L.as_device(nu, dtype), L.as_device(nu, dtype))
        source['psd'] = _real(psd_fcn(nu_r, **psd_fcn_kwargs))
        if tuple(source['psd'].shape) != shape:
            raise ValueError(f"the PSD function returned shape {tuple(source['psd'].shape)} for frequencies of shape {shape}")
    if isinstance(mask, str):
        source['circle'] = (size / 2, size / samples)      # make_xy_grid(samples, diameter=size): the step is size / samples
    elif mask is not None:
        m = mask if isinstance(mask, torch.Tensor) else L.as_device(np.asarray(mask))
        if tuple(m.shape) != shape:
            raise ValueError(f'the mask has shape {tuple(m.shape)}, the surface {shape}')
        source['mask'] = L.as_device(m if m.dtype in (torch.bool, torch.uint8) else m != 0)
    dx, z = _synthesize(shape, dtype, nu[0], randnums=randnums, seed=seed, batch=batch, rms=rms, **source)
    x, y = _axes(shape, dx, dtype)
    return x, y, z


def fit_psd(f, psd, callable=abc_psd, guess=None, return_='coefficients'):      # noqa: A002 -- the reference's name
    """Fit the parameters of a PSD model to a 1-D curve in log10 space (interferogram.py:435-544): ab_psd in closed form after dropping
    the first five samples (no scipy needed), abc_psd from a seed taken from the data with bounds (0, inf), any other callable
    unbounded from `guess` or [100, 1, ...].  f and psd are read back once; the fit runs on the host."""
    host = [v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (f, psd)]
    if callable is abc_psd:
        return PP.fit_psd(host[0], host[1], PP.abc, PP.ABC, guess, return_)
    if callable is ab_psd:
        return PP.fit_psd(host[0], host[1], PP.ab, PP.AB, guess, return_)
    return PP.fit_psd(host[0], host[1], callable, None, guess, return_)


def make_random_subaperture_mask(shape, mask):
    """A bool array of `shape` that holds `mask` at a random offset and False elsewhere (interferogram.py:635-665)."""
    shape = tuple(int(s) for s in shape)
    dy, dx = PP.subaperture_offsets(shape, tuple(np.shape(mask)))      # a mask that does not fit is refused before the device is touched
    m = L.as_device(mask if isinstance(mask, torch.Tensor) else np.asarray(mask))
    out = torch.zeros(shape, dtype=torch.bool, device=L.device())
    out[dy:dy + m.shape[0], dx:dx + m.shape[1]] = m != 0
    return out


def hann2d(M, N):
    """Rotationally symmetric Hann window of M rows and N columns (interferogram.py:547-558)."""
    return _ops.ifg_iir((M, N), _rdtype(), 1.0, 0.0, parts=L.PM_IFG_IIR_HANN)[0]


def ideal_lpf_iir2d(r, dx, fc_over_nyq):
    """Ideal impulse response of a 2-D lowpass filter (interferogram.py:561-565)."""
    r = as_map(r)
    return _ops.ifg_iir(tuple(r.shape), r.dtype, dx, fc_over_nyq, r=r, parts=L.PM_IFG_IIR_LPF)[0]


def _design(shape, dtype, dx, fc, typ, complex_out, **radius):
    t = IP.filter_type(typ)
    lo, hi = IP.corner_frequencies(fc, t, dx)
    hl, hh = _ops.ifg_iir(shape, dtype, dx, lo, hi, **radius)
    Hl = _abs_spectrum(hl)
    Hh = _abs_spectrum(hh) if hh is not None else None
    return _ops.ifg_combine(t, Hl, Hh, complex_out=complex_out)


def _abs_spectrum(h):
    """|fft2(h)| of a real array: the Hermitian path with its |.| epilogue for powers of two, the half-size transform and untangling
    sweep for other even widths, the complex transform and pm_abs_arg for an odd width"""
    if _pow2(tuple(h.shape)):
        try:
            return _ops.fft2(h, direction=-1, scale=1.0, epilogue=L.PM_EPI_ABS)
        except NotImplementedError:      # a power of two outside the Hermitian path (a very small or very long row)
            pass
    if _ops.real_pairs_ok(h):
        return _ops.fft2_real(h, epilogue=L.PM_EPI_ABS)
    return _ops.abs_arg(_ops.fft2(h, direction=-1, scale=1.0))[0]


def designfilt2d(r, dx, fc, typ='lowpass'):
    """Transfer function of a rotationally symmetric filter for 2-D data (interferogram.py:568-632): typ lowpass / highpass with a
    corner frequency, bandpass / bandreject with a (lower, upper) pair, or the two-letter shorthands."""
    r = as_map(r)
    return _design(tuple(r.shape), r.dtype, dx, fc, typ, False, r=r)


class Interferogram(RichData):
    """Logic and data for working with interferometric data (interferogram.py:668-1225)."""

    def __init__(self, phase, dx=0, wavelength=HeNe, intensity=None, meta=None):
        if not wavelength and meta:
            # a header's wavelength is in metres under either spelling of the key
            metres = next((meta[k] for k in ('wavelength', 'Wavelength') if meta.get(k) is not None), None)
            if metres is not None:
                wavelength = metres * 1e6
        self._data = None
        self._grid = self._xy = self._rt = self._cache = None
        super().__init__(data=phase, dx=dx, wavelength=wavelength)
        self.intensity = intensity
        self.meta = meta
        self._latcaled = dx != 0

    # ---- data and coordinates
    @property
    def data(self):
        return self._data

    @data.setter
    def data(self, data):
        old = None if self._data is None else tuple(self._data.shape)
        self._data = as_map(data)
        if old is not None and old != tuple(self._data.shape):      # as the reference: a new shape forgets the coordinates
            self._grid = self._xy = self._rt = None

    @property
    def grid(self):
        """(origin row, origin column, step) of the generated coordinates -- x = (col - origin column) step --, None while arrays are
        in use"""
        if self._xy is not None:
            return None
        return IP.grid_current(self._grid, self.shape, self.dx)

    def _looked_at(self):
        """the grid in force, now explicit: whatever reads the coordinates -- .x, .y, .r, .t, remove_tiptilt, filter -- fixes them, so
        a later crop carries them as the reference carries its arrays.  None while arrays are in use"""
        g = self.grid
        if g is not None:
            self._grid = g
        return g

    def _materialise(self):
        """x and y as arrays from the grid: views of make_xy_grid on a grid large enough to hold the origin at its centre, so the
        elements are make_xy_grid's to the bit"""
        if self._xy is None:
            oy, ox, step = self.grid
            self._grid = (oy, ox, step)      # looked at: carried through crop from now on, as the reference's arrays are
            key = (self.shape, self._grid)
            if self._cache is None or self._cache[0] != key:
                rows, cols = self.shape
                R, C = 2 * max(abs(oy), abs(rows - oy)) + 2, 2 * max(abs(ox), abs(cols - ox)) + 2
                gx, gy = make_xy_grid((R, C), dx=step)
                r0, c0 = R // 2 - oy, C // 2 - ox
                self._cache = (key, (gx[r0:r0 + rows, c0:c0 + cols], gy[r0:r0 + rows, c0:c0 + cols]))
            return self._cache[1]
        return self._xy

    @property
    def x(self):
        return self._materialise()[0]

    @x.setter
    def x(self, x):
        other = self._materialise()[1]
        self._xy, self._grid, self._rt = (x, other), None, None

    @property
    def y(self):
        return self._materialise()[1]

    @y.setter
    def y(self, y):
        other = self._materialise()[0]
        self._xy, self._grid, self._rt = (other, y), None, None

    @property
    def r(self):
        if self._rt is None:
            self._rt = cart_to_polar(self.x, self.y)
        return self._rt[0]

    @property
    def t(self):
        if self._rt is None:
            self._rt = cart_to_polar(self.x, self.y)
        return self._rt[1]

    def _coords(self):
        g = self._looked_at()
        if g is None:
            return _array_coords(self._xy[0], self._xy[1], self.data.dtype)
        return _ops.ifg_coords(self.data.dtype, L.PM_COORDS_GRID, origin=(g[0], g[1]), dx=g[2])

    # ---- statistics
    @property
    def dropout_percentage(self):
        """Percentage of pixels that are NaN."""
        return float(record(self.data)[L.PM_IFG_NNAN]) / self.data.numel() * 100

    @property
    def pv(self):
        """Peak-to-valley phase error.  DIN/ISO St."""
        return pv(self.data)

    @property
    def rms(self):
        """RMS phase error.  DIN/ISO Sq."""
        return rms(self.data)

    @property
    def Sa(self):
        """Sa phase error.  DIN/ISO Sa."""
        return Sa(self.data)

    @property
    def std(self):
        """Standard deviation of phase error."""
        return std(self.data)

    @property
    def strehl(self):
        """Strehl ratio of the data as wavefront error (Welford, Aberrations of Optical Systems, Eq. (13.2))."""
        wvl = self.wavelength * 1e3      # um to nm
        return math.exp(-(2 * math.pi * std(self.data) / wvl) ** 2)

    @staticmethod
    def pvr_check(shape, normalization_radius):
        """the reference's refusal (interferogram.py:771-774), from the shape alone"""
        if normalization_radius is None and shape[0] != shape[1]:
            raise ValueError('pvr: if normalization_radius is None, data must be square')

    def pvr(self, normalization_radius=None):
        """Peak-to-valley residual (interferogram.py:743-795; C. Evans, "Robust Estimation of PV for Optical Surface Specification and
        Testing", OF&T 2008, OWA4): the PV of the fit of the fringe Zernikes 1..37 over r <= 1 plus three times the RMS of what the
        fit leaves.  normalization_radius None: the data must be square and the radius is r[rows - 1, cols // 2], read on the device.
        The coefficients never leave the device; the only host reads are those of the two statistics."""
        from .polynomials import fringe_to_nm, lstsq, zernike_nm_seq
        from .polynomials.zernike import _sum
        self.pvr_check(self.shape, normalization_radius)
        r, t = self.r, self.t
        if normalization_radius is None:
            normalization_radius = r[self.shape[0] - 1, self.shape[1] // 2]      # _rmax_square_array (interferogram.py:26-32)
        r = r / normalization_radius
        outside = r > 1
        nan = torch.full((), float('nan'), dtype=self.data.dtype, device=self.data.device)
        data = torch.where(outside, nan, self.data)
        nms = [fringe_to_nm(j) for j in range(1, 38)]
        basis = zernike_nm_seq(nms, r, t, norm=False)
        coefs = lstsq(basis, data)
        projected = torch.where(outside, nan, _sum(coefs, nms, r, t, False, L.PM_ZERNIKE_POLAR))
        return pv(projected) + 3 * rms(data - projected)

    # ---- edits
    def fill(self, _with=0):
        """Fill NaN values, in place."""
        _ops.ifg_edit(self.data, L.PM_IFG_FILL, value=_with)
        return self

    def crop(self):
        """Crop to the rectangle bounding the finite region: one host read of the box, then a view."""
        box = IP.crop_box(record(self.data), self.shape)
        if box is None:
            return self
        r0, r1, c0, c1 = box
        carried = None
        if self._xy is not None:
            carried = ('xy', tuple(v[r0:r1, c0:c1] if v.dim() == 2 else v[(c0, r0)[i]:(c1, r1)[i]] for i, v in enumerate(self._xy)))
        elif self._grid is not None:
            carried = ('grid', IP.grid_crop(self._grid, r0, c0))
        rt = None if self._rt is None or carried is None else tuple(v[r0:r1, c0:c1] for v in self._rt)
        self.data = self._data[r0:r1, c0:c1]
        if carried is not None:
            if carried[0] == 'xy':
                self._xy = carried[1]
            else:
                self._grid = carried[1]
            self._rt = rt
        return self

    def recenter(self):
        """Move the coordinates' origin to sample (rows // 2, cols // 2)."""
        if self._xy is not None:
            c = tuple(s // 2 for s in self.shape)
            x, y = self._xy
            self._xy = (x - (x[c] if x.dim() == 2 else x[c[1]]), y - (y[c] if y.dim() == 2 else y[c[0]]))
        else:
            self._grid = IP.grid_recenter(self._grid, self.shape, self.dx)
        self._rt = None
        return self

    def remove_piston(self):
        """Subtract the mean of the finite pixels."""
        co = _ops.ifg_coords(self.data.dtype, L.PM_COORDS_GRID)      # a piston reads no coordinate
        _ops.ifg_remove(self.data, L.PM_IFG_TERM_PISTON, co, _ops.ifg_fit(self.data, L.PM_IFG_TERM_PISTON, co))
        return self

    def remove_tiptilt(self):
        """Subtract the least-squares plane c0 x + c1 y (fitted without a piston term)."""
        co = self._coords()
        _ops.ifg_remove(self.data, _TILT, co, _ops.ifg_fit(self.data, _TILT, co))
        return self

    def remove_power(self):
        """Subtract the rho^2 term of the least-squares fit of {rho^2, 1} on linspace(-1, 1, n) grids."""
        co = _linspace_coords(self.shape, self.data.dtype)
        _ops.ifg_remove(self.data, L.PM_IFG_TERM_R2, co, _ops.ifg_fit(self.data, _POWER, co))
        return self

    def mask(self, mask):
        """NaN where the mask is False, in place."""
        _ops.ifg_edit(self.data, L.PM_IFG_MASK, mask=mask)
        return self

    def strip_latcal(self):
        """Strip the lateral calibration and revert to pixels."""
        self.dx = 1.
        self._grid, self._xy, self._rt = IP.grid_default(self.shape, 1.), None, None
        self._latcaled = False
        return self

    def latcal(self, plate_scale):
        """Lateral calibration: centred coordinates with plate_scale between samples."""
        self.strip_latcal()
        self._grid = IP.grid_default(self.shape, plate_scale)
        self.dx = plate_scale
        self._latcaled = True
        return self

    def pad(self, value=np.nan, *, samples=None, shape=None):
        """Pad with `value` around the data; exactly one of samples (to add per axis) or shape (to reach) is given."""
        shape = IP.pad_shape(self.shape, samples, shape)
        self.data = pad2d(self.data, value=value, out_shape=shape)
        return self.latcal(self.dx)

    def spike_clip(self, nsigma=3):
        """NaN where |data| exceeds nsigma standard deviations; the deviation stays on the device."""
        _ops.ifg_edit(self.data, L.PM_IFG_CLIP, value=nsigma, record=_ops.ifg_stats(self.data))
        return self

    # ---- spectra
    def psd(self):
        """Power spectral density, ~nm^2/mm^2 for z in nm and x, y in mm, as a RichData with x, y, data."""
        p = _psd(self.data, self.dx)
        ux, uy = broadcast_1d_to_2d(forward_ft_unit(self.dx, p.shape[1]), forward_ft_unit(self.dx, p.shape[0]))
        out = RichData(p, 0, self.wavelength)
        out.x, out.y = ux, uy
        out.dx = ux[1] - ux[0]      # as the reference writes it: the difference of two ROWS of the broadcast axis
        out._default_twosided = False
        return out

    def filter(self, fc, typ='lowpass'):
        """Frequency-domain filter: lowpass / highpass with a corner frequency, bandpass / bandreject with a (lower, upper) pair."""
        g = self._looked_at()
        if g is None:
            radius = dict(r=self.r)
        else:
            radius = dict(origin=(g[0], g[1]), r_dx=g[2])
        H = _design(self.shape, self.data.dtype, self.dx, fc, typ, True, **radius)
        x = self.data if self.data.is_contiguous() else self.data.contiguous()
        M, N = self.shape
        self.data = _ops.fft2_mul_ifft2(x, scale=1.0 / (M * N), mul=H, real_out=True)
        return self

    def bandlimited_rms(self, wllow=None, wlhigh=None, flow=None, fhigh=None):
        """Band-limited RMS from the PSD, between two spatial periods or two spatial frequencies."""
        flow, fhigh = IP.band_limits(wllow, wlhigh, flow, fhigh)
        out = _ops.ifg_band(_psd(self.data, self.dx), flow, fhigh, dx=self.dx)
        return math.sqrt(float(out[0]))

    def total_integrated_scatter(self, wavelength, incident_angle=0):
        """Total integrated scatter for an angle or angles; the spatial units are taken to be mm, the wavelength microns."""
        upper_limit = 1000 / wavelength
        kernel = 4 * np.pi * np.cos(np.radians(incident_angle))
        kernel = kernel * (self.bandlimited_rms(fhigh=upper_limit) / wavelength)
        return 1 - np.exp(-kernel ** 2)

    def slope(self):
        """Slope in x, in y and its magnitude, as three RichData."""
        dx = self.dx
        gx, gy, gr = _ops.ifg_slope(self.data, dx)
        return RichData(gx, dx, None), RichData(gy, dx, None), RichData(gr, dx, None)

    @staticmethod
    def render_from_psd(size, samples, rms=None, mask='circle', psd_fcn=abc_psd, **kw):
        """An Interferogram of a synthetic surface (interferogram.py:1191-1225): render_synthetic_surface with the circular mask by
        default, dx the spacing of its x axis, the HeNe wavelength.  seed= and randnums= are passed on."""
        x, _, z = render_synthetic_surface(size, samples, rms=rms, mask=mask, psd_fcn=psd_fcn, **kw)
        if z.dim() != 2:
            raise ValueError('an Interferogram holds one surface: render a stack with render_synthetic_surface')
        samples = PP.check_samples(samples)
        dx = PP.window(PP.freq_vector(samples, size / (samples - 1))[0], (samples, samples))[0]      # x[1] - x[0] without a host read
        return Interferogram(phase=z, dx=dx, wavelength=HeNe)

    def copy(self):
        out = Interferogram(self.data.clone(), self.dx, self.wavelength, self.intensity, self.meta)
        out._grid, out._xy, out._latcaled = self._grid, self._xy, self._latcaled
        return out

    def __str__(self):
        z_unit = 'mm' if self._latcaled else 'px'
        diameter_y, diameter_x = self.shape[0] * self.dx, self.shape[1] * self.dx
        return f'Interferogram with:\nSize: ({diameter_x:.3f}x{diameter_y:.3f}){z_unit}\n{self.pv:.3f} PV, {self.rms:.3f} RMS nm'
