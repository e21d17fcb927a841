"""Point Diffraction Interferometry on the device (prysm/x/pdi.py): rectangle_pulse, PSPDI and evaluate_test_ref_arm_matching.

A forward model is one grating pass (pm_grating, csrc/sensors.hip: the grating is evaluated at the shifted coordinate and multiplied
into the field as it is stored; the reference makes the shifted coordinates, the grating and the product as separate arrays), the
two Wavefront.to_fpm_and_back calls on executors prepared once in the constructor, and one combination pass (pm_beam_combine: the
test arm's transmissivity, the sum of the arms and its squared modulus, stored once).

Kept from the reference: the grating is ALWAYS applied along self.x -- forward_model never reads self.y (pdi.py:215-222) --
and grating_axis only moves the test arm's window (test_arm_shift, pdi.py:159-162).  rectangle_pulse wraps with numpy's mod (the
result has the period's sign) and sets samples with |x mod period| < eps of the dtype to the offset, after the two levels.
"""
from functools import partial

import numpy as np
import torch

from .. import _lib as L
from .. import _ops
from .._richdata import RichData
from ..coordinates import make_xy_grid, _real_dtype
from ..geometry import circle
from ..propagation import Wavefront as WF, prepare_executor
from . import sensors_plan as SP

__all__ = ['rectangle_pulse', 'PSPDI', 'evaluate_test_ref_arm_matching']


def _grating(kind, p, x, shift=0.0, field=None):
    """the grating `kind` on the coordinates x (any shape), or field (2-D, x's shape) times it: one launch"""
    dt = _real_dtype(x)
    shp = tuple(np.shape(x))
    xd, ldx = _ops._rows(x, dt)
    rows, cols = xd.shape
    if field is not None:
        field = L.as_device(field)
        cdt = L._COMPLEX_OF[dt]
        if field.dtype != cdt:
            field = field.to(cdt)
        if tuple(field.shape) != (rows, cols):
            raise ValueError(f'the field has shape {tuple(field.shape)}, the coordinates {shp}')
    out = _ops.grating(kind, p, dt, L.PM_COORDS_POINTWISE, rows, cols, x=xd, ldx=ldx, shift=shift, field=field)
    return out if field is not None else out.reshape(shp)


def rectangle_pulse(x, duty=0.5, amplitude=0.5, offset=0.5, period=2 * np.pi):
    """Rectangular pulse; generalized square wave (pdi.py:11-51): offset + amplitude where mod(x, period) < duty period, offset -
    amplitude elsewhere, offset where |mod(x, period)| < eps.  One launch; float32 x gives float32."""
    return _grating(SP.GRATING_PULSE, SP.pulse_params(duty, amplitude, offset, period), x)


class PSPDI:
    """Phase Shifting Point Diffraction Interferometer (Medecki Interferometer) (pdi.py:54-253)."""

    def __init__(self, x, y, efl, epd, wavelength,
                 test_arm_offset=64,
                 test_arm_fov=64,
                 test_arm_samples=256,
                 test_arm_transmissivity=1,
                 pinhole_diameter=0.25,
                 pinhole_samples=128,
                 grating_rulings=64,
                 grating_type='sin_amp',
                 grating_axis='x'):
        """Create a new PS/PDI or Medecki Interferometer (pdi.py:57-193); arguments and attributes as the reference.

        x, y: coordinates of the arrays forward_model will take, mm; efl: focal length behind the grating, mm; epd: entrance pupil
        diameter, mm; wavelength: um; test_arm_offset, test_arm_fov: lambda/D; pinhole_diameter: lambda/D; grating_rulings: per EPD;
        grating_type: 'sin_amp' or 'ronchi'; grating_axis: 'x' or 'y' (moves the test arm's window only, see the module docstring)."""
        grating_type = grating_type.lower()
        grating_axis = grating_axis.lower()
        if grating_type not in ('ronchi', 'sin_amp'):
            raise ValueError('unsupported grating type')
        dt = _real_dtype(x, y)
        self.x = L.as_device(x, dt)
        self.y = L.as_device(y, dt)
        self.dx = float(self.x[0, 1] - self.x[0, 0])
        self.efl = efl
        self.epd = epd
        self.wavelength = wavelength
        self.fno = efl / epd
        self.flambd = self.fno * self.wavelength

        self.grating_rulings = grating_rulings
        self.grating_period = self.epd / grating_rulings
        self.grating_type = grating_type
        self.grating_axis = grating_axis
        if grating_type == 'ronchi':
            self._grating = (SP.GRATING_PULSE, SP.pulse_params(0.5, 0.5, 0.5, self.grating_period))
        else:
            self._grating = (SP.GRATING_SIN_AMP, SP.sin_amp_params(grating_rulings, epd))
        self.grating_func = partial(_grating, *self._grating)

        self.test_arm_offset = test_arm_offset
        self.test_arm_fov = test_arm_fov
        self.test_arm_samples = test_arm_samples
        self.test_arm_eps = test_arm_fov / test_arm_samples
        self.test_arm_fov_compute = (test_arm_fov + self.test_arm_eps) * self.flambd
        self.test_arm_mask_rsq = (test_arm_fov * self.flambd / 2) ** 2
        self.test_arm_transmissivity = test_arm_transmissivity

        if self.grating_axis == 'x':
            self.test_arm_shift = (grating_rulings * self.flambd, 0)
        else:
            self.test_arm_shift = (0, grating_rulings * self.flambd)

        self.pinhole_diameter = pinhole_diameter * self.flambd
        self.pinhole_samples = pinhole_samples
        self.dx_pinhole = pinhole_diameter / (pinhole_samples - 1)
        self.pinhole_fov_radius = pinhole_samples / 2 * self.dx_pinhole

        xph, yph = make_xy_grid(pinhole_samples, diameter=2 * self.pinhole_fov_radius)
        self.pinhole = circle((pinhole_diameter / 2) ** 2, xph * xph + yph * yph)

        xt, yt = make_xy_grid(test_arm_samples, diameter=self.test_arm_fov_compute)
        self.dx_test_arm = float(xt[0, 1] - xt[0, 0])
        self.test_mask = circle(self.test_arm_mask_rsq, xt * xt + yt * yt)
        del xph, yph, xt, yt

        pupil_samples = tuple(self.x.shape)
        self.pinhole_executor = prepare_executor(
            pupil_dx=self.dx, pupil_samples=pupil_samples,
            focal_dx=self.dx_pinhole, focal_samples=tuple(self.pinhole.shape),
            wavelength=self.wavelength, efl=self.efl,
        )
        self.test_executor = prepare_executor(
            pupil_dx=self.dx, pupil_samples=pupil_samples,
            focal_dx=self.dx_test_arm, focal_samples=tuple(self.test_mask.shape),
            wavelength=self.wavelength, efl=self.efl, focal_shift=self.test_arm_shift,
        )

    def forward_model(self, wave_in, phase_shift=0, debug=False):
        """Perform a forward model, returning the intensity at the detector plane (pdi.py:195-253).

        wave_in: the complex field at the input (an array or a Wavefront); phase_shift: radians, 2 pi = one grating period;
        debug: return the dictionary of the fields in each arm ('total_field', 'at_camera', 'at_fpm') instead."""
        shift = 0.0
        if phase_shift != 0:
            shift = phase_shift / (2 * np.pi) * self.grating_period
        field = wave_in.data if isinstance(wave_in, WF) else wave_in
        i = WF(_grating(*self._grating, self.x, shift=shift, field=field), self.wavelength, self.dx)

        if debug:
            ref_beam, ref_at_fpm, ref_after_fpm = i.to_fpm_and_back(self.pinhole, self.pinhole_executor, return_more=True)
            test_beam, test_at_fpm, test_after_fpm = i.to_fpm_and_back(self.test_mask, self.test_executor, return_more=True)
        else:
            ref_beam = i.to_fpm_and_back(self.pinhole, self.pinhole_executor)
            test_beam = i.to_fpm_and_back(self.test_mask, self.test_executor)

        t = self.test_arm_transmissivity
        a, b = ref_beam.data, test_beam.data
        if a.dtype != b.dtype:
            a, b = a.to(torch.promote_types(a.dtype, b.dtype)), b.to(torch.promote_types(a.dtype, b.dtype))
        if t != 1:
            test_beam = test_beam * t
        self.ref_beam = ref_beam
        self.test_beam = test_beam
        inten, total = _ops.beam_combine(a, 1.0, b, t, want_total=debug, want_intensity=not debug)
        if debug:
            return {
                'total_field': WF(total, self.wavelength, self.dx),
                'at_camera': {
                    'ref': ref_beam,
                    'test': test_beam,
                },
                'at_fpm': {
                    'ref': (ref_at_fpm, ref_after_fpm),
                    'test': (test_at_fpm, test_after_fpm),
                }
            }
        return RichData(inten, self.dx, self.wavelength)


def evaluate_test_ref_arm_matching(debug_dict):
    """(ratio, I1, I2) of the two arms at the camera (pdi.py:256-261): ratio = mean(I_ref) / mean(I_test), a 0-d device tensor."""
    pak = debug_dict['at_camera']
    I1 = pak['ref'].intensity
    I2 = pak['test'].intensity
    ratio = I1.data.mean() / I2.data.mean()
    return ratio, I1, I2
