"""Self-Referenced Interferometer on the device (prysm/x/sri.py): overlap_integral, to_photonic_fiber_and_back and
SelfReferencedInterferometer.

The reference arm focuses onto a single-mode fibre, couples into its mode and returns to the pupil.  Nothing of that is read on the
host here: one pass over the focal field and the mode (pm_overlap, csrc/fibers.hip) leaves the power at the facet and the coupling on
the device, pm_fiber_scale (csrc/sensors.hip) reads both there and stores Efib sqrt(P eta) exp(i phi) once, and pm_beam_combine adds
the two arms with the beamsplitter's amplitudes and takes the squared modulus in one pass.  The reference forms the intensity at the
facet, its sum, the overlap, the scale and the phase factor as separate array operations with host scalars between them.

to_photonic_fiber_and_back builds an executor when none is given, as the reference does; SelfReferencedInterferometer keeps the one
it needs per input shape, so a second forward_model on the same shape builds nothing.
"""
import warnings

import torch

from .. import _lib as L
from .. import _ops
from .._richdata import RichData
from ..coordinates import make_xy_grid, cart_to_polar, _real_dtype
from ..propagation import Wavefront, prepare_executor
from .fibers import smf_mode_field, overlap

__all__ = ['overlap_integral', 'to_photonic_fiber_and_back', 'SelfReferencedInterferometer']

WF = Wavefront


def overlap_integral(E1, E2, sumI1, sumI2):
    """|sum conj(E1) E2|^2 / (sumI1 sumI2) (sri.py:18-22), a 0-d tensor on the device; the sum is one pass and a fixed-order fold."""
    res = overlap(E1, E2)
    return (res[0] * res[0] + res[1] * res[1]) / (sumI1 * sumI2)


def to_photonic_fiber_and_back(self, efl, Efib, fib_dx, Ifibsum, executor=None, shift=(0, 0), phase_shift=0, return_more=False):
    """Focus onto a single-mode fiber and return to the pupil (sri.py:25-85).

    self: the Wavefront at the pupil; efl: focal length, mm; Efib: the (real) fibre mode at the facet; fib_dx: sample spacing at the
    facet, um; Ifibsum: the sum of the mode's intensity (a number or a 0-d tensor); executor: a prepared pupil <-> facet operator;
    shift: of the facet relative to the focus; phase_shift: of the emitted field, radians.  Returns the Wavefront at the next pupil,
    with return_more also the field at the facet, the emitted field and the coupling (a 0-d device tensor).  Nothing is read on the
    host."""
    Efib = L.as_device(Efib)
    if Efib.is_complex():
        raise TypeError('the fibre mode must be real')
    fib_samples = tuple(Efib.shape)
    input_samples = tuple(self.data.shape)
    if executor is None:
        executor = prepare_executor(
            pupil_dx=self.dx, pupil_samples=input_samples,
            focal_dx=fib_dx, focal_samples=fib_samples,
            wavelength=self.wavelength, efl=efl, focal_shift=shift,
        )
    at_fpm = self.focus_dft(executor)
    E = at_fpm.data
    rdt = L._REAL_OF[E.dtype]
    if Efib.dtype != rdt:
        Efib = Efib.to(rdt)
    res = overlap(E, Efib)        # Re S, Im S, sum |E|^2, sum Efib^2, eta: one pass, nothing read back
    input_power = res[2]
    if isinstance(Ifibsum, torch.Tensor):
        Ifibsum = Ifibsum.to(device=res.device, dtype=rdt)
    coupling_loss = (res[0] * res[0] + res[1] * res[1]) / (input_power * Ifibsum)
    Eout = _ops.fiber_scale(Efib, input_power, coupling_loss, float(phase_shift))
    field_at_next_pupil = executor.adjoint(Eout)

    if input_samples[0] != input_samples[1]:
        warnings.warn(f'Forward propagation had input shape {input_samples} which was not uniform between axes, scaling is off')
    if fib_samples[0] != fib_samples[1]:
        warnings.warn(f'Forward propagation had fiber shape {fib_samples} which was not uniform between axes, scaling is off')

    out = Wavefront(field_at_next_pupil, self.wavelength, self.dx, self.space)
    if return_more:
        return out, at_fpm, Wavefront(Eout, self.wavelength, fib_dx, 'psf'), coupling_loss
    return out


class SelfReferencedInterferometer:
    """Self-Referenced Interferometer (sri.py:88-178)."""

    def __init__(self, x, y, efl, epd, wavelength,
                 fiber_V=2.3, fiber_b=0.5, fiber_a=1.95 / 2,
                 fiber_samples=256,
                 beamsplitter_RT=(0.8, 0.2)):
        """Create a new Self-Referenced Interferometer (sri.py:90-144); arguments and attributes as the reference.

        x, y: coordinates of the arrays forward_model will take, mm; efl: focal length, mm; epd: entrance pupil diameter, mm;
        wavelength: um; fiber_V, fiber_b, fiber_a: the fibre's V-number, normalised propagation constant and core radius (um);
        fiber_samples: samples across the facet; beamsplitter_RT: power to the reference and test arms."""
        dt = _real_dtype(x, y)
        self.x = L.as_device(x, dt)
        self.y = L.as_device(y, dt)
        self.dx = float(self.x[0, 1] - self.x[0, 0])
        self.efl = efl
        self.epd = epd
        self.wavelength = wavelength
        self.fno = efl / epd
        self.flambd = self.fno * self.wavelength

        fiber_fov_radius = 10 * 1.25 * fiber_a
        self.dx_pinhole = (2 * fiber_fov_radius) / fiber_samples

        xfib, yfib = make_xy_grid(fiber_samples, diameter=2 * fiber_fov_radius)
        rfib, tfib = cart_to_polar(xfib, yfib)
        self.Efib = smf_mode_field(fiber_V, fiber_a, fiber_b, rfib)
        self.Efib = self.Efib / (self.Efib ** 2).sum() ** 0.5
        self.Ifib = abs(self.Efib) ** 2
        self.Ifibsum = self.Ifib.sum()
        self.dxfib = float(xfib[0, 1] - xfib[0, 0])

        self.ref_r = beamsplitter_RT[0] ** 0.5
        self.test_t = beamsplitter_RT[1] ** 0.5
        self._executors = {}

    def _executor(self, shape):
        ex = self._executors.get(shape)
        if ex is None:
            ex = self._executors[shape] = prepare_executor(
                pupil_dx=self.dx, pupil_samples=shape, focal_dx=self.dxfib, focal_samples=tuple(self.Efib.shape),
                wavelength=self.wavelength, efl=self.efl, focal_shift=(0, 0))
        return ex

    def forward_model(self, wave_in, phase_shift=0, debug=False):
        """Perform a forward model, returning the intensity at the detector plane (sri.py:146-178).

        wave_in: the complex field at the input (an array or a Wavefront); phase_shift: of the reference beam, radians; debug:
        return {'at_camera': {'ref': ..., 'test': ...}} instead.  No host read: power, overlap and scale stay on the device."""
        if not isinstance(wave_in, WF):
            wave_in = WF(L.as_complex(wave_in), self.wavelength, self.dx)
        ref = to_photonic_fiber_and_back(wave_in, self.efl, self.Efib, self.dxfib, self.Ifibsum,
                                         executor=self._executor(tuple(wave_in.data.shape)), phase_shift=phase_shift)
        if debug:
            return {
                'at_camera': {'ref': ref * self.ref_r, 'test': wave_in * self.test_t},
            }
        a, b = ref.data, L.as_complex(wave_in.data)
        if a.dtype != b.dtype:
            cdt = torch.promote_types(a.dtype, b.dtype)
            a, b = a.to(cdt), b.to(cdt)
        inten, _ = _ops.beam_combine(a, self.ref_r, b, self.test_t)
        return RichData(inten, self.dx, self.wavelength)
