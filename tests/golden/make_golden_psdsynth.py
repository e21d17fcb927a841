"""Writes tests/golden/psdsynth.npz from the reference (prysm/interferogram.py, which runs on numpy and scipy).  Run by hand, with the
reference's directory given; the file holds data only:

    python tests/golden/make_golden_psdsynth.py /path/to/prysm

Cases and bounds: tests/psdsynth_common.py.  numpy.random.rand is replaced by a function that returns the case's stored random
numbers, so the reference and the code under test see the same ones.  Per precision tag in (f64, f32) -- f32 is the reference run in
float64 on the float32-rounded random numbers:

  <even|odd|asym>_<tag>_z, _dx          z and dx = x[1] - x[0] of synthesize_surface_from_psd
  render_<name>_<tag>_z, _dx            z and x[1] - x[0] of render_synthetic_surface
  fit_noisy                             the coefficients fit_psd finds on tests/psdsynth_common.noisy_curve()

Asserts the reference's acceptance figures (RMS exactly as requested, NaN at [0, 0], x[1] - x[0] = 100 / 63 for the 'circle' case) and
that the odd and the asymmetric cases have an inverse transform with an imaginary part far above rounding, and prints the numpy
model's deviation from the reference for every case.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])

import psdsynth_common as C  # noqa: E402
from prysm import interferogram as ref  # noqa: E402
from prysm_amd import psdsynth_plan as PP  # noqa: E402

warnings.simplefilter('ignore')

_next = []


def _rand(*shape):
    u = _next.pop()
    assert u.shape == tuple(shape)
    return u


np.random.rand = _rand


def main():
    out = {}
    for name, (shape, seed) in C.SYNTH.items():
        psd, nu_x, nu_y = C.synth_case(name)
        for dt in C.DTYPES:
            u = C.randnums(shape, seed, dt)
            _next.append(u.astype(np.float64))
            x, _, z = ref.synthesize_surface_from_psd(psd, nu_x, nu_y)
            key = f'{name}_{C.tag(dt)}'
            out[f'{key}_z'], out[f'{key}_dx'] = z, x[1] - x[0]
            dx, f = PP.synthesize(psd.astype(dt), nu_y[0], u)
            imag = np.abs(f.imag).max() / np.abs(f.real).max()
            print(f'{key}: model vs reference {C.deviation(f.real, z, dt):.2f} eps, dx {abs(dx - out[f"{key}_dx"]):.1e}, |imag| / |real| {imag:.2e}')
            assert (imag > 1e-3) == (name != 'even'), 'the even symmetric case is Hermitian, the others are not'
    for name, (size, samples, rms, _, which, kw, seed) in C.RENDER.items():
        fcn = {'abc': ref.abc_psd, 'ab': ref.ab_psd, 'user': C.gauss_psd}[which]
        mask = C.render_mask(name)
        for dt in C.DTYPES:
            u = C.randnums((samples, samples), seed, dt)
            _next.append(u.astype(np.float64))
            x, _, z = ref.render_synthetic_surface(size, samples, rms=rms, mask=mask, psd_fcn=fcn, **kw)
            key = f'render_{name}_{C.tag(dt)}'
            out[f'{key}_z'], out[f'{key}_dx'] = z, x[1] - x[0]
            if which == 'user':
                nu = PP.freq_vector(samples, size / (samples - 1))
                source = dict(psd=C.gauss_psd(np.hypot(nu[None, :], nu[:, None]), **kw).astype(dt))
            else:
                source = dict(model=PP.model_record(PP.ABC if which == 'abc' else PP.AB, kw))
            kind = PP.MASK_NONE if mask is None else PP.MASK_CIRCLE if isinstance(mask, str) else PP.MASK_ARRAY
            _, zm = PP.render(size, samples, u, rms=rms, mask_kind=kind, mask=None if isinstance(mask, str) else mask, **source)
            print(f'{key}: model vs reference {C.deviation(zm, z, dt):.2f} eps')
            if name == 'circle':
                fin = np.isfinite(z)
                assert abs(np.sqrt((z[fin] ** 2).mean()) - 5.0) < 1e-12 and np.isnan(z[0, 0]) and abs(x[1] - x[0] - 100 / 63) < 1e-12
    out['fit_noisy'] = np.asarray(ref.fit_psd(C.FIT_F, C.noisy_curve()))
    print('fit_noisy', out['fit_noisy'], 'model', PP.fit_psd(C.FIT_F, C.noisy_curve(), PP.abc, PP.ABC))
    np.savez_compressed(C.GOLDEN_FILE, **out)
    print('wrote', C.GOLDEN_FILE, os.path.getsize(C.GOLDEN_FILE), 'bytes')


if __name__ == '__main__':
    main()
