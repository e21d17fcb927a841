"""Generate the detector fixture (tests/golden/detector.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_detector.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores:
- `bin_<name>_in`, `bin_<name>_out` and `tile_<name>_in`, `tile_<name>_out` with their arguments in `bins` / `tiles` (JSON): bindown and
  tile for a 2-D array, a stack ([1, fy, fx]) and unequal factors, in both modes, fp64 (non-negative data);
- `pix_x`, `pix_y` (a 20 x 24 grid), `pixel`, `pixel_ft`, `olpf_ft` with the widths in `pixel_args` (JSON);
- Detector.expose with numpy.random.poisson / numpy.random.normal wrapped so that the draws are RECORDED: per case `<c>_img`,
  `<c>_prnu`, `<c>_dcnu`, `<c>_lut` (where the case has them), `<c>_mean` (the lam handed to poisson, reshaped), `<c>_shot`, `<c>_read`
  (what the generator returned) and `<c>_dn` (the reference's output), with the scalar parameters in `cases` (JSON).  8-, 12-, 16- and
  24-bit detectors, with and without prnu, dcnu and lut, 3 frames of a 24 x 32 image (one case of 1 frame: the squeezed shape).

Asserted for every exposure case: some sample clips at the full well, some at the ADC cap, some at 0.  If an assertion fails, change
the parameters, not the assertion.
"""
import json
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm import detector as RD  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
M, N = 24, 32

# name: bits, gain (e-/DN), fwc, bias, read noise, dark current, exposure time, peak (e-/s), prnu, dcnu, lut, frames
CASES = {
    'b8': dict(bits=8, conversion_gain=10.0, fwc=3000.0, bias=-15.0, read_noise=6.5, dark_current=2.5, exposure_time=0.5, peak=9000.0,
               prnu=False, dcnu=False, lut=False, frames=3),
    'b8_maps_lut': dict(bits=8, conversion_gain=10.0, fwc=3000.0, bias=-15.0, read_noise=6.5, dark_current=2.5, exposure_time=0.5,
                        peak=9000.0, prnu=True, dcnu=True, lut=True, frames=3),
    'b12': dict(bits=12, conversion_gain=3.7, fwc=17000.0, bias=-9.0, read_noise=4.25, dark_current=11.0, exposure_time=0.1, peak=2.5e5,
                prnu=True, dcnu=False, lut=False, frames=3),
    'b12_lut': dict(bits=12, conversion_gain=3.7, fwc=17000.0, bias=-9.0, read_noise=4.25, dark_current=11.0, exposure_time=0.1,
                    peak=2.5e5, prnu=False, dcnu=True, lut=True, frames=1),
    'b16': dict(bits=16, conversion_gain=0.83, fwc=60000.0, bias=-12.0, read_noise=3.1, dark_current=0.7, exposure_time=2.0, peak=4.5e4,
                prnu=True, dcnu=True, lut=False, frames=3),
    'b24': dict(bits=24, conversion_gain=0.011, fwc=200000.0, bias=-7.0, read_noise=2.2, dark_current=5.0, exposure_time=1.5,
                peak=2.4e5, prnu=False, dcnu=False, lut=False, frames=3),
}


class Recorder:
    def __init__(self):
        self.poisson, self.normal = np.random.poisson, np.random.normal
        self.lam = self.shot = self.read = None

    def __enter__(self):
        def poisson(lam, size=None):
            self.lam = np.array(lam, copy=True)
            self.shot = self.poisson(lam, size)
            return self.shot

        def normal(loc, scale, size=None):
            self.read = self.normal(loc, scale, size)
            return self.read
        np.random.poisson, np.random.normal = poisson, normal
        return self

    def __exit__(self, *exc):
        np.random.poisson, np.random.normal = self.poisson, self.normal
        return False


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    # ---- bindown / tile
    bins, tiles = [], []
    for name, shape, factor in (('2d', (24, 36), 3), ('2d_uneq', (24, 36), (2, 4)), ('stack', (3, 16, 20), (1, 4, 2)), ('one', (6, 10), 1)):
        a = rng.random(shape) * 100
        small = rng.random(tuple(s // f for s, f in zip(shape, factor if isinstance(factor, tuple) else (factor,) * len(shape)))) * 100
        for mode in ('avg', 'sum'):
            key = f'{name}_{mode}'
            out[f'bin_{key}_in'], out[f'bin_{key}_out'] = a, RD.bindown(a, factor, mode)
            out[f'tile_{key}_in'], out[f'tile_{key}_out'] = small, np.array(RD.tile(small, factor, mode))
            bins.append(dict(name=key, factor=factor, mode=mode))
            tiles.append(dict(name=key, factor=factor, scaling=mode))
    out['bins'], out['tiles'] = json.dumps(bins), json.dumps(tiles)
    # ---- pixel, pixel_ft, olpf_ft
    x, y = np.meshgrid(np.linspace(-6.1, 6.3, 24), np.linspace(-5.2, 4.9, 20))
    pa = dict(width_x=4.4, width_y=3.1)
    out['pix_x'], out['pix_y'], out['pixel_args'] = x, y, json.dumps(pa)
    out['pixel'] = RD.pixel(x, y, **pa)
    out['pixel_ft'] = RD.pixel_ft(x * 0.1, y * 0.1, **pa)
    out['olpf_ft'] = RD.olpf_ft(x * 0.1, y * 0.1, **pa)
    # ---- exposures with recorded draws
    np.random.seed(777)
    yy, xx = np.mgrid[0:M, 0:N]
    ramp = ((xx + N * yy) / (M * N - 1.0)) ** 2          # 0 at one corner, 1 at the other
    cases = {}
    for name, c in CASES.items():
        img = ramp * c['peak'] * (1 + 0.01 * rng.standard_normal((M, N))).clip(0.9, 1.1)
        img[0, :4] = 0.0                                    # dark pixels: with a negative bias they clip at 0
        prnu = 1 + 0.03 * rng.standard_normal((M, N)) if c['prnu'] else None
        dcnu = np.abs(1 + 0.2 * rng.standard_normal((M, N))) if c['dcnu'] else None
        lut = None
        if c['lut']:
            k = np.arange(2 ** c['bits'], dtype=np.float64)
            lut = np.round(k ** 0.985 + 3).astype(np.uint16)      # a compressive nonlinearity with an offset
        det = RD.Detector(c['dark_current'], c['read_noise'], c['bias'], c['fwc'], c['conversion_gain'], c['bits'], c['exposure_time'],
                          prnu=prnu, dcnu=dcnu, lut=lut)
        with Recorder() as rec:
            dn = det.expose(img, frames=c['frames'])
        F = c['frames']
        shot, read = rec.shot.reshape(F, M, N), rec.read.reshape(F, M, N)
        x_ = shot + read + c['bias']
        y_ = np.minimum(x_, c['fwc']) * (1 / c['conversion_gain'])
        assert (x_ > c['fwc']).any(), f'{name}: no sample reaches the full well'
        assert ((y_ > 2 ** c['bits'] - 1) & (x_ <= c['fwc'])).any(), f'{name}: no sample reaches the ADC cap below the full well'
        assert (y_ < 0).any(), f'{name}: no sample clips at 0'
        assert dn.shape == ((F, M, N) if F > 1 else (M, N))
        out[f'{name}_img'], out[f'{name}_mean'] = img, rec.lam.reshape(M, N)
        out[f'{name}_shot'], out[f'{name}_read'], out[f'{name}_dn'] = shot, read, dn
        for k_, v in (('prnu', prnu), ('dcnu', dcnu), ('lut', lut)):
            if v is not None:
                out[f'{name}_{k_}'] = v
        cases[name] = {k_: v for k_, v in c.items() if k_ not in ('peak',)}
    out['cases'] = json.dumps(cases)
    path = os.path.join(HERE, 'detector.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
