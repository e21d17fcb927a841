"""Generate the Bayer fixture (tests/golden/bayer.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_bayer.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores data only:
- demosaic_malvar: `dem_<m>x<n>_<dtype>_in` and `dem_<m>x<n>_<dtype>_<cfa>` for the shapes of SHAPES, both CFAs, float64 and float32
  (normal data, signed, except the non-negative (24, 32) case), listed in `demosaic` (JSON); `dem_u16_in` (a 12-bit uint16 frame of
  the reference's Detector.expose) with `dem_u16_<cfa>` at config.precision = float64;
- composite / decomposite / recomposite / deinterlace for (6, 8) and (24, 32), both CFAs: `pl_<m>x<n>_{r,g1,g2,b}` (full-size planes),
  `comp_<m>x<n>_<cfa>`, `mos_<m>x<n>`, `dec_<m>x<n>_<cfa>` (the four planes stacked), `recomp_<m>x<n>_<cfa>` (of those planes; equals
  the mosaic), `deint_<m>x<n>_<cfa>`;
- wb_prescale / wb_postscale: `wb_mosaic`, `wb_rgb` and per case of `wb` (JSON: kind, gains, cfa, safe, saturation, regime)
  `wb_<name>_out`, float64 and float32 (`..._out32` from the float32 copy of the input);
- assemble_superresolved: `sr_<m>x<n>_{r,g1,g2,b}` and `sr_<m>x<n>_z<zoom>` listed in `superres` (JSON).

Asserted: among the safe white-balance cases one has a scalar saturation with one plane setting the ratio, one per-plane saturations
with a ratio above 1, one a ratio of exactly 1.  If an assertion fails, change the data, not the assertion.
"""
import json
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm import bayer as RB  # noqa: E402
from prysm import detector as RD  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (1, 5), (2, 2), (3, 3), (2, 7), (6, 4), (5, 8), (24, 32), (37, 70)]
CFAS = ('rggb', 'bggr')


def ratio_of(planes, gains, sats):
    ratio = 1
    for p, g, s in zip(planes, gains, sats):
        rat = p.max() * g / s
        if rat > 1 and rat > ratio:
            ratio = rat
    return ratio


def main():
    rng = np.random.default_rng(20261018)
    out = {}
    # ---- demosaic
    dem = []
    for m, n in SHAPES:
        a = rng.standard_normal((m, n)) * 100
        if (m, n) == (24, 32):
            a = np.abs(a)
        for dt in ('float64', 'float32'):
            x = a.astype(dt)
            key = f'dem_{m}x{n}_{dt}'
            out[key + '_in'] = x
            for cfa in CFAS:
                res = RB.demosaic_malvar(x.copy(), cfa)
                assert res.dtype == x.dtype and res.shape == (m, n, 3)
                out[f'{key}_{cfa}'] = res
            dem.append(dict(key=key, shape=[m, n], dtype=dt))
    out['demosaic'] = json.dumps(dem)
    np.random.seed(4242)
    yy, xx = np.mgrid[0:24, 0:32]
    scene = 2.0e4 * (0.2 + ((xx + 32 * yy) / (24 * 32 - 1.0)) ** 2) * (1 + 0.5 * ((yy & 1) * 2 + (xx & 1) == 0))
    det = RD.Detector(dark_current=5.0, read_noise=4.0, bias=20.0, fwc=30000.0, conversion_gain=7.0, bits=12, exposure_time=1.0)
    dn = det.expose(scene)
    assert dn.dtype == np.uint16 and dn.max() <= 4095 and dn.min() < dn.max()
    out['dem_u16_in'] = dn
    for cfa in CFAS:
        res = RB.demosaic_malvar(dn, cfa)
        assert res.dtype == np.float64
        out[f'dem_u16_{cfa}'] = res
    # ---- composite / decomposite / recomposite / deinterlace
    for m, n in ((6, 8), (24, 32)):
        planes = [rng.standard_normal((m, n)) for _ in range(4)]
        mos = rng.standard_normal((m, n))
        out[f'mos_{m}x{n}'] = mos
        for name, p in zip(('r', 'g1', 'g2', 'b'), planes):
            out[f'pl_{m}x{n}_{name}'] = p
        for cfa in CFAS:
            out[f'comp_{m}x{n}_{cfa}'] = RB.composite_bayer(*planes, cfa=cfa)
            dec = RB.decomposite_bayer(mos, cfa)
            out[f'dec_{m}x{n}_{cfa}'] = np.stack(dec)
            rec = RB.recomposite_bayer(*dec, cfa=cfa)
            assert np.array_equal(rec, mos)
            out[f'recomp_{m}x{n}_{cfa}'] = rec
            out[f'deint_{m}x{n}_{cfa}'] = RB.demosaic_deinterlace(mos, cfa)
    # ---- white balance
    mosaic = rng.random((24, 32)) * 1000 + 5
    rgb = rng.random((12, 16, 3)) * 1000 + 5
    out['wb_mosaic'], out['wb_rgb'] = mosaic, rgb
    wb = [
        dict(name='pre_u1', kind='pre', gains=[1.9, 1.0, 1.02, 1.6], cfa='rggb', safe=False, saturation=None),
        dict(name='pre_u2', kind='pre', gains=[2.1, 0.97, 1.0, 1.4], cfa='bggr', safe=False, saturation=None),
        dict(name='post_u', kind='post', gains=[1.7, 1.0, 1.3], safe=False, saturation=None),
        dict(name='pre_s_scalar', kind='pre', gains=[1.9, 1.0, 1.02, 1.6], cfa='rggb', safe=True, saturation=1200.0),
        dict(name='pre_s_planes', kind='pre', gains=[1.2, 1.0, 1.02, 1.6], cfa='bggr', safe=True, saturation=[1500.0, 1100.0, 900.0, 1250.0]),
        dict(name='pre_s_one', kind='pre', gains=[1.1, 1.0, 1.02, 1.05], cfa='rggb', safe=True, saturation=4000.0),
        dict(name='post_s_scalar', kind='post', gains=[1.7, 1.0, 1.3], safe=True, saturation=1100.0),
        dict(name='post_s_planes', kind='post', gains=[1.7, 1.0, 1.3], safe=True, saturation=[2500.0, 900.0, 1200.0]),
        dict(name='post_s_one', kind='post', gains=[1.7, 1.0, 1.3], safe=True, saturation=5000.0),
    ]
    regimes = set()
    for c in wb:
        for dt, suffix in (('float64', '_out'), ('float32', '_out32')):
            if c['kind'] == 'pre':
                x = mosaic.astype(dt)
                planes = RB.decomposite_bayer(x, c['cfa'])
                RB.wb_prescale(x, *c['gains'], cfa=c['cfa'], safe=c['safe'], saturation=c['saturation'])
            else:
                x = rgb.astype(dt)
                planes = [x[..., i].copy() for i in range(3)]
                RB.wb_postscale(x, *c['gains'], safe=c['safe'], saturation=c['saturation'])
            out[f"wb_{c['name']}{suffix}"] = x
        if c['safe']:
            src = mosaic if c['kind'] == 'pre' else rgb
            pl = RB.decomposite_bayer(src, c['cfa']) if c['kind'] == 'pre' else [src[..., i] for i in range(3)]
            sats = c['saturation'] if isinstance(c['saturation'], list) else [c['saturation']] * len(pl)
            ratio = ratio_of(pl, c['gains'], sats)
            scalar = not isinstance(c['saturation'], list)
            c['regime'] = 'one' if ratio == 1 else ('scalar' if scalar else 'planes')
            c['ratio'] = float(ratio)
            regimes.add((c['kind'], c['regime']))
    for kind in ('pre', 'post'):
        assert (kind, 'scalar') in regimes, f'{kind}: no safe case where a scalar saturation sets a ratio above 1'
        assert (kind, 'planes') in regimes, f'{kind}: no safe case where per-plane saturations set a ratio above 1'
        assert (kind, 'one') in regimes, f'{kind}: no safe case with a ratio of 1'
    out['wb'] = json.dumps(wb)
    # ---- assemble_superresolved
    sr = []
    for (m, n), zoom in (((16, 20), 3), ((15, 18), 2.5)):
        planes = [rng.random((m, n)) * 100 for _ in range(4)]
        for name, p in zip(('r', 'g1', 'g2', 'b'), planes):
            out[f'sr_{m}x{n}_{name}'] = p
        out[f'sr_{m}x{n}_z{zoom}'] = RB.assemble_superresolved(*planes, zoom)
        sr.append(dict(shape=[m, n], zoomfactor=zoom))
    out['superres'] = json.dumps(sr)
    path = os.path.join(HERE, 'bayer.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
