"""Writes tests/golden/imagechain.npz from the reference (prysm/objects.py, degradations.py, psf.py, detector.py, coordinates.py, which
run on numpy and scipy).  Run by hand, with the reference's directory given; the file holds data only:

    python tests/golden/make_golden_imagechain.py /path/to/prysm

  <grid>_<target>, <grid>_<target>_f32    the targets of imagechain_common.TARGETS on float64 coordinates and on the same coordinates
                                          rounded to float32 (grids a, b); EXTRA_TARGETS on float64 only; c_crossed[_f32] the crossed edge
  <grid>_tf_<name>                        the transfer functions of imagechain_common.TFS and their product on float64 frequencies, at
                                          the flat indices <grid>_idx
  <grid>_airydisk, <grid>_airydisk_efield the Airy pattern over imagechain_common.airy_radius, at the same indices
  <grid>_polar                            uniform_cart_to_polar of imagechain_common.smooth_data, at the same indices
  psf_*                                   the displaced Gaussian on (65, 64): centroid in pixels and spatial units, autocrop to 100 and
                                          to 20 samples, its polar map, the four size metrics (also on float32-rounded data); the Airy
                                          pattern's first / last crossing of AIRY_LEVEL
  size_dev32                              |float32 model - float64 reference| of the size metrics, in their order

Prints, per function, the float64 numpy model's deviation from the reference next to the bound of imagechain_common, and the count of
samples on which the reference's float32 and float64 runs of each binary target disagree.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])

import imagechain_common as C  # noqa: E402
from prysm import objects, degradations, psf, detector, coordinates  # noqa: E402
from prysm_amd import imagechain_plan as IP  # noqa: E402

REF = {'objects': objects, 'degradations': degradations, 'psf': psf, 'detector': detector}
SIZES = (('fwhm', psf.fwhm), ('one_over_e', psf.one_over_e), ('one_over_e_sq', psf.one_over_e_sq))


def model_tf(name, tag):
    """the float64 numpy model of a transfer function on the grid's frequency vectors"""
    fx, fy = C.freq_vectors(tag)
    spec = {'smear': IP.smear_spec(*C.SMEAR), 'smear_x': IP.smear_spec(C.SMEAR[0], 0), 'jitter': IP.jitter_spec(C.JITTER),
            'pinhole_ft': IP.pinhole_spec(C.PINHOLE_R), 'slit_ft': IP.slit_spec(*C.SLITW), 'slit_ft_x': IP.slit_spec(C.SLITW[0], None),
            'slit_ft_y': IP.slit_spec(None, C.SLITW[1]), 'airydisk_ft': IP.airydisk_ft_spec(C.AIRY_FNO, C.AIRY_WVL),
            'pixel': IP.pixel_spec(*C.PIXEL), 'olpf': IP.olpf_spec(*C.OLPF)}
    specs = [spec[n] for n in C.PRODUCT] if name == 'product' else [spec[name]]
    return IP.tf_product(C.SHAPES[tag], specs, np.float64, fx=fx, fy=fy, out_complex=False)


def main():
    out = {}
    print('binary targets: samples on which the reference on float32 and on float64 coordinates disagree')
    for tag in ('a', 'b'):
        x, y = C.grid_xy(tag)
        x32, y32 = C.grid_xy(tag, np.float32)
        for name in C.TARGETS:
            r64 = np.asarray(C.call_target(objects, name, x, y))
            r32 = np.asarray(C.call_target(objects, name, x32, y32))
            out[f'{tag}_{name}'], out[f'{tag}_{name}_f32'] = r64, r32
            flips = int(np.sum(r64 != r32.astype(r64.dtype))) if r64.dtype == bool else int(np.sum(np.abs(r64 - r32) > 1e-3))
            print(f'  {tag} {name:14s} {flips} of {r64.size}')
            assert flips == 0
        for name in C.EXTRA_TARGETS:
            out[f'{tag}_{name}'] = np.asarray(C.call_target(objects, name, x, y))
    x, y = C.grid_xy('c')
    x32, y32 = C.grid_xy('c', np.float32)
    out['c_crossed'] = objects.slantededge(x, y, angle=4, crossed=True)
    out['c_crossed_f32'] = objects.slantededge(x32, y32, angle=4, crossed=True)
    print(f"  c crossed        {int(np.sum(np.abs(out['c_crossed'] - out['c_crossed_f32']) > 1e-3))} of {x.size}")

    print('transfer functions: max|float64 model - reference| and the bound (sum of 16 eps (1 + max|argument|))')
    for tag in ('a', 'b'):
        idx = C.sub_index(tag)
        out[f'{tag}_idx'] = idx.astype(np.int32)
        fxv, fyv = C.freq_vectors(tag)
        fx, fy = np.meshgrid(fxv, fyv)
        fr = np.hypot(fx, fy)
        prod = 1.0
        for name in C.TFS:
            ref = np.asarray(C.call_tf(REF, name, fx.copy(), fy.copy(), fr.copy()), np.float64)
            ref = np.broadcast_to(ref, fx.shape)
            out[f'{tag}_tf_{name}'] = ref.reshape(-1)[idx]
            if name in C.PRODUCT:
                prod = prod * ref
            dev, bound = np.abs(model_tf(name, tag) - ref).max(), C.tf_bound(name, tag, np.float64)
            print(f'  {tag} {name:12s} measured {dev:.2e}  bound {bound:.2e}')
            assert dev <= bound
        out[f'{tag}_tf_product'] = prod.reshape(-1)[idx]
        dev, bound = np.abs(model_tf('product', tag) - prod).max(), C.tf_bound('product', tag, np.float64)
        print(f'  {tag} {"product":12s} measured {dev:.2e}  bound {bound:.2e}')
        assert dev <= bound
        rad = C.airy_radius(tag)
        for name, fn, ef in (('airydisk', psf.airydisk, False), ('airydisk_efield', psf.airydisk_efield, True)):
            ref = np.asarray(fn(rad.copy(), C.AIRY_FNO, C.AIRY_WVL), np.float64)
            out[f'{tag}_{name}'] = ref.reshape(-1)[idx]
            mod = IP.tf_product(C.SHAPES[tag], [IP.airydisk_spec(C.AIRY_FNO, C.AIRY_WVL, efield=ef)], np.float64, fr=rad, out_complex=False)
            dev, bound = np.abs(mod - ref).max(), C.airy_bound(tag, np.float64, ef)
            print(f'  {tag} {name:12s} measured {dev:.2e}  bound {bound:.2e}')
            assert dev <= bound
        xv, yv = C.grid_vectors(tag)
        data = C.smooth_data(tag)
        rho, phi, pol = coordinates.uniform_cart_to_polar(xv, yv, data)
        out[f'{tag}_polar'] = np.asarray(pol, np.float64).reshape(-1)[idx]
        _, _, mod = IP.polar_resample(xv, yv, data, np.float64)
        dev, bound = np.abs(mod - pol), C.polar_bound(xv, yv, data, np.float64)
        print(f'  {tag} {"polar":12s} measured {dev.max():.2e}  bound {bound:.2e}  over the bound: {int((dev > bound).sum())} (none excluded)')
        assert dev.max() <= bound

    print('PSF metrics')
    d = C.gaussian_psf()
    dx = C.psf_dx()
    out['psf_centroid_px'] = np.array(psf.centroid(d, unit='pixels'))
    out['psf_centroid_spatial'] = np.array(psf.centroid(d, dx=dx))
    print('  centroid px', out['psf_centroid_px'], 'spatial', out['psf_centroid_spatial'])
    out['psf_autocrop100'], out['psf_autocrop20'] = psf.autocrop(d, 100), psf.autocrop(d, 20)
    xv, yv = C.psf_grid()
    rho, phi, pol = coordinates.uniform_cart_to_polar(xv, yv, d)
    out['psf_polar'] = np.asarray(pol, np.float64)
    out['psf_sizes'] = np.array([fn(d, dx=dx) for _, fn in SIZES] + [psf.estimate_size(d, 0.3, dx=dx)])
    d32 = d.astype(np.float32)
    out['psf_sizes_ref32'] = np.array([fn(d32, dx=dx) for _, fn in SIZES] + [psf.estimate_size(d32, 0.3, dx=dx)])
    metrics = ['fwhm', '1/e', '1/e^2', 0.3]
    x32, y32 = C.psf_grid(np.float32)
    r32, _, p32 = IP.polar_resample(x32, y32, d32, np.float32)
    r64, _, p64 = IP.polar_resample(xv, yv, d, np.float64)
    m32 = np.array([IP.estimate_size(p32, r32, m)[0] * (1 if m == 0.3 else 2) for m in metrics])
    m64 = np.array([IP.estimate_size(p64, r64, m)[0] * (1 if m == 0.3 else 2) for m in metrics])
    out['size_dev32'] = np.abs(m32 - out['psf_sizes'])
    print('  sizes (fwhm, 1/e, 1/e^2, level 0.3):', out['psf_sizes'])
    print('  float64 model - reference:', np.abs(m64 - out['psf_sizes']))
    print('  float32 model - reference:', out['size_dev32'], ' (the float32 tests allow four times this)')
    airy = C.airy_psf()
    out['psf_airy_first'] = np.array(psf.estimate_size(airy, C.AIRY_LEVEL, dx=dx, criteria='first'))
    out['psf_airy_last'] = np.array(psf.estimate_size(airy, C.AIRY_LEVEL, dx=dx, criteria='last'))
    _, _, pa = IP.polar_resample(xv, yv, airy, np.float64)
    mf, ml = IP.estimate_size(pa, r64, C.AIRY_LEVEL, 'first')[0], IP.estimate_size(pa, r64, C.AIRY_LEVEL, 'last')[0]
    print('  airy first / last:', out['psf_airy_first'], out['psf_airy_last'], ' float64 model - reference:',
          abs(mf - out['psf_airy_first']), abs(ml - out['psf_airy_last']))
    _, _, pa32 = IP.polar_resample(x32, y32, airy.astype(np.float32), np.float32)
    out['airy_dev32'] = np.array([abs(IP.estimate_size(pa32, r32, C.AIRY_LEVEL, c)[0] - out[f'psf_airy_{c}']) for c in ('first', 'last')])
    print('  airy float32 model - reference:', out['airy_dev32'])
    path = os.path.join(HERE, 'imagechain.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
