"""Writes tests/golden/polarization.npz from the reference (prysm/x/polarization.py, which runs on numpy).  Run by hand, with the
reference's directory given; the file holds data only:

    python tests/golden/make_golden_polarization.py /path/to/prysm

  in_theta, in_delta, in_alpha, in_angle, in_field, in_t     the inputs (polarization_common.make_inputs; t from cart_to_polar)
  <case>_64 / <case>_32      every case of polarization_common.MAP_CASES and SCALAR_CASES with the reference's precision at 64 / 32
  vvr_theta_after_64         the caller's theta after the reference's vector_vortex_retarder (it is multiplied by the charge in place)
  cpv_left, cpv_right, pauli_<k>     circular_pol_vector and pauli_spin_matrix
  chain6, chainv, chainc     a six-operand product, a product ending in a vector, a product with constants among the maps
  apply                      apply_polarization_optic(field, J)
  pauli                      pauli_coefficients of a random Jones map, (4, *GRID)
  kron                       broadcast_kron of two single 2 x 2
  mueller_nobroadcast        jones_to_mueller(CONST_A, broadcast=False)

Where the reference cannot take a map (theta of linear_retarder / linear_diattenuator and the wave plates, alpha) it is called pixel
by pixel with scalars.  Prints the deviation of the numpy model (prysm_amd/x/polarization_plan.py) from the reference in eps, per
case and precision, next to the bound the host test uses: the lines to copy into polarization_common.MODEL_DEV.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])

import polarization_common as C  # noqa: E402
from prysm.conf import config as ref_config  # noqa: E402
from prysm.coordinates import cart_to_polar, make_xy_grid  # noqa: E402
from prysm.x import polarization as ref  # noqa: E402
from prysm_amd.x import polarization_plan as PP  # noqa: E402

warnings.simplefilter('ignore')


def per_pixel(fn, *maps):
    """fn(scalars...) -> 2 x 2 at every pixel"""
    out = np.empty((*C.GRID, 2, 2), dtype=ref_config.precision_complex)
    for idx in np.ndindex(*C.GRID):
        out[idx] = fn(*[m[idx] for m in maps])
    return out


def reference_cases(precision, i):
    ref_config.precision = precision
    c = C.cdt(precision)
    mats, vec = C.jones_operands(precision)
    out = {
        'rot': ref.jones_rotation_matrix(i['theta'], shape=C.GRID),
        'ret': per_pixel(lambda d, t: ref.linear_retarder(d, t), i['delta'], i['theta']),
        'diat': per_pixel(lambda a, t: ref.linear_diattenuator(a, t), i['alpha'], i['theta']),
        'hwp': per_pixel(lambda t: ref.half_wave_plate(t), i['theta']),
        'pol': per_pixel(lambda t: ref.linear_polarizer(t), i['theta']),
        'vvr2': ref.vector_vortex_retarder(2, i['t'].copy(), C.VVR_RETARDANCE, C.VVR_ROTATE),
        'vvr6': ref.vector_vortex_retarder(6, i['t'].copy(), C.VVR_RETARDANCE, C.VVR_ROTATE),
        'lpv': ref.linear_pol_vector(i['angle']),
        'mueller': ref.jones_to_mueller(mats[0]),
        'rot_s': ref.jones_rotation_matrix(0.3),
        'ret_s': ref.linear_retarder(1.1, 0.4),
        'diat_s': ref.linear_diattenuator(0.3, 0.4),
        'hwp_s': ref.half_wave_plate(0.7),
        'qwp_s': ref.quarter_wave_plate(0.7),
        'pol_s': ref.linear_polarizer(0.7),
        'lpv_s': ref.linear_pol_vector(30.0),
        'mueller_s': ref.jones_to_mueller(C.CONST_A.astype(c)),
    }
    # Mawet 2009 eq. 7: the leakage term on both diagonal elements; the reference's own products around it
    lhs = out['vvr2'] * 0
    th = i['t'] * 2
    lhs[..., 0, 0], lhs[..., 0, 1], lhs[..., 1, 0], lhs[..., 1, 1] = np.cos(th), np.sin(th), np.sin(th), -np.cos(th)
    lhs = lhs * np.sin(C.VVR_RETARDANCE / 2)
    jc = -1j * np.cos(C.VVR_RETARDANCE / 2)
    lhs[..., 0, 0] += jc
    lhs[..., 1, 1] += jc
    out['vvr2_leak'] = (ref.jones_rotation_matrix(-C.VVR_ROTATE) @ lhs @ ref.jones_rotation_matrix(C.VVR_ROTATE)).astype(c)
    out['mueller_ret'] = C.mueller_samples(ref.jones_to_mueller(out['ret']))
    out['mueller_vvr2'] = C.mueller_samples(ref.jones_to_mueller(out['vvr2']))
    extra = {
        'chain6': mats[0] @ mats[1] @ mats[2] @ mats[3] @ mats[4] @ mats[5],
        'chainv': mats[0] @ mats[1] @ vec,
        'chainc': C.CONST_A.astype(c) @ mats[0] @ C.CONST_B.astype(c) @ mats[1],
        'apply': ref.apply_polarization_optic(i['field'], mats[0]),
        'pauli': np.stack(ref.pauli_coefficients(mats[0])),
        'kron': ref.broadcast_kron(C.CONST_A.astype(c), C.CONST_B.astype(c)),
        'mueller_nobroadcast': ref.jones_to_mueller(C.CONST_A.astype(c), broadcast=False),
        'cpv_left': ref.circular_pol_vector('left'), 'cpv_right': ref.circular_pol_vector('right'),
    }
    for k in range(4):
        extra[f'pauli_{k}'] = ref.pauli_spin_matrix(k)
    return out, extra


def main():
    ref_config.precision = 64
    x, y = make_xy_grid(C.GRID, diameter=2)
    _, t = cart_to_polar(x, y)
    data = C.make_inputs(t)
    lines = {}
    for precision in C.PRECISIONS:
        r, c = C.rdt(precision), C.cdt(precision)
        i = {k[3:]: v.astype(c if k == 'in_field' else r) for k, v in data.items()}
        cases, extra = reference_cases(precision, i)
        if precision == 64:
            th = i['t'].copy()
            ref.vector_vortex_retarder(2, th, C.VVR_RETARDANCE, C.VVR_ROTATE)
            data['vvr_theta_after_64'] = th
        for name, v in {**cases, **extra}.items():
            v = np.asarray(v)
            want = r if name.startswith('mueller') else c
            assert v.dtype == want, (name, v.dtype, want)
            data[f'{name}_{precision}'] = v
        model = C.model_cases(precision, i)
        for name in C.MAP_CASES + C.SCALAR_CASES:
            scale = C.case_scale(name, precision, data)
            lines.setdefault(name, []).append(C.dev_eps(model[name], cases[name], precision, scale))
        mats, vec = C.jones_operands(precision)
        print(f'precision {precision}: model vs reference, largest |d| / bound (<= 1 passes)')
        for name, ops, tail in (('chain6', mats, False), ('chainv', [mats[0], mats[1], vec], True),
                                ('chainc', [C.CONST_A.astype(c), mats[0], C.CONST_B.astype(c), mats[1]], False)):
            d = np.abs(PP.chain(ops, tail) - extra[name])
            print(f'  {name:8s} {np.max(d / C.chain_bound(ops, precision)):.3f} of 4 (K - 1) eps prod|A|')
        d = np.abs(PP.scale(mats[0], i['field']) - extra['apply'])
        print(f'  apply    {np.max(d / C.scale_bound(mats[0], i["field"], precision)):.3f} of {C.SCALE_C} eps |field| |J|')
        print(f'  pauli    array_equal: {np.array_equal(PP.pauli(mats[0]), extra["pauli"])}')
        print(f'  mueller_nobroadcast vs model: {C.dev_eps(PP.mueller(C.CONST_A.astype(c)), extra["mueller_nobroadcast"], precision):.2f} eps')
    ref_config.precision = 64
    print('MODEL_DEV, in eps (precision 64, precision 32); the host test bounds each case by four times its figure:')
    for name, (a, b) in lines.items():
        print(f"    '{name}': ({a:.3g}, {b:.3g}),    # bound {4 * a:.3g}, {4 * b:.3g}")
    path = os.path.join(HERE, 'polarization.npz')
    np.savez_compressed(path, **data)
    print(f'{path}: {os.path.getsize(path)} bytes, {len(data)} arrays')


if __name__ == '__main__':
    main()
