"""What tests/test_polarization_host.py, tests/test_gpu_polarization.py and tests/golden/make_golden_polarization.py share: the cases,
the inputs, access to tests/golden/polarization.npz and the bounds.  Imports without a GPU.

The golden.  GRID = (19, 35).  Stored inputs (seed SEED): theta and delta uniform in (-3.1, 3.1), alpha uniform in (0, 1), angle in
degrees uniform in (-180, 180), a complex field, the vortex angle t of coordinates.cart_to_polar on make_xy_grid(GRID, diameter=2).
The Jones operands of the products (jones_operands, seed SEED + 1) are regenerated, not stored.  Outputs <case>_64 / <case>_32 come
from the reference with its precision at 64 / 32 and the inputs rounded to that precision.  Where the reference cannot take a map
(theta of the retarder and the diattenuator, alpha: the departures in prysm_amd/x/polarization.py) the golden is the reference called
pixel by pixel with scalars.  Mueller matrices of generated optics are stored at every MUELLER_STRIDE-th pixel (flat index) to keep
the file small; every stored sample is compared.

Bounds.
  exact       relayout, to_planes / from_planes, pauli_coefficients (one correctly rounded add, an exact halving, an exact 1j *),
              pauli_spin_matrix, the polarization vectors' constants, Mueller of the identity, linear_retarder(0).
  scale       |d| <= 2.5 eps |field| |J_ij|: each side is within sqrt(5) / 2 eps of the exact complex product (SCALE_C).
  chain       |d_ij| <= 4 (K - 1) eps (|A_1| ... |A_K|)_ij on identical operands: a 2-term complex inner product carries at most
              (sqrt(5) / 2 + 1 / 2) eps relative to sum |a| |b|, doubled for the two sides (chain_bound).
  generators  absolute, in eps of the precision, the components being O(1): four times the largest deviation measured from the golden
              of the same precision.  MODEL_DEV: the numpy model (polarization_plan.py), printed by make_golden_polarization.py --
              the host test's constants.  GPU_DEV: the kernels on an MI355X -- the GPU test's constants.  Both in eps.
  Mueller     relative to ||J||_F^2 of the pixel, in eps, by the same rule (case 'mueller').
The scalar cases (single 2 x 2 and 2-vectors) are host numpy in both tests and take MODEL_DEV.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'polarization.npz')
_golden = None

GRID = (19, 35)
SEED = 31
CHARGES = (2, 6)
VVR_RETARDANCE, VVR_ROTATE = 2.5, 0.3
MUELLER_STRIDE = 4
PRECISIONS = (64, 32)
SCALE_C = 2.5

# generator cases on maps: name -> the largest deviation from the golden in eps, (precision 64, precision 32)
MAP_CASES = ('rot', 'ret', 'diat', 'hwp', 'pol', 'vvr2', 'vvr6', 'vvr2_leak', 'lpv', 'mueller', 'mueller_ret', 'mueller_vvr2')
SCALAR_CASES = ('rot_s', 'ret_s', 'diat_s', 'hwp_s', 'qwp_s', 'pol_s', 'lpv_s', 'mueller_s')
# measured: make_golden_polarization.py (numpy model against the reference), in eps
MODEL_DEV = {
    'rot': (0, 0), 'ret': (0.75, 1.12), 'diat': (1, 1), 'hwp': (0.5, 0.5), 'pol': (0, 0), 'vvr2': (1, 1), 'vvr6': (1, 1),
    'vvr2_leak': (1.03, 1.03), 'lpv': (2, 2), 'mueller': (0.697, 0.733), 'mueller_ret': (1, 1), 'mueller_vvr2': (0.789, 1.05),
    'rot_s': (0, 0), 'ret_s': (0.707, 0.5), 'diat_s': (0, 0.25), 'hwp_s': (0.125, 0.125), 'qwp_s': (0, 0), 'pol_s': (0, 0),
    'lpv_s': (0, 0), 'mueller_s': (0.327, 0.327),
}
# measured on an MI355X: tests/test_gpu_polarization.py prints each figure before it asserts, in eps
GPU_DEV = {
    'rot': (0.5, 0.5), 'ret': (1.581, 1.601), 'diat': (2, 1.5), 'hwp': (1.5, 1.5), 'pol': (1, 1), 'vvr2': (1, 1), 'vvr6': (1, 1),
    'vvr2_leak': (1.031, 1.031), 'lpv': (2, 2), 'mueller': (0.6968, 0.7332), 'mueller_ret': (1.75, 1.5),
    'mueller_vvr2': (0.7892, 1.052),
}


def bound(case, precision, gpu):
    """the constant of a case, in eps: four times the measured deviation"""
    table = GPU_DEV if gpu and case in GPU_DEV else MODEL_DEV
    return 4.0 * table[case][PRECISIONS.index(precision)]


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def rdt(precision):
    return np.float32 if precision == 32 else np.float64


def cdt(precision):
    return np.complex64 if precision == 32 else np.complex128


def eps(precision):
    return float(np.finfo(rdt(precision)).eps)


def make_inputs(t):
    """the stored inputs, float64 / complex128; t: the vortex angle (the generator takes it from the reference's cart_to_polar)"""
    rng = np.random.default_rng(SEED)
    out = {
        'in_theta': rng.uniform(-3.1, 3.1, GRID), 'in_delta': rng.uniform(-3.1, 3.1, GRID), 'in_alpha': rng.uniform(0, 1, GRID),
        'in_angle': rng.uniform(-180, 180, GRID),
        'in_field': rng.standard_normal(GRID) + 1j * rng.standard_normal(GRID),
    }
    out['in_t'] = np.asarray(t, dtype=np.float64)
    return out


def inputs(precision):
    """theta, delta, alpha, angle, field, t of the golden rounded to the precision"""
    g = golden()
    r, c = rdt(precision), cdt(precision)
    return {k[3:]: g[k].astype(c if k == 'in_field' else r) for k in g if k.startswith('in_')}


def jones_operands(precision, shape=GRID, count=6, seed=SEED + 1):
    """count random Jones maps (*shape, 2, 2) and one vector map (*shape, 2, 1), rounded to the precision"""
    rng = np.random.default_rng(seed)
    c = cdt(precision)
    mats = [(rng.standard_normal((*shape, 2, 2)) + 1j * rng.standard_normal((*shape, 2, 2))).astype(c) for _ in range(count)]
    vec = (rng.standard_normal((*shape, 2, 1)) + 1j * rng.standard_normal((*shape, 2, 1))).astype(c)
    return mats, vec


CONST_A = np.array([[0.3 - 0.2j, 1.1 + 0.4j], [-0.7 + 0.9j, 0.5 + 0.1j]])
CONST_B = np.array([[1.2 + 0.0j, -0.3 + 0.8j], [0.6 - 0.5j, -0.9 + 0.2j]])
CONST_V = np.array([[0.4 + 0.3j], [-0.8 + 0.1j]])


def chain_bound(operands, precision):
    """4 (K - 1) eps (|A_1| ... |A_K|)_ij"""
    ops = [np.abs(np.asarray(o)).astype(np.float64) for o in operands]
    acc = ops[0]
    for o in ops[1:]:
        acc = acc @ o
    return 4 * (len(ops) - 1) * eps(precision) * acc


def scale_bound(jones, field, precision):
    return SCALE_C * eps(precision) * np.abs(np.asarray(field))[..., None, None] * np.abs(np.asarray(jones))


def mueller_scale(jones):
    """||J||_F^2 per pixel, shaped to broadcast against (..., 4, 4)"""
    j = np.asarray(jones).astype(np.complex128)
    return np.sum(np.abs(j) ** 2, axis=(-2, -1))[..., None, None]


def mueller_samples(m):
    """the stored samples of a (*GRID, 4, 4) Mueller map of a generated optic"""
    return np.asarray(m).reshape(-1, 4, 4)[::MUELLER_STRIDE]


def dev_eps(got, want, precision, scale=1.0):
    """the largest |got - want| / scale in eps of the precision"""
    d = np.abs(np.asarray(got).astype(np.complex128) - np.asarray(want).astype(np.complex128)) / scale
    return float(np.max(d)) / eps(precision) if d.size else 0.0


def model_cases(precision, inp=None):
    """every generator and Mueller case from the numpy model (prysm_amd/x/polarization_plan.py), name -> array, shaped as the golden"""
    from prysm_amd.x import polarization_plan as PP
    i = inputs(precision) if inp is None else inp
    c = cdt(precision)
    mats, _ = jones_operands(precision)
    out = {
        'rot': PP.optic(PP.ROTATION, [i['theta']], GRID, c),
        'ret': PP.optic(PP.RETARDER, [i['delta'], i['theta']], GRID, c),
        'diat': PP.optic(PP.DIATTENUATOR, [i['alpha'], i['theta']], GRID, c),
        'hwp': PP.optic(PP.RETARDER, [np.pi, i['theta']], GRID, c),
        'pol': PP.optic(PP.DIATTENUATOR, [0, i['theta']], GRID, c),
        'vvr2': PP.optic(PP.VORTEX, [i['t'], VVR_RETARDANCE, VVR_ROTATE], GRID, c, charge=2),
        'vvr6': PP.optic(PP.VORTEX, [i['t'], VVR_RETARDANCE, VVR_ROTATE], GRID, c, charge=6),
        'vvr2_leak': PP.optic(PP.VORTEX, [i['t'], VVR_RETARDANCE, VVR_ROTATE], GRID, c, charge=2, leak=True),
        'lpv': PP.optic(PP.LINPOL_VECTOR, [i['angle']], GRID, c, charge=np.pi / 180),
        'mueller': PP.mueller(mats[0]),
        'rot_s': PP.optic(PP.ROTATION, [0.3], (), c),
        'ret_s': PP.optic(PP.RETARDER, [1.1, 0.4], (), c),
        'diat_s': PP.optic(PP.DIATTENUATOR, [0.3, 0.4], (), c),
        'hwp_s': PP.optic(PP.RETARDER, [np.pi, 0.7], (), c),
        'qwp_s': PP.optic(PP.RETARDER, [np.pi / 2, 0.7], (), c),
        'pol_s': PP.optic(PP.DIATTENUATOR, [0, 0.7], (), c),
        'lpv_s': PP.optic(PP.LINPOL_VECTOR, [30.0], (), c, charge=np.pi / 180).reshape(2),
        'mueller_s': PP.mueller(CONST_A.astype(c)),
    }
    out['mueller_ret'] = mueller_samples(PP.mueller(out['ret']))
    out['mueller_vvr2'] = mueller_samples(PP.mueller(out['vvr2']))
    return out


def case_scale(name, precision, g=None):
    """what a case's deviation is relative to: 1 for the generators, ||J||_F^2 of the pixel for the Mueller cases (J: the golden's)"""
    if not name.startswith('mueller'):
        return 1.0
    tag = f'_{precision}'
    if name == 'mueller':
        return mueller_scale(jones_operands(precision)[0][0])
    if name == 'mueller_s':
        return mueller_scale(CONST_A.astype(cdt(precision)))
    g = golden() if g is None else g
    return mueller_scale(g[name[len('mueller_'):] + tag]).reshape(-1, 1, 1)[::MUELLER_STRIDE]
