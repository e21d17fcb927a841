"""What tests/test_sensors_host.py, tests/test_gpu_sensors.py and tests/golden/make_golden_sensors.py share: the cases, the inputs,
access to tests/golden/sensors.npz and the bounds.  Imports without a GPU.

PSI.  Frames are PSI_AMPL (1 + PSI_VIS cos(phi + shift_k)) on PSI_SHAPE = (33, 70), phi uniform in (-3.1, 3.1) (stored in the golden).
Schemes: SCHWIDER, ZYGO_THIRTEEN_FRAME, design_scheme(7), design_scheme(9, stepsize=pi / 3); the reference's sign and error for the
unwindowed schemes are part of the golden.  Compared: the wrapped difference angle(exp(i (w - w_ref))).
  float frames     PSI_EPS_MULT eps of the output dtype: four times the largest deviation measured on an MI355X from the reference's
                   result of the same precision, which was 4.0 eps in float64 (design_scheme(7); 2.0 eps for the other three) and
                   4.0 eps in float32 (ZYGO_THIRTEEN_FRAME; 2.0 eps for the other three) -> 16.  For orientation: the reference's own
                   float64 run is 4.4e-16 = 2 eps from the truth, its float32 run, which accumulates in float32, 3.3e-7 = 2.8 eps;
                   the sums here run in double and are rounded once.
  integer frames   against phi itself.  A frame sample is off by at most 0.5 after rounding, so the numerator is off by at most
                   en = 0.5 sum|s_k| and the denominator by ed = 0.5 sum|c_k|.  The exact pair has length R = ampl vis G with the
                   scheme's gain G = |sum_k s_k sin(shift_k)| (= |sum_k c_k cos(shift_k)| for these schemes).  A vector of length R
                   moved by at most e = hypot(en, ed) turns by at most asin(e / R) (>= the atan(e / R) of a perpendicular move):
                   int_bound().  Plus 8 eps of the output dtype for the final rounding and atan2.

Shack-Hartmann.  SH_CASES on dx = 4 / 64, efl = 50, wavelength = 0.5, float64 and float32-rounded coordinates.  In float64 the set
of samples whose lenslet count differs from the reference's must be empty.  The field agrees within SH_C eps max|arg|, max|arg| =
|k| (4 lenslets) (hw^2 + hh^2) / (2 efl) = 251 rad for the square apertures: four times the largest deviation measured on an MI355X,
which was 0.003 eps max|arg| in float64 (1.6e-16) and in float32 (8.4e-08) on every case -> c = 0.012.  That is one unit in the last
place of cos / sin and no more, because the argument k total is formed in the coordinates' precision exactly as the reference forms
it (to the bit).  This settles the float32 kernel's argument: forming it in double would move the float32 result AWAY from the
reference's float32 run by one rounding of a 251 rad argument, 1.5e-5 rad, two hundred times the deviation measured now.  Samples
where the reference's float32 and float64 runs disagree on membership are left out of the float32 comparison; the generator prints
their number (0 on every case), at most SH_EXCLUDE_CAP of the samples.

PS/PDI and SRI.  Compared relative to the golden's peak with the bounds the executor tests use for to_fpm_and_back (gpu_common.TOL64 /
TOL32, taken from tests/test_gpu_executors.py).
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sensors.npz')
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def eps(dt):
    return float(np.finfo(dt).eps)


def wrapped_diff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))))


# ---------------------------------------------------------------- PSI
PSI_SHAPE = (33, 70)
PSI_AMPL, PSI_VIS = 2000.0, 0.8
PSI_SEED = 20
PSI_SCHEMES = ('schwider', 'zygo13', 'design7', 'design9')
PSI_EPS_MULT = {np.float64: 16.0, np.float32: 16.0}
INT_AMPL = {np.uint16: 2000.0, np.uint8: 141.0}      # 141 (1 + 0.8) = 253.8 <= 255


def make_phi():
    return np.random.default_rng(PSI_SEED).uniform(-3.1, 3.1, PSI_SHAPE)


def scheme(mod, name):
    """a scheme of PSI_SCHEMES from a psi module (the reference's or this library's)"""
    if name == 'schwider':
        return mod.SCHWIDER
    if name == 'zygo13':
        return mod.ZYGO_THIRTEEN_FRAME
    if name == 'design7':
        return mod.design_scheme(7)
    return mod.design_scheme(9, stepsize=np.pi / 3)


def frames(phi, shifts, dtype=np.float64, ampl=PSI_AMPL):
    """the K frames in float64, then rounded to the nearest value of dtype"""
    out = []
    for d in np.asarray(shifts, dtype=np.float64):
        g = ampl * (1 + PSI_VIS * np.cos(phi + d))
        out.append(np.rint(g).astype(dtype) if np.dtype(dtype).kind == 'u' else g.astype(dtype))
    return out


def int_bound(sch, ampl, out_dtype):
    s, c, d = (np.asarray(v, dtype=np.float64) for v in (sch.s, sch.c, sch.shifts))
    gain = abs(np.sum(s * np.sin(d)))
    e = math.hypot(0.5 * np.sum(np.abs(s)), 0.5 * np.sum(np.abs(c)))
    return math.asin(e / (ampl * PSI_VIS * gain)) + 8 * eps(out_dtype)


PSI_COLS = (1, 63, 64, 65, 257)
PSI_TALL = (262145, 3, 5)      # rows, cols, K: the second trip of the row loop (65535 x 4 rows per trip)


def random_frames(K, shape, dtype, seed=3):
    rng = np.random.default_rng(seed + K)
    if np.dtype(dtype).kind == 'u':
        return [rng.integers(0, np.iinfo(dtype).max, shape, endpoint=True).astype(dtype) for _ in range(K)]
    return [rng.uniform(0, 4000, shape).astype(dtype) for _ in range(K)]


def random_weights(K, seed=5):
    rng = np.random.default_rng(seed + K)
    return rng.uniform(-2, 2, K), rng.uniform(-2, 2, K)


# ---------------------------------------------------------------- Shack-Hartmann
SH_DX, SH_EFL, SH_WVL = 4 / 64, 50.0, 0.5
SH_EXCLUDE_CAP = 0.01
SH_C = {np.float64: 0.012, np.float32: 0.012}
# name: (n, grid shape, shift, pitch, aperture, aperture_kwargs)
SH_CASES = {
    'n3_48': (3, (48, 48), False, 1.0, 'rectangle', {}),
    'n4_64': (4, (64, 64), False, 1.0, 'rectangle', {}),
    'n4_64_shift': (4, (64, 64), True, 1.0, 'rectangle', {}),
    'n3_50': (3, (50, 50), False, 1.0, 'rectangle', {}),
    'n23_40x56_shift': ((2, 3), (40, 56), True, 1.0, 'rectangle', {}),
    'n4_61_p093': (4, (61, 61), False, 0.93, 'rectangle', {}),
    'circle_n4_64': (4, (64, 64), False, 1.0, 'circle', {}),
    'height_n3_48': (3, (48, 48), False, 1.0, 'rectangle', {'height': 0.3}),
    'n6_48_overhang': (6, (48, 48), False, 1.0, 'rectangle', {}),
}
SH_TIE_CASES = ('n3_48', 'n4_64', 'n4_64_shift', 'n3_50', 'n23_40x56_shift')
SH_FORMS_CASE = 'n23_40x56_shift'
# lenslets wholly off the grid: the reference raises IndexError on their empty windows, so this case's golden is the windowless sum of
# sensors_plan.lenslet_screen, which equals the reference to the bit (float64) on every case the reference runs
SH_MODEL_CASES = ('n6_48_overhang',)


def sh_vectors(shape, dtype=np.float64):
    ny, nx = shape
    x = np.arange(-(nx // 2), -(nx // 2) + nx, dtype=np.float64) * SH_DX
    y = np.arange(-(ny // 2), -(ny // 2) + ny, dtype=np.float64) * SH_DX
    return x.astype(dtype), y.astype(dtype)


def sh_xy(shape, dtype=np.float64):
    return np.meshgrid(*sh_vectors(shape, dtype))


def sh_max_arg(total_max):
    return 2 * math.pi / (SH_WVL / 1e3) * total_max


# ---------------------------------------------------------------- PS/PDI and SRI
IF_N, IF_EPD, IF_EFL, IF_WVL = 96, 10.0, 100.0, 0.6328
PDI_KW = dict(test_arm_offset=16, test_arm_fov=16, grating_rulings=16, test_arm_samples=48, pinhole_samples=24)
PDI_CASES = [(gt, ax, ps) for gt in ('sin_amp', 'ronchi') for ax in ('x', 'y') for ps in (0, 1.3)]
SRI_FIBER_SAMPLES = 32
SRI_SHIFTS = (0, 0.3)
PDI_FIELDS = ('intensity', 'total_field', 'cam_ref', 'cam_test', 'fpm_ref_at', 'fpm_ref_after', 'fpm_test_at', 'fpm_test_after')
# rectangle_pulse: x mod period == 0 (0, +-period, 2 period), the duty edge (duty period and just either side), negative x
PULSE_KW = dict(duty=0.3, amplitude=0.4, offset=0.6, period=1.5)
PULSE_X = np.array([0.0, 1.5, -1.5, 3.0, 0.45, 0.45 - 1e-9, 0.45 + 1e-9, -0.2, -1.2, -1.05, 0.1, 1.4999, 2.0, -7.3, 1e-17, -1e-17])


def pdi_key(gt, ax, ps):
    return f'pdi_{gt}_{ax}_{"0" if ps == 0 else "1p3"}'


def pupil():
    """(x, y, amp, opd) on IF_N samples across IF_EPD, numpy float64: a circle with 40 nm of Z(3,1) plus 25 nm of Z(2,2) (orthonormal:
    sqrt(8) (3 r^3 - 2 r) cos t and sqrt(6) r^2 cos 2t on the unit disc); x = fftrange(N) EPD / N"""
    v = np.arange(-(IF_N // 2), -(IF_N // 2) + IF_N, dtype=np.float64) * (IF_EPD / IF_N)
    x, y = np.meshgrid(v, v)
    r, t = np.sqrt(x * x + y * y), np.arctan2(y, x)
    rn = r / (IF_EPD / 2)
    amp = (r <= IF_EPD / 2).astype(np.float64)
    opd = 40 * math.sqrt(8) * (3 * rn ** 3 - 2 * rn) * np.cos(t) + 25 * math.sqrt(6) * rn ** 2 * np.cos(2 * t)
    return x, y, amp, opd


def pupil_field(amp, opd):
    """amp exp(i 2 pi / (wavelength 1e3) opd) in complex128, numpy"""
    return amp * np.exp(1j * (2 * np.pi / (IF_WVL * 1e3)) * opd)


def sample_idx(shape, stride):
    """flat indices at which a map is stored: every stride-th sample plus the central row and column (whole maps would be megabytes)"""
    ny, nx = shape
    idx = set(range(0, ny * nx, stride))
    idx.update((ny // 2) * nx + np.arange(nx))
    idx.update(np.arange(ny) * nx + nx // 2)
    return np.array(sorted(idx), dtype=np.int64)


PDI_STRIDE = {'pupil': 23, 'fpm_ref': 3, 'fpm_test': 7}


def pdi_fields(model_out, debug):
    """the eight compared arrays of a forward model, in PDI_FIELDS order, as numpy-convertible objects"""
    return (model_out, debug['total_field'], debug['at_camera']['ref'], debug['at_camera']['test'], debug['at_fpm']['ref'][0],
            debug['at_fpm']['ref'][1], debug['at_fpm']['test'][0], debug['at_fpm']['test'][1])


def pdi_stride(field):
    return PDI_STRIDE['fpm_ref' if field.startswith('fpm_ref') else 'fpm_test' if field.startswith('fpm_test') else 'pupil']
