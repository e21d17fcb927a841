"""What tests/test_psdsynth_host.py, tests/test_gpu_psdsynth.py and tests/golden/make_golden_psdsynth.py share: the cases, access to
tests/golden/psdsynth.npz, the bounds and the comparison helpers.  Imports without a GPU.

Cases.  The random numbers of every case are default_rng(seed).random(shape), float32-rounded for the float32 runs; the golden is the
reference run in float64 on them (numpy.random.rand replaced by a function that returns them).
  EVEN (64, 48) and ODD (33, 47): synthesize_surface_from_psd with abc_psd(a = 1e4, b = 0.1, c = 2.5) on the frequency vectors of
    render_synthetic_surface (centre replaced) for a spacing of 0.1.
  ASYM: EVEN with the psd multiplied by 1 + 0.5 j / (cols - 1) along the columns: not symmetric about the centre, so the signal is
    not Hermitian and a half-spectrum inverse gives another real part.
  RENDER: 'circle' (100, 64, rms 5, 'circle', abc_psd a = 1e4, b = 1/100, c = 2), 'ab' (10, 33, no rms, no mask, ab_psd a = 1e2, b = 2),
    'hole' (20, 48, rms 2, an array mask: a disc with a hole), 'user' (10, 40, no rms, 'circle', a Gaussian callable).
  FIT: the reference's own cases -- abc on logspace(-2, 1, 200) with (100, 0.5, 3.5) to 1e-4, ab with (10, 2.5) to 1e-10 in both return
    forms -- and a noisy abc curve against the reference's coefficients.

Bounds.  The deviation is max|got - want| in units of eps(dtype) max|want|.  GOLDEN[key] is four times the deviation measured on an
MI355X (profiles/psdsynth/parity.txt), MODEL[key] the same against the numpy model (prysm_amd/psdsynth_plan.py) and never below
FLOOR = 2 (one rounding by the kernel, one by the model); each is capped at m n, the terms of one output sample's sum.  HOST[key]
bounds the numpy model against the golden on the host: four times what make_golden_psdsynth.py prints.
"""
import os

import numpy as np

from prysm_amd import psdsynth_plan as PP

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'psdsynth.npz')
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN_FILE))
    return _golden


def eps(dt):
    return float(np.finfo(dt).eps)


def tag(dt):
    return 'f32' if np.dtype(dt) == np.float32 else 'f64'


DTYPES = (np.float64, np.float32)

# ---------------------------------------------------------------- cases
EVEN, ODD = (64, 48), (33, 47)
SYNTH = {'even': (EVEN, 21), 'odd': (ODD, 22), 'asym': (EVEN, 23)}      # name: (shape, seed of the random numbers)
DXG = 0.1
ABC = dict(a=1e4, b=0.1, c=2.5)


def randnums(shape, seed, dtype=np.float64):
    return np.random.default_rng(seed).random(shape).astype(dtype)


def synth_case(name):
    """(psd, nu_x, nu_y) of a synthesize_surface_from_psd case, float64"""
    shape = SYNTH[name][0]
    nu_y, nu_x = PP.freq_vector(shape[0], DXG), PP.freq_vector(shape[1], DXG)
    nu = np.hypot(nu_x[None, :], nu_y[:, None])
    psd = ABC['a'] / (1 + (nu / ABC['b']) ** ABC['c'])
    if name == 'asym':
        psd = psd * (1 + 0.5 * np.arange(shape[1]) / (shape[1] - 1))[None, :]
    return psd, nu_x, nu_y


def gauss_psd(nu, a, s):
    """the user callable of the RENDER cases: a exp(-(nu / s)^2), on numpy arrays and on device tensors"""
    if isinstance(nu, np.ndarray):
        return a * np.exp(-(nu / s) ** 2)
    import torch
    return a * torch.exp(-(nu / s) ** 2)


def hole_mask(samples=48):
    j = np.arange(samples) - samples // 2
    r = np.hypot(j[None, :], j[:, None] + 0.5)
    return (r < 0.45 * samples) & (np.hypot(j[None, :] - 5, j[:, None] + 3) > 4.2)


# name: (size, samples, rms, mask, which function, its keyword arguments, seed of the random numbers)
RENDER = {
    'circle': (100, 64, 5, 'circle', 'abc', dict(a=1e4, b=1 / 100, c=2), 31),
    'ab': (10, 33, None, None, 'ab', dict(a=1e2, b=2), 32),
    'hole': (20, 48, 2, 'hole', 'abc', dict(a=1e3, b=0.05, c=3), 33),
    'user': (10, 40, None, 'circle', 'user', dict(a=50.0, s=0.8), 34),
}


def render_mask(name):
    m = RENDER[name][3]
    return hole_mask(RENDER[name][1]) if m == 'hole' else m


FIT_F = np.logspace(-2, 1, 200)
FIT_ABC, FIT_AB = (100.0, 0.5, 3.5), (10.0, 2.5)
FIT_RTOL_ABC, FIT_RTOL_AB = 1e-4, 1e-10
# the noisy curve against the reference's coefficients: both run scipy's least_squares from the same seed on the same residuals and
# stop at its ftol of 1e-8, so the coefficients agree far inside 1e-6
FIT_RTOL_NOISY = 1e-6


def noisy_curve():
    rng = np.random.default_rng(9)
    return PP.abc(FIT_F, *FIT_ABC) * 10.0 ** (0.05 * rng.standard_normal(FIT_F.size))


# ---------------------------------------------------------------- kernel coverage
COLS = (63, 64, 65)
COLS_ROWS = 9
FRAME = (4, 6)                       # rows and columns of frame around a window with ld > cols
SECOND_TRIP_SHAPE = (1024, 513)      # 525312 elements >= 2 x 256 x 1024: every first-stage thread of pm_psd_finish makes a second trip


def spectrum(shape, dtype, seed=41, zeros=True, batch=None):
    """a complex array with normal parts, a few exact zeros among them"""
    rng = np.random.default_rng(seed)
    full = ((batch,) if batch else ()) + tuple(shape)
    X = (rng.standard_normal(full) + 1j * rng.standard_normal(full)).astype(PP.cdtype(dtype))
    if zeros:
        X.reshape(-1)[::17] = 0
    return X


def positive(shape, dtype, seed=42):
    return (np.random.default_rng(seed).random(shape) * 3 + 0.01).astype(dtype)


def integer_field(shape, dtype, seed=43, batch=None):
    """|re| <= 1000 integers (the imaginary part is noise): the count and the sum of squares are exact in double in any order"""
    rng = np.random.default_rng(seed)
    full = ((batch,) if batch else ()) + tuple(shape)
    return (rng.integers(-1000, 1000, full, endpoint=True) + 1j * rng.standard_normal(full)).astype(PP.cdtype(dtype))


# ---------------------------------------------------------------- bounds, in units of eps(dtype) max|want|
FLOOR = 2.0
# key: (four times the measured deviation on an MI355X in float64, in float32, cap); the measured deviations are in the comments and in
# profiles/psdsynth/parity.txt.  The reference chain alone supports about 2 eps64 and 3 eps32 on the host; the device stays within
# an order of that
_N_EVEN, _N_ODD = EVEN[0] * EVEN[1], ODD[0] * ODD[1]
HOST = {
    'even': (13.4, 2.7),        # 3.33, 0.66
    'odd': (14.4, 2.2),         # 3.60, 0.55
    'asym': (11.3, 2.2),        # 2.81, 0.55
    'circle': (10.6, 3.0),      # 2.65, 0.75
    'ab': (17.4, 2.8),          # 4.35, 0.70
    'hole': (15.2, 2.9),        # 3.80, 0.71
    'user': (10.8, FLOOR),      # 2.69, 0.47
}
GOLDEN = {
    'even': (20.0, 13.5, _N_EVEN),          # 4.99, 3.37 (member 0 of a stack)
    'odd': (15.2, 5.8, _N_ODD),             # 3.79, 1.44
    'asym': (15.8, 8.4, _N_EVEN),           # 3.93, 2.09
    'circle': (15.8, 14.8, 64 * 64),        # 3.94, 3.70
    'ab': (20.2, 10.4, 33 * 33),            # 5.04, 2.59
    'hole': (18.9, 10.0, 48 * 48),          # 4.71, 2.49
    'user': (13.5, 9.7, 40 * 40),           # 3.37, 2.40
}
MODEL = {
    'z': (23.2, 24.0, 33 * 33),             # 5.79 ('hole'), 6.00 (member 1 of a batch of 64 x 64): the device's transforms against numpy's in double
    'signal': (FLOOR, FLOOR, 8),            # 1.46, 1.46 (hypot and the divide against numpy's)
    'scale': (FLOOR, FLOOR, 8),             # 0, 0
    'sums': (8.0, 8.0, SECOND_TRIP_SHAPE[0] * SECOND_TRIP_SHAPE[1]),      # 1.99 (the tree's order against numpy's pairwise sum)
}

measured = []      # (table, key, dtype tag, label, deviation, bound): what compare() saw, for the parity log


def deviation(got, want, dtype):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), 'NaN or inf positions differ'
    if not fin.any():
        return 0.0
    scale = np.abs(want[fin]).max()
    d = np.abs(got[fin] - want[fin]).max()
    return float(d / (eps(dtype) * scale)) if scale > 0 else float(d / eps(dtype))


def compare(table, key, got, want, dtype, label=''):
    """print measured against bound, remember it, and assert"""
    row = {'golden': GOLDEN, 'model': MODEL, 'host': HOST}[table][key]
    bound = row[1] if np.dtype(dtype) == np.float32 else row[0]
    if len(row) > 2:
        bound = min(bound, row[2])
    dev = deviation(got, want, dtype)
    measured.append((table, key, tag(dtype), label, dev, bound))
    print(f'{table:6s} {key:8s} {tag(dtype)} {label:28s} measured {dev:10.3f} eps   bound {bound:8.2f} eps')
    assert dev <= bound, f'{table} {key} {label}: {dev:.3f} eps above the bound of {bound:.2f} eps'
    return dev
