"""What tests/test_interferogram_host.py, tests/test_gpu_interferogram.py and tests/golden/make_golden_interferogram.py share: the cases,
access to tests/golden/interferogram.npz, the bounds and the comparison helper.  Imports without a GPU.

Cases.  MAIN: shape (37, 53), dx 0.1, make_xy_grid coordinates, default_rng(3): z = 5 N(0, 1) + 30 x - 20 y + 8 (x^2 + y^2) + 1000,
12 pixels chosen without replacement get +-200 added, NaN where r > 1.7, where hypot(x - 0.4, y + 0.3) < 0.25, in the first 3 columns
and in the last 2 rows.  The reference gives a dropout of 55.33 %, crop() to (33, 33), rms = std = 15.88 after piston, tip/tilt, power
and piston removal, and spike_clip(3) then invalidates 5 of 876 valid pixels.  MAIN as float32: the golden is the reference run in
float64 on the float32-rounded input.  INF: MAIN with +inf at INF_AT.  SQUARE: (64, 48), dx 0.1, default_rng(5), no NaN, for the
windows, the PSD, the band-limited RMS and the four filters.

Bounds.  A floating result is compared with the reference's float64 result in the golden; the deviation is max|got - want| in units
of eps(dtype) max|want| (dtype: the precision the compared value was rounded to -- float64 for the statistics, which are sums in
double whatever the data's precision).  BOUND[key] is four times the deviation measured on an MI355X (profiles/interferogram/
parity.txt has the measurements), as for the sensors, and never above the cap that is the third entry of BOUND[key]: n eps of the sum
of the magnitudes for a sum of n terms, i.e. n in these units.  Where four times the measured deviation is below it the bound is
FLOOR = 2: one rounding of the result by the kernel and one by the reference.  pv in float64 is exact, the clipped set, the counts,
the boxes and the positions of NaN are compared exactly.

Against the numpy model (prysm_amd/interferogram_plan.py) the kernels do the same arithmetic but for the order of the long sums, so
MODEL[key] bounds those by the same rule; small-integer data must agree to the bit.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'interferogram.npz')
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def eps(dt):
    return float(np.finfo(dt).eps)


def tag(dt):
    return 'f32' if np.dtype(dt) == np.float32 else 'f64'


# ---------------------------------------------------------------- cases
MAIN_SHAPE, DX, MAIN_SEED = (37, 53), 0.1, 3
CROPPED = (33, 33)
INF_AT = (20, 30)
SQUARE_SHAPE, SQUARE_SEED = (64, 48), 5
NSIGMA = 3
FILTERS = (('lp', 1.0), ('hp', 1.0), ('bp', (0.5, 2.0)), ('br', (0.5, 2.0)))
BANDS = (('f', dict(flow=0.3, fhigh=2.0)), ('wl', dict(wllow=0.5)))
TIS_WVL = 0.6328
PAD_SAMPLES = (4, 7)
STAGES = ('piston', 'tilt', 'power', 'piston2')


def grid(shape, dx=DX):
    """make_xy_grid(shape, dx=dx) in float64 numpy"""
    x = (np.arange(shape[1]) - shape[1] // 2) * dx
    y = (np.arange(shape[0]) - shape[0] // 2) * dx
    return np.meshgrid(x, y)


def main_case(dtype=np.float64, inf=False):
    x, y = grid(MAIN_SHAPE)
    rng = np.random.default_rng(MAIN_SEED)
    z = 5 * rng.standard_normal(MAIN_SHAPE) + 30 * x - 20 * y + 8 * (x * x + y * y) + 1000
    idx = rng.choice(z.size, 12, replace=False)
    z.flat[idx] += 200 * rng.choice([-1.0, 1.0], 12)
    z[np.hypot(x, y) > 1.7] = np.nan
    z[np.hypot(x - 0.4, y + 0.3) < 0.25] = np.nan
    z[:, :3] = np.nan
    z[-2:, :] = np.nan
    if inf:
        assert np.isfinite(z[INF_AT])
        z[INF_AT] = np.inf
    return z.astype(dtype)


def user_mask():
    """the mask of the mask() test: a disc that cuts into the valid region"""
    x, y = grid(MAIN_SHAPE)
    return np.hypot(x + 0.3, y) < 1.2


def square_case(dtype=np.float64):
    x, y = grid(SQUARE_SHAPE)
    rng = np.random.default_rng(SQUARE_SEED)
    z = 20 * np.sin(2 * np.pi * 0.7 * x) * np.cos(2 * np.pi * 0.4 * y) + 6 * rng.standard_normal(SQUARE_SHAPE) + 3 * x - 2 * y + 15
    return z.astype(dtype)


# ---------------------------------------------------------------- kernel coverage
TINY_SHAPES = ((1, 1), (1, 7), (5, 1))
ALL_NAN_SHAPE = (3, 5)
COLS = (63, 64, 65)
COLS_ROWS = 9
SECOND_TRIP_SHAPE = (1024, 513)      # 525312 elements >= 2 x 256 x 1024: every first-stage thread makes a second trip; below 2^22
FRAME = (4, 6)                       # rows and columns of frame around a window with ld > cols
FIT_SHAPE, FIT_A, FIT_B = (17, 23), 0.375, -1.25      # z = a x + b y on integer coordinates: every product and sum exact in double


def integer_data(shape, dtype, seed=11, nan_every=37):
    """|z| <= 1000 integers with a few NaN: count, sum, sum of squares, extrema and mean are exact in double in any order"""
    rng = np.random.default_rng(seed)
    z = rng.integers(-1000, 1000, shape, endpoint=True).astype(dtype)
    z.flat[::nan_every] = np.nan
    return z


def noisy_data(shape, dtype, seed=7):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    z = 40 * rng.standard_normal(shape) + 0.3 * xx - 0.2 * yy + 500
    z[rng.random(shape) < 0.2] = np.nan
    return z.astype(dtype)


# ---------------------------------------------------------------- bounds, in units of eps(dtype) max|want|
FLOOR = 2.0
# key: (four times the measured deviation on an MI355X in float64, in float32, cap); the measured deviations are in the comments and in
# profiles/interferogram/parity.txt
_N_MAIN, _N_SQ = 876, SQUARE_SHAPE[0] * SQUARE_SHAPE[1]
BOUND = {
    'stat': (2.5, FLOOR, _N_MAIN),          # 0.63 (1.01 on the raw data: the mean of 876 values around 1000), 0.12
    'coef': (9.4, 2.1, _N_MAIN),            # 2.34 (fit_plane; normal equations against the reference's SVD), 0.52
    'removed': (23.8, 2.3, _N_MAIN),        # 5.94: a mean of 1005 off by one unit in its last place, seen on data of +-250; 0.57
    'slope': (5.8, 4.5, 8),                 # 1.43, 1.11
    'psd': (FLOOR, 9.5, _N_SQ),             # 0.13, 2.37 (Welch: coordinates rounded to float32)
    'H': (14.0, 6.3, _N_SQ),                # 3.48, 1.57 (bandpass)
    'filtered': (15.8, 14.8, _N_SQ),        # 3.95 (bandreject), 3.68 (bandpass)
    'band': (3.7, FLOOR, _N_SQ),            # 0.91, 0.40
}
MODEL = {
    'stat': (6.5, 6.5, 1024),               # 1.61 (sum (z - mean)^2 on the second-trip shape)
    'coef': (6.1, 6.1, 1024),               # 1.52 (all four terms)
    'hypot': (FLOOR, FLOOR, 8),             # 0.49
    'window': (16.1, 13.5, 64),             # 4.02, 3.35 (Welch: pow and hypot of the device against numpy's)
    's2': (5.5, FLOOR, _N_SQ),              # 1.36, 0.42
    'band': (4.1, 4.1, _N_SQ),              # 1.01
    'iir': (5.3, FLOOR, 64),                # 1.31, 0.50
    'psd_model': (3.9, FLOOR, 64),          # 0.95, 0
    'psd': (7.2, 3.6, _N_SQ),               # 1.79, 0.90 (odd shapes)
}

# the numpy model against the golden, on the host: (float64, float32), four times the largest deviation make_golden_interferogram.py
# and tests/test_interferogram_host.py print for the key (in parentheses), FLOOR where that is below it
HOST = {
    'stat': (FLOOR, FLOOR),            # 0
    'stat_final': (FLOOR, FLOOR),      # 0.03, 0.12
    'coef': (10.2, FLOOR),             # 2.54 (sphere, normal equations against lstsq), 0.18
    'removed': (4.0, 2.3),             # 0.99, 0.57
    'slope': (5.8, 3.9),               # 1.44, 0.99: of data that differs by the deviation above
    'psd': (FLOOR, FLOOR),             # 0.20
    'band': (7.3, 7.3),                # 1.81
    'H': (11.9, 11.9),                 # 2.98 (bandpass)
    'filtered': (16.1, 16.1),          # 4.03 (bandpass)
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
    f64, f32, cap = (BOUND if table == 'golden' else MODEL)[key]
    bound = min(f32 if np.dtype(dtype) == np.float32 else f64, cap)
    dev = deviation(got, want, dtype)
    measured.append((table, key, tag(dtype), label, dev, bound))
    print(f'{table:6s} {key:10s} {tag(dtype)} {label:28s} measured {dev:10.3f} eps   bound {bound:8.2f} eps')
    assert dev <= bound, f'{table} {key} {label}: {dev:.3f} eps above the bound of {bound:.2f} eps'
    return dev
