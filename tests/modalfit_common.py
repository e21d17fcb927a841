"""What tests/test_modalfit_host.py, tests/test_gpu_modalfit.py and tests/golden/make_golden_modalfit.py share: the cases, access to
tests/golden/modalfit.npz, the bounds and the comparison helper.  Imports without a GPU.

Cases.  The golden file stores coordinates, (n, m) indices, seeds, data and the reference's outputs, not the bases: a basis is
basis(case, dtype), the float64 numpy model of the Zernike kernels (prysm_amd/polynomials/zernike_plan.py) at the stored polar
coordinates, rounded once to dtype, so host and device tests fit the same numbers.
  z37   33 x 41, make_xy_grid(diameter=2), fringe 1..37 without norm; data = a random combination (default_rng(Z37_SEED)) + 5 % noise,
        NaN where r > 1 and on a seeded 5 % of the pixels.  float32: the reference run in float64 on the float32-rounded basis and data.
  z11a  64 x 64, fringe 1..11 over the annulus 0.3 <= r <= 1, for orthogonalize_modes and normalize_modes (the 3-D normalize outputs
        are stored on every fourth row to keep the file small).
  pvr   48 x 48 with the radius taken from the array, and 40 x 56 with normalization_radius given, both with dropout.

Bounds, in units of eps(dtype) max|want| as in tests/interferogram_common.py: four times the deviation measured on an MI355X (on the CPU
for the HOST table; profiles/modalfit/parity.txt has the measurements, the value is in the comment beside each bound), never below
FLOOR = 2 and never above the cap K kappa^2 -- the normal equations' own error growth, with kappa from the golden file -- which stops a
bound from hiding a failure and is not a target.  Orthogonality max|Q Q^T - I| over the mask, evaluated in double on the host: at most
four times the larger of the reference's own figure on the case and the measured one, floor 2 eps(dtype).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'modalfit.npz')
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
Z37_SHAPE, Z37_SEED, Z37_NOISE, Z37_DROP = (33, 41), 21, 0.05, 0.05
Z11A_SHAPE, Z11A_INNER = (64, 64), 0.3
NORM_ROWS = slice(None, None, 4)          # the rows of the 3-D normalize outputs the golden file keeps
PVR_CASES = {'sq': ((48, 48), 0.25, None, 31), 'rect': ((40, 56), 0.25, 5.5, 32)}      # shape, dx, normalization_radius, seed
HOPKINS = ((2, 2, 2), (-1, 3, 1), (0, 4, 0))
HOPKINS_H = 0.7


def fringe_to_nm(j):
    from prysm_amd.polynomials import fringe_to_nm as f
    return f(j)


def nms_of(case):
    return [fringe_to_nm(j) for j in range(1, 38 if case == 'z37' else 12)]


def grid(shape, dx=0.0, diameter=0.0):
    """make_xy_grid(shape, dx=dx, diameter=diameter) in float64 numpy, and its polar form"""
    if diameter:
        dx = diameter / max(shape)
    x = (np.arange(shape[1]) - shape[1] // 2) * dx
    y = (np.arange(shape[0]) - shape[0] // 2) * dx
    x, y = np.meshgrid(x, y)
    return x, y, np.hypot(x, y), np.arctan2(y, x)


def basis(case, dtype=np.float64):
    """(K, rows, cols): the float64 model of the Zernike kernels at the golden file's (r, t), rounded once to dtype"""
    from prysm_amd.polynomials import zernike_plan as ZP
    G = golden()
    nms = [tuple(int(v) for v in nm) for nm in G[f'{case}_nms']]
    return ZP.evaluate(ZP.plan(nms, False, np.float64), G[f'{case}_r'], G[f'{case}_t'], len(nms), True).astype(dtype)


def z37_data(basis64, r):
    """the z37 measurement from the float64 basis: (data with NaN, the coefficients it was made from)"""
    rng = np.random.default_rng(Z37_SEED)
    c = rng.standard_normal(basis64.shape[0])
    clean = np.tensordot(c, basis64, axes=1)
    data = clean + Z37_NOISE * np.nanstd(clean[r <= 1]) * rng.standard_normal(r.shape)
    data[r > 1] = np.nan
    data[rng.random(r.shape) < Z37_DROP] = np.nan
    return data, c


def annulus(r):
    return (r >= Z11A_INNER) & (r <= 1)


def pvr_map(name):
    """the surface of a pvr case in float64: low-order shape + mid-spatial ripple + noise, a seeded 4 % dropout and a NaN corner block"""
    shape, dx, _, seed = PVR_CASES[name]
    x, y, r, _ = grid(shape, dx=dx)
    rng = np.random.default_rng(seed)
    z = 40 * (x * x - y * y) / r.max() ** 2 + 25 * x * y / r.max() ** 2 + 6 * np.sin(1.7 * x) * np.cos(1.1 * y) + 3 * rng.standard_normal(shape) + 12
    z[rng.random(shape) < 0.04] = np.nan
    z[:3, :4] = np.nan
    return z


# ---------------------------------------------------------------- kernel coverage (tests/test_gpu_modalfit.py)
EXACT_NPTS = (1, 255, 1027)
EXACT_K = (1, 16, 17, 37, 128)
EXACT_NRHS = (0, 1, 3)


def integer_case(K, npts, nrhs, dtype, seed=5):
    """modes |m| <= 8, data |d| <= 100 (NaN on every 11th point of data[0], and NaN in mode 0 at a masked-out point), a byte mask:
    every product and every sum is an integer far below 2^53, exact in double in any order"""
    rng = np.random.default_rng(seed + 1000 * K + npts)
    modes = rng.integers(-8, 8, (K, npts), endpoint=True).astype(dtype)
    data = rng.integers(-100, 100, (max(nrhs, 1), npts), endpoint=True).astype(dtype)
    data[0, ::11] = np.nan
    mask = (rng.random(npts) < 0.8).astype(np.uint8)
    mask[0] = 1
    if npts > 3:
        mask[3] = 0
        modes[0, 3] = np.nan          # a NaN mode value at an invalid point: no trace
    return modes, data, mask


# ---------------------------------------------------------------- bounds, in units of eps(dtype) max|want|
FLOOR = 2.0


def cap(key, case):
    """K kappa^2 of the case, for coefficients and Q"""
    G = golden()
    K = len(G[f'{case}_nms'])
    return K * float(G[f'{case}_kappa']) ** 2


# key: (float64 bound, float32 bound): four times the deviation measured on an MI355X (in the comment; profiles/modalfit/parity.txt)
BOUND = {
    'coef': (743.4, FLOOR),           # 185.83 (normal equations against the reference's SVD; kappa 28.1, K = 37), 0.19
    'Q': (163.4, FLOOR),              # 40.83 (single-pass Cholesky QR against Householder; the cap K kappa^2 = 94.5 is what holds), 0
    'norm': (7.8, FLOOR),             # 1.93 ('std' of the stack: np.std against the two-pass sums in double), 0
    'pvr': (70.0, FLOOR),             # 17.48 (the 40 x 56 map; pv of the fit and rms of its residual), 0 (coordinates, basis and fit are float64 there)
    'small': (FLOOR, FLOOR),          # 0: the device's small algebra and transform against the numpy model on the device's own record
    'frames': (FLOOR, FLOOR),         # 0: a prepared fit of a stack against lstsq frame by frame
}
# the numpy model against the golden file on the host
HOST = {
    'coef': (585.0, FLOOR),           # 146.2 (normal equations against the reference's SVD; kappa 28.1, K = 37), 0.19
    'Q': (163.4, FLOOR),              # 40.8 (single-pass Cholesky QR against Householder; the cap K kappa^2 = 94.5 is what holds), 0
    'norm': (6.8, FLOOR),             # 1.70 ('std' of mode 4: the reference's np.std against the two-pass sums), 0
    'hopkins': (FLOOR, FLOOR),        # 0: the same numpy calls
}

measured = []      # (table, key, dtype tag, label, deviation, bound)


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


def compare(table, key, got, want, dtype, label='', case=None):
    """print measured against bound, remember it, and assert"""
    f64, f32 = (BOUND if table == 'golden' else HOST)[key]
    bound = f32 if np.dtype(dtype) == np.float32 else f64
    if case is not None:
        bound = min(bound, cap(key, case))
    dev = deviation(got, want, dtype)
    measured.append((table, key, tag(dtype), label, dev, bound))
    print(f'{table:6s} {key:8s} {tag(dtype)} {label:32s} measured {dev:10.3f} eps   bound {bound:8.2f} eps')
    assert dev <= bound, f'{table} {key} {label}: {dev:.3f} eps above the bound of {bound:.2f} eps'
    return dev


def orthogonality(Q, mask):
    """max|Q Q^T - I| over the mask, in double"""
    q = np.asarray(Q, dtype=np.float64)[:, np.asarray(mask, dtype=bool)]
    return float(np.abs(q @ q.T - np.eye(q.shape[0])).max())


def check_orthogonality(Q, mask, dtype, ref_figure, label=''):
    """at most four times the larger of the reference's own figure and ORTHO_MEASURED, floor 2 eps(dtype)"""
    got = orthogonality(Q, mask)
    bound = max(4 * max(ref_figure, ORTHO_MEASURED[tag(dtype)] * eps(dtype)), FLOOR * eps(dtype))
    measured.append(('ortho', 'QQt-I', tag(dtype), label, got / eps(dtype), bound / eps(dtype)))
    print(f'ortho  QQt-I    {tag(dtype)} {label:32s} measured {got / eps(dtype):10.3f} eps   bound {bound / eps(dtype):8.2f} eps')
    assert got <= bound, (got, bound)


ORTHO_MEASURED = {'f64': 19.5, 'f32': 0.28}       # eps(dtype): max|Q Q^T - I| measured on an MI355X on z11a
