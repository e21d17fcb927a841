"""What tests/test_modal_scale_host.py and tests/test_gpu_modal_scale.py share: the sizes at which the modal reductions take the second
trip of their grid-stride loops, a model of which (workgroup, wave, trip) owns which points, the float64 references, and three checks
whose bounds do not grow with the point count.  Imports without a GPU.

Sizes.  A projection launches groups(n) = min(ceil(n / 1024), cap) workgroups of 4 waves, a wave tile is 256 points and a workgroup
tile 1024; workgroup wg, wave w reads the tiles at (wg * 4 + w) * 256 + trip * groups * 1024.  groups(n) is read back from the ABI's
workspace queries (bytes / (nmodes * itemsize)) and the cap is where it stops growing, so a changed cap moves the sizes with it and
the host test, which pins the numbers, fails loudly.  With tile = 1024:
  n_one = cap * tile + 1              the second trip is one lane of one wave of workgroup 0
  n_vec = cap * tile + 5 * tile + 516 a multiple of 4 (16-byte path), six workgroups take a second trip, the last wave tile is ragged
  n_odd = n_vec + 3                   not a multiple of 4: the whole launch goes element-wise

Checks on out[k] = sum_p g[p] Z_k[p] (eps and TOL of the precision under test, TOL the unit's forward tolerance):
  exact   g[p] = 1 + p mod 3 against a mode that is exactly 1: every partial sum is an integer below 2^24, so the result is sum(g)
          in any order, in float32 too; one point dropped or doubled changes it.
  probe   g the indicator of a set S of at most 1024 points (the complement of all probes, float64 only, is the one larger set):
          |out[k] - sum_S Z_k| <= |S| TOL max|Z_k| + 16 eps sum_S |Z_k|.
  dense   random g, asserted in float64: |out[k] - ref| <= TOL max|Z_k| sum|g| + 32 eps sum|g Z_k|.  32 is the depth of the summation
          in csrc/modal_tile.h: 3 adds per lane, 6 butterfly levels, lane 0's adds over at most 7 trips, 3 over the waves, then in
          reduce_partials_kernel at most 4 serial adds, 6 levels and 3 over its waves, and the rounding of the product.
"""
import functools

import numpy as np

TILE, WAVE_TILE, WAVES = 1024, 256, 4
TOL_ZERNIKE = {np.float64: 1e-12, np.float32: 2e-5}       # TOL of tests/test_gpu_zernike.py, recur_common.py, test_gpu_segmented.py
TOL_QPOLY = {np.float64: 1e-12, np.float32: 5e-5}         # TOL of tests/test_gpu_qpoly.py
FIBER_V = 5.5


def eps(dt):
    return float(np.finfo(dt).eps)


def tol_fiber(dt):
    """tests/fibers_common.py mode_bound: 16 (1 + V) eps max|mode_k|"""
    return 16 * (1 + FIBER_V) * eps(dt)


# ----------------------------------------------------------------------------- sizes from the ABI

def _lib():
    from prysm_amd import _lib as L
    return L, L.load()


def groups(unit, n, dt=np.float64, nmodes=8):
    """workgroups (partials per output) of unit's reduction over n points, from its workspace query"""
    L, lib = _lib()
    code = L.PM_F32 if np.dtype(dt) == np.float32 else L.PM_F64
    item = np.dtype(dt).itemsize
    if unit == 'overlap':
        return lib.pm_overlap_workspace(code, n) // (4 * item)
    if unit == 'segment':
        return lib.pm_segment_project_workspace(code, n, 1, nmodes, 1) // (nmodes * item)
    fn = getattr(lib, {'zernike': 'pm_zernike_project_workspace', 'qpoly': 'pm_qpoly_project_workspace',
                       'recur': 'pm_recur_project_workspace', 'fiber': 'pm_fiber_project_workspace'}[unit])
    return fn(code, n, nmodes, 1) // (nmodes * item)


@functools.lru_cache(None)
def cap_of(unit):
    """the value at which groups(n) stops growing"""
    g = 1
    while g <= 1 << 22:
        got = groups(unit, TILE * g)
        if got < g:
            assert groups(unit, TILE * got) == got == groups(unit, TILE * got + 1) and groups(unit, TILE * (got - 1)) == got - 1
            return int(got)
        g *= 2
    raise AssertionError(f'{unit}: the workgroup count never stops growing')


def sizes(cap):
    """(n_one, n_vec, n_odd)"""
    n_vec = cap * TILE + 5 * TILE + 516
    return cap * TILE + 1, n_vec, n_vec + 3


def tiles_by_trip(n, ngroups):
    """[(workgroup, wave, trip, lo, hi)]: the points lo .. hi - 1 each (workgroup, wave, trip) owns"""
    out = []
    stride = ngroups * TILE
    for trip in range(-(-n // stride)):
        for wg in range(ngroups):
            for wave in range(WAVES):
                lo = (wg * WAVES + wave) * WAVE_TILE + trip * stride
                if lo < n:
                    out.append((wg, wave, trip, lo, min(lo + WAVE_TILE, n)))
    return out


def probe_sets(n, cap):
    """{name: ascending point indices}; every set has at most 1024 points"""
    last = (-(-n // WAVE_TILE) - 1) * WAVE_TILE
    edge = cap * TILE
    sets = {'last wave tile': np.arange(last, n), 'first tile of trip 2': np.arange(edge, min(edge + TILE, n)),
            'last tile of trip 1': np.arange(edge - TILE, edge)}
    for p in (edge - 1, edge, edge + 1, n - 1):
        if p < n:
            sets[f'point {p}'] = np.array([p])
    return sets


# ----------------------------------------------------------------------------- the battery of inputs and its checks

class Battery:
    """The rows of G (B, n), each with its check.  ref (K, n) float64: the modes at the coordinates as the kernel reads them."""

    def __init__(self, ref, n, cap, dt, tol, piston=None, seed=0, dense=3):
        self.ref, self.n, self.dt, self.tol, self.piston = ref[:, :n], n, dt, tol, piston
        self.zmax = np.max(np.abs(self.ref), axis=1)
        self._exp = {}
        rows = []
        if piston is not None:
            rows.append(('exact', 'exact', (1 + np.arange(n) % 3).astype(dt)))
        union = np.zeros(n, dtype=bool)
        for name, S in probe_sets(n, cap).items():
            g = np.zeros(n, dtype=dt)
            g[S] = 1
            union[S] = True
            rows.append((name, 'probe', g))
        if dt == np.float64:
            rows.append(('complement', 'probe', (~union).astype(dt)))
        rng = np.random.default_rng(seed)
        self.dense0 = len(rows)
        for i in range(dense):
            rows.append((f'dense {i}', 'dense', rng.standard_normal(n).astype(dt)))
        self.rows = rows
        self.G = np.stack([g for _, _, g in rows])

    def placement(self):
        """every probe has a mode whose sum over it is at least a tenth of |S| max|Z_k| (so some point of it has |Z_k| > 0.1 max|Z_k|)"""
        for name, kind, g in self.rows:
            if kind == 'probe' and name != 'complement':
                S = np.flatnonzero(g)
                assert np.any(np.abs(self.ref[:, S].sum(axis=1)) >= 0.1 * len(S) * self.zmax), name

    def _expected(self, i):
        """(the float64 result row i should give, its bound), formed once"""
        if i not in self._exp:
            _, kind, g = self.rows[i]
            g64, e = g.astype(np.float64), eps(self.dt)
            if kind == 'exact':
                self._exp[i] = float(g64.sum()), 0.0
            else:
                idx = np.flatnonzero(g64)
                z, gs = (self.ref, g64) if 2 * len(idx) > self.n else (self.ref[:, idx], g64[idx])
                want, mag = z @ gs, np.abs(z) @ np.abs(gs)
                if kind == 'probe':
                    bound = len(idx) * self.tol * self.zmax + 16 * e * mag
                else:
                    bound = self.tol * self.zmax * np.abs(gs).sum() + 32 * e * mag
                self._exp[i] = want, bound
        return self._exp[i]

    def verify(self, A, label=''):
        """[(row name, worst ratio to the bound)] of the rows of A (B, K) that miss their check; prints every figure"""
        A = np.asarray(A, dtype=np.float64)
        bad = []
        for i, ((name, kind, g), a) in enumerate(zip(self.rows, A)):
            want, bound = self._expected(i)
            if kind == 'exact':
                ratio = 0.0 if a[self.piston] == want else np.inf
                note = f'got {a[self.piston]:.1f} want {want:.1f}'
            else:
                ratio = float(np.max(np.abs(a - want) / bound))
                note = f'deviation / bound {ratio:.3e}'
                if kind == 'dense' and self.dt == np.float32:
                    note += ' (printed, not asserted in float32)'
                    ratio = 0.0 if np.all(np.isfinite(a)) else np.inf
            if label:
                print(f'{label} {np.dtype(self.dt).name} n={self.n} {name}: {note}')
            if not ratio <= 1:
                bad.append((name, ratio))
        return bad


# ----------------------------------------------------------------------------- the kernels' summation order in numpy

def tile_totals(Z, g, dt):
    """(K, wave tiles): the sum a wave forms over each of its tiles, in the precision dt and the kernel's order -- the product, the
    lane's four points in turn (a lane holds 16-byte runs: four consecutive float32, two pairs of float64 128 points apart), the
    butterfly over the 64 lanes.  Only the tiles where g is non-zero are formed."""
    K, n = Z.shape
    nt = -(-n // WAVE_TILE)
    out = np.zeros((K, nt), dtype=dt)
    tiles = np.unique(np.flatnonzero(g) // WAVE_TILE)
    for lo in range(0, len(tiles), 512):
        tl = tiles[lo:lo + 512]
        P = np.zeros((K, len(tl) * WAVE_TILE), dtype=dt)
        if tl[-1] - tl[0] + 1 == len(tl):                     # a run of tiles: no gather
            a, b = tl[0] * WAVE_TILE, min((tl[-1] + 1) * WAVE_TILE, n)
            P[:, :b - a] = Z[:, a:b].astype(dt, copy=False) * g[a:b].astype(dt, copy=False)
        else:
            idx = (tl[:, None] * WAVE_TILE + np.arange(WAVE_TILE)[None, :]).ravel()
            ok = idx < n
            P[:, ok] = Z[:, idx[ok]].astype(dt) * g[idx[ok]].astype(dt)
        if np.dtype(dt) == np.float32:
            q = P.reshape(K, len(tl), 64, 4)
            s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
        else:
            q = P.reshape(K, len(tl), 2, 64, 2)
            s = ((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + q[:, :, 1, :, 0]) + q[:, :, 1, :, 1]
        out[:, tl] = _butterfly(s)
    return out


def _butterfly(s):
    for off in (32, 16, 8, 4, 2, 1):
        s = s[..., :off] + s[..., off:2 * off]
    return s[..., 0]


FAULTS = ('second trip skipped', 'ragged last tile skipped', 'one tile counted twice')


def combine(tt, ngroups, dt, fault=None, twice=None):
    """(K,): the tile sums through lane 0's adds over the trips, the adds over the waves and reduce_partials_kernel's order, with one
    of FAULTS injected (twice: the tile `one tile counted twice` doubles)"""
    K, nt = tt.shape
    per = ngroups * WAVES
    trips = -(-nt // per)
    T = np.zeros((K, trips * per), dtype=dt)
    T[:, :nt] = tt
    if fault == FAULTS[0]:
        T[:, per:] = 0
    elif fault == FAULTS[1]:
        T[:, nt - 1] = 0
    elif fault == FAULTS[2]:
        T[:, twice] += T[:, twice]
    elif fault is not None:
        raise ValueError(fault)
    T = T.reshape(K, trips, ngroups, WAVES)
    w = T[:, 0]
    for t in range(1, trips):
        w = w + T[:, t]
    part = w[..., 0]
    for v in range(1, WAVES):
        part = part + w[..., v]
    m = -(-ngroups // 256)
    Pp = np.zeros((K, m * 256), dtype=dt)
    Pp[:, :ngroups] = part
    Pp = Pp.reshape(K, m, 256)
    s = Pp[:, 0]
    for i in range(1, m):
        s = s + Pp[:, i]
    s = _butterfly(s.reshape(K, WAVES, 64))
    out = s[:, 0]
    for v in range(1, WAVES):
        out = out + s[:, v]
    return out


# ----------------------------------------------------------------------------- coordinates and float64 references

ZERNIKE_NMS = [(0, 0), (1, 1), (1, -1), (2, 0), (2, 2), (3, -1), (4, 0), (5, 3)]
Q2D_NMS = [(0, 0), (1, 0), (2, 0), (0, 1), (1, -1), (2, 2), (1, -3), (3, 1)]
QCON_NS = list(range(7))
JACOBI = (0.0, 2.0)
JACOBI_NS = [0, 1, 2, 4, 7, 9]
RADIUS = 1.1
FAMILY_NS = list(range(7))


@functools.lru_cache(None)
def coords(cap, dt=np.float64):
    """x, y of n_odd points, uniform in [-0.7, 0.7] as the stack tests draw them and rounded once to dt (so input rounding is charged to
    nobody); a smaller size reads a prefix.  The single-point probes of the three sizes sit at radius 0.67, where the lowest mode of
    every unit is above a tenth of its maximum."""
    n = sizes(cap)[2]
    rng = np.random.default_rng(15)
    x, y = (rng.uniform(-0.7, 0.7, n) for _ in range(2))
    special = sorted({p for m in sizes(cap) for p in (cap * TILE - 1, cap * TILE, cap * TILE + 1, m - 1)})
    for j, p in enumerate(special):
        x[p], y[p] = 0.62 - 0.004 * j, 0.25 + 0.004 * j
    return x.astype(dt), y.astype(dt)


def polar(x, y, dt):
    x, y = x.astype(np.float64), y.astype(np.float64)
    return np.hypot(x, y).astype(dt), np.arctan2(y, x).astype(dt)


def fiber_mode_dict():
    import fibers_common as FC
    return FC.mode_dict('V5.5')


def model(unit, u, v, dt=np.float64):
    """(K, n): the numpy model of `unit` in the precision dt at the points (u, v)"""
    if unit in ('zernike', 'zernike polar'):
        from prysm_amd.polynomials import zernike_plan as ZP
        return ZP.evaluate(ZP.plan(ZERNIKE_NMS, True, dt), u, v, len(ZERNIKE_NMS), unit == 'zernike polar')
    if unit == 'q2d':
        from prysm_amd.polynomials import qpoly_plan as QP
        return QP.evaluate(QP.plan(Q2D_NMS, QP.Q2D, dt), u, v, len(Q2D_NMS))
    if unit == 'qcon':
        from prysm_amd.polynomials import qpoly_plan as QP
        return QP.evaluate(QP.plan(QCON_NS, QP.QCON, dt), u, None, len(QCON_NS), QP.RADIAL)
    from prysm_amd.polynomials import recur_plan as RP
    if unit == 'jacobi radial':
        u, v = np.asarray(u, dtype=dt), np.asarray(v, dtype=dt)
        arg = dt(2) * (u * u + v * v) * dt(1 / RADIUS ** 2) - dt(1)
        return RP.evaluate(RP.plan('jacobi', JACOBI_NS, *JACOBI, dtype=dt), arg)[0]
    if unit == 'jacobi':
        return RP.evaluate(RP.plan('jacobi', JACOBI_NS, *JACOBI, dtype=dt), u)[0]
    if unit in ('cheby1', 'legendre'):
        return RP.evaluate(RP.plan(unit, FAMILY_NS, dtype=dt), u)[0]
    if unit == 'fiber':
        import fibers_common as FC
        from prysm_amd.x import fibers_plan as FP
        table, k = FP.mode_table(FIBER_V, fiber_mode_dict(), dt)
        return FP.walk(table, k, FC.A, u, v)
    raise ValueError(unit)


# unit -> (the ABI unit whose cap sizes it, the forward tolerance, the index of a mode that is exactly 1 or None)
UNITS = {'zernike': ('zernike', TOL_ZERNIKE, 0), 'zernike polar': ('zernike', TOL_ZERNIKE, 0), 'q2d': ('qpoly', TOL_QPOLY, None),
         'qcon': ('qpoly', TOL_QPOLY, None), 'jacobi': ('recur', TOL_ZERNIKE, 0), 'jacobi radial': ('recur', TOL_ZERNIKE, 0),
         'cheby1': ('recur', TOL_ZERNIKE, 0), 'legendre': ('recur', TOL_ZERNIKE, 0),
         'fiber': ('fiber', {np.float64: tol_fiber(np.float64), np.float32: tol_fiber(np.float32)}, None)}


@functools.lru_cache(4)
def unit_coords(unit, dt):
    """the two coordinate arrays of n_odd points the unit's entry point is given, in dt (a smaller size reads a prefix): (x, y), (r, t)
    for the polar Zernike form and the fibre (radii out to 1.5 core radii), (|x|, the same) for the radial Qcon"""
    cap = cap_of(UNITS[unit][0])
    if unit == 'fiber':
        x, y = coords(cap)
        return polar(6 * x, 6 * y, dt)
    x, y = coords(cap, dt)
    if unit == 'qcon':
        return np.abs(x), np.abs(x)
    return polar(x, y, dt) if unit == 'zernike polar' else (x, y)


@functools.lru_cache(4)
def reference(unit, dt):
    """(K, n_odd) float64 at the coordinates rounded to dt; the last few are kept, which is one evaluation per unit and precision for
    tests that run unit by unit"""
    u, v = unit_coords(unit, dt)
    return model(unit, u.astype(np.float64), v.astype(np.float64), np.float64)


def battery(unit, n, dt, seed=0, dense=3):
    abi, tol, piston = UNITS[unit]
    return Battery(reference(unit, dt), n, cap_of(abi), dt, tol[dt], piston, seed, dense)
