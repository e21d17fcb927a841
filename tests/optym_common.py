"""What tests/test_optym_host.py and tests/test_gpu_optym_kernels.py share: the cases, the references and the bounds of the optym
kernels (csrc/optym.hip) at the C ABI, guard bands, and one call of each entry point with everything around it asserted.  Imports
without a GPU.

References.  The reference's formulas (prysm/x/optym) in np.longdouble on the inputs AFTER they are rounded to the dtype under test.
np.longdouble is the x87 extended type here (eps 2^-64 <= 2^-63, asserted below once); a numpy without it would need exact sums
(fractions.Fraction) instead, and this module refuses to import rather than compare against a float64 that calls itself long double.

Bands.  Every array a kernel reads or writes is n elements inside ONE buffer of LEAD + n + TAIL elements filled with a sentinel (NaN for
floats, 0xA5 for bytes).  After a call the band around an output must hold the sentinel still, bit for bit (Band.read), and an input
must be unchanged everywhere (Band.unchanged).  TAIL is larger than the 256-element row of the flat sweeps, so a sweep without its
`i >= n` guard writes the band and not foreign memory.

Bounds (each is derived here, none is measured; `ratio` is always measured / bound and must be <= 1):

  cost, bias and gain invariant.  gradient, normwise: max|got - want| / max|want| <= 8 eps64 (|alpha| max|I| + |beta| + max|D|) / max|raw|
      + 2 eps(T).  The first term is the conditioning of raw = (alpha I + beta) - D itself, evaluated in float64 from values of that size
      (8 covers the order of the sums that feed alpha and beta), the second the rounding of the output.  cost, relative:
      16 eps64 (pedestal / SPREAD + 1) + 2 eps(T) with SPREAD = 0.9, the width of the U(0.1, 1) the intensities are drawn from.
  cost on small integers: N, the sums of MSE and the first-pass and centred sums of BGI are integers below 2^53, exact in any order, so
      the MSE cost and gradient and the BGI gradient equal the model bit for bit.  The BGI cost is R sum(raw^2) of non-integers: kernel
      and model add the same 624 291 positive terms in different trees, each of depth < 32, so they differ by at most 64 eps64 relative
      before the one rounding to T: bound 64 eps64 + eps(T).
  steps: bit for bit against optym_plan.step fed the coefficients read back from the device.
  advance: 1 - beta^k carries pow's error, an ulp or two of beta^k <= 1, and the subtraction is exact or rounds once: |got - want| <=
      4 eps64 ABSOLUTE (4 ulp of a double at 1; relative to a small difference it would be a statement about cancellation, not about
      the kernel).  sqrt(1 - beta2^k) halves that relative error and rounds once: bound 4 eps64 / (2 want) + eps64 want.
      rho = rhoinf - 2 k b / (1 - b): d/db of b / (1 - b) is 1 / (1 - b)^2, and three roundings of terms as large as rhoinf:
      |got - want| <= 2 k 4 eps64 / (1 - b)^2 + 8 eps64 rhoinf.
  activations, elementwise: the larger of 4 |model - want| (numpy in the same precision, not the code under test) and
      4 eps(T) max(1, |want|).
  softmax forward, elementwise and relative: |y - want| <= 4 (2 + |x - max x|) eps(T) want; row sums within K eps(T) of 1.
  softmax backprop: |gin - want| <= eps(T) |want| + 4 K eps64 max|g| y / tau, want the kernel's expression y (g S - sum g y) / tau
      in long double on the stored y.
  Gumbel softmax against optym_plan.softmax in the same dtype.  The two sides differ in the two logarithms of every logit
      l = (x + G) / tau, G = -log(w), w = -log(u + eps) + eps: an ulp each way on the inner one is 2 eps relative on w (3 eps with the
      add's rounding), which is 3 eps ABSOLUTE on G; the outer one adds 2 eps |G|; the sum with x and the division may then round
      the other way, 2 eps |l|.  So |dl| <= eps ((3 + 2 |G|) / tau + 2 |l|) =: dl_j, and a probability moves by its own dl, the
      maximum's and the weighted mean of all of them: relative bound 4 (2 + |l - max l|) eps(T) + 3 max_j dl_j.

Measured on an MI355X, largest measured / bound per group as tests/test_gpu_optym_kernels.py prints them (RECORDED there holds the same
figures; float64 then float32):
  bias-and-gain-invariant cost, all pedestals and sizes   0.069  0.216     at a pedestal of 1e4 and n = 624 291: gradient 1.4e-11 of a
      bound of 2.3e-10 and 4.3e-8 of 2.4e-7, cost 7.3e-14 of 3.9e-11 and 1.0e-8 of 2.4e-7.  The one-pass sums this replaced measured, on
      the same device and inputs, 2.2 and 22 times the gradient bound at a pedestal of 1e2 in float64 (n = 2479, 624 291), 970 and 3900
      times at 1e4, and 2.3 times in float32 at 1e4 (n = 2479)
  costs at n = 1, 255, 256, 257                           0.142  0.207
  integer costs: bit for bit; the BGI cost measured 0 of its bound as well
  steps, second trip, spatial gradient: bit for bit
  advance (double only)                                   0.111
  activations                                             0.308  0.487
  softmax forward / row sums / backprop                   0.179 / 0.401 / 0.117    0.136 / 0.361 / 0.496
  Gumbel softmax against the model                        0.056  0.072
"""
import ctypes
import functools

import numpy as np

from prysm_amd import _lib as L
from prysm_amd.x import optym_plan as OP

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, 'np.longdouble is not an extended type here: the references of this module need one'

EPS64 = float(np.finfo(np.float64).eps)
DTYPES = (np.float64, np.float32)
CODE = {np.dtype(np.float32): L.PM_F32, np.dtype(np.float64): L.PM_F64}
TINY32 = float(np.finfo(np.float32).tiny)


def eps_of(dt):
    return float(np.finfo(dt).eps)


def frozen(a):
    a.setflags(write=False)
    return a


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want):
    """NaN in the same places and nowhere else, every other element equal bit for bit (so -0 is not +0)"""
    got, want = np.atleast_1d(np.asarray(got)), np.atleast_1d(np.asarray(want))
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != 'f':
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def same_specials(got, want):
    """the pattern of NaN, +inf and -inf"""
    return all(np.array_equal(f(got), f(want)) for f in (np.isnan, np.isposinf, np.isneginf))


# ----------------------------------------------------------------------------- bands

LEAD, TAIL = 64, 320


class Band:
    """n elements inside LEAD + n + TAIL of sentinel on the device (see the module docstring)"""

    def __init__(self, values=None, n=None, dtype=None):
        import torch
        if values is not None:
            values = np.ascontiguousarray(values).ravel()
            if values.dtype == bool:
                values = values.view(np.uint8)
            n, dtype = values.size, values.dtype
        dtype = np.dtype(dtype)
        self.n = n
        self.host = np.full(LEAD + n + TAIL, 0xA5 if dtype.kind == 'u' else np.nan, dtype=dtype)
        if values is not None:
            self.host[LEAD:LEAD + n] = values
        self.dev = torch.from_numpy(self.host).cuda()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + LEAD * self.host.dtype.itemsize)

    def read(self):
        """the n elements after a call; asserts that the band is the sentinel still"""
        h = self.dev.cpu().numpy()
        for name, sl in (('before', slice(0, LEAD)), ('behind', slice(LEAD + self.n, None))):
            bad = np.flatnonzero(bits(h[sl]) != bits(self.host[sl]))
            assert bad.size == 0, f'{bad.size} elements of the band {name} the {self.n} values were written, the first {bad[0]} into it'
        return h[LEAD:LEAD + self.n].copy()

    def unchanged(self):
        return np.array_equal(bits(self.dev.cpu().numpy()), bits(self.host))


def null():
    return ctypes.c_void_p(0)


# ----------------------------------------------------------------------------- costs

SPREAD = 0.9
PEDESTALS = (0.0, 1e2, 1e4)
N_SMALL = 37 * 67
N_LARGE = 2 * OP.COST_THREADS * OP.COST_WGS + 100003           # every first-stage workgroup loops and the last trip ends ragged
COST_SIZES = (N_SMALL, N_LARGE)
GUARD_SIZES = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def bgi_inputs(pedestal, n, dtname):
    """(I, D, mask): I = pedestal + U(0.1, 1), D = 1.7 I + 0.3 + 0.05 N(0, 1), rounded to the dtype; a 70 % mask whose FIRST element is
    false, so that a form shifted by the first element would have to skip it"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng([int(pedestal), n])
    I = pedestal + rng.uniform(0.1, 1.0, n)  # noqa: E741
    D = 1.7 * I + 0.3 + 0.05 * rng.standard_normal(n)
    mask = rng.random(n) < 0.7
    mask[0] = False
    if n > 1:
        mask[1] = True
    return frozen(I.astype(dt)), frozen(D.astype(dt)), frozen(mask)


def bgi_reference(I, D, keep=None):  # noqa: E741
    """prysm/x/optym/cost.py:30-70 in long double: dict(cost, grad, alpha, beta, raw_max, I_max, D_max); grad zero where keep is false"""
    I, D = np.asarray(I).ravel(), np.asarray(D).ravel()  # noqa: E741
    keep = np.ones(I.shape, bool) if keep is None else np.asarray(keep).astype(bool).ravel()
    Ik, Dk = I[keep].astype(LD), D[keep].astype(LD)
    Ihat, Dhat = Ik - Ik.mean(), Dk - Dk.mean()
    alpha = (Ihat * Dhat).sum() / (Ihat * Ihat).sum()
    beta = Dk.mean() - alpha * Ik.mean()
    R = 1 / (Dk * Dk).sum()
    raw = (alpha * Ik + beta) - Dk
    grad = np.zeros(I.shape, LD)
    grad[keep] = 2 * R * alpha * raw
    return dict(cost=R * (raw * raw).sum(), grad=grad, alpha=alpha, beta=beta, raw_max=np.abs(raw).max(), I_max=np.abs(Ik).max(),
                D_max=np.abs(Dk).max())


@functools.lru_cache(maxsize=None)
def bgi_case(pedestal, n, dtname, masked):
    I, D, mask = bgi_inputs(pedestal, n, dtname)  # noqa: E741
    return bgi_reference(I, D, mask if masked else None)


def bgi_bounds(ref, pedestal, dt):
    grad = 8 * EPS64 * float((abs(ref['alpha']) * ref['I_max'] + abs(ref['beta']) + ref['D_max']) / ref['raw_max']) + 2 * eps_of(dt)
    cost = 16 * EPS64 * (pedestal / SPREAD + 1) + 2 * eps_of(dt)
    return grad, cost


def bgi_errors(cost, grad, ref):
    """(normwise gradient error, relative cost error) of a result against bgi_reference's"""
    g = np.asarray(grad).ravel().astype(LD)
    return float(np.abs(g - ref['grad']).max() / np.abs(ref['grad']).max()), float(abs(LD(cost) - ref['cost']) / abs(ref['cost']))


def mse_reference(M, D, keep=None):
    M, D = np.asarray(M).ravel(), np.asarray(D).ravel()
    keep = np.ones(M.shape, bool) if keep is None else np.asarray(keep).astype(bool).ravel()
    diff = M[keep].astype(LD) - D[keep].astype(LD)
    grad = np.zeros(M.shape, LD)
    grad[keep] = 2 * diff / diff.size
    return (diff * diff).sum() / diff.size, grad


@functools.lru_cache(maxsize=None)
def integer_case(dtname):
    """(I, D, mask) of N_LARGE small integers, |values| <= 8, with sum I = 0 and sum D = N exactly: I is +-v in pairs and one 0,
    D = 2 I + 1 + e with e = +-1 in pairs, so both means (0 and 1) and with them every centred sum are integers"""
    dt = np.dtype(dtname)
    n = N_LARGE
    rng = np.random.default_rng(77)
    v = rng.integers(0, 4, n // 2)
    I = np.concatenate([v, -v, [0]])  # noqa: E741
    w = rng.integers(0, 2, n // 2)
    e = np.concatenate([w, -w, [0]])
    rng.shuffle(e)
    D = 2 * I + 1 + e
    order = rng.permutation(n)
    I, D = I[order], D[order]  # noqa: E741
    assert I.sum() == 0 and D.sum() == n and np.abs(D).max() <= 8 and I.size == n
    return frozen(I.astype(dt)), frozen(D.astype(dt)), frozen(rng.random(n) < 0.7)


INTEGER_COST_BOUND = 64 * EPS64


def run_cost(kind, M, D, mask=None, d_scalar=0.0):
    """one pm_optym_cost call: (cost, grad) as numpy; asserts the return code, the bands behind cost and grad and that no input was
    written.  The workspace is filled with 0xFF bytes (NaN as doubles) first: nothing a call finds there can help it."""
    import torch
    lib = L.load()
    M = np.asarray(M)
    m = Band(M)
    d = Band(np.asarray(D, dtype=M.dtype)) if D is not None else None
    k = Band(mask) if mask is not None else None
    cost, grad = Band(n=1, dtype=M.dtype), Band(n=M.size, dtype=M.dtype)
    nbytes = lib.pm_optym_cost_workspace()
    ws = torch.full((nbytes + 8,), 0xFF, dtype=torch.uint8, device='cuda')
    L.check(lib.pm_optym_cost(CODE[M.dtype], kind, M.size, m.ptr, d.ptr if d else null(), float(d_scalar), k.ptr if k else null(), cost.ptr,
                              grad.ptr, L.ptr(ws), nbytes, L.stream_ptr()))
    c, g = cost.read()[0], grad.read()
    assert ws[nbytes:].cpu().numpy().tolist() == [0xFF] * 8, 'the cost wrote past pm_optym_cost_workspace() bytes'
    assert m.unchanged() and (d is None or d.unchanged()) and (k is None or k.unchanged())
    return c, g.reshape(M.shape)


# ----------------------------------------------------------------------------- steps

KINDS = ('GradientDescent', 'AdaGrad', 'RMSProp', 'Adam', 'RAdam', 'AdaMomentum', 'Yogi')
STEP_SIZES = (1, 255, 256, 257, 1027)
STEP_COUNT = 8
BETAS = ((0.9, 0.999), (0.5, 0.9))
ADVANCE_KS = (1, 2, 5, 6, 7, 1000, 10 ** 6)


@functools.lru_cache(maxsize=None)
def step_case(n, dtname):
    """dict(x, lower, upper, t, w, special, signs, nan_g, nan_x, inf_lo, inf_hi): bounds per element from {-inf, finite} x {finite, +inf},
    every eighth x exactly on its finite lower bound and the one after it on its finite upper bound, with gradients +, -, 0 in turn
    there.  inf_lo: an x = -inf whose lower bound is -inf, with a positive gradient, inf_hi its mirror image: x <= lower holds there, and
    only isfinite(lower) keeps the gradient from being projected away and the bound from counting as active"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng(1000 + n)
    lower = np.where(rng.random(n) < 0.5, -np.inf, -0.5 - 0.1 * rng.random(n)).astype(dt)
    upper = np.where(rng.random(n) < 0.5, np.inf, 0.5 + 0.1 * rng.random(n)).astype(dt)
    x = np.minimum(np.maximum(rng.standard_normal(n).astype(dt), lower), upper)
    i = np.arange(n)
    on_lower, on_upper = (i % 8 == 0) & np.isfinite(lower), (i % 8 == 1) & np.isfinite(upper)
    x[on_lower], x[on_upper] = lower[on_lower], upper[on_upper]
    special = np.flatnonzero(on_lower | on_upper | (i % 8 == 2))           # i % 8 == 2: an x off its bounds with the same gradients
    signs = np.array([1.0, -1.0, 0.0, -0.0])[np.arange(special.size) % 4].astype(dt)
    nan_g = n // 2 if n > 2 else None
    nan_x = n // 3 if n > 2 else None
    if nan_x is not None:
        x[nan_x] = np.nan
    free = (i % 8 >= 3) & (i != nan_g) & (i != nan_x)
    inf_lo = next(iter(np.flatnonzero(free & np.isneginf(lower))), None)
    inf_hi = next(iter(np.flatnonzero(free & np.isposinf(upper) & (i != inf_lo))), None)
    if inf_lo is not None:
        x[inf_lo] = -np.inf
    if inf_hi is not None:
        x[inf_hi] = np.inf
    return dict(inf_lo=inf_lo, inf_hi=inf_hi, x=frozen(x), lower=frozen(lower), upper=frozen(upper), t=frozen(rng.standard_normal(n).astype(dt)),
                w=frozen(rng.uniform(0.5, 2.0, n).astype(dt)), special=special, signs=signs, nan_g=nan_g, nan_x=nan_x)


def step_gradient(case, x, k):
    """the gradient of step k at x: the quadratic's, with +, -, 0 (rotated by k) at the special elements and one NaN"""
    g = case['w'] * (x - case['t'])
    if case['special'].size:
        g[case['special']] = np.roll(case['signs'], k) * (1 + np.abs(g[case['special']]))
    if case['nan_g'] is not None:
        g[case['nan_g']] = np.nan
    if case['inf_lo'] is not None:
        g[case['inf_lo']] = 1.5
    if case['inf_hi'] is not None:
        g[case['inf_hi']] = -1.5
    return g.astype(x.dtype)


def coefficients_reference(kind, k, beta1, beta2):
    """pm_optym_advance's coefficients in long double, from the DOUBLES beta1 and beta2: (1 - b1^k, 1 - b2^k, rho, r, flag, sqrt(1 - b2^k))"""
    b1k, b2k = np.power(LD(beta1), LD(k)), np.power(LD(beta2), LD(k))
    rho = r = LD(0)
    flag = 0.0
    if kind == OP.RADAM:
        rhoinf = 2 / (1 - LD(beta2)) - 1
        rho = rhoinf - (2 * LD(k) * b2k) / (1 - b2k)
        if rho >= 5:
            r, flag = np.sqrt(((rho - 4) * (rho - 2) * rhoinf) / ((rhoinf - 4) * (rhoinf - 2) * rho)), 1.0
    return 1 - b1k, 1 - b2k, rho, r, flag, np.sqrt(1 - b2k)


def coefficient_bounds(want, k, beta2):
    """the absolute bounds on coefficients 0, 1, 2 and 5 (see the module docstring)"""
    one = 4 * EPS64
    rhoinf = 2 / (1 - beta2) - 1
    return {0: one, 1: one, 2: 2 * k * one / float(want[1]) ** 2 + 8 * EPS64 * rhoinf, 5: one / (2 * float(want[5])) + EPS64 * float(want[5])}


def advance(kind, beta1, beta2, counter, coef):
    lib = L.load()
    L.check(lib.pm_optym_advance(kind, float(beta1), float(beta2), L.ptr(counter), L.ptr(coef), L.stream_ptr()))
    return coef.cpu().numpy().copy()


STEP_OUTPUTS = ('x', 's1', 's2', 'x_prev', 'g_step', 'active')


def run_step(kind, x, g, s1, s2, lower, upper, coef_dev, alpha, beta1, beta2, eps):
    """one bounded pm_optym_step call on numpy arrays: dict of STEP_OUTPUTS as numpy, every one of the six read out of its band; asserts
    the return code and that g and the bounds were not written"""
    lib = L.load()
    dt, n = x.dtype, x.size
    b = {key: Band(a) for key, a in (('x', x), ('g', g), ('s1', s1), ('s2', s2), ('lower', lower), ('upper', upper))}
    b['x_prev'], b['g_step'], b['active'] = Band(n=n, dtype=dt), Band(n=n, dtype=dt), Band(n=n, dtype=np.uint8)
    L.check(lib.pm_optym_step(CODE[dt], kind, n, b['x'].ptr, b['g'].ptr, b['s1'].ptr, b['s2'].ptr, b['lower'].ptr, b['upper'].ptr, float(alpha),
                              float(beta1), float(beta2), float(eps), L.ptr(coef_dev), b['x_prev'].ptr, b['g_step'].ptr, b['active'].ptr,
                              L.stream_ptr()))
    out = {key: b[key].read() for key in STEP_OUTPUTS}
    assert b['g'].unchanged() and b['lower'].unchanged() and b['upper'].unchanged()
    return out


SECOND_TRIP_N = 256 * (4 * 65535) + 257           # pm_sweep.h: 4 rows of 256 per workgroup, 65535 workgroups down the rows, then the stride


# ----------------------------------------------------------------------------- activations

ACTIVATIONS = ('Tanh', 'Arctan', 'Softplus', 'Sigmoid')
ACT_SIZES = (1, 255, 256, 257)
ACT_PARAMS = ((1.7, 0.3, -0.2), (1.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def activation_input(n, dtname, a, x0):
    """+-0, +-inf, NaN, the x where a (x - x0) is +-100 and +-1000, the smallest and the largest denormal of either sign, then N(0, 2)"""
    dt = np.dtype(dtname)
    fi = np.finfo(dt)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, x0 + 100 / a, x0 - 100 / a, x0 + 1000 / a, x0 - 1000 / a, float(fi.smallest_subnormal),
               -float(fi.smallest_subnormal), float(fi.tiny) * (1 - float(fi.eps)), -float(fi.tiny) * (1 - float(fi.eps))]
    noise = 2 * np.random.default_rng(n).standard_normal(max(n, 1))
    x = np.concatenate([special, noise])[:n] if n > 1 else np.array([0.5])
    return frozen(x.astype(dt))


def activation_reference(kind, x, a, x0, y0, backprop):
    """the expression of optym_plan.activation (the kernel's) in long double, on the input and the parameters as the dtype rounds them"""
    x = np.asarray(x)
    T = x.dtype.type
    a_, m2a, ma, x0, y0 = (LD(T(v)) for v in (a, -2.0 * a, -a, x0, y0))
    xs = x.astype(LD) - x0
    with np.errstate(all='ignore'):
        fwd = {OP.TANH: lambda: 2 / (1 + np.exp(m2a * xs)) - 1, OP.ARCTAN: lambda: np.arctan(a_ * xs), OP.SOFTPLUS: lambda: np.log(1 + np.exp(a_ * xs)),
               OP.SIGMOID: lambda: 1 / (1 + np.exp(ma * xs))}[kind]
        if not backprop:
            return fwd() + y0
        if kind == OP.TANH:
            return a_ * (1 - fwd() ** 2)
        if kind == OP.ARCTAN:
            return a_ / ((a_ * xs) ** 2 + 1)
        if kind == OP.SOFTPLUS:
            return a_ / (1 + np.exp(ma * xs))
        return a_ * fwd() * (1 - fwd())


def activation_ratio(got, model, want):
    """largest |got - want| / bound over the entries where the model is finite (0 where there is none)"""
    fin = np.isfinite(model)
    if not fin.any():
        return 0.0
    g, m, w = got[fin].astype(LD), model[fin].astype(LD), want[fin]
    bound = np.maximum(4 * np.abs(m - w), 4 * eps_of(got.dtype) * np.maximum(1, np.abs(w)))
    return float((np.abs(g - w) / bound).max())


def run_activation(kind, backprop, x, a, x0, y0):
    lib = L.load()
    xin, out = Band(x), Band(n=x.size, dtype=x.dtype)
    L.check(lib.pm_optym_activation(CODE[x.dtype], kind, int(backprop), x.size, xin.ptr, float(a), float(x0), float(y0), out.ptr, L.stream_ptr()))
    got = out.read()
    assert xin.unchanged()
    return got


# ----------------------------------------------------------------------------- softmax

SOFTMAX_K = (1, 2, 3, 33, 63, 64, 65, 128, 129, 200)
SPECIAL_K = (3, 4, 64, 100, 128)
GUMBEL_K = (7, 65, 200)
GUMBEL_TAU = (0.7, 1.0)
SPECIAL_ROWS = ('equal', 'saturated', 'some -inf', 'all -inf', '+-1e4')


def softmax_rows(K):
    per = 256 // OP.softmax_group(K)
    return sorted({r for r in (1, per - 1, per, per + 1, 3 * per + 1) if r >= 1})


@functools.lru_cache(maxsize=None)
def softmax_input(K, rows, dtname):
    """U(-20, 20) logits, row r shifted by r: no two rows give the same probabilities to rounding, so a row read from the wrong place
    cannot pass"""
    rng = np.random.default_rng([K, rows])
    x = rng.uniform(-20, 20, (rows, K)) + np.arange(rows)[:, None]
    return frozen(x.astype(np.dtype(dtname))), frozen(rng.standard_normal((rows, K)).astype(np.dtype(dtname)))


def softmax_reference(x):
    x = np.asarray(x).astype(LD)
    with np.errstate(invalid='ignore'):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def softmax_ratio(got, x, want, extra=0.0):
    """largest |y - want| / (4 (2 + |x - max x|) eps(T) + extra) want over the entries with 0 < want, finite; every one of them counts"""
    x = np.asarray(x).astype(LD)
    keep = np.isfinite(want) & (want > 0)
    if not keep.any():
        return 0.0
    with np.errstate(invalid='ignore'):
        rel = 4 * (2 + np.abs(x - x.max(axis=-1, keepdims=True))) * eps_of(got.dtype) + extra
    return float((np.abs(got.astype(LD) - want)[keep] / (rel[keep] * want[keep])).max())


def row_sum_ratio(got):
    K = got.shape[-1]
    return float(np.abs(got.astype(LD).sum(axis=-1) - 1).max() / (K * eps_of(got.dtype)))


def softmax_backprop_reference(y, g, tau):
    """the kernel's expression y (g S - sum g y) / tau, S = sum y, in long double on the STORED y"""
    y, g = np.asarray(y).astype(LD), np.asarray(g).astype(LD)
    with np.errstate(invalid='ignore'):
        return y * (g * y.sum(axis=-1, keepdims=True) - (g * y).sum(axis=-1, keepdims=True)) / LD(tau)


def softmax_backprop_naive(y, g, tau):
    """the reference's own expression y (g - sum g y) / tau evaluated in y's dtype: what the kernel does NOT do"""
    y, g = np.asarray(y), np.asarray(g, dtype=np.asarray(y).dtype)
    return y * (g - (g * y).sum(axis=-1, keepdims=True)) / y.dtype.type(tau)


def softmax_backprop_ratio(got, y, g, want, tau):
    keep = np.isfinite(want)
    if not keep.any():
        return 0.0
    K = y.shape[-1]
    bound = eps_of(got.dtype) * np.abs(want) + 4 * K * EPS64 * np.abs(np.asarray(g).astype(LD)).max() * np.asarray(y).astype(LD) / LD(tau)
    err = np.abs(got.astype(LD) - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0, err / bound)            # 0 / 0 where y is exactly 0: the result must then be exactly 0
    return float(ratio[keep].max())


@functools.lru_cache(maxsize=None)
def special_rows(K, dtname):
    """the rows of SPECIAL_ROWS, in that order, and a gradient"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng(500 + K)
    x = np.empty((len(SPECIAL_ROWS), K))
    x[0] = 2.5
    x[1] = rng.uniform(-1, 1, K)
    x[1, K // 2] = x[1].max() + (30 if dt == np.float32 else 20)
    x[2] = rng.uniform(-5, 5, K)
    x[2, ::3] = -np.inf
    if K < 3:
        x[2, 1:] = 0.0
    x[3] = -np.inf
    x[4] = np.where(np.arange(K) % 2 == 0, 1e4, -1e4)
    return frozen(x.astype(dt)), frozen(rng.standard_normal(x.shape).astype(dt))


@functools.lru_cache(maxsize=None)
def gumbel_input(K, dtname):
    """(x, u, g, eps): u in [0, 1) with exact zeros and values one ulp below 1 in every row"""
    dt = np.dtype(dtname)
    rows = 3 * (256 // OP.softmax_group(K)) + 1
    rng = np.random.default_rng(900 + K)
    x = rng.uniform(-3, 3, (rows, K)).astype(dt)
    u = rng.random((rows, K)).astype(dt)
    u[u >= 1] = 0.5
    u[:, 0] = 0
    u[:, K - 1] = np.nextafter(dt.type(1), dt.type(0))
    u[::2, K // 2] = np.nextafter(dt.type(1), dt.type(0))
    return frozen(x), frozen(u), frozen(rng.standard_normal((rows, K)).astype(dt)), eps_of(dt)


def gumbel_extra(x, u, tau, eps):
    """3 max_j dl_j per row, the widening of the forward bound by the roundings of the logits (module docstring); and the logits"""
    T = x.dtype.type
    with np.errstate(all='ignore'):
        G = -np.log(-np.log(u + T(eps)) + T(eps))
    logits = OP.gumbel_logits(x, u, tau, eps)
    dl = eps_of(x.dtype) * ((3 + 2 * np.abs(G.astype(LD))) / LD(tau) + 2 * np.abs(logits.astype(LD)))
    return 3 * dl.max(axis=-1, keepdims=True), logits


def run_softmax(x, u=None, tau=1.0, eps=0.0):
    lib = L.load()
    rows, K = x.shape
    xin, uin, out = Band(x), Band(u) if u is not None else None, Band(n=x.size, dtype=x.dtype)
    L.check(lib.pm_optym_softmax(CODE[x.dtype], rows, K, xin.ptr, uin.ptr if uin else null(), float(tau), float(eps), out.ptr, L.stream_ptr()))
    got = out.read().reshape(rows, K)
    assert xin.unchanged() and (uin is None or uin.unchanged()), 'pm_optym_softmax wrote an input'
    return got


def run_softmax_backprop(y, g, tau=1.0):
    lib = L.load()
    rows, K = y.shape
    yin, gin_, out = Band(y), Band(g), Band(n=y.size, dtype=y.dtype)
    L.check(lib.pm_optym_softmax_backprop(CODE[y.dtype], rows, K, yin.ptr, gin_.ptr, float(tau), out.ptr, L.stream_ptr()))
    got = out.read().reshape(rows, K)
    assert yin.unchanged() and gin_.unchanged()
    return got


# ----------------------------------------------------------------------------- spatial gradient

GRADIENT_SHAPES = ((1, 5), (5, 1), (2, 7), (7, 2), (3, 63), (4, 64), (5, 65), (9, 129))
GRADIENT_OPS = {'forward_x': OP.FORWARD_X, 'adjoint_x': OP.ADJOINT_X, 'forward_y': OP.FORWARD_Y, 'adjoint_y': OP.ADJOINT_Y}


def run_spatial_gradient(op, a):
    lib = L.load()
    m, n = a.shape
    ain, out = Band(a), Band(n=a.size, dtype=a.dtype)
    L.check(lib.pm_optym_spatial_gradient(CODE[a.dtype], op, m, n, ain.ptr, out.ptr, L.stream_ptr()))
    got = out.read().reshape(m, n)
    assert ain.unchanged()
    return got
