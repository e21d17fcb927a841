"""GPU: PrysmLBFGSB (prysm_amd/x/optym/lbfgsb.py on csrc/lbfgsb.hip) against the reference's fixture and against the numpy model
(prysm_amd/x/lbfgsb_plan.py); the kernels at the C ABI at the shapes where they can go wrong; bit reproducibility; run_until; the
host reads of a step; a NaN gradient.  Every test prints the figures it asserts on."""

import numpy as np
import pytest
import torch

import lbfgsb_common as C
from conftest import rel_max
from prysm_amd import _lib as L
from prysm_amd.x import lbfgsb_plan as plan
from test_lbfgsb_host import model_result, model_step

pytestmark = pytest.mark.gpu

TD = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
DTYPES = [np.float64, np.float32]
IDS = ['f64', 'f32']


def tonp(t):
    return t.detach().cpu().numpy()


def device_opt(st, dtype, f_on_device=True):
    from prysm_amd.x.optym import PrysmLBFGSB
    return PrysmLBFGSB(C.fg_torch(TD[np.dtype(dtype)], f_on_device, C.A_of(st)), st['x'].astype(dtype), memory=C.MEMORY, **C.bounds_of(st, dtype))


def device_result(opt):
    S, Y = opt._history()
    core, P = opt._core, opt._passes
    bounded = core.has_bounds
    return dict(x_new=tonp(opt.x), pair=(tonp(S[-1]), tonp(Y[-1])) if len(S) else None, theta=opt.theta, metadata=opt.last_step_metadata,
                evals=P.evals, accepted=core.last_pair_accepted, xc=tonp(P.xc) if bounded else None,
                c=core.last_cauchy['c'] if bounded else None, free=tonp(P.free) if bounded else None)


def as_want(res):
    """a result in the fixture's layout, to hold another result against"""
    md = res['metadata']
    want = dict(x_new=res['x_new'], theta_new=res['theta'], alpha=md['alpha'], free_vars=md['free_vars'], cauchy_breaks=md['cauchy_breaks'],
                mode=C.MODES[md['subspace_mode']], evals=np.zeros(res['evals']), accepted=res['accepted'])
    if res['pair'] is not None:
        want['s_new'], want['y_new'] = res['pair']
    if res['xc'] is not None:
        want.update(xc=res['xc'], c=res['c'], free=res['free'])
    return want


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('label,st', C.STATES, ids=C.STATE_IDS)
def test_every_fixture_step_through_the_class(pa, label, st, dtype):
    opt = device_opt(st, dtype)
    reads0 = opt.host_reads
    stopped = C.step_from(opt, st)
    m, mstopped = model_step(st, dtype)
    assert stopped == mstopped
    if stopped is not None:
        C.compare_step(label, st, stopped, None, None, None, None, None, None, dtype)
        assert np.array_equal(tonp(opt.x), st['x'].astype(dtype)) and opt.last_step_metadata == {'reason': 'no_descent'}
        return
    res = device_result(opt)
    name = np.dtype(dtype).name
    C.compare_step(f'{label} {name} device-reference', st, None, dtype=dtype, **res)
    C.compare_step(f'{label} {name} device-model', st, None, dtype=dtype, want=as_want(model_result(m)), **res)
    assert opt.iter == 1 and opt.nfev == 1 and np.array_equal(tonp(opt.x_prev), st['x'].astype(dtype))
    # the Gram matrices the device keeps (pm_lbfgsb_small updated them in place; a full history dropped its oldest pair) against the model's
    kk, MH = opt._core.H.k, m.core.H
    assert (kk, opt._core.H.start, opt._core.H.slot) == (MH.k, MH.start, MH.slot)
    for name_, got, want_ in zip(('SS', 'SY', 'YY'), opt._passes.gram_matrices(), (MH.SS, MH.SY, MH.YY)):
        gerr = rel_max(got[:kk, :kk], want_[:kk, :kk]) if kk else 0.0
        print(f'{label} {name} device Gram {name_} against the model {gerr:.2e}')
        assert gerr <= 1e-12      # double sums of the same products in another order
    # the host reads of the step are the module docstring's formula
    k, md, E = int(st['k']), opt.last_step_metadata, res['evals']
    if md['subspace_mode'] == 'unbounded':
        want = 1 + E + 1
    else:
        want = 1 + opt._core.last_cauchy['chunks'] + 1 + E + 1      # the issue's budget: 3, one per chunk, one for the direction
    print(f'{label} {name} host reads {opt.host_reads - reads0}, formula {want}')
    assert opt.host_reads - reads0 == want
    if md['subspace_mode'] == 'unbounded' and E == 1:
        assert opt.host_reads - reads0 <= 3


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_refused_pair_leaves_the_history_and_the_next_step_reuses_its_row(pa, dtype):
    """hand-2 (a non-convex objective): the update pass writes the free row, the curvature test refuses the pair, x moves on; the next
    step from there is held against the model's second step"""
    st = dict(C.STATES)['hand-2-refused-pair']
    opt = device_opt(st, dtype)
    assert C.step_from(opt, st) is None
    m, _ = model_step(st, dtype)
    H = opt._core.H
    assert not opt._core.last_pair_accepted and (H.k, H.slot, opt.theta) == (0, 0, 1.0) and opt.iter == 1
    s0 = tonp(opt._passes.S[0])
    assert np.array_equal(s0, tonp(opt.x) - tonp(opt.x_prev)) and np.any(s0)
    opt.step()
    m.step()
    assert opt.last_step_metadata['cauchy_breaks'] == m.last_step_metadata['cauchy_breaks']
    assert opt.last_step_metadata['subspace_mode'] == m.last_step_metadata['subspace_mode'] and H.k == m.core.H.k
    assert opt._core.last_pair_accepted == m.core.last_pair_accepted and opt._passes.evals == m.passes.evals
    err = rel_max(tonp(opt.x), m.x)
    print(f'second step after the refused pair, {np.dtype(dtype).name}: device-model x {err:.2e}, k {H.k}')
    assert err <= C.TOL[np.dtype(dtype)]
    assert H.slot in (0, 1) and not np.array_equal(tonp(opt._passes.S[0]), s0)      # accepted or not, the update pass rewrote the free row


def test_an_unbounded_step_at_a_stationary_point_stops_before_any_trial(pa):
    from prysm_amd.x.optym import PrysmLBFGSB
    calls = [0]

    def fg(x):
        calls[0] += 1
        return torch.sum(x * 0), torch.zeros_like(x)
    opt = PrysmLBFGSB(fg, np.ones(300), memory=3)
    with pytest.raises(StopIteration) as stop:
        opt.step()
    assert stop.value.value.message == 'no descent direction' and calls[0] == 1 and opt.host_reads == 1
    assert opt.last_step_metadata == {'reason': 'no_descent'}


def test_f_as_a_python_float_gives_the_same_step(pa):
    st = dict(C.STATES)['bounded-6']
    a, b = device_opt(st, np.float64, True), device_opt(st, np.float64, False)
    assert C.step_from(a, st) is None and C.step_from(b, st) is None
    assert torch.equal(a.x, b.x) and a.host_reads == b.host_reads


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('label', ['free-7', 'bounded-0', 'bounded-7'])
def test_the_same_step_twice_gives_the_same_bits(pa, label, dtype):
    st = dict(C.STATES)[label]
    runs = []
    for _ in range(2):
        opt = device_opt(st, dtype)
        assert C.step_from(opt, st) is None
        runs.append([tonp(opt.x), tonp(opt._passes.S), tonp(opt._passes.Y), *opt._passes.gram_matrices(), np.float64(opt.theta)])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))


# ---------------------------------------------------------------------------------------------------------------- the kernels

class Bench:
    """a history of k pairs in a ring that starts at a nonzero row, rows `ld` apart, on the device and in a NumpyPasses model"""

    def __init__(self, n, k, dtype, pad, seed):
        rng = np.random.default_rng(seed)
        self.n, self.k, self.dtype, self.code = n, k, np.dtype(dtype), L.PM_F32 if np.dtype(dtype) == np.float32 else L.PM_F64
        self.ring, self.start, self.ld = k + 1, (2 if k > 1 else 0), n + pad
        self.lo, self.hi = np.full(n, -0.5, dtype), np.full(n, 0.7, dtype)
        x = np.clip(rng.standard_normal(n), -0.5, 0.7).astype(dtype)
        self.P = P = plan.NumpyPasses(None, x, max(k, 1), self.lo, self.hi)
        P.S, P.Y = rng.standard_normal((self.ring, n)).astype(dtype), rng.standard_normal((self.ring, n)).astype(dtype)
        P.H = plan.History(max(k, 1), dtype)
        P.H.ring, P.H.k, P.H.start = self.ring, k, self.start
        P.g = rng.standard_normal(n).astype(dtype)
        P.g[::7] = 0
        self.rng = rng
        self.lib = L.load()
        self.S, self.Y = self.rows(P.S), self.rows(P.Y)
        self.ws_bytes = self.lib.pm_lbfgsb_workspace()
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device='cuda')
        self.rec = torch.full((4096,), np.nan, dtype=torch.float64, device='cuda')

    def rows(self, a):
        t = torch.zeros((self.ring, self.ld), dtype=TD[self.dtype], device='cuda')
        t[:, :self.n] = torch.from_numpy(a).cuda()
        return t

    def dev(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def hist(self):
        return (self.code, self.n, L.ptr(self.S), L.ptr(self.Y), self.ld, self.ring, self.start, self.k)

    def tail(self):
        return (L.ptr(self.rec), L.ptr(self.ws), self.ws_bytes, None)

    def record(self, count):
        torch.cuda.synchronize()
        return self.rec[:count].cpu().numpy()


def close(label, got, want, scale=None):
    """double sums of the same products in another order: 1e-12 of the sum of magnitudes"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.max(np.abs(got - want))) if got.size else 0.0
    bound = 1e-12 * (float(np.max(np.abs(want))) if scale is None else scale) + 1e-300
    print(f'{label}: err {err:.2e} bound {bound:.2e}')
    assert err <= bound, (label, err, bound)


# (n, k, the padding of a row).  W = [Y, theta S] always has an even number of rows, so the fewest is 2 (k = 1): a single row cannot
# be asked for.  k = 5 is 10 rows, a ragged second tile and three tile pairs; k = 32 the cap, 8 tiles and 36 pairs.  The last two are
# the second trip of the grid-stride loops, of the dots / combine passes and of the Gram pass (with three tile pairs).  k = 0 at the
# C ABI (no history: phi' = g . p) is test_small_algebra_at_the_c_abi's and every step's evaluate()
SHAPES = [(1, 1, 0), (2, 5, 0), (255, 1, 3), (1027, 5, 5), (1027, 32, 0), (L.PM_LBFGSB_THREADS * L.PM_LBFGSB_WGS + 3, 5, 0),
          (L.PM_LBFGSB_THREADS * L.PM_LBFGSB_GRAM_WGS + 3, 5, 1)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('n,k,pad', SHAPES, ids=[f'n{n}-k{k}-pad{p}' for n, k, p in SHAPES])
def test_kernels_against_the_model(pa, n, k, pad, dtype):
    B = Bench(n, k, dtype, pad, seed=n + k)
    P, lib, T = B.P, B.lib, np.dtype(dtype).type
    W = P._W()
    mag = float(np.max(np.abs(W) @ np.abs(P.g.astype(np.float64)))) + 1.0
    masks = [None, np.ones(n, np.uint8), np.zeros(n, np.uint8), np.eye(1, n, n // 2, dtype=np.uint8)[0]]
    g = B.dev(P.g)
    # ---- dots and the free-set Gram under every mask
    for mi, mask in enumerate(masks):
        md = B.dev(mask)
        L.check(lib.pm_lbfgsb_dots(*B.hist(), L.ptr(g), None, L.ptr(md), *B.tail()))
        prod, (vv,) = plan.unpack_dots(B.record(plan.tiles_of(k) * 9), k, 1, 1)
        sel = slice(None) if mask is None else mask.astype(bool)
        g64 = P.g.astype(np.float64)
        close(f'dots mask {mi}', prod[:, 0], W[:, sel] @ g64[sel], mag)
        close(f'dots v.v mask {mi}', vv, g64[sel] @ g64[sel], mag)
        L.check(lib.pm_lbfgsb_gram(*B.hist(), L.ptr(md), *B.tail()))
        G = plan.unpack_gram(B.record(plan.gram_record_doubles(k)), k)
        close(f'gram mask {mi}', G, W[:, sel] @ W[:, sel].T, float(np.max(np.abs(W) @ np.abs(W).T)))
    # ---- breakpoints
    t, d0 = torch.zeros(n, dtype=TD[B.dtype], device='cuda'), torch.zeros(n, dtype=TD[B.dtype], device='cuda')
    x, lo, hi = B.dev(P.x), B.dev(B.lo), B.dev(B.hi)
    L.check(lib.pm_lbfgsb_breakpoints(*B.hist(), L.ptr(x), L.ptr(g), L.ptr(lo), L.ptr(hi), L.ptr(t), L.ptr(d0), *B.tail()))
    prod, extra = plan.unpack_dots(B.record(plan.tiles_of(k) * 11), k, 1, 3)
    wp, wdd, wzero, wpos, _ = P.breakpoints()
    assert np.array_equal(tonp(t), P.t) and np.array_equal(tonp(d0), P.d0) and (extra[1], extra[2]) == (wzero, wpos)
    assert wzero > 0 or n < 10
    close('breakpoints W^T d0', prod[:, 0], wp, mag)
    close('breakpoints d0.d0', extra[0], wdd, mag)
    # ---- the Cauchy point
    finite = np.sort(P.t[np.isfinite(P.t)])
    t_last = float(finite[len(finite) // 2]) if len(finite) else 0.0
    xc, free = torch.zeros(n, dtype=TD[B.dtype], device='cuda'), torch.zeros(n, dtype=torch.uint8, device='cuda')
    L.check(lib.pm_lbfgsb_cauchy_point(B.code, n, L.ptr(x), L.ptr(g), L.ptr(t), t_last, t_last + 0.01, L.ptr(xc), L.ptr(free), None))
    P.cauchy_point(t_last, t_last + 0.01)
    assert np.array_equal(tonp(xc), P.xc) and np.array_equal(tonp(free).astype(bool), P.free)
    # ---- the combinations: the direction, the residual, the subspace tail
    coef = B.rng.standard_normal(2 * k)
    cd = B.dev(coef)
    p, r, ph = (torch.zeros(n, dtype=TD[B.dtype], device='cuda') for _ in range(3))
    L.check(lib.pm_lbfgsb_combine(B.code, L.PM_LBFGSB_DIRECTION, n, *B.hist()[2:], -0.7, L.ptr(g), 0.0, None, None, L.ptr(cd), None, None, None,
                                  None, None, L.ptr(g), L.ptr(p), None, *B.tail()))
    P.direction(-0.7, coef)
    rec = B.record(5)
    tolT = 4 * float(np.finfo(dtype).eps)
    err = rel_max(tonp(p), P.p)
    print(f'direction: p {err:.2e}')
    assert err <= tolT
    gp = P.g.astype(np.float64) @ tonp(p).astype(np.float64)
    close('direction g.p', rec[0], gp, mag * 10)
    assert rec[1] == np.sum(tonp(p) != 0) and rec[4] == np.inf
    L.check(lib.pm_lbfgsb_combine(B.code, L.PM_LBFGSB_RESIDUAL, n, *B.hist()[2:], 1.0, L.ptr(g), 1.3, L.ptr(xc), L.ptr(x), L.ptr(cd), None, None,
                                  None, None, None, None, L.ptr(r), None, None, None, 0, None))
    P.residual(1.3, coef)
    err = rel_max(tonp(r), P.r)
    print(f'residual: r {err:.2e}')
    assert err <= tolT
    P.r = tonp(r)      # the same r on both sides of the next pass
    L.check(lib.pm_lbfgsb_combine(B.code, L.PM_LBFGSB_SUBSPACE, n, *B.hist()[2:], -0.4, L.ptr(r), 0.0, None, None, L.ptr(cd), L.ptr(free), L.ptr(xc),
                                  L.ptr(x), L.ptr(lo), L.ptr(hi), L.ptr(g), L.ptr(p), L.ptr(ph), *B.tail()))
    P.subspace(-0.4, coef)
    rec = B.record(5)
    e1, e2 = rel_max(tonp(p), P.p), rel_max(tonp(ph), P.p_hat)
    print(f'subspace: p {e1:.2e} p_hat {e2:.2e}')
    assert e1 <= 4 * tolT and e2 <= 4 * tolT and np.all(tonp(x) + tonp(p) <= B.hi + tolT) and np.all(tonp(x) + tonp(p) >= B.lo - tolT)
    dp, dph, g64 = tonp(p).astype(np.float64), tonp(ph).astype(np.float64), P.g.astype(np.float64)
    close('subspace g.p', rec[0], g64 @ dp, mag * 10)
    close('subspace g.p_hat', rec[2], g64 @ dph, mag * 10)
    assert rec[1] == np.sum(dp != 0) and rec[3] == np.sum(dph != 0)
    with np.errstate(all='ignore'):
        php, xx = tonp(ph), tonp(x)
        ba = np.where(php > 0, (B.hi - xx) / php, np.where(php < 0, (B.lo - xx) / php, np.inf))
    assert rec[4] == float(np.min(ba.astype(np.float64)))
    # ---- the trial point, free and clipped
    xt = torch.zeros(n, dtype=TD[B.dtype], device='cuda')
    P.p = tonp(p)
    for bounded in (False, True):
        L.check(lib.pm_lbfgsb_trial(B.code, n, L.ptr(x), L.ptr(p), 0.37, L.ptr(lo if bounded else None), L.ptr(hi if bounded else None),
                                    L.ptr(xt), None))
        P.bounded = bounded
        P.trial(0.37)
        assert np.array_equal(tonp(xt), P.xt)
    # ---- the history update: the pair into the free row, the 4k + 3 products
    gn = B.dev((P.g + B.rng.standard_normal(n).astype(dtype) * T(0.1)))
    P.g_new = tonp(gn)
    for bounded in (True, False):
        P.bounded = bounded
        slot = P.H.slot
        L.check(lib.pm_lbfgsb_update(*B.hist(), slot, L.ptr(xt if bounded else None), L.ptr(x if bounded else None), L.ptr(p), 0.37, L.ptr(gn),
                                     L.ptr(g), *B.tail()))
        prod, extra = plan.unpack_dots(B.record(plan.tiles_of(k) * 19), k, 2, 3)
        live_S, live_Y = P.S[P.H.rows()].copy(), P.Y[P.H.rows()].copy()
        wprod, wextra = P.update(0.37)
        assert np.array_equal(tonp(B.S[slot, :n]), P.S[slot]) and np.array_equal(tonp(B.Y[slot, :n]), P.Y[slot])
        assert np.array_equal(tonp(B.S[:, :n])[P.H.rows()], live_S) and np.array_equal(tonp(B.Y[:, :n])[P.H.rows()], live_Y)
        assert not pad or float(B.S[:, n:].abs().max()) == 0.0      # nothing is written between the rows
        close(f'update products bounded={bounded}', prod, wprod, mag)
        close(f'update s.s s.y y.y bounded={bounded}', extra, wextra, mag)


@pytest.mark.parametrize('k', [1, 5, 32])
def test_small_algebra_at_the_c_abi(pa, k):
    """pm_lbfgsb_small by itself against lbfgsb_plan.History, up to the cap (2k = 64 fills the matrix in LDS): the direction's
    coefficients from the maintained Gram matrices, the subspace's with no variable active (the same matrices), M in the breakpoint
    record, M^-1 c, and an update on a full history (the matrices move up and left)"""
    n, lib = 1027, L.load()
    rng = np.random.default_rng(k)
    S = rng.standard_normal((k, n))
    Y = 2.0 * S + 0.3 * rng.standard_normal((k, n))
    H = plan.History(k, np.float64)
    H.rebuild(S, Y)
    B = Bench(n, k, np.float64, 0, seed=k)
    B.start = 0
    B.S[:k, :n], B.Y[:k, :n] = torch.from_numpy(S).cuda(), torch.from_numpy(Y).cuda()
    state = torch.zeros(lib.pm_lbfgsb_state_doubles(k), dtype=torch.float64, device='cuda')
    state[:3 * k * k + 1] = torch.from_numpy(np.concatenate([H.SS.ravel(), H.SY.ravel(), H.YY.ravel(), [H.theta]])).cuda()
    coef = torch.zeros(64, dtype=torch.float64, device='cuda')
    rec = torch.zeros(4352, dtype=torch.float64, device='cuda')
    g = rng.standard_normal(n)
    gd = B.dev(g)
    nparts = min(L.PM_LBFGSB_WGS, -(-n // L.PM_LBFGSB_THREADS))
    W = np.concatenate([Y, S])

    def small(op, c_in=None):
        L.check(lib.pm_lbfgsb_small(L.PM_F64, op, k, k, nparts, 0, L.ptr(state), L.ptr(c_in), L.ptr(coef), L.ptr(rec), L.ptr(B.ws), None, None))
        torch.cuda.synchronize()
    for op in (L.PM_LBFGSB_SMALL_DIRECTION, L.PM_LBFGSB_SMALL_SUBSPACE):
        L.check(lib.pm_lbfgsb_dots(*B.hist(), L.ptr(gd), None, None, None, L.ptr(B.ws), B.ws_bytes, None))
        small(op)
        want = H.solve_N(H.raw_gram(), W @ g)
        err = rel_max(tonp(coef)[:2 * k], want)
        print(f'small op {op} k {k}: coef {err:.2e}')
        assert err <= 1e-9
    assert abs(float(rec[0]) - g @ g) <= 1e-12 * (g @ g)
    x = B.dev(B.P.x)
    t, d0 = torch.zeros(n, dtype=torch.float64, device='cuda'), torch.zeros(n, dtype=torch.float64, device='cuda')
    L.check(lib.pm_lbfgsb_breakpoints(*B.hist(), L.ptr(x), L.ptr(gd), L.ptr(B.dev(B.lo)), L.ptr(B.dev(B.hi)), L.ptr(t), L.ptr(d0), None, L.ptr(B.ws),
                                      B.ws_bytes, None))
    small(L.PM_LBFGSB_SMALL_BREAK)
    n2 = 2 * k
    raw = tonp(rec)[:n2 + 4 + n2 * n2]
    d0n = tonp(d0)
    assert np.array_equal(raw[n2 + 4:].reshape(n2, n2), H.M()) and raw[n2 + 3] == H.theta
    close('small break W^T d0', raw[:n2], W @ d0n, float(np.max(np.abs(W) @ np.abs(d0n))) + 1)
    assert raw[n2 + 1] == np.sum(tonp(t) <= 0) and raw[n2 + 2] == np.sum((tonp(t) > 0) & np.isfinite(tonp(t)))
    c = rng.standard_normal(n2)
    small(L.PM_LBFGSB_SMALL_RESIDUAL, B.dev(c))
    err = rel_max(tonp(coef)[:n2], -H.scale() * np.linalg.solve(H.M(), c))
    print(f'small residual k {k}: coef {err:.2e}')
    assert err <= 1e-9
    # the update on a full history: the pair goes into the ring's free row (row k of k + 1), the oldest pair leaves the matrices
    xt, p = B.dev(B.P.x + 0.1 * rng.standard_normal(n)), B.dev(np.zeros(n))
    gn = B.dev(g + 0.2 * (tonp(xt) - B.P.x) + 0.01 * rng.standard_normal(n))
    L.check(lib.pm_lbfgsb_update(*B.hist(), k, L.ptr(xt), L.ptr(x), L.ptr(p), 1.0, L.ptr(gn), L.ptr(gd), None, L.ptr(B.ws), B.ws_bytes, None))
    small(L.PM_LBFGSB_SMALL_UPDATE)
    s, y = tonp(xt) - B.P.x, tonp(gn) - g
    assert float(rec[0]) == 1.0
    H.accept(Y @ s, S @ s, Y @ y, S @ y, s @ s, s @ y, y @ y)
    host = tonp(state)
    for i, want in enumerate((H.SS, H.SY, H.YY)):
        err = rel_max(host[i * k * k:(i + 1) * k * k].reshape(k, k), want)
        print(f'small update k {k}: matrix {i} {err:.2e}')
        assert err <= 1e-12
    assert abs(host[3 * k * k] - H.theta) <= 1e-12 * H.theta and abs(float(rec[4]) - H.theta) <= 1e-12 * H.theta


# ---------------------------------------------------------------------------------------------------------------- runs

class ProjectedGradientTolerance:
    """stops when ||x - P(x - g)||_inf <= tol (a Governor of the test's own: under bounds the plain gradient does not vanish)"""

    def __init__(self, tol, lo, hi):
        self.tol, self.lo, self.hi = tol, lo, hi

    def observe(self, record):
        from prysm_amd.x.optym import GovernorDecision
        pg = float(torch.max(torch.abs(record.x - torch.clamp(record.x - record.g, self.lo, self.hi))))
        return GovernorDecision(pg <= self.tol, pg <= self.tol, 'projected gradient tolerance reached')


def test_run_until_free(pa):
    from prysm_amd.x.optym import GradientTolerance, PrysmLBFGSB, run_until
    gtol = 1e-6
    opt = PrysmLBFGSB(C.fg_torch(torch.float64), C.PROBLEM['x0'], memory=C.MEMORY)
    res = run_until(opt, GradientTolerance(gtol), maxiter=300)
    assert res.success and res.message == 'gradient tolerance reached', res.message
    x = tonp(res.records[-1].x)
    fg = C.fg_numpy(np.float64)
    g, xs = fg(x)[1], C.PROBLEM['xstar_free']
    dist, bound = np.linalg.norm(x - xs), 2 * (np.linalg.norm(g) + np.linalg.norm(fg(xs)[1]))
    print(f'free: {len(res.records)} steps, |g|inf {np.max(np.abs(g)):.2e}, |x - x*| {dist:.2e} <= {bound:.2e}')
    assert np.max(np.abs(g)) <= gtol and dist <= bound


def test_run_until_bounded(pa):
    from prysm_amd.x.optym import AnyGovernor, GradientTolerance, PrysmLBFGSB, run_until
    gtol = 1e-6
    lo, hi = float(C.PROBLEM['lo']), float(C.PROBLEM['hi'])
    fs, inside = [], []

    class Watch(ProjectedGradientTolerance):
        def observe(self, record):
            fs.append(float(record.f))
            inside.append(bool(torch.all((record.x_next >= lo) & (record.x_next <= hi))))
            return super().observe(record)
    opt = PrysmLBFGSB(C.fg_torch(torch.float64), C.PROBLEM['x0'], memory=C.MEMORY, lower_bounds=np.full(C.N, lo), upper_bounds=np.full(C.N, hi))
    assert bool(torch.all((opt.x >= lo) & (opt.x <= hi)))
    res = run_until(opt, AnyGovernor([GradientTolerance(gtol), Watch(gtol, lo, hi)]), maxiter=300)
    assert res.success and res.message == 'projected gradient tolerance reached', res.message
    x = tonp(res.records[-1].x)
    g = C.fg_numpy(np.float64)(x)[1]
    pg = np.max(np.abs(x - np.clip(x - g, lo, hi)))
    print(f'bounded: {len(res.records)} steps, projected gradient {pg:.2e}, f {fs[0]:.6e} -> {fs[-1]:.6e}')
    assert all(inside) and all(b <= a for a, b in zip(fs, fs[1:])) and pg <= gtol


@pytest.mark.parametrize('after', [0, 3, 8])
def test_a_nan_gradient_is_data(pa, after):
    """a NaN in the gradient from evaluation `after` + 1 on (at a step's start, or inside a search): the search fails, the stop is
    'line search failed', x is what it was when the step began, nothing faults.  Under bounds the reference's search ACCEPTS a trial
    point pinned at the cap whatever its slope, so a NaN travels on there; that run must only not fault."""
    from prysm_amd.x.optym import MaxIterations, PrysmLBFGSB, run_until
    good = C.fg_torch(torch.float64)
    calls, begun = [0], [None]

    def fg(x):
        calls[0] += 1
        if x.data_ptr() == opt.x.data_ptr():
            begun[0] = x.clone()
        f, g = good(x)
        if calls[0] > after:
            g = g.clone()
            g[5] = float('nan')
        return f, g
    opt = PrysmLBFGSB(fg, C.PROBLEM['x0'], memory=C.MEMORY)
    res = run_until(opt, MaxIterations(20))
    assert not res.success and res.message == 'line search failed', res.message
    assert opt.last_step_metadata == {'reason': 'linesearch_fail'} and torch.equal(opt.x, begun[0]) and bool(torch.all(torch.isfinite(opt.x)))
    print(f'NaN gradient after {after} evaluations: stopped in step {opt.iter + 1} after {calls[0]} evaluations')
    calls[0] = 0
    opt = PrysmLBFGSB(fg, C.PROBLEM['x0'], memory=C.MEMORY, lower_bounds=np.full(C.N, -0.4), upper_bounds=np.full(C.N, 0.6))
    res = run_until(opt, MaxIterations(3))
    torch.cuda.synchronize()
    assert res.message in ('maximum iterations reached', 'line search failed', 'no descent direction'), res.message


def test_reset_clears_the_history_in_place(pa):
    st = dict(C.STATES)['free-7']
    opt = device_opt(st, np.float64)
    ptrs = (opt.x.data_ptr(), opt.x_prev.data_ptr(), opt._passes.S.data_ptr())
    assert C.step_from(opt, st) is None and opt._core.H.k == C.MEMORY
    opt.reset()
    assert (opt.iter, opt.nfev, opt._core.H.k, opt.theta) == (0, 0, 0, 1.0) and opt.last_step_metadata == {}
    assert ptrs == (opt.x.data_ptr(), opt.x_prev.data_ptr(), opt._passes.S.data_ptr())
    assert np.array_equal(tonp(opt.x), st['x'].astype(np.float64)) and float(opt._passes.S.abs().max()) == 0.0
    opt.step()
    assert opt.iter == 1 and opt._core.H.k == 1
