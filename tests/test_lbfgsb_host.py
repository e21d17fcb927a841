"""CPU: L-BFGS-B without a device -- the numpy model (prysm_amd/x/lbfgsb_plan.py) against every step of the reference's fixture
(tests/golden/make_golden_lbfgsb.py), the strong-Wolfe search against the reference's on recorded scalar functions, the incremental Gram
update against full products, and the argument checks of the entry points of csrc/lbfgsb.hip.

Figures, model against the reference's float64 step from the same float32 state (rel_max, the worst over the 31 states that step;
per state in profiles/lbfgsb/parity.txt, printed by the tests): float64 model x_new 6.5e-16, the worst of x_new, s, y, theta, xc
5.7e-11 (xc of bounded-12), TOL64 = 1e-10; float32 model x_new 2.0e-7, s 5.6e-6, theta 6.3e-6, y 6.3e-5 at bounded-13, where the
reference's OWN float32-against-float64 gap is 7.1e-6 / 5.3e-6 / 6.3e-5 (y = g_new - g cancels as the steps shrink): figures above
TOL32 = 5e-6 are held to 4 x that gap (bounded-7, 8, 11, 12, 13), everything else to TOL32."""
import ctypes
import os

import numpy as np
import pytest

import lbfgsb_common as C
from lbfgsb_linesearch_cases import CASES
from prysm_amd import _lib as L
from prysm_amd.x import lbfgsb_plan as plan


def model_step(st, dtype):
    m = plan.LBFGSBModel(C.fg_numpy(dtype, C.A_of(st)), st['x'].astype(dtype), memory=C.MEMORY, **C.bounds_of(st, dtype))
    stopped = C.step_from(m, st)
    return m, stopped


def model_result(m):
    S, Y = m._history()
    core, P = m.core, m.passes
    bounded = core.has_bounds
    return dict(x_new=P.x, pair=(S[-1], Y[-1]) if len(S) else None, theta=m.theta, metadata=m.last_step_metadata, evals=P.evals,
                accepted=core.last_pair_accepted, xc=P.xc if bounded else None,
                c=core.last_cauchy['c'] if bounded else None, free=P.free if bounded else None)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('label,st', C.STATES, ids=C.STATE_IDS)
def test_model_against_every_fixture_step(label, st, dtype):
    m, stopped = model_step(st, dtype)
    if stopped is not None:
        C.compare_step(label, st, stopped, None, None, None, None, None, None, dtype)
        assert np.array_equal(m.x, st['x'].astype(dtype)) and m.last_step_metadata == {'reason': 'no_descent'}
        return
    C.compare_step(f'{label} {np.dtype(dtype).name} model-reference', st, None, dtype=dtype, **model_result(m))
    assert m.iter == 1 and m.nfev == 1


def test_model_covers_the_sweep_cases_of_the_fixture():
    """the bounded k = 0 state passes the first chunk of 64; the hand state exhausts its path in the second chunk"""
    st = dict(C.STATES)['bounded-0']
    m, _ = model_step(st, np.float64)
    assert m.core.last_cauchy['chunks'] >= 2 and int(st['zeros']) > 100
    st = dict(C.STATES)['hand-0-subset-box']
    m, _ = model_step(st, np.float64)
    assert m.core.last_cauchy['chunks'] == 2 and m.last_step_metadata['cauchy_breaks'] == 150 and 'bracket by increase' in m.core.last_branches


def test_model_runs_the_truncated_branch_and_the_refused_pair():
    """hand-3: BLNZ truncation, the search starts and ends at alpha_max < 1; hand-2: the pair is refused, the history stays empty, the
    refused pair sits in the free row, and the next step starts from the new x and overwrites that row"""
    st = dict(C.STATES)['hand-3-truncated']
    m, stopped = model_step(st, np.float64)
    md = m.last_step_metadata
    assert stopped is None and md['subspace_mode'] == 'truncated' and 0 < md['alpha'] < 1 and m.passes.evals == 1      # the first trial, AT the cap
    st = dict(C.STATES)['hand-2-refused-pair']
    m, stopped = model_step(st, np.float64)
    H, P = m.core.H, m.passes
    assert stopped is None and not m.core.last_pair_accepted and (H.k, H.slot, H.theta) == (0, 0, 1.0) and m.iter == 1
    assert np.array_equal(P.S[0], P.x - P.x_prev) and np.any(P.S[0]) and float(P.S[0].astype(np.float64) @ P.Y[0].astype(np.float64)) < 0
    x1, refused = P.x.copy(), P.S[0].copy()
    m.step()
    assert np.array_equal(P.x_prev, x1) and m.iter == 2 and H.slot in (0, 1)
    assert not np.array_equal(P.S[0], refused) and H.k == int(m.core.last_pair_accepted)      # the free row is rewritten either way


@pytest.mark.parametrize('name', list(CASES))
def test_line_search_against_the_reference(name):
    phi, maxalpha, c2, maxiter = CASES[name]
    seq, branches = [], []

    def logged(a):
        seq.append(a)
        return phi(a)
    f0, d0 = phi(0.0)
    alpha = plan.strong_wolfe(logged, f0, d0, maxalpha=maxalpha, c1=1e-4, c2=c2, maxiter=maxiter, branches=branches)[0]
    want, result = C.PROBLEM[f'ls_{name}_alphas'], float(C.PROBLEM[f'ls_{name}_result'])
    assert seq == list(want), (name, seq, want)
    assert (alpha is None and np.isnan(result)) or alpha == result, (name, alpha, result)
    assert alpha is None or alpha == seq[-1]      # the accepted alpha is the last one evaluated: the caller's gradient goes with it


def test_line_search_cases_reach_every_branch():
    seen = set()
    for phi, maxalpha, c2, maxiter in CASES.values():
        branches = []
        plan.strong_wolfe(phi, *phi(0.0), maxalpha=maxalpha, c1=1e-4, c2=c2, maxiter=maxiter, branches=branches)
        seen |= set(branches)
        for i, b in enumerate(branches[1:], 1):      # cubic rejected -> quadratic rejected -> bisection, past the zoom's first turn
            seen |= {'bisection after cubic'} if b == 'bisection' and branches[i - 1] in ('cubic', 'quadratic', 'bisection') else set()
    assert seen >= {'accepted', 'bracket by increase', 'bracket by slope', 'doubling', 'pinned', 'alpha1 == 0', 'cubic', 'quadratic', 'bisection',
                    'bisection after cubic', 'accepted in zoom', 'zoom exhausted', 'bracket exhausted'}, seen


def test_incremental_gram_update_through_a_wrapping_ring_and_a_refused_pair():
    rng = np.random.default_rng(5)
    n, m = 37, 4
    H = plan.History(m, np.float64)
    S, Y = [], []
    for it in range(3 * m + 1):
        s = rng.standard_normal(n)
        y = s * rng.uniform(0.5, 2.0, n)
        if it == 2 * m + 1:       # a pair the curvature test refuses: nothing may move
            y = -y
        Sa, Ya = np.array(S[-m:]).reshape(-1, n), np.array(Y[-m:]).reshape(-1, n)
        assert H.k == len(Sa)
        ss, sy, yy = s @ s, s @ y, y @ y
        before = (H.k, H.start, H.SS.copy(), H.SY.copy(), H.YY.copy(), H.theta)
        if H.curvature_ok(sy, yy):
            H.accept(Ya @ s, Sa @ s, Ya @ y, Sa @ y, ss, sy, yy)
            S.append(s), Y.append(y)
        else:
            assert it == 2 * m + 1
            assert (H.k, H.start, H.theta) == (before[0], before[1], before[5]) and all(np.array_equal(a, b) for a, b in zip(
                (H.SS, H.SY, H.YY), before[2:5]))
            continue
        Sa, Ya = np.array(S[-m:]), np.array(Y[-m:])
        k = len(Sa)
        for G, want in ((H.SS, Sa @ Sa.T), (H.SY, Sa @ Ya.T), (H.YY, Ya @ Ya.T)):
            assert np.max(np.abs(G[:k, :k] - want)) <= 1e-13 * np.max(np.abs(want))
        assert H.theta == yy / sy and H.slot not in H.rows() and len(set(H.rows())) == k
    assert len(S) == 3 * m and H.k == m and H.start != 0


def test_record_layouts_round_trip():
    """unpack_dots / unpack_gram against the layouts csrc/lbfgsb.hip documents"""
    k = 5
    raw = np.arange(2 * 19, dtype=np.float64)      # two tiles of the update's record
    prod, extra = plan.unpack_dots(raw, k, 2, 3)
    assert prod.shape == (10, 2) and prod[0, 1] == 1 and prod[8, 0] == 19 and list(extra) == [16, 17, 18]
    G = plan.unpack_gram(np.arange(3 * 64, dtype=np.float64), k)
    assert G.shape == (10, 10) and G[0, 1] == 1 and G[1, 0] == 8 and G[0, 8] == 64 and G[8, 0] == 64 and G[9, 9] == 128 + 9
    assert plan.gram_record_doubles(32) == 36 * 64 and plan.tiles_of(0) == 1 and plan.tiles_of(32) == 8


# ---------------------------------------------------------------------------------------------------------------- argument checks

P = ctypes.c_void_p(16)         # never dereferenced
ARG, UNSUP, WS = L.PM_ERR_ARG, L.PM_ERR_UNSUPPORTED, L.PM_ERR_WORKSPACE
BIG = 1 << 40


def _call(lib, name, dt=L.PM_F32, n=8, p=P, ld=8, ring=6, start=0, k=5, ws=BIG, mode=0, slot=5):
    hist = (dt, n, p, p, ld, ring, start, k)
    tail = (p, p, ws, None)
    if name == 'pm_lbfgsb_dots':
        return lib.pm_lbfgsb_dots(*hist, p, None, None, *tail)
    if name == 'pm_lbfgsb_breakpoints':
        return lib.pm_lbfgsb_breakpoints(*hist, p, p, p, p, p, p, *tail)
    if name == 'pm_lbfgsb_update':
        return lib.pm_lbfgsb_update(*hist, slot, p, p, p, 1.0, p, p, *tail)
    if name == 'pm_lbfgsb_gram':
        return lib.pm_lbfgsb_gram(*hist, None, *tail)
    if name == 'pm_lbfgsb_combine':
        return lib.pm_lbfgsb_combine(dt, mode, n, p, p, ld, ring, start, k, 1.0, p, 0.0, None, None, p, p, p, p, p, p, p, p, p, *tail)
    if name == 'pm_lbfgsb_cauchy_point':
        return lib.pm_lbfgsb_cauchy_point(dt, n, p, p, p, 0.0, 1.0, p, p, None)
    return lib.pm_lbfgsb_trial(dt, n, p, p, 1.0, None, None, p, None)


HIST = ['pm_lbfgsb_dots', 'pm_lbfgsb_breakpoints', 'pm_lbfgsb_update', 'pm_lbfgsb_gram', 'pm_lbfgsb_combine']
ALL = HIST + ['pm_lbfgsb_cauchy_point', 'pm_lbfgsb_trial']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _expect(lib, rc, name, want, word):
    msg = lib.pm_last_error().decode()
    assert rc == want and name in msg and word in msg, (name, rc, msg)


@pytest.mark.parametrize('name', ALL)
def test_entry_points_refuse_bad_arguments_before_any_launch(lib, name):
    for dt in (L.PM_C64, 99):
        _expect(lib, _call(lib, name, dt=dt), name, ARG, 'dtype')
    for n in (0, -3):
        _expect(lib, _call(lib, name, n=n), name, ARG, 'n must be at least 1')
    _expect(lib, _call(lib, name, p=None), name, ARG, 'null pointer')
    _expect(lib, _call(lib, name, dt=99, p=None), name, ARG, 'dtype')      # the dtype is looked at first


@pytest.mark.parametrize('name', HIST)
def test_entry_points_with_a_history_check_it(lib, name):
    _expect(lib, _call(lib, name, k=33, ring=34), name, UNSUP, 'PM_LBFGSB_MAX_MEMORY')
    _expect(lib, _call(lib, name, k=33, ring=34, p=None), name, UNSUP, 'PM_LBFGSB_MAX_MEMORY')      # the cap before the pointers
    _expect(lib, _call(lib, name, ld=7), name, ARG, 'row stride')
    _expect(lib, _call(lib, name, k=-1), name, ARG, 'k must not be negative')
    _expect(lib, _call(lib, name, ring=4), name, ARG, 'ring')
    _expect(lib, _call(lib, name, start=6), name, ARG, 'ring')
    if name != 'pm_lbfgsb_combine':      # the residual's combination leaves no sums and needs no workspace
        _expect(lib, _call(lib, name, ws=0), name, WS, 'workspace')


def test_entry_points_further_pins(lib):
    _expect(lib, _call(lib, 'pm_lbfgsb_update', slot=2), 'pm_lbfgsb_update', ARG, 'live row')
    _expect(lib, _call(lib, 'pm_lbfgsb_update', slot=6), 'pm_lbfgsb_update', ARG, 'outside the ring')
    _expect(lib, _call(lib, 'pm_lbfgsb_update', k=0, ld=7), 'pm_lbfgsb_update', ARG, 'row stride')
    _expect(lib, _call(lib, 'pm_lbfgsb_gram', k=0), 'pm_lbfgsb_gram', ARG, 'k must be at least 1')
    _expect(lib, _call(lib, 'pm_lbfgsb_combine', mode=7), 'pm_lbfgsb_combine', ARG, 'mode')
    _expect(lib, _call(lib, 'pm_lbfgsb_combine', ws=0), 'pm_lbfgsb_combine', WS, 'workspace')
    _expect(lib, lib.pm_lbfgsb_trial(L.PM_F32, 8, P, P, 1.0, P, None, P, None), 'pm_lbfgsb_trial', ARG, 'come together')
    small = lambda **kw: lib.pm_lbfgsb_small(*[{**dict(dt=L.PM_F64, op=0, m=5, k=3, np_=4, gp=0, st=P, c=P, coef=P, rec=P, part=P, gpart=None), **kw}[key]  # noqa: E731
                                               for key in ('dt', 'op', 'm', 'k', 'np_', 'gp', 'st', 'c', 'coef', 'rec', 'part', 'gpart')], None)
    for kw, rc, word in ((dict(dt=99), ARG, 'dtype'), (dict(op=9), ARG, 'op'), (dict(m=33, k=33), UNSUP, 'PM_LBFGSB_MAX_MEMORY'), (dict(k=6), ARG, 'memory'),
                         (dict(st=None), ARG, 'null pointer'), (dict(part=None), ARG, 'partials'), (dict(np_=2000), ARG, 'partials'),
                         (dict(gp=3), ARG, 'Gram'), (dict(op=2, c=None, part=None), ARG, 'null pointer: c'), (dict(coef=None), ARG, 'coef')):
        _expect(lib, small(**kw), 'pm_lbfgsb_small', rc, word)
    assert lib.pm_lbfgsb_state_doubles(5) == 83 and lib.pm_lbfgsb_state_doubles(33) == 0
    assert lib.pm_lbfgsb_workspace() == 8 * max(8 * 1024 * 19, 36 * 256 * 64, 1024 * 5)
    assert (L.PM_LBFGSB_MAX_MEMORY, L.PM_LBFGSB_TILE) == (plan.MAX_MEMORY, plan.TILE)


def test_memory_above_the_cap_is_refused_without_a_device():
    from prysm_amd.x.optym import PrysmLBFGSB
    with pytest.raises(NotImplementedError):
        PrysmLBFGSB(lambda x: (0.0, x), np.zeros(4), memory=plan.MAX_MEMORY + 1)
