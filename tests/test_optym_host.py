"""CPU: the optym model (prysm_amd/x/optym_plan.py, the numpy restatement of csrc/optym.hip) against the reference's results
(tests/golden/optym.npz and optym_<Optimizer>_<mode>.npz), the argument checks of the C entry points, the governors and runners on a
pure-Python optimizer, and the reference's error types; and the cases, references and bounds that tests/test_gpu_optym_kernels.py
holds the kernels to (tests/optym_common.py), on the model: the centred bias-and-gain-invariant cost against long double at pedestals
where the one-pass form it replaced fails, the coefficient override of the step, the edges of the activations and of the softmax."""
import ctypes
import os
import re

import numpy as np
import pytest

import optym_common as OC
from conftest import rel_max
from prysm_amd.x import optym_plan as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64, TOL32 = 1e-10, 5e-6      # the project's tolerances (tests/gpu_common.py)
NAMES = ('GradientDescent', 'AdaGrad', 'RMSProp', 'Adam', 'RAdam', 'AdaMomentum', 'Yogi')
MODES = ('free', 'bounded')
STEPS = 12
SYMBOLS = ('pm_optym_cost_workspace', 'pm_optym_cost', 'pm_optym_advance', 'pm_optym_step', 'pm_optym_activation', 'pm_optym_softmax',
           'pm_optym_softmax_backprop', 'pm_optym_spatial_gradient')
COSTS = (('mse', OP.COST_MSE, 'cost_I', 'cost_D'), ('bgi', OP.COST_BGI, 'cost_I', 'cost_D'), ('nll', OP.COST_NLL, 'cost_y', 'cost_yhat'),
         ('nlls', OP.COST_NLL, 'cost_y', 'cost_nll_scalar'))


@pytest.fixture(scope='module')
def g(golden):
    return golden('optym')


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as gr
        gr.build()
    return _lib.load()


def bounds_of(mode, n, dtype):
    if mode == 'free':
        return None, None
    return np.full(n, -0.4, dtype=dtype), np.full(n, 0.6, dtype=dtype)


def start_of(g, mode, dtype):
    x0 = g['opt_x0'].astype(dtype)
    lo, hi = bounds_of(mode, x0.size, dtype)
    return x0 if lo is None else np.minimum(np.maximum(x0, lo), hi)


def gradient(g, x):
    return g['opt_w'].astype(x.dtype) * (x - g['opt_t'].astype(x.dtype))


def test_cost_model_equals_the_reference(g):
    worst = 0.0
    for key, kind, a, b in COSTS:
        for tag, mask in (('', None), ('_masked', g['cost_mask'])):
            for dt, tol in ((np.float64, TOL64), (np.float32, TOL32)):
                D = g[b] if g[b].ndim else float(g[b])
                c, gr = OP.cost(kind, g[a].astype(dt), D, mask)
                assert c.dtype == dt and gr.dtype == dt and gr.shape == g[a].shape and c.shape == ()
                ec, eg = rel_max(c, g[f'cost_{key}{tag}_f']), rel_max(gr, g[f'cost_{key}{tag}_g'])
                assert ec <= tol and eg <= tol, (key, tag, dt, ec, eg)
                if mask is not None:
                    assert np.all(gr[~mask] == 0)
                if dt == np.float64:
                    worst = max(worst, ec, eg)
    assert worst <= TOL64


def test_cost_model_on_an_all_false_mask(g):
    for key, kind, a, b in COSTS:
        D = g[b] if g[b].ndim else float(g[b])
        c, gr = OP.cost(kind, g[a], D, np.zeros(g[a].shape, dtype=bool))
        assert np.isnan(c) and np.all(gr == 0)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', NAMES)
def test_step_model_follows_the_float64_trajectories(g, golden, name, mode):
    tr = golden(f'optym_{name}_{mode}')
    kind = NAMES.index(name)
    x = start_of(g, mode, np.float64)
    lo, hi = bounds_of(mode, x.size, np.float64)
    s1, s2 = np.zeros_like(x), np.zeros_like(x)
    for k in range(1, STEPS + 1):
        r = OP.step(kind, k, x, gradient(g, x), s1, s2, lo, hi, alpha=0.05)
        x, s1, s2 = r['x'], r['s1'], r['s2']
        assert rel_max(x, tr['x'][k - 1]) <= TOL64, (name, mode, k)
        for key, s in (('s1', s1), ('s2', s2)):
            if key in tr.files:
                assert rel_max(s, tr[key][k - 1]) <= TOL64, (name, mode, k, key)
        if mode == 'bounded':
            assert rel_max(r['g_step'], tr['gstep'][k - 1]) <= TOL64
            assert np.array_equal(r['active'], tr['active'][k - 1]) and int(r['active'].sum()) == int(tr['nbounded'][k - 1])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', NAMES)
def test_float32_step_model_against_single_float64_steps(g, golden, name, mode):
    """each of the 12 steps from the float32 rounding of the previous stored result (the generator's states)"""
    tr = golden(f'optym_{name}_{mode}')
    kind = NAMES.index(name)
    lo, hi = bounds_of(mode, g['opt_x0'].size, np.float32)
    x = start_of(g, mode, np.float32)
    s1, s2 = np.zeros_like(x), np.zeros_like(x)
    for k in range(1, STEPS + 1):
        r = OP.step(kind, k, x, gradient(g, x), s1, s2, lo, hi, alpha=0.05)
        assert r['x'].dtype == np.float32
        assert rel_max(r['x'], tr['nx'][k - 1]) <= TOL32, (name, mode, k)
        for key, s in (('ns1', r['s1']), ('ns2', r['s2'])):
            if key in tr.files:
                assert rel_max(s, tr[key][k - 1]) <= TOL32, (name, mode, k, key)
        x = tr['nx'][k - 1].astype(np.float32)
        s1 = tr['ns1'][k - 1].astype(np.float32) if 'ns1' in tr.files else s1
        s2 = tr['ns2'][k - 1].astype(np.float32) if 'ns2' in tr.files else s2


def test_radam_branch_is_crossed_inside_the_trajectory():
    flags = [OP.coefficients(OP.RADAM, k, 0.9, 0.999)[4] for k in range(1, STEPS + 1)]
    assert flags == [0.0] * 5 + [1.0] * 7
    rho = [OP.coefficients(OP.RADAM, k, 0.9, 0.999)[2] for k in (5, 6)]
    assert abs(rho[0] - 4.996) < 1e-3 and abs(rho[1] - 5.994) < 1e-3


def test_activation_model_equals_the_reference(g):
    x = g['act_x']
    for kind, name in enumerate(('Tanh', 'Arctan', 'Softplus', 'Sigmoid')):
        for back, key in ((False, 'f'), (True, 'b')):
            assert rel_max(OP.activation(kind, x, 1.7, 0.3, -0.2, backprop=back), g[f'act_{name}_{key}']) <= TOL64, (name, key)
            got32 = OP.activation(kind, x.astype(np.float32), 1.7, 0.3, -0.2, backprop=back)
            assert got32.dtype == np.float32 and rel_max(got32, g[f'act_{name}_{key}']) <= TOL32, (name, key)


def test_softmax_model_equals_the_reference(g):
    assert [OP.softmax_group(K) for K in (1, 2, 5, 64, 65, 100)] == [1, 2, 8, 64, 64, 64]
    for K in (2, 5, 64, 100):
        y = OP.softmax(g[f'sm_x_{K}'])
        assert rel_max(y, g[f'sm_f_{K}']) <= TOL64 and rel_max(OP.softmax_backprop(y, g[f'sm_g_{K}']), g[f'sm_b_{K}']) <= TOL64
    y = OP.softmax(g['gum_x'], g['gum_u'], 0.7, float(g['gum_eps']))
    assert rel_max(y, g['gum_f']) <= TOL64 and rel_max(OP.softmax_backprop(y, g['gum_g'], 0.7), g['gum_b']) <= TOL64
    # float32, every row by itself as well (a saturated row alone sets a small max|want|): forward from the float32 logits
    for K in (2, 5, 64, 100):
        x32, g32 = g[f'sm_x_{K}'].astype(np.float32), g[f'sm_g_{K}'].astype(np.float32)
        y32 = OP.softmax(x32)
        b32 = OP.softmax_backprop(y32, g32)
        assert y32.dtype == np.float32 and b32.dtype == np.float32
        for rows in (slice(0, 3), slice(0, 1), slice(1, 2), slice(2, 3)):
            assert rel_max(y32[rows], g[f'sm_f_{K}'][rows]) <= TOL32 and rel_max(b32[rows], g[f'sm_b_{K}'][rows]) <= TOL32, (K, rows)
    y32 = OP.softmax(g['gum_x'].astype(np.float32), g['gum_u'].astype(np.float32), 0.7, float(g['gum_eps']))
    assert rel_max(y32, g['gum_f']) <= TOL32 and rel_max(OP.softmax_backprop(y32, g['gum_g'].astype(np.float32), 0.7), g['gum_b']) <= TOL32
    # DiscreteEncoder over 5 levels: the contraction the package leaves to torch
    lv = np.arange(5)
    y = OP.softmax(g['enc_x'])
    assert rel_max((y * lv).sum(-1), g['enc_f']) <= TOL64
    assert rel_max(OP.softmax_backprop(y, g['enc_g'][:, None] * lv[None, :]), g['enc_b']) <= TOL64
    assert np.array_equal(lv[np.argmax(y, axis=-1)], g['enc_d'])


def test_spatial_gradient_model_equals_the_reference(g):
    rng = np.random.default_rng(5)
    for m, n in ((1, 1), (2, 2), (3, 3), (67, 130)):
        a = g[f'sg_{m}x{n}_in']
        for op, key in ((OP.FORWARD_X, 'fx'), (OP.ADJOINT_X, 'ax'), (OP.FORWARD_Y, 'fy'), (OP.ADJOINT_Y, 'ay')):
            assert np.array_equal(OP.spatial_gradient(op, a), g[f'sg_{m}x{n}_{key}']), (m, n, key)
        y = rng.standard_normal((m, n))
        for f, t in ((OP.FORWARD_X, OP.ADJOINT_X), (OP.FORWARD_Y, OP.ADJOINT_Y)):
            lhs, rhs = np.vdot(OP.spatial_gradient(f, a), y), np.vdot(a, OP.spatial_gradient(t, y))
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_the_model_imports_neither_oracle_nor_reference():
    src = open(os.path.join(ROOT, 'prysm_amd', 'x', 'optym_plan.py')).read()
    assert not re.search(r'^\s*(from|import)\s+(oracle|prysm|torch)\b', src, flags=re.M)


# ----------------------------------------------------------------------------- the C ABI without a device

def test_symbols_are_declared_exported_and_bound(lib):
    from prysm_amd import _lib as L
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'prysm_amd.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, header), s
        assert hasattr(lib, s) and s in L.SIGNATURES
        assert getattr(lib, s).argtypes == L.SIGNATURES[s][1]
    assert lib.pm_version() == 107
    assert lib.pm_optym_cost_workspace() == OP.cost_workspace_bytes() == 8 * (8 + 1024 * 6 + 1024)
    assert (L.PM_COST_MSE, L.PM_COST_BGI, L.PM_COST_NLL) == (OP.COST_MSE, OP.COST_BGI, OP.COST_NLL)
    assert (L.PM_OPT_GD, L.PM_OPT_ADAGRAD, L.PM_OPT_RMSPROP, L.PM_OPT_ADAM, L.PM_OPT_RADAM, L.PM_OPT_ADAMOMENTUM, L.PM_OPT_YOGI) == tuple(range(7))


def test_argument_errors_before_any_device_work(lib):
    from prysm_amd import _lib as L
    p = ctypes.c_void_p(16)
    ws = lib.pm_optym_cost_workspace()

    def cost(dt=L.PM_F32, kind=0, n=8, M=p, D=p, mask=None, c=p, gr=p, w=p, wsb=ws):
        return lib.pm_optym_cost(dt, kind, n, M, D, 0.5, mask, c, gr, w, wsb, None)

    def advance(kind=L.PM_OPT_ADAM, counter=p, coef=p):
        return lib.pm_optym_advance(kind, 0.9, 0.999, counter, coef, None)

    def step(dt=L.PM_F32, kind=L.PM_OPT_ADAM, n=8, x=p, gr=p, s1=p, s2=p, lo=None, hi=None, coef=p, xp=p, gs=None, act=None):
        return lib.pm_optym_step(dt, kind, n, x, gr, s1, s2, lo, hi, 0.05, 0.9, 0.999, 1e-7, coef, xp, gs, act, None)

    def activation(dt=L.PM_F32, kind=0, n=8, x=p, out=p):
        return lib.pm_optym_activation(dt, kind, 0, n, x, 1.0, 0.0, 0.0, out, None)

    def softmax(dt=L.PM_F32, rows=4, K=5, x=p, u=None, tau=1.0, out=p):
        return lib.pm_optym_softmax(dt, rows, K, x, u, tau, 0.0, out, None)

    def softmax_backprop(dt=L.PM_F32, rows=4, K=5, y=p, gr=p, tau=1.0, gin=p):
        return lib.pm_optym_softmax_backprop(dt, rows, K, y, gr, tau, gin, None)

    def spatial_gradient(dt=L.PM_F32, op=0, m=4, n=4, a=p, out=ctypes.c_void_p(1024)):
        return lib.pm_optym_spatial_gradient(dt, op, m, n, a, out, None)

    def refused(rc, word):
        assert rc == L.PM_ERR_ARG and word in lib.pm_last_error(), (rc, lib.pm_last_error())
        with pytest.raises(ValueError):
            L.check(rc)

    for fn in (cost, step, activation, softmax, softmax_backprop, spatial_gradient):
        for bad in (L.PM_C64, L.PM_C128, L.PM_BOOL, L.PM_U16, 99):
            refused(fn(dt=bad), b'dtype')
        assert ('pm_optym_' + fn.__name__).encode() in lib.pm_last_error()
    # null pointers
    for kw in (dict(M=None), dict(D=None), dict(c=None), dict(gr=None), dict(w=None)):
        refused(cost(**kw), b'null pointer')
    for kw in (dict(counter=None), dict(coef=None)):
        refused(advance(**kw), b'null pointer')
    for kw in (dict(x=None), dict(gr=None), dict(xp=None), dict(s1=None), dict(s2=None), dict(coef=None)):
        refused(step(**kw), b'null pointer')
    refused(step(lo=p), b'bounds')
    refused(step(hi=p), b'bounds')
    refused(step(lo=p, hi=p), b'null pointer')
    refused(step(lo=p, hi=p, gs=p), b'null pointer')
    refused(step(kind=L.PM_OPT_ADAGRAD, s1=None, s2=None), b'null pointer')
    for kw in (dict(x=None), dict(out=None)):
        refused(activation(**kw), b'null pointer')
        refused(softmax(**kw), b'null pointer')
    for kw in (dict(y=None), dict(gr=None), dict(gin=None)):
        refused(softmax_backprop(**kw), b'null pointer')
    for kw in (dict(a=None), dict(out=None)):
        refused(spatial_gradient(**kw), b'null pointer')
    refused(spatial_gradient(out=p), b'differ')
    # unknown kind codes
    refused(cost(kind=3), b'kind')
    refused(cost(kind=-1), b'kind')
    refused(advance(kind=7), b'kind')
    refused(step(kind=7), b'kind')
    refused(step(kind=-1), b'kind')
    refused(activation(kind=4), b'kind')
    refused(spatial_gradient(op=4), b'op')
    # sizes
    refused(cost(n=0), b'at least 1')
    refused(step(n=0), b'at least 1')
    refused(activation(n=0), b'at least 1')
    refused(softmax(rows=0), b'at least 1')
    refused(softmax(K=0), b'at least 1')
    refused(softmax_backprop(K=0), b'at least 1')
    refused(spatial_gradient(m=0), b'at least 1')
    refused(softmax(u=p, tau=0.0), b'tau')
    refused(softmax_backprop(tau=-1.0), b'tau')
    # the workspace
    assert cost(wsb=ws - 1) == L.PM_ERR_WORKSPACE and cost(wsb=0) == L.PM_ERR_WORKSPACE
    assert b'pm_optym_cost_workspace' in lib.pm_last_error()
    refused(cost(w=ctypes.c_void_p(12)), b'aligned')
    # a scalar target belongs to the likelihood alone
    refused(cost(kind=L.PM_COST_MSE, D=None), b'scalar')
    refused(cost(kind=L.PM_COST_BGI, D=None), b'scalar')


# ----------------------------------------------------------------------------- governors and runners: host logic

class Halving:
    """a pure-Python optimizer: f = x^2 / 2 on a list of floats, every step halves x"""

    def __init__(self, x0, stop_after=None):
        self.x = np.array(x0, dtype=float)
        self.nfev = 0
        self.stop_after = stop_after
        self.last_step_metadata = None

    def step(self):
        if self.stop_after is not None and self.nfev >= self.stop_after:
            raise StopIteration
        x = self.x
        f, g = 0.5 * float(x @ x), x.copy()
        self.nfev += 1
        self.x = x - 0.5 * g
        return x, f, g


def test_runN_and_run_until_on_a_python_optimizer():
    from prysm_amd.x import optym as O
    opt = Halving([8.0, -4.0])
    seen = list(O.runN(opt, 3))
    assert len(seen) == 3 and np.array_equal(seen[0][0], [8.0, -4.0]) and np.array_equal(opt.x, [1.0, -0.5]) and seen[1][1] == 10.0
    res = O.run_until(Halving([8.0, -4.0]), O.MaxIterations(4))
    assert isinstance(res, O.OptimizationResult) and res.nit == 4 and not res.success and res.message == 'maximum iterations reached'
    assert np.array_equal(res.x, [0.5, -0.25]) and res.nfev == 4 and res.njev is None and 'nit=4' in repr(res)
    assert [r.iteration for r in res.records] == [1, 2, 3, 4] and res.records[0].metadata == {} and isinstance(res.records[0].f, float)
    res = O.run_until(Halving([8.0]), O.Governor(), maxiter=3)
    assert res.nit == 3 and not res.success and res.decision.stop
    res = O.run_until(Halving([8.0]), O.Governor(), maxiter=0)
    assert res.nit == 0 and res.message == 'maximum iterations reached' and np.array_equal(res.x, [8.0])
    res = O.run_until(Halving([8.0], stop_after=2), O.Governor())
    assert res.nit == 2 and res.success and res.message == 'optimizer stopped'
    res = O.run_until(Halving([8.0]), O.GradientTolerance(0.3))
    assert res.success and res.message == 'gradient tolerance reached' and res.records[-1].g[0] == 0.25
    res = O.run_until(Halving([8.0]), O.StepTolerance(0.2, relative=False))
    assert res.success and res.message == 'step tolerance reached' and abs(res.records[-1].x_next[0] - res.records[-1].x[0]) <= 0.2
    res = O.run_until(Halving([8.0]), O.FunctionTolerance(1e-3))
    assert res.success and res.message == 'function tolerance reached' and res.nit > 2
    res = O.run_until(Halving([8.0]), O.MaxEvaluations(5))
    assert res.nit == 5 and res.message == 'maximum function evaluations reached'


def test_governors_compose_and_validate():
    from prysm_amd.x import optym as O

    def rec(i, f=1.0, g=(1.0,), x=(0.0,), xn=(1.0,), md=None, opt=None):
        return O.StepRecord(opt, i, np.array(x), f, np.array(g), np.array(xn), md)

    any_ = O.AnyGovernor([O.MaxIterations(3), O.GradientTolerance(0.5)])
    assert not any_.observe(rec(1)) and any_.observe(rec(3)).message == 'maximum iterations reached'
    assert any_.observe(rec(1, g=(0.1,))).success
    all_ = O.AllGovernor([O.MaxIterations(2), O.GradientTolerance(0.5)])
    assert not all_.observe(rec(1, g=(0.1,)))            # only the gradient has stopped
    dec = all_.observe(rec(2))                          # now both have, at least once
    assert dec.stop and not dec.success and dec.message == 'maximum iterations reached; gradient tolerance reached'
    assert not O.AllGovernor([]).observe(rec(1))
    ft = O.FunctionTolerance(0.1, relative=False)
    assert not ft.observe(rec(1, f=5.0)) and not ft.observe(rec(2, f=4.0)) and ft.observe(rec(3, f=3.95)).success
    assert O.FunctionTolerance(0.1).observe(rec(1, f=5.0, md={'f_next': 4.9})).success      # f_next: the first record compares
    ct = O.ConstraintTolerance(1e-3)
    assert not ct.observe(rec(1)) and ct.observe(rec(1, md={'constraint_violation': 1e-4})).success

    class WithViolation:
        constraint_violation = 0.0
    assert ct.observe(rec(1, opt=WithViolation())).success
    assert O.GradientTolerance(1.5, norm=2).observe(rec(1, g=(1.0, 1.0))).success and not O.GradientTolerance(1.0, norm='inf').observe(rec(1, g=(1.0, 1.5)))
    assert O.StepTolerance(1e-3).observe(rec(1, x=(2.0,), xn=(2.001,))).success       # relative: 1e-3 * max(1, 2)
    for make in (lambda: O.MaxIterations(-1), lambda: O.MaxEvaluations(-1), lambda: O.FunctionTolerance(-1.0), lambda: O.GradientTolerance(-1.0),
                 lambda: O.StepTolerance(-1.0), lambda: O.ConstraintTolerance(-1.0)):
        with pytest.raises(ValueError):
            make()
    d = O.GovernorDecision(True, False, 'x')
    assert bool(d) and not O.GovernorDecision()


def test_the_references_error_types():
    from prysm_amd.x import optym as O
    with pytest.raises(TypeError):
        O.as_problem(3)
    assert O.as_problem(len).fg([1, 2]) == 2

    class P:
        def fg(self, x):
            return 0.0, x
    p = P()
    assert O.as_problem(p) is p
    a32, a64 = np.ones((3, 3), dtype=np.float32), np.ones((3, 3))
    for cost in (O.mean_square_error, O.bias_and_gain_invariant_error, O.negative_loglikelihood):
        with pytest.raises(TypeError):
            cost(a32, a64)
        with pytest.raises(TypeError):
            cost(a64, a32, mask=np.ones((3, 3), dtype=bool))
    x0 = np.zeros(5)
    for cls in (O.GradientDescent, O.AdaGrad, O.RMSProp, O.Adam, O.RAdam, O.AdaMomentum, O.Yogi):
        with pytest.raises(TypeError):
            cls(3, x0, 0.1)
        with pytest.raises(ValueError):
            cls(len, x0, 0.1, lower_bounds=np.zeros(4))
        with pytest.raises(ValueError):
            cls(len, x0, 0.1, lower_bounds=np.ones(5), upper_bounds=np.zeros(5))
    with pytest.raises(AssertionError):
        O.Softmax().forward(np.ones(4))
    with pytest.raises(AssertionError):
        O.Softmax().backprop(np.ones((2, 2)))
    with pytest.raises(AssertionError):
        O.GumbelSoftmax().forward(np.ones(4))
    for fn in ('forward_x', 'adjoint_x', 'forward_y', 'adjoint_y'):
        with pytest.raises(AssertionError):
            getattr(O.SpatialGradient2D(), fn)(np.ones(4))
    assert O.GumbelSoftmax().eps == np.finfo(np.float64).eps and O.GumbelSoftmax(tau=0.5, eps=1e-3).eps == 1e-3
    assert np.array_equal(O.DiscreteEncoder(O.Softmax(), 4).levels, np.arange(4))
    t = O.Tanh(2, 1, 3)
    assert (t.a, t.x0, t.y0) == (2, 1, 3) and (O.Sigmoid().a, O.Sigmoid().x0, O.Sigmoid().y0) == (1, 0, 0)


# ----------------------------------------------------------------------------- the cases and bounds of tests/test_gpu_optym_kernels.py

def one_pass_bgi(I, D, keep=None):  # noqa: E741
    """the cost model as it was before the sums were centred: sum(I D) - sum(I) Dmean and sum(I I) - sum(I) Imean in float64"""
    keep = np.ones(I.shape, bool) if keep is None else keep
    m, d = I[keep].astype(np.float64), D[keep].astype(np.float64)
    N = np.float64(m.size)
    sI, sD, sID, sII, sDD = m.sum(), d.sum(), (m * d).sum(), (m * m).sum(), (d * d).sum()
    alpha = (sID - sI * (sD / N)) / (sII - sI * (sI / N))
    beta = sD / N - alpha * (sI / N)
    raw = (alpha * m + beta) - d
    g = np.zeros(I.shape)
    g[keep] = 2.0 * (1.0 / sDD) * alpha * raw
    return np.asarray((1.0 / sDD) * (raw * raw).sum()).astype(I.dtype), g.astype(I.dtype)


@pytest.mark.parametrize('n', OC.COST_SIZES)
def test_centred_cost_model_meets_the_pedestal_bounds_and_the_one_pass_form_does_not(n):
    failed_before = set()
    for dt in OC.DTYPES:
        name = np.dtype(dt).name
        for ped in OC.PEDESTALS:
            I, D, mask = OC.bgi_inputs(ped, n, name)  # noqa: E741
            for masked in (False, True):
                keep = mask if masked else None
                ref = OC.bgi_case(ped, n, name, masked)
                bg, bc = OC.bgi_bounds(ref, ped, dt)
                eg, ec = OC.bgi_errors(*OP.cost(OP.COST_BGI, I, D, keep), ref)
                og, oc = OC.bgi_errors(*one_pass_bgi(I, D, keep), ref)
                print(f'bgi model {name} n={n} pedestal {ped:g} masked={masked}: gradient {eg:.2e} (one-pass {og:.2e}) bound {bg:.2e}, '
                      f'cost {ec:.2e} (one-pass {oc:.2e}) bound {bc:.2e}')
                assert eg <= bg and ec <= bc, (name, ped, masked, eg, bg, ec, bc)
                if og > bg:
                    failed_before.add((name, ped))
            if keep is not None:        # what the mask drops leaves no trace, whatever it holds
                In, Dn = I.copy(), D.copy()
                In[~mask], Dn[~mask] = np.nan, np.inf
                c, g = OP.cost(OP.COST_BGI, In, Dn, mask)
                c0, g0 = OP.cost(OP.COST_BGI, I, D, mask)
                assert OC.same_bits(c, c0) and OC.same_bits(g, g0)
    assert failed_before >= {('float64', 1e2), ('float64', 1e4), ('float32', 1e4)}, failed_before


def test_integer_costs_are_exact_in_the_model():
    for dt in OC.DTYPES:
        I, D, mask = OC.integer_case(np.dtype(dt).name)  # noqa: E741
        assert np.array_equal(I, np.round(I)) and np.abs(I).max() <= 8 and np.abs(D).max() <= 8
        for keep in (None, mask):
            wc, wg = OC.mse_reference(I, D, keep)
            c, g = OP.cost(OP.COST_MSE, I, D, keep)
            # the sum is exact; 1 / N, the product with it and the rounding to the dtype are the model's only roundings
            assert abs(OC.LD(c) - wc) <= (2 * OC.EPS64 + OC.eps_of(dt)) * wc
            assert np.abs(g.astype(OC.LD) - wg).max() <= (2 * OC.EPS64 + OC.eps_of(dt)) * np.abs(wg).max()
        ref = OC.bgi_reference(I, D)
        c, g = OP.cost(OP.COST_BGI, I, D)
        # the means are 0 and 1, the centred sums integers: alpha and beta are one division and one product from exact numbers
        assert abs(float(np.float64(ref['alpha']))) > 1 and np.abs(g.astype(OC.LD) - ref['grad']).max() <= 8 * OC.eps_of(dt) * np.abs(ref['grad']).max()
        assert abs(OC.LD(c) - ref['cost']) <= (OC.INTEGER_COST_BOUND + OC.eps_of(dt)) * ref['cost']


def test_step_model_with_given_coefficients_equals_the_default_path():
    for dt in OC.DTYPES:
        case = OC.step_case(257, np.dtype(dt).name)
        for kind in range(7):
            x, s1, s2 = case['x'].copy(), np.zeros(257, dt), np.zeros(257, dt)
            for k in range(1, 8):
                g = OC.step_gradient(case, x, k)
                a = OP.step(kind, k, x, g, s1, s2, case['lower'], case['upper'], alpha=0.05, beta1=0.5, beta2=0.9)
                b = OP.step(kind, k, x, g, s1, s2, case['lower'], case['upper'], alpha=0.05, beta1=0.5, beta2=0.9,
                            coef=OP.coefficients(kind, k, 0.5, 0.9))
                for key in OC.STEP_OUTPUTS:
                    if a[key] is not None:
                        assert OC.same_bits(np.asarray(a[key]), np.asarray(b[key])), (kind, k, key)
                # a NaN x and a NaN gradient stay where they are and go nowhere else
                nan = np.isnan(a['x'])
                assert nan[case['nan_x']] and (kind != OP.GD or nan[case['nan_g']]) and nan.sum() <= 2
                assert set(np.unique(a['active'])) <= {False, True}
                x, s1, s2 = a['x'], a['s1'] if a['s1'] is not None else s1, a['s2'] if a['s2'] is not None else s2
        # a wrong coefficient is used: the override is not ignored
        co = OP.coefficients(OP.ADAM, 3, 0.9, 0.999)
        co[0] *= 2
        g = OC.step_gradient(case, case['x'], 1)
        z = np.zeros(257, dt)
        assert not OC.same_bits(OP.step(OP.ADAM, 3, case['x'], g, z, z, coef=co)['x'], OP.step(OP.ADAM, 3, case['x'], g, z, z)['x'])


def test_step_cases_hold_what_they_promise():
    for n in OC.STEP_SIZES:
        case = OC.step_case(n, 'float32')
        lo, hi, x = case['lower'], case['upper'], case['x']
        assert np.all(np.isneginf(lo) | np.isfinite(lo)) and np.all(np.isposinf(hi) | np.isfinite(hi))
        if n >= 255:
            combos = {(bool(np.isfinite(a)), bool(np.isfinite(b))) for a, b in zip(lo, hi)}
            assert len(combos) == 4 and (x == lo).sum() >= 8 and (x == hi).sum() >= 8
            gs = [OC.step_gradient(case, x, k) for k in range(1, 5)]
            for on in (x == lo, x == hi):
                seen = {s for g in gs for s in np.sign(g[on]).tolist()}
                assert seen >= {1.0, -1.0, 0.0}
            assert np.isnan(x).sum() == 1 and all(np.isnan(g).sum() == 2 for g in gs)       # the gradient's own NaN and the one x hands on
            a, b = case['inf_lo'], case['inf_hi']
            assert x[a] == -np.inf and lo[a] == -np.inf and x[b] == np.inf and hi[b] == np.inf and all(g[a] > 0 and g[b] < 0 for g in gs)
            # there the reference's np.isfinite decides: the gradient passes and the bound is not active
            r = OP.step(OP.ADAM, 1, x, gs[0], np.zeros_like(x), np.zeros_like(x), lo, hi)
            assert r['g_step'][a] == gs[0][a] and r['g_step'][b] == gs[0][b] and not r['active'][a] and not r['active'][b]


def test_coefficient_model_against_long_double():
    for b1, b2 in OC.BETAS:
        flags = []
        for k in OC.ADVANCE_KS:
            got = OP.coefficients(OP.RADAM, k, b1, b2)
            want = OC.coefficients_reference(OP.RADAM, k, b1, b2)
            for i, bound in OC.coefficient_bounds(want, k, b2).items():
                assert abs(OC.LD(got[i]) - want[i]) <= bound, (b1, b2, k, i)
            assert got[4] == want[4]
            flags.append(want[4])
        assert flags[0] == 0.0 and flags[-1] == 1.0 and flags == sorted(flags)


def test_activation_model_at_the_edges():
    for dt in OC.DTYPES:
        for a, x0, y0 in OC.ACT_PARAMS:
            for n in OC.ACT_SIZES:
                x = OC.activation_input(n, np.dtype(dt).name, a, x0)
                if n > 1:
                    with np.errstate(invalid='ignore'):
                        arg = a * (x.astype(np.float64) - x0)
                    assert np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2 and (x == 0).sum() >= 2 and np.signbit(x[1]) and not np.signbit(x[0])
                    assert all(np.any(np.abs(arg - v) < 1e-3 * abs(v)) for v in (100, -100, 1000, -1000))
                    assert ((x != 0) & (np.abs(x) < np.finfo(dt).tiny)).sum() == 4
                for kind in range(4):
                    for back in (False, True):
                        with np.errstate(all='ignore'):
                            model = OP.activation(kind, x, a, x0, y0, backprop=back)
                        want = OC.activation_reference(kind, x, a, x0, y0, back)
                        assert model.dtype == dt and np.array_equal(np.isnan(model), np.isnan(want))
                        # the model overflows where the dtype does (softplus of 1000 is inf, in float32 of 100 too): never where it is finite
                        fin = np.isfinite(model)
                        assert np.isfinite(want[fin]).all()
                        err = np.abs(model[fin].astype(OC.LD) - want[fin]) / np.maximum(1, np.abs(want[fin]))
                        assert err.max(initial=0) <= 8 * OC.eps_of(dt), (dt, a, n, kind, back, float(err.max()))


def test_softmax_model_and_inputs_at_the_edges():
    smallest = np.inf
    for dt in OC.DTYPES:
        name = np.dtype(dt).name
        for K in OC.SOFTMAX_K:
            rows = OC.softmax_rows(K)
            assert rows[0] == 1 and rows[-1] == 3 * (256 // OP.softmax_group(K)) + 1
            for r in rows:
                x, g = OC.softmax_input(K, r, name)
                want = OC.softmax_reference(x)
                smallest = min(smallest, float(want.min()))
                y = OP.softmax(x)
                # every entry counts: none is excluded, none is sub-normal even in float32
                assert (want > OC.TINY32).all() and np.isfinite(want).all()
                assert OC.softmax_ratio(y, x, want) <= 1 and OC.row_sum_ratio(y) <= 1, (name, K, r)
                if r > 1 and K > 1:          # K = 1 is 1.0 whatever is read
                    assert not np.array_equal(y[0], y[1])
                back = OP.softmax_backprop(y, g)
                assert OC.softmax_backprop_ratio(back, y, g, OC.softmax_backprop_reference(y, g, 1.0), 1.0) <= 1, (name, K, r)
        for K in OC.SPECIAL_K:
            x, g = OC.special_rows(K, name)
            with np.errstate(invalid='ignore'):
                y = OP.softmax(x)
            want = OC.softmax_reference(x)
            row = dict(zip(OC.SPECIAL_ROWS, y))
            assert np.all(row['equal'] == dt(1) / dt(K)) or K & (K - 1)
            assert np.allclose(row['equal'], 1 / K)
            assert row['saturated'][K // 2] == 1 or dt == np.float64
            assert np.array_equal(row['some -inf'] == 0, np.isneginf(x[2])) and np.isnan(row['all -inf']).all()
            assert set(np.unique(row['+-1e4'])) == {0, dt(1) / dt((K + 1) // 2)}
            assert np.array_equal(np.isnan(y), np.isnan(want)) and OC.softmax_ratio(y, x, want) <= 1
            back = OP.softmax_backprop(y, g)
            ratio = OC.softmax_backprop_ratio(back, y, g, OC.softmax_backprop_reference(y, g, 1.0), 1.0)
            assert ratio <= 1 and np.all(back[y == 0] == 0) and np.isnan(back[3]).all()
            # the reference's own expression cancels on the saturated row: the bound tells the two forms apart
            naive = OC.softmax_backprop_ratio(OC.softmax_backprop_naive(y[1:2], g[1:2], 1.0), y[1:2], g[1:2],
                                              OC.softmax_backprop_reference(y[1:2], g[1:2], 1.0), 1.0)
            print(f'softmax backprop model {name} K={K}: ratio {ratio:.2e}, the reference\'s expression on the saturated row {naive:.2e}')
            assert naive > 1 or dt == np.float64       # it misses the bound the kernel's form meets
        for K in OC.GUMBEL_K:
            x, u, g, eps = OC.gumbel_input(K, name)
            assert (u == 0).any(axis=1).all() and (u == np.nextafter(dt(1), dt(0))).any(axis=1).all() and (u < 1).all() and eps > 0
            for tau in OC.GUMBEL_TAU:
                y = OP.softmax(x, u, tau, eps)
                extra, logits = OC.gumbel_extra(x, u, tau, eps)
                assert np.isfinite(logits).all() and np.isfinite(y).all()
                assert OC.softmax_ratio(y, logits, OC.softmax_reference(logits), extra) <= 1
    assert smallest > OC.TINY32
    print(f'softmax inputs: the smallest probability of any case is {smallest:.2e} (float32 tiny {OC.TINY32:.2e})')
