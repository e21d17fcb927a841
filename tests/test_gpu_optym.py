"""GPU: prysm_amd.x.optym (csrc/optym.hip) against the reference's results (tests/golden/optym.npz, optym_<Optimizer>_<mode>.npz),
rel_max at the project's tolerances.  Every test prints the figures it asserts on.  No test provokes a fault: bad values are data,
never addresses."""
import numpy as np
import pytest
import torch

from conftest import rel_max
from gpu_common import TOL32, TOL64
from prysm_amd.x import optym_plan as OP

pytestmark = pytest.mark.gpu

NAMES = ('GradientDescent', 'AdaGrad', 'RMSProp', 'Adam', 'RAdam', 'AdaMomentum', 'Yogi')
MODES = ('free', 'bounded')
STEPS = 12
DTYPES = ((np.float32, TOL32), (np.float64, TOL64))
COSTS = (('mse', 'mean_square_error', 'cost_I', 'cost_D'), ('bgi', 'bias_and_gain_invariant_error', 'cost_I', 'cost_D'),
         ('nll', 'negative_loglikelihood', 'cost_y', 'cost_yhat'), ('nlls', 'negative_loglikelihood', 'cost_y', 'cost_nll_scalar'))


@pytest.fixture(scope='module')
def g(golden):
    return golden('optym')


@pytest.fixture(scope='module')
def O(pa):
    from prysm_amd.x import optym
    return optym


def tonp(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def report(what, value):
    print(f'optym rel_max {what}: {value:.3e}')
    return value


def err(got, want):
    """rel_max over the finite entries; the NaN entries must coincide"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    keep = ~np.isnan(want)
    return rel_max(got[keep], want[keep]) if keep.any() else 0.0


# the reference's formulas in float64 numpy, for the shapes the fixture does not hold
def np_mse(M, D):
    diff = M - D
    return (diff * diff).sum() / diff.size, 2 * diff / diff.size


def np_bgi(I, D):  # noqa: E741
    with np.errstate(all='ignore'):
        Ihat, Dhat = I - I.mean(), D - D.mean()
        alpha = (Ihat * Dhat).sum() / (Ihat * Ihat).sum()
        beta = D.mean() - alpha * I.mean()
        R = 1 / (D * D).sum()
        raw = (alpha * I + beta) - D
        return R * (raw * raw).sum(), 2 * R * alpha * raw


def np_nll(y, yhat):
    return -(yhat * np.log(y) + (1 - yhat) * np.log(1 - y)).sum() / y.size, ((-yhat / y) + ((1 - yhat) / (1 - y))) / y.size


NP_COSTS = (('mean_square_error', np_mse), ('bias_and_gain_invariant_error', np_bgi), ('negative_loglikelihood', np_nll))


def np_masked(fn, a, b, mask):
    if mask is None:
        return fn(a, b)
    c, gk = fn(a[mask], b[mask])
    grad = np.zeros_like(a)
    grad[mask] = gk
    return c, grad


# ----------------------------------------------------------------------------- costs

@pytest.mark.parametrize('dt,tol', DTYPES)
def test_costs_of_the_fixture(O, g, dt, tol):
    for key, fn, a, b in COSTS:
        for tag, mask in (('', None), ('_masked', g['cost_mask'])):
            D = dev(g[b].astype(dt)) if g[b].ndim else float(g[b])
            c, grad = getattr(O, fn)(dev(g[a].astype(dt)), D, mask=None if mask is None else dev(mask))
            assert c.is_cuda and c.shape == () and grad.shape == g[a].shape and tonp(c).dtype == dt and tonp(grad).dtype == dt
            ec = report(f'cost {key}{tag} {np.dtype(dt).name} f', rel_max(tonp(c), g[f'cost_{key}{tag}_f']))
            eg = report(f'cost {key}{tag} {np.dtype(dt).name} g', rel_max(tonp(grad), g[f'cost_{key}{tag}_g']))
            assert ec <= tol and eg <= tol, (key, tag, ec, eg)
            if mask is not None:
                assert np.all(tonp(grad)[~mask] == 0)
    # numpy arrays, a numpy mask and an integer mask go in as they are
    c, grad = O.mean_square_error(g['cost_I'], g['cost_D'], mask=g['cost_mask'].astype(np.int32))
    assert rel_max(tonp(c), g['cost_mse_masked_f']) <= TOL64 and rel_max(tonp(grad), g['cost_mse_masked_g']) <= TOL64


@pytest.mark.parametrize('n', [1, 63, 64, 65])
def test_costs_of_short_flat_arrays(O, n):
    rng = np.random.default_rng(100 + n)
    I = rng.uniform(0.1, 1.0, n).astype(np.float32).astype(np.float64)  # noqa: E741
    D = (1.7 * I + 0.3 + 0.05 * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
    yhat = (rng.random(n) > 0.5).astype(np.float64)
    mask = np.ones(n, dtype=bool) if n == 1 else rng.random(n) < 0.7
    mask[0] = True
    for dt, tol in DTYPES:
        for name, fn in NP_COSTS:
            b = yhat if fn is np_nll else D
            for m in (None, mask):
                wc, wg = np_masked(fn, I, b, m)
                c, grad = getattr(O, name)(dev(I.astype(dt)), dev(b.astype(dt)), mask=None if m is None else dev(m))
                ec, eg = err(tonp(c), wc), err(tonp(grad), wg)
                report(f'cost n={n} {name} {np.dtype(dt).name}', max(ec, eg))
                assert ec <= tol and eg <= tol, (n, name, dt, ec, eg)


def test_costs_where_every_workgroup_loops_and_ends_ragged(O):
    """from the implementation's constants: every first-stage workgroup strides at least twice, some a third time, and the last
    stride ends inside a workgroup"""
    stride = OP.COST_THREADS * OP.COST_WGS
    n = 2 * stride + 100003
    assert n // stride >= 2 and (n % stride) % OP.COST_THREADS != 0 and n % stride > OP.COST_THREADS
    rng = np.random.default_rng(11)
    I = rng.uniform(0.1, 1.0, n).astype(np.float32).astype(np.float64)  # noqa: E741
    D = (1.7 * I + 0.3 + 0.05 * rng.standard_normal(n)).astype(np.float32).astype(np.float64)
    yhat = (rng.random(n) > 0.5).astype(np.float64)
    mask = rng.random(n) < 0.7
    for dt, tol in DTYPES:
        for name, fn in NP_COSTS:
            b = yhat if fn is np_nll else D
            wc, wg = np_masked(fn, I, b, mask)
            c, grad = getattr(O, name)(dev(I.astype(dt)), dev(b.astype(dt)), mask=dev(mask))
            ec, eg = rel_max(tonp(c), wc), rel_max(tonp(grad), wg)
            report(f'cost n={n} {name} {np.dtype(dt).name}', max(ec, eg))
            assert ec <= tol and eg <= tol, (name, dt, ec, eg)


def test_an_all_false_mask_gives_nan_and_a_zero_gradient(O, g):
    none = dev(np.zeros(g['cost_I'].shape, dtype=bool))
    for dt, _ in DTYPES:
        for key, fn, a, b in COSTS:
            D = dev(g[b].astype(dt)) if g[b].ndim else float(g[b])
            c, grad = getattr(O, fn)(dev(g[a].astype(dt)), D, mask=none)
            assert np.isnan(tonp(c)) and np.all(tonp(grad) == 0), (key, dt)


def test_costs_are_bit_reproducible(O):
    rng = np.random.default_rng(3)
    n = OP.COST_THREADS * OP.COST_WGS + 12345
    a, b = (dev((0.05 + 0.9 * rng.random(n)).astype(np.float32)) for _ in range(2))      # inside (0, 1): the likelihood takes logs
    mask = dev(rng.random(n) < 0.7)
    for fn in (O.mean_square_error, O.bias_and_gain_invariant_error, O.negative_loglikelihood):
        c1, g1 = fn(a, b, mask=mask)
        c1, g1 = c1.clone(), g1.clone()
        c2, g2 = fn(a, b, mask=mask)
        assert torch.isfinite(c1) and torch.equal(c1, c2) and torch.equal(g1, g2)


# ----------------------------------------------------------------------------- optimizers

def quadratic(g, dt):
    t, w = dev(g['opt_t'].astype(dt)), dev(g['opt_w'].astype(dt))

    def fg(x):
        d = x - t
        return 0.5 * torch.sum(w * d * d), w * d
    return fg


def bounds_kw(mode, n, dt):
    return {} if mode == 'free' else dict(lower_bounds=np.full(n, -0.4, dtype=dt), upper_bounds=np.full(n, 0.6, dtype=dt))


def state_of(opt):
    if hasattr(opt, 'accumulator'):
        return [opt.accumulator]
    if hasattr(opt, 'm'):
        return [opt.m, opt.v]
    return []


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', NAMES)
def test_float64_trajectories(O, g, golden, name, mode):
    tr = golden(f'optym_{name}_{mode}')
    n = g['opt_x0'].size
    opt = getattr(O, name)(quadratic(g, np.float64), g['opt_x0'], 0.05, **bounds_kw(mode, n, np.float64))
    worst = 0.0
    before = tonp(opt.x)
    for k in range(STEPS):
        xp, f, grad = opt.step()
        assert xp is opt.x_prev and np.array_equal(tonp(xp), before) and f.shape == ()
        before = tonp(opt.x)
        worst = max(worst, rel_max(before, tr['x'][k]))
        for key, s in zip(('s1', 's2'), state_of(opt)):
            worst = max(worst, rel_max(tonp(s), tr[key][k]))
        md = opt.last_step_metadata
        if mode == 'bounded':
            worst = max(worst, rel_max(tonp(md['projected_gradient']), tr['gstep'][k]))
            assert np.array_equal(tonp(md['active_bounds']), tr['active'][k]) and md['bounded_variables'] == int(tr['nbounded'][k])
            assert isinstance(md['bounded_variables'], int) and 'bounded_variables' in md
        else:
            assert md == {}
    report(f'optimizer {name} {mode} float64', worst)
    assert worst <= TOL64 and opt.iter == STEPS and int(opt.counter.item()) == STEPS
    assert [s in tr.files for s in ('s1', 's2')] == [len(state_of(opt)) >= 1, len(state_of(opt)) >= 2]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', NAMES)
def test_float32_single_steps(O, g, golden, name, mode):
    """each of the 12 steps from the stored state: the float32 rounding of the previous stored result"""
    tr = golden(f'optym_{name}_{mode}')
    n = g['opt_x0'].size
    opt = getattr(O, name)(quadratic(g, np.float32), g['opt_x0'].astype(np.float32), 0.05, **bounds_kw(mode, n, np.float32))
    assert opt.eps == float(np.finfo(np.float32).eps)
    worst = 0.0
    for k in range(STEPS):
        if k:
            opt.x.copy_(dev(tr['nx'][k - 1].astype(np.float32)))
            for key, s in zip(('ns1', 'ns2'), state_of(opt)):
                s.copy_(dev(tr[key][k - 1].astype(np.float32)))
        assert int(opt.counter.item()) == k
        opt.step()
        assert opt.x.dtype == torch.float32
        worst = max(worst, rel_max(tonp(opt.x), tr['nx'][k]))
        for key, s in zip(('ns1', 'ns2'), state_of(opt)):
            worst = max(worst, rel_max(tonp(s), tr[key][k]))
    report(f'optimizer {name} {mode} float32', worst)
    assert worst <= TOL32


@pytest.mark.parametrize('n', [1, 65])
def test_short_vectors_follow_the_model(O, n):
    rng = np.random.default_rng(n)
    t, w, x0 = rng.standard_normal(n), rng.uniform(0.5, 2.0, n), rng.standard_normal(n)
    td, wd = dev(t), dev(w)
    lo, hi = np.full(n, -0.4), np.full(n, 0.6)
    for kind, name in enumerate(NAMES):
        opt = getattr(O, name)(lambda x: (0.5 * torch.sum(wd * (x - td) ** 2), wd * (x - td)), x0, 0.05, lower_bounds=lo, upper_bounds=hi)
        x = np.minimum(np.maximum(x0, lo), hi)
        s1, s2 = np.zeros(n), np.zeros(n)
        for k in range(1, 8):
            r = OP.step(kind, k, x, w * (x - t), s1, s2, lo, hi, alpha=0.05)
            x, s1, s2 = r['x'], r['s1'], r['s2']
            opt.step()
            assert rel_max(tonp(opt.x), x) <= TOL64, (name, n, k)
            assert np.array_equal(tonp(opt.last_step_metadata['active_bounds']), r['active'])


def test_reset_restores_the_start_in_place(O, g):
    opt = O.Adam(quadratic(g, np.float64), g['opt_x0'], 0.05, lower_bounds=np.full(1027, -0.4), upper_bounds=np.full(1027, 0.6))
    start, where = tonp(opt.x), (opt.x.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), opt.counter.data_ptr())
    first = [tonp(opt.step()[0]) for _ in range(3)][-1]
    assert opt.reset() is opt
    assert np.array_equal(tonp(opt.x), start) and not tonp(opt.m).any() and not tonp(opt.v).any() and int(opt.counter.item()) == 0 and opt.iter == 0
    assert where == (opt.x.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), opt.counter.data_ptr()) and opt.last_step_metadata == {}
    again = [tonp(opt.step()[0]) for _ in range(3)][-1]
    assert np.array_equal(first, again)
    opt.reset(np.zeros(1027))
    assert not tonp(opt.x).any()


def test_a_captured_adam_iteration_replays_the_eager_steps(pa, O, g):
    """cost kernel, the quadratic's gradient in torch, step(): recorded once on one stream, reset, replayed twelve times"""
    from prysm_amd import graph
    t, w = dev(g['opt_t'].astype(np.float32)), dev(g['opt_w'].astype(np.float32))
    x0 = g['opt_x0'].astype(np.float32)
    half_n = 0.5 * t.numel()

    def fg(x):
        f, dM = O.mean_square_error(x, t)           # (x - t) 2 / N
        return f, w * (dM * half_n)

    eager = O.Adam(fg, x0, 0.05)
    for _ in range(STEPS):
        eager.step()
    opt = O.Adam(fg, x0, 0.05)
    model = graph.capture(lambda: opt.step()[1])
    opt.reset()
    assert int(opt.counter.item()) == 0
    for _ in range(STEPS):
        f = model()
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == STEPS and torch.equal(opt.x, eager.x) and torch.equal(opt.m, eager.m) and torch.equal(opt.v, eager.v)
    assert np.isfinite(float(f))


# ----------------------------------------------------------------------------- activations and operators

@pytest.mark.parametrize('dt,tol', DTYPES)
def test_affine_activations(O, g, dt, tol):
    x = dev(g['act_x'].astype(dt))
    for name in ('Tanh', 'Arctan', 'Softplus', 'Sigmoid'):
        node = getattr(O, name)(1.7, 0.3, -0.2)
        for key, got in (('f', node.forward(x)), ('b', node.backprop(x))):
            e = report(f'activation {name} {key} {np.dtype(dt).name}', rel_max(tonp(got), g[f'act_{name}_{key}']))
            assert tonp(got).dtype == dt and got.shape == x.shape and e <= tol, (name, key, e)


@pytest.mark.parametrize('rows', [1, 3, 1000])
@pytest.mark.parametrize('K', [2, 5, 64, 100])
def test_softmax_and_its_backprop(O, g, K, rows):
    def tiled(a):
        return np.tile(a, (rows // 3 + 1, 1))[:rows]
    x, gr, wf, wb = (tiled(g[f'sm_{k}_{K}']) for k in ('x', 'g', 'f', 'b'))
    for dt, tol in DTYPES:
        sm = O.Softmax()
        y = sm.forward(dev(x.astype(dt)))
        back = sm.backprop(dev(gr.astype(dt)))
        ef, eb = rel_max(tonp(y), wf), rel_max(tonp(back), wb)
        report(f'softmax K={K} rows={rows} {np.dtype(dt).name}', max(ef, eb))
        assert y.shape == x.shape and back.shape == x.shape and tonp(y).dtype == dt and tonp(back).dtype == dt
        assert ef <= tol and eb <= tol, (K, rows, dt, ef, eb)
    y3 = O.Softmax().forward(dev(x.reshape(1, rows, K)))       # leading axes are independent variables
    assert y3.shape == (1, rows, K) and rel_max(tonp(y3)[0], wf) <= TOL64


def test_gumbel_softmax_with_stored_variates(O, g):
    for dt, tol in DTYPES:
        node = O.GumbelSoftmax(tau=0.7, eps=float(g['gum_eps']))
        y = node.forward(dev(g['gum_x'].astype(dt)), u=dev(g['gum_u'].astype(dt)))
        back = node.backprop(dev(g['gum_g'].astype(dt)))
        ef, eb = rel_max(tonp(y), g['gum_f']), rel_max(tonp(back), g['gum_b'])
        report(f'gumbel {np.dtype(dt).name}', max(ef, eb))
        assert ef <= tol and eb <= tol, (dt, ef, eb)
    drawn = tonp(O.GumbelSoftmax(tau=0.7).forward(dev(g['gum_x'])))
    assert np.all(np.isfinite(drawn)) and np.allclose(drawn.sum(-1), 1.0) and not np.allclose(drawn, g['gum_f'])


def test_discrete_encoder(O, g):
    for dt, tol in DTYPES:
        enc = O.DiscreteEncoder(O.Softmax(), 5)
        f = enc.forward(dev(g['enc_x'].astype(dt)))
        b = enc.backprop(dev(g['enc_g'].astype(dt)))
        ef, eb = rel_max(tonp(f), g['enc_f']), rel_max(tonp(b), g['enc_b'])
        report(f'encoder {np.dtype(dt).name}', max(ef, eb))
        assert ef <= tol and eb <= tol, (dt, ef, eb)
        assert enc.tmpshape == g['enc_x'].shape
        assert np.array_equal(tonp(enc.discretize(dev(g['enc_x'].astype(dt)))), g['enc_d'])


@pytest.mark.parametrize('shape', [(1, 1), (2, 2), (3, 3), (67, 130)])
def test_spatial_gradient_and_its_adjoint(O, g, shape):
    m, n = shape
    a = g[f'sg_{m}x{n}_in']
    op = O.SpatialGradient2D()
    for dt in (np.float32, np.float64):
        for key in ('fx', 'ax', 'fy', 'ay'):
            fn = {'fx': op.forward_x, 'ax': op.adjoint_x, 'fy': op.forward_y, 'ay': op.adjoint_y}[key]
            got = tonp(fn(dev(a.astype(dt))))
            code = {'fx': OP.FORWARD_X, 'ax': OP.ADJOINT_X, 'fy': OP.FORWARD_Y, 'ay': OP.ADJOINT_Y}[key]
            assert got.dtype == dt and np.array_equal(got, OP.spatial_gradient(code, a.astype(dt))), (shape, key)      # one subtraction per element
            assert rel_max(got, g[f'sg_{m}x{n}_{key}']) <= (0.0 if dt == np.float64 else TOL32), (shape, key)
    # <forward(x), y> == <x, adjoint(y)> in float64.  Each side is a dot product of m n terms evaluated on the host: its rounding
    # error is at most (m n) eps sum |terms| (the classical bound for a sum of products), so the two sides differ by no more than the
    # sum of their bounds; the kernels' own differences add one rounding per term, which the factor 2 covers
    rng = np.random.default_rng(m * 1000 + n)
    x, y = rng.standard_normal(shape), rng.standard_normal(shape)
    eps = np.finfo(np.float64).eps
    for fwd, adj in ((op.forward_x, op.adjoint_x), (op.forward_y, op.adjoint_y)):
        Fx, Fty = tonp(fwd(dev(x))), tonp(adj(dev(y)))
        lhs, rhs = np.vdot(Fx, y), np.vdot(x, Fty)
        bound = 2 * m * n * eps * (np.abs(Fx * y).sum() + np.abs(x * Fty).sum())
        print(f'optym dot test {shape}: {lhs!r} {rhs!r} bound {bound:.3e}')
        assert abs(lhs - rhs) <= bound
