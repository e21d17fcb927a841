"""GPU: the optym kernels (csrc/optym.hip) at the C ABI against the reference's formulas in long double, at the sizes, values and edges
where they can go wrong.  Cases, references, bounds, guard bands and the call helpers are tests/optym_common.py's; tests/test_optym_host.py
holds the numpy model to the same cases on the CPU.  Every comparison prints what it measured beside its bound (as a ratio: 1 is the
bound), and test_recorded_figures prints the worst ratio of every group.  No test provokes a fault: bad values are data, never
addresses, and what a kernel writes past its n elements lands in the band of its own buffer.

costs        the bias-and-gain-invariant cost under pedestals of 0, 1e2 and 1e4 on I and D, at 37 x 67 and at a size where every
             workgroup loops and ends ragged, plain, under a 70 % mask and with what the mask drops set to NaN / inf; small integers,
             where cost and gradient are the model's to the bit; bands behind cost and grad at n = 1, 255, 256, 257; mask bytes 2, 255
steps        all seven optimizers, 8 steps, per-element bounds from {-inf, finite} x {finite, +inf}, x on a bound with a gradient of
             either sign or 0, x = -inf / +inf on an infinite bound (where only isfinite() keeps the bound from acting), a NaN
             gradient, a NaN x: the six outputs bit for bit the model's, each inside its band
advance      the coefficients at k = 1 .. 10^6 against long double, RAdam's flag, the counter
second trip  one GradientDescent step over 256 (4 x 65535) + 257 float32 variables: the row loop's second trip under the flat sweep
activations  +-0, +-inf, NaN, saturating arguments and denormals through the four functions, forward and backprop
softmax      K around the lane groups and the wavefront, rows around a workgroup's share, every row distinct; saturated, equal, -inf
             rows; the backprop's form; Gumbel noise with u = 0 and u one ulp below 1, on the long-row path too
gradient     SpatialGradient2D with an axis of 1 or 2 and at 63 / 64 / 65 columns, bit for bit
"""
import numpy as np
import pytest
import torch

import optym_common as OC
from prysm_amd import _lib as L
from prysm_amd.x import optym_plan as OP

pytestmark = pytest.mark.gpu

DT = [np.float64, np.float32]
IDS = ['float64', 'float32']

# largest measured / bound per group as printed on an MI355X; a record, not a bound
RECORDED = {'activation float32': 0.487, 'activation float64': 0.308, 'advance': 0.111, 'bgi float32': 0.216, 'bgi float64': 0.069,
            'guard float32': 0.207, 'guard float64': 0.142, 'gumbel float32': 0.072, 'gumbel float64': 0.056, 'integers float32': 0.0,
            'integers float64': 0.0, 'softmax backprop float32': 0.496, 'softmax backprop float64': 0.117, 'softmax float32': 0.136,
            'softmax float64': 0.179, 'softmax sums float32': 0.361, 'softmax sums float64': 0.401}

_worst = {}


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return L.load()


def report(group, what, measured, bound):
    """prints one comparison, keeps the group's worst ratio, returns the ratio (the caller asserts it)"""
    ratio = float(measured) / float(bound) if bound > 0 else (0.0 if measured == 0 else np.inf)
    _worst[group] = max(_worst.get(group, 0.0), ratio)
    print(f'optym {group} {what}: measured {float(measured):.3e} bound {float(bound):.3e} ratio {ratio:.3e}')
    return ratio


def name_of(dt):
    return np.dtype(dt).name


# ----------------------------------------------------------------------------- costs

@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('n', OC.COST_SIZES)
def test_bgi_cost_under_a_pedestal(lib, n, dt):
    for ped in OC.PEDESTALS:
        I, D, mask = OC.bgi_inputs(ped, n, name_of(dt))  # noqa: E741
        In, Dn = I.copy(), D.copy()
        In[~mask], Dn[~mask] = np.nan, np.inf
        Dn[0] = np.nan
        results = {}
        for tag, (a, b, keep) in (('plain', (I, D, None)), ('masked', (I, D, mask)), ('masked, NaN outside', (In, Dn, mask))):
            ref = OC.bgi_case(ped, n, name_of(dt), keep is not None)
            bg, bc = OC.bgi_bounds(ref, ped, dt)
            c, g = OC.run_cost(L.PM_COST_BGI, a, b, keep)
            assert c.dtype == dt and g.dtype == dt and np.isfinite(c) and np.isfinite(g).all()
            eg, ec = OC.bgi_errors(c, g, ref)
            rg = report(f'bgi {name_of(dt)}', f'n={n} pedestal {ped:g} {tag} gradient', eg, bg)
            rc = report(f'bgi {name_of(dt)}', f'n={n} pedestal {ped:g} {tag} cost', ec, bc)
            assert rg <= 1 and rc <= 1
            if keep is not None:
                assert not g[~keep].any()
            results[tag] = (c, g)
        # what the mask drops leaves no trace
        assert OC.same_bits(results['masked'][0], results['masked, NaN outside'][0])
        assert OC.same_bits(results['masked'][1], results['masked, NaN outside'][1])


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_integer_costs_equal_the_model_to_the_bit(lib, dt):
    """N_LARGE small integers: every sum but the BGI cost's is exact in any order, so a dropped or doubled element at a seam of the
    grid-stride loop shows in the last bit, which no tolerance on 624 291 elements does"""
    I, D, mask = OC.integer_case(name_of(dt))  # noqa: E741
    for keep in (None, mask):
        c, g = OC.run_cost(L.PM_COST_MSE, I, D, keep)
        wc, wg = OP.cost(OP.COST_MSE, I, D, keep)
        assert OC.same_bits(c, wc[()]) and OC.same_bits(g, wg), 'mean_square_error on integers'
    c, g = OC.run_cost(L.PM_COST_BGI, I, D)
    wc, wg = OP.cost(OP.COST_BGI, I, D)
    assert OC.same_bits(g, wg), 'bias_and_gain_invariant_error on integers: the gradient'
    r = report(f'integers {name_of(dt)}', 'bgi cost against the model', abs(OC.LD(c) - OC.LD(wc)) / OC.LD(wc), OC.INTEGER_COST_BOUND + OC.eps_of(dt))
    assert r <= 1


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('n', OC.GUARD_SIZES)
def test_costs_stay_inside_their_outputs(lib, n, dt):
    """run_cost asserts the bands behind cost and grad and the bytes behind the workspace.  The values: BGI against long double under
    the bounds of the pedestal test; MSE and NLL against the model, whose sums are the same <= 257 terms of one sign in another order
    (n eps64 relative) and whose logarithms are numpy's (an ulp each way, 8 eps64 with the arithmetic around them)"""
    rng = np.random.default_rng(n)
    M = rng.uniform(0.1, 0.9, n).astype(dt)
    D = (1.7 * M + 0.3 + 0.05 * rng.standard_normal(n)).astype(dt)
    yhat = (rng.random(n) > 0.5).astype(dt)
    mask = rng.random(n) < 0.7
    mask[0] = True
    for kind, target in ((L.PM_COST_MSE, D), (L.PM_COST_BGI, D), (L.PM_COST_NLL, yhat), (L.PM_COST_NLL, None)):
        for keep in (None, mask):
            c, g = OC.run_cost(kind, M, target, keep, d_scalar=0.25)
            what = f'kind {kind} n={n} masked={keep is not None}'
            if keep is not None:
                assert not g[~keep].any()
            if kind == L.PM_COST_BGI:
                if n < 3:
                    continue            # one point has no variance: the bands are what this size is here for
                ref = OC.bgi_reference(M, D, keep)
                (eg, ec), (bg, bc) = OC.bgi_errors(c, g, ref), OC.bgi_bounds(ref, 0.0, dt)
                assert report(f'guard {name_of(dt)}', what + ' gradient', eg, bg) <= 1 and report(f'guard {name_of(dt)}', what + ' cost', ec, bc) <= 1
                continue
            wc, wg = OP.cost(kind, M, 0.25 if target is None else target, keep)
            tol = (n + 8) * OC.EPS64 + 2 * OC.eps_of(dt)
            ec = abs(float(c) - float(wc)) / abs(float(wc))
            eg = float(np.abs(g.astype(np.float64) - wg).max() / np.abs(wg).max())
            assert report(f'guard {name_of(dt)}', what, max(ec, eg), tol) <= 1


@pytest.mark.parametrize('dt', DT, ids=IDS)
def test_any_nonzero_mask_byte_keeps_its_element(lib, dt):
    I, D, mask = OC.bgi_inputs(0.0, OC.N_SMALL, name_of(dt))  # noqa: E741
    odd = mask.view(np.uint8) * np.where(np.arange(mask.size) % 2, 2, 255).astype(np.uint8)
    assert set(np.unique(odd)) == {0, 2, 255}
    for kind in (L.PM_COST_MSE, L.PM_COST_BGI):
        c1, g1 = OC.run_cost(kind, I, D, mask)
        c2, g2 = OC.run_cost(kind, I, D, odd)
        assert OC.same_bits(c1, c2) and OC.same_bits(g1, g2)


# ----------------------------------------------------------------------------- steps

@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('kind', range(7), ids=OC.KINDS)
def test_steps_equal_the_model_to_the_bit(lib, kind, dt):
    alpha, (beta1, beta2), eps = 0.05, OC.BETAS[0], OC.eps_of(dt)
    for n in OC.STEP_SIZES:
        case = OC.step_case(n, name_of(dt))
        lo, hi = case['lower'], case['upper']
        x, s1, s2 = case['x'].copy(), np.zeros(n, dt), np.zeros(n, dt)
        counter = torch.zeros(1, dtype=torch.int64, device='cuda')
        coef = torch.full((8,), float('nan'), dtype=torch.float64, device='cuda')
        for k in range(1, OC.STEP_COUNT + 1):
            g = OC.step_gradient(case, x, k)
            co = OC.advance(kind, beta1, beta2, counter, coef)
            got = OC.run_step(kind, x, g, s1, s2, lo, hi, coef, alpha, beta1, beta2, eps)
            want = OP.step(kind, k, x, g, s1, s2, lo, hi, alpha=alpha, beta1=beta1, beta2=beta2, eps=eps, coef=co)
            want['s1'] = s1 if want['s1'] is None else want['s1']            # state the optimizer does not have is not touched
            want['s2'] = s2 if want['s2'] is None else want['s2']
            want['active'] = want['active'].astype(np.uint8)
            for key in OC.STEP_OUTPUTS:
                same = OC.same_bits(got[key], want[key])
                if not same:
                    bad = np.flatnonzero(~((got[key] == want[key]) | (np.isnan(got[key]) & np.isnan(want[key])))) if key != 'active' else \
                        np.flatnonzero(got[key] != want[key])
                    print(f'optym step {OC.KINDS[kind]} {name_of(dt)} n={n} k={k} {key}: {bad.size} differ, first {bad[:4]}, got {got[key][bad[:4]]} '
                          f'want {want[key][bad[:4]]}')
                assert same, (OC.KINDS[kind], n, k, key)
            assert set(np.unique(got['active'])) <= {0, 1}
            x, s1, s2 = got['x'], got['s1'], got['s2']
        assert int(counter.item()) == OC.STEP_COUNT
        if case['nan_x'] is not None:
            assert np.isnan(x[case['nan_x']]) and np.isnan(x).sum() <= 2
        print(f'optym step {OC.KINDS[kind]} {name_of(dt)} n={n}: {OC.STEP_COUNT} steps, x s1 s2 x_prev g_step active equal the model bit for bit '
              f'(measured 0 differing bits, bound 0); {int(np.isnan(x).sum())} NaN in x')


def test_advance_against_long_double(lib):
    for beta1, beta2 in OC.BETAS:
        flags = []
        for kind in (L.PM_OPT_ADAM, L.PM_OPT_RADAM):
            counter = torch.zeros(1, dtype=torch.int64, device='cuda')
            coef = torch.full((9,), float('nan'), dtype=torch.float64, device='cuda')
            done = 0
            for k in OC.ADVANCE_KS:
                if k > 1000:
                    counter.fill_(k - 1)          # a million launches would prove no more than the thousand before them
                    done = k - 1
                while done < k:
                    got = OC.advance(kind, beta1, beta2, counter, coef)
                    done += 1
                assert int(counter.item()) == k
                want = OC.coefficients_reference(kind, k, beta1, beta2)
                for i, bound in OC.coefficient_bounds(want, k, beta2).items():
                    if i == 2 and kind != L.PM_OPT_RADAM:
                        assert got[2] == 0
                        continue
                    r = report('advance', f'kind {kind} betas ({beta1}, {beta2}) k={k} coefficient {i}', abs(OC.LD(got[i]) - want[i]), bound)
                    assert r <= 1
                assert got[4] == want[4] and got[6] == 0 and got[7] == 0 and np.isnan(got[8])
                if kind == L.PM_OPT_RADAM:
                    flags.append(got[4])
                    assert (got[3] > 0) == (got[4] == 1) and got[3] <= 1 + 4 * OC.EPS64
                else:
                    assert got[3] == 0 and got[4] == 0
        assert flags[0] == 0 and flags[-1] == 1 and flags == sorted(flags)


def test_a_gradient_descent_step_on_the_second_trip_of_the_row_loop(lib):
    """256 (4 x 65535) + 257 float32 variables, built and checked on the device.  Integers and alpha = 0.5: x - alpha g is exact, so
    every element, the last 257 included, must have been stepped exactly once"""
    n = OC.SECOND_TRIP_N
    assert (n + 255) // 256 > 4 * 65535 and n % 256 != 0
    gen = torch.Generator(device='cuda').manual_seed(5)
    tail = OC.TAIL

    def framed(values):
        buf = torch.full((n + tail,), float('nan'), dtype=torch.float32, device='cuda')
        if values is not None:
            buf[:n] = values
        return buf
    x = framed(torch.randint(-8, 9, (n,), generator=gen, device='cuda').float())
    g = framed(torch.randint(-8, 9, (n,), generator=gen, device='cuda').float())
    old = x[:n].clone()
    x_prev = framed(None)
    L.check(lib.pm_optym_step(L.PM_F32, L.PM_OPT_GD, n, L.ptr(x), L.ptr(g), None, None, None, None, 0.5, 0.9, 0.999, 1e-7, None, L.ptr(x_prev),
                              None, None, L.stream_ptr()))
    torch.cuda.synchronize()
    stepped = int((x[:n] == old - 0.5 * g[:n]).sum().item())
    kept = int((x_prev[:n] == old).sum().item())
    print(f'optym second trip: {stepped} of {n} stepped once, {kept} of {n} pre-step iterates stored (bound: all)')
    assert stepped == n and kept == n
    assert bool((x[n - 257:n] == (old - 0.5 * g[:n])[n - 257:]).all()) and bool((g[:n] != 0).any())
    assert bool(torch.isnan(x[n:]).all()) and bool(torch.isnan(x_prev[n:]).all()) and bool(torch.isnan(g[n:]).all())


# ----------------------------------------------------------------------------- activations

@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('kind', range(4), ids=OC.ACTIVATIONS)
def test_activations_at_the_edges(lib, kind, dt):
    for a, x0, y0 in OC.ACT_PARAMS:
        for n in OC.ACT_SIZES:
            x = OC.activation_input(n, name_of(dt), a, x0)
            for back in (False, True):
                got = OC.run_activation(kind, back, x, a, x0, y0)
                with np.errstate(all='ignore'):
                    model = OP.activation(kind, x, a, x0, y0, backprop=back)
                want = OC.activation_reference(kind, x, a, x0, y0, back)
                assert got.dtype == dt and OC.same_specials(got, model), (OC.ACTIVATIONS[kind], a, n, back, got[:13], model[:13])
                r = report(f'activation {name_of(dt)}', f'{OC.ACTIVATIONS[kind]} a={a} n={n} backprop={back}', OC.activation_ratio(got, model, want), 1.0)
                assert r <= 1


# ----------------------------------------------------------------------------- softmax

@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('K', OC.SOFTMAX_K)
def test_softmax_rows_and_groups(lib, K, dt):
    for rows in OC.softmax_rows(K):
        x, g = OC.softmax_input(K, rows, name_of(dt))
        y = OC.run_softmax(x)
        want = OC.softmax_reference(x)
        assert y.dtype == dt and np.isfinite(y).all() and (want > OC.TINY32).all()
        rf = report(f'softmax {name_of(dt)}', f'K={K} rows={rows} forward', OC.softmax_ratio(y, x, want), 1.0)
        rs = report(f'softmax sums {name_of(dt)}', f'K={K} rows={rows} row sums', OC.row_sum_ratio(y), 1.0)
        back = OC.run_softmax_backprop(y, g)
        rb = report(f'softmax backprop {name_of(dt)}', f'K={K} rows={rows} backprop',
                    OC.softmax_backprop_ratio(back, y, g, OC.softmax_backprop_reference(y, g, 1.0), 1.0), 1.0)
        assert rf <= 1 and rs <= 1 and rb <= 1
        if K == 1:
            assert np.all(y == 1) and np.all(back == 0)


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('K', OC.SPECIAL_K)
def test_softmax_special_rows(lib, K, dt):
    x, g = OC.special_rows(K, name_of(dt))
    with np.errstate(invalid='ignore'):
        model = OP.softmax(x)
    y = OC.run_softmax(x)
    for f in (np.isnan, lambda v: v == 0, lambda v: v == 1):
        assert np.array_equal(f(y), f(model)), (K, y, model)
    row = dict(zip(OC.SPECIAL_ROWS, y))
    if K & (K - 1) == 0:
        assert np.all(row['equal'] == dt(1) / dt(K))
    assert np.isnan(row['all -inf']).all() and np.array_equal(row['some -inf'] == 0, np.isneginf(x[2]))
    assert set(np.unique(row['+-1e4'])) == {0, dt(1) / dt((K + 1) // 2)}
    assert report(f'softmax {name_of(dt)}', f'K={K} special rows forward', OC.softmax_ratio(y, x, OC.softmax_reference(x)), 1.0) <= 1
    back = OC.run_softmax_backprop(y, g)
    assert np.all(back[y == 0] == 0) and np.isnan(back[3]).all() and np.isfinite(back[[0, 1, 2, 4]]).all()
    want = OC.softmax_backprop_reference(y, g, 1.0)
    assert report(f'softmax backprop {name_of(dt)}', f'K={K} special rows backprop', OC.softmax_backprop_ratio(back, y, g, want, 1.0), 1.0) <= 1
    # the saturated row is where the reference's own expression cancels: the measured ratio of that form, for the record
    naive = OC.softmax_backprop_ratio(OC.softmax_backprop_naive(y[1:2], g[1:2], 1.0), y[1:2], g[1:2], want[1:2], 1.0)
    print(f'optym softmax backprop {name_of(dt)} K={K}: y (g - sum g y) in the dtype on the saturated row would measure {naive:.3e} of the bound')


@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('K', OC.GUMBEL_K)
def test_gumbel_softmax(lib, K, dt):
    x, u, g, eps = OC.gumbel_input(K, name_of(dt))
    for tau in OC.GUMBEL_TAU:
        y = OC.run_softmax(x, u, tau, eps)          # asserts that x and u were not written
        model = OP.softmax(x, u, tau, eps)
        extra, logits = OC.gumbel_extra(x, u, tau, eps)
        assert y.dtype == dt and np.isfinite(y).all() and np.isfinite(model).all() and (model > 0).all()
        rf = report(f'gumbel {name_of(dt)}', f'K={K} tau={tau} forward against the model', OC.softmax_ratio(y, logits, model.astype(OC.LD), extra), 1.0)
        rs = report(f'softmax sums {name_of(dt)}', f'K={K} tau={tau} gumbel row sums', OC.row_sum_ratio(y), 1.0)
        back = OC.run_softmax_backprop(y, g, tau)
        rb = report(f'softmax backprop {name_of(dt)}', f'K={K} tau={tau} gumbel backprop',
                    OC.softmax_backprop_ratio(back, y, g, OC.softmax_backprop_reference(y, g, tau), tau), 1.0)
        assert rf <= 1 and rs <= 1 and rb <= 1


# ----------------------------------------------------------------------------- spatial gradient

@pytest.mark.parametrize('dt', DT, ids=IDS)
@pytest.mark.parametrize('shape', OC.GRADIENT_SHAPES, ids=str)
def test_spatial_gradient_equals_the_model_to_the_bit(lib, shape, dt):
    a = np.random.default_rng(shape[0] * 1000 + shape[1]).standard_normal(shape).astype(dt)
    for name, op in OC.GRADIENT_OPS.items():
        got = OC.run_spatial_gradient(op, a)
        want = OP.spatial_gradient(op, a)
        assert OC.same_bits(got, want), (shape, name)
        axis = 1 if name.endswith('x') else 0
        assert got.any() == (shape[axis] >= 3)
    print(f'optym spatial gradient {name_of(dt)} {shape}: four operators equal the model bit for bit (measured 0 differing bits, bound 0)')


def test_recorded_figures():
    """runs last: the worst ratio of every group in this session, for the record in tests/optym_common.py"""
    for k, v in sorted(_worst.items()):
        print(f'optym {k}: worst measured / bound {v:.3e} (recorded {RECORDED.get(k)})')
    assert all(v <= 1.0 for v in _worst.values())
