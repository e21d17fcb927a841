"""GPU: pm_tf_stack and pm_tf_thickness_grad through prysm_amd.thinfilm and prysm_amd.x.coatings, against the reference's stored
results (tests/golden/coatings.npz), against the numpy model at sizes the fixture does not hold, and against themselves (both
polarisations in one sweep, repeated runs, the accumulate flag, a captured optimizer step).  Tolerances: tests/coatings_common.py."""
import numpy as np
import pytest
import torch

import coatings_common as CC
from gpu_common import tonp
from prysm_amd import thinfilm_plan as plan

pytestmark = pytest.mark.gpu

DTYPES = [np.complex128, np.complex64]


def _real(dt):
    return np.float64 if np.dtype(dt) == np.complex128 else np.float32


def _stack(case, dt):
    from prysm_amd.x import coatings as C
    g = CC.golden()
    n, d = g[case + '_n'], g[case + '_d']
    scalar = lambda v: v.item() if v.ndim == 0 else v  # noqa: E731
    stack = C.Stack(list(n), torch.from_numpy(d.astype(_real(dt))), scalar(g[case + '_nsub']), scalar(g[case + '_n0']))
    return stack, g[case + '_wvl'], np.radians(g[case + '_aoi'])


def _check(got, case, pol, quantity, dt):
    got = tonp(got)
    assert got.dtype == (np.dtype(dt) if quantity in ('r', 'r_tf', 't', 't_tf', 'E', 'H') else _real(dt)), (quantity, got.dtype)
    dev = CC.deviation(got, case, pol, quantity)
    print(f'{case} {pol} {quantity} {np.dtype(dt).name}: deviation {dev:.2e}, bound {CC.tolerance(case, quantity, dt):.2e}')
    assert dev <= CC.tolerance(case, quantity, dt), (case, pol, quantity, dev)


@pytest.mark.parametrize('case', CC.CASES)
@pytest.mark.parametrize('dt', DTYPES)
def test_fixture_cases_forward(pa, case, dt):
    from prysm_amd import thinfilm as T
    from prysm_amd.x import coatings as C
    g = CC.golden()
    stack, wvl, theta = _stack(case, dt)
    for pol in CC.POLS:
        r, t = C.stack_rt(stack, wvl, theta, pol)
        _check(r, case, pol, 'r', dt), _check(t, case, pol, 't', dt)
        R, Tr, A = C.RTA(stack, wvl, theta, pol)
        _check(R, case, pol, 'R', dt), _check(Tr, case, pol, 'T', dt), _check(A, case, pol, 'A', dt)
        E, H = C.internal_fields(stack, wvl, theta, pol)
        _check(E, case, pol, 'E', dt), _check(H, case, pol, 'H', dt)
        # multilayer_stack_rt: degrees, its own t for p (oblique angles in every case but the first row of a grid)
        rtf, ttf = T.multilayer_stack_rt(g[case + '_n'], g[case + '_d'].astype(_real(dt)), g[case + '_wvl'], pol, g[case + '_nsub'],
                                         aoi=g[case + '_aoi'], ambient_index=g[case + '_n0'])
        _check(rtf, case, pol, 'r_tf', dt), _check(ttf, case, pol, 't_tf', dt)
        fwd = C.forward_eval(stack, wvl, theta, pol)
        _check(fwd.r, case, pol, 'r', dt), _check(fwd.R_value, case, pol, 'R', dt), _check(fwd.T_value, case, pol, 'T', dt)
        _check(fwd.E, case, pol, 'E', dt), _check(fwd.A_value, case, pol, 'A', dt)
        assert torch.equal(fwd.Esq_value, fwd.E.real ** 2 + fwd.E.imag ** 2)


@pytest.mark.parametrize('dt', DTYPES)
def test_total_internal_reflection(pa, dt):
    from prysm_amd.x import coatings as C
    g = CC.golden()
    stack, wvl, theta = _stack('c2_tir', dt)
    beyond = g['c2_tir_aoi'] > np.degrees(np.arcsin(1 / 1.5))
    assert beyond.sum() == 2
    for pol in CC.POLS:
        fwd = C.forward_eval(stack, wvl, theta, pol)
        for a in (fwd.r, fwd.t, fwd.E, fwd.H, fwd.R_value, fwd.T_value, fwd.A_value):
            assert bool(torch.all(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a)))
        r = tonp(fwd.r)
        assert np.max(np.abs(np.abs(r[beyond]) - 1)) <= CC.tolerance('c2_tir', 'r', dt) and np.all(np.abs(r[~beyond]) < 0.99)


@pytest.mark.parametrize('dt', DTYPES)
def test_both_polarisations_are_bitwise_the_two_sweeps(pa, dt):
    from prysm_amd import _ops
    from prysm_amd.x.coatings.stack import operands
    for case in ('c1_L5', 'c3_map'):
        stack, wvl, theta = _stack(case, dt)
        op, _ = operands(stack, wvl, theta)
        want = ('R', 'T', 'fields', 'A')
        both, s, p = _ops.tf_stack(op, 'both', want=want), _ops.tf_stack(op, 's', want=want), _ops.tf_stack(op, 'p', want=want)
        for k in both:
            assert both[k].shape[0] == 2 and torch.equal(both[k][0], s[k][0]) and torch.equal(both[k][1], p[k][0]), k


def _random_operands(rng, K, L, per_sample):
    mats = np.array(CC.MATERIALS)
    n = np.array([mats[j % 4] for j in range(L)]).reshape(L, 1)
    d = rng.uniform(0.05, 0.25, (L, 1))
    if per_sample:
        n = n + 1e-3 * rng.random((L, K))
        d = d * (1 + 0.05 * rng.random((L, K)))
    return dict(indices=n, thicknesses=d, wvl=rng.uniform(0.45, 0.75, K), theta=np.radians(rng.uniform(0, 70, K)),
                nsub=(1.458461 + 0.02 * rng.random(K)) if per_sample else np.array([1.458461]), n0=np.array([1.0]))


@pytest.mark.parametrize('K', [1, 65, 201, 1027])
@pytest.mark.parametrize('per_sample', [False, True])
@pytest.mark.parametrize('dt', DTYPES)
def test_sample_counts_against_the_model(pa, K, per_sample, dt):
    """a lone thread, one wavefront plus one, several workgroups with a tail; shared and per-sample tables; five layers of the
    fixture's materials"""
    from prysm_amd import _ops
    rng = np.random.default_rng(1000 + K)
    flat = _random_operands(rng, K, 5, per_sample)
    cd = torch.complex128 if np.dtype(dt) == np.complex128 else torch.complex64
    op = _ops.TfOperands(cd, K, flat['wvl'], flat['theta'], flat['indices'], flat['thicknesses'], flat['nsub'], flat['n0'])
    dR, dT, dR2 = rng.standard_normal(K), rng.standard_normal(K), rng.standard_normal((2, K))
    single = np.dtype(dt) == np.complex64

    # float64: the fixture's bound.  complex64: the same construction in that format -- layers x about 20 operations x unit roundoff
    # (2^-24), a decade on top: 6e-5.  (The model's own complex64 deviation on ONE random draw of seeds swings between 6e-7 and 4e-6
    # and is no stable yardstick for another evaluation of the same draw.)  Both against the float64 model.
    lim = 10 * 5 * 20 * 2.0 ** -24 if single else CC.F64_TOL
    ref = plan.stack(pol=plan.BOTH, **flat)
    got = _ops.tf_stack(op, 'both', want=('R', 'T', 'fields', 'A'))
    for k in ('r', 't', 'R', 'T', 'E', 'H', 'A'):
        scale = max(np.max(np.abs(ref[k])), 1.0 if k == 'A' else 0.0)      # A: a difference of fluxes of the unit incident power
        dev = np.max(np.abs(tonp(got[k]) - ref[k])) / scale
        print(f'K={K} per_sample={per_sample} {k} {np.dtype(dt).name}: deviation {dev:.2e}, bound {lim:.2e}')
        assert got[k].dtype == ((cd if k in 'rtEH' else op.rdtype)) and dev <= lim, (k, dev, lim)
    for pol, seeds in (('both', dict(dR=dR, dT=dT)), ('both', dict(dR=dR2)), ('s', dict(dT=dT))):
        gref = plan.thickness_grad(pol=plan.BOTH if pol == 'both' else plan.S, **seeds, **flat)
        ggot = tonp(_ops.tf_thickness_grad(op, pol, seeds.get('dR'), seeds.get('dT')))
        dev = np.max(np.abs(ggot - gref)) / np.max(np.abs(gref))
        print(f'K={K} per_sample={per_sample} grad {pol} {sorted(seeds)} {np.dtype(dt).name}: deviation {dev:.2e}, bound {lim:.2e}')
        assert dev <= lim, (pol, dev, lim)


@pytest.mark.parametrize('dt', DTYPES)
def test_no_layers_is_the_bare_interface(pa, dt):
    from prysm_amd import thinfilm as T
    from prysm_amd.x import coatings as C
    theta = np.radians(np.array([0.0, 23.0, 60.0]))
    n0, n1 = 1.0, 1.458461
    theta1 = T.snell_aor(n0, n1, theta, deg=False)
    stack = C.Stack([], torch.zeros(0, dtype=torch.float64 if np.dtype(dt) == np.complex128 else torch.float32), n1, n0)
    assert len(stack) == 0
    tol = 1e-14 if np.dtype(dt) == np.complex128 else 8 * np.finfo(np.float32).eps      # about eight roundings of values of order 1
    for pol, fr, ft in (('s', T.fresnel_rs, T.fresnel_ts), ('p', T.fresnel_rp, T.fresnel_tp)):
        r, t = C.stack_rt(stack, 0.5, theta, pol)
        scale = np.cos(theta) / np.cos(theta1) if pol == 'p' else 1.0
        assert np.max(np.abs(tonp(r) - fr(n0, n1, theta, theta1))) <= tol and np.max(np.abs(tonp(t) - ft(n0, n1, theta, theta1) / scale)) <= tol
        R, Tr, A = C.RTA(stack, 0.5, theta, pol)
        assert A.shape == (0, 3) and np.max(np.abs(tonp(R) + tonp(Tr) - 1)) <= tol
        E, H = C.internal_fields(stack, 0.5, theta, pol)
        assert E.shape == (1, 3) and np.max(np.abs(tonp(E) - tonp(t))) <= tol
        assert C.thickness_gradient(C.forward_eval(stack, 0.5, theta, pol), dR=np.ones(3)).shape == (0,)


@pytest.mark.parametrize('case', CC.CASES)
@pytest.mark.parametrize('dt', DTYPES)
def test_fixture_cases_gradient(pa, case, dt):
    from prysm_amd.x import coatings as C
    stack, wvl, theta = _stack(case, dt)
    for pol in CC.POLS:
        fwd = C.forward_eval(stack, wvl, theta, pol)
        for quantity in CC.GRADS:
            dR, dT = CC.seeds(case, quantity[5:])
            _check(C.thickness_gradient(fwd, dR=dR, dT=dT), case, pol, quantity, dt)


def test_gradient_against_central_differences_of_the_device_forward(pa):
    """float64, F = sum_k dR_k R_k + dT_k T_k on the 5-layer case; h and the bound as in the host test (truncation 6e-8, roundoff
    1e-10 of the derivative's scale, bound 1e-6 of the largest component)."""
    from prysm_amd.x import coatings as C
    g = CC.golden()
    stack, wvl, theta = _stack('c1_L5', np.complex128)
    dR, dT = (torch.from_numpy(g['c1_L5_' + k]).cuda() for k in ('dR', 'dT'))
    h = 1e-5
    for pol in CC.POLS:
        grad = tonp(C.thickness_gradient(C.forward_eval(stack, wvl, theta, pol), dR=dR, dT=dT))
        d0 = stack.thicknesses.clone()
        for j in (0, 2, 4):
            F = []
            for sgn in (1, -1):
                d = d0.clone()
                d[j] += sgn * h
                R, Tr, _ = C.RTA(C.Stack(stack.indices, d, stack.substrate_index, stack.ambient_index), wvl, theta, pol)
                F.append(float(torch.sum(dR * R + dT * Tr)))
            fd = (F[0] - F[1]) / (2 * h)
            assert abs(fd - grad[j]) <= 1e-6 * np.max(np.abs(grad)), (pol, j, fd, grad[j])


@pytest.mark.parametrize('dt', DTYPES)
def test_gradient_repeats_bitwise_and_accumulates(pa, dt):
    from prysm_amd import _ops
    from prysm_amd.x import coatings as C
    rng = np.random.default_rng(5)
    K = 1027
    flat = _random_operands(rng, K, 5, True)
    cd = torch.complex128 if np.dtype(dt) == np.complex128 else torch.complex64
    op = _ops.TfOperands(cd, K, flat['wvl'], flat['theta'], flat['indices'], flat['thicknesses'], flat['nsub'], flat['n0'])
    dR, dT = rng.standard_normal(K), rng.standard_normal(K)
    a, b = _ops.tf_thickness_grad(op, 's', dR, dT), _ops.tf_thickness_grad(op, 's', dR, dT)
    assert torch.equal(a, b)
    p = _ops.tf_thickness_grad(op, 'p', dR, dT)
    acc = _ops.tf_thickness_grad(op, 'p', dR, dT, grad=a.clone())
    assert torch.equal(acc, a + p)
    # through the public function: out= adds
    stack, wvl, theta = _stack('c1_L5', dt)
    g = CC.golden()
    fs, fp = C.forward_eval(stack, wvl, theta, 's'), C.forward_eval(stack, wvl, theta, 'p')
    gs = C.thickness_gradient(fs, dR=g['c1_L5_dR'])
    gp = C.thickness_gradient(fp, dR=g['c1_L5_dR'])
    both = C.thickness_gradient(fp, dR=g['c1_L5_dR'], out=gs.clone())
    assert torch.equal(both, gs + gp)


@pytest.mark.parametrize('dt', DTYPES)
def test_gradient_fold_past_256_partials_places_every_partial(pa, dt):
    """K = 64 * 257 + 1 samples give 258 partials per layer, so the folding workgroup's threads 0 and 1 make a second trip and the last
    partial comes from a wavefront with one live lane.  With dR one-hot at sample k every other partial is an exact zero, and a sum
    of one value and zeros is that value in any order: the gradient must be, bit for bit, the gradient of sample k alone with
    dR = 1.  k = 0: the first partial; k = 64 * 256: the first partial of the second trip; k = K - 1: the ragged last wavefront.  A
    dropped, doubled or misplaced partial shows as a mismatch."""
    from prysm_amd import _ops
    K, Ly = 64 * 257 + 1, 2
    assert -(-K // 64) == 258      # parts_of(K) of csrc/thinfilm.hip: one partial per wavefront
    flat = _random_operands(np.random.default_rng(258), K, Ly, True)
    cd = torch.complex128 if np.dtype(dt) == np.complex128 else torch.complex64
    op = _ops.TfOperands(cd, K, flat['wvl'], flat['theta'], flat['indices'], flat['thicknesses'], flat['nsub'], flat['n0'])
    for k in (0, 64 * 256, K - 1):
        dR = np.zeros(K)
        dR[k] = 1.0
        got = _ops.tf_thickness_grad(op, 's', dR, None)
        one = _ops.TfOperands(cd, 1, flat['wvl'][k:k + 1], flat['theta'][k:k + 1], flat['indices'][:, k:k + 1], flat['thicknesses'][:, k:k + 1],
                              flat['nsub'][k:k + 1], flat['n0'])
        want = _ops.tf_thickness_grad(one, 's', np.ones(1), None)
        print(f'k={k} {np.dtype(dt).name}: fold {tonp(got)}, sample alone {tonp(want)}')
        assert float(want.abs().min()) > 0 and torch.equal(got, want), (k, tonp(got), tonp(want))


def _refinement(C, O, term=None):
    n6, W, A, nsub = CC.traj_operands()
    term = C.Reflectance(W, A, 'avg', 0.0, 1.0) if term is None else term
    stack = C.Stack(list(n6), np.array(CC.TRAJ_D0), nsub)

    def fg(x):
        stack.thicknesses = x
        return term.value_and_grad(stack)
    return O.Adam(fg, np.array(CC.TRAJ_D0), CC.TRAJ_ALPHA), stack, term


def test_refinement_trajectory_with_adam(pa):
    from prysm_amd.x import coatings as C
    from prysm_amd.x import optym as O
    g = CC.golden()
    opt, stack, term = _refinement(C, O)
    for k in range(1, CC.TRAJ_STEPS + 1):
        _, f, grad = opt.step()
        assert f.dim() == 0 and f.is_cuda and grad.shape == (6,) and grad.is_cuda
        assert abs(float(f) - g['traj_f'][k - 1]) <= CC.TRAJ_TOL * abs(g['traj_f'][k - 1]), (k, float(f))
        assert np.max(np.abs(tonp(opt.x) - g['traj_x'][k]) / np.abs(g['traj_x'][k])) <= CC.TRAJ_TOL, k
    stack.thicknesses = opt.x
    assert abs(term.value(stack) - g['traj_f'][-1]) <= CC.TRAJ_TOL * g['traj_f'][-1]
    merit = C.MeritFunction([term, C.Transmittance(0.55, 0.0, 's', 1.0, 2.0)])
    v, gr = merit.value_and_grad(stack)
    assert abs(float(v) - merit.value(stack)) <= 1e-12 * merit.value(stack) and gr.shape == (6,)
    res = merit.residuals(stack)
    assert res.shape == (3 * 67 + 1,) and abs(float(torch.sum(res * res)) - float(v)) <= 1e-12 * float(v)


def test_captured_step_replays_the_eager_steps(pa):
    from prysm_amd import graph
    from prysm_amd.x import coatings as C
    from prysm_amd.x import optym as O
    eager, _, _ = _refinement(C, O)
    for _ in range(CC.TRAJ_STEPS):
        eager.step()
    opt, _, _ = _refinement(C, O)
    model = graph.capture(lambda: opt.step()[1])
    opt.reset()
    for _ in range(CC.TRAJ_STEPS):
        f = model()
    torch.cuda.synchronize()
    assert int(opt.counter.item()) == CC.TRAJ_STEPS and torch.equal(opt.x, eager.x) and torch.equal(opt.m, eager.m)
    assert np.isfinite(float(f))
