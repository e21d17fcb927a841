"""GPU: prysm_amd.polynomials' Forbes Q polynomials -- Qbfs, Qcon and Q2D bases, compute_z_* and the sums against the reference
fixture in both precisions (Q2D in both coordinate forms), against the numpy walk of the kernels' table at 1024^2, stacks, odd point
counts and views, adjoint identities, bitwise reproducibility (also under graph replay), and the gradient of a PSF loss back to the
Q2D coefficients against finite differences."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_common import tonp

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 5e-5}


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'qpoly.npz'))


def _nms(a):
    return [tuple(int(v) for v in row) for row in a]


def _rel_per_mode(got, ref):
    ax = tuple(range(1, ref.ndim))
    return np.max(np.max(np.abs(got - ref), axis=ax) / np.max(np.abs(ref), axis=ax))


def _rel(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_radial_bases_match_the_reference(fx, dt):
    from prysm_amd import polynomials as P
    u = fx['u'].astype(dt)
    ns = list(range(21))
    for fn, one, key in ((P.Qbfs_seq, P.Qbfs, 'qbfs_seq'), (P.Qcon_seq, P.Qcon, 'qcon_seq')):
        got = tonp(fn(ns, u))
        assert got.dtype == dt and got.shape == fx[key].shape
        assert _rel_per_mode(got, fx[key]) < TOL[dt]
        for n in (0, 1, 2, 13):
            assert _rel(tonp(one(n, u)), fx[key][n]) < TOL[dt]
    assert tuple(P.Qbfs_seq([], u).shape) == (0, len(u))


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('polar', [True, False])
def test_q2d_basis_matches_the_reference(fx, dt, polar):
    from prysm_amd import _lib as L
    from prysm_amd.polynomials import qpoly as Q
    u, v = (fx['r'].astype(dt), fx['t'].astype(dt)) if polar else (fx['x'].astype(dt), fx['y'].astype(dt))
    coords = L.PM_ZERNIKE_POLAR if polar else L.PM_ZERNIKE_CARTESIAN
    for key, seq in (('nms8', 'q2d_seq8'), ('nms20', 'q2d_seq20'), ('nms_single', 'q2d_single')):
        got = tonp(Q._seq(_nms(fx[key]), Q.Q2D, u, v, coords))
        assert got.dtype == dt and got.shape == fx[seq].shape
        assert _rel_per_mode(got, fx[seq]) < TOL[dt], key
    if polar:
        assert _rel_per_mode(tonp(Q.Q2d_seq(_nms(fx['nms8']), u, v)), fx['q2d_seq8']) < TOL[dt]
        for (n, m), want in zip(_nms(fx['nms_single']), fx['q2d_single']):
            assert _rel(tonp(Q.Q2d(n, m, u, v)), want) < TOL[dt], (n, m)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_compute_z_and_sums_match_the_reference(fx, dt):
    from prysm_amd import polynomials as P
    u = fx['u'].astype(dt)
    got = tonp(P.compute_z_Qbfs(fx['zbfs_coefs'], u, u * u))
    assert got.dtype == dt and _rel(got, fx['zbfs']) < TOL[dt]
    nms = _nms(fx['nms8'])
    c = fx['z2d_coefs']
    cm0, ams, bms = P.Q2d_nm_c_to_a_b(nms, c)
    r, t = fx['r'].astype(dt), fx['t'].astype(dt)
    assert _rel(tonp(P.compute_z_Q2d(cm0, ams, bms, r, t)), fx['z2d']) < TOL[dt]
    x, y = fx['x'].astype(dt), fx['y'].astype(dt)
    assert _rel(tonp(P.Q2d_sum(c.astype(dt), nms, x, y)), fx['z2d']) < TOL[dt]
    # Qcon_sum against the fixture basis; the adjoints against the fixture basis too
    cc = np.linspace(-1, 1, 21)
    assert _rel(tonp(P.Qcon_sum(cc.astype(dt), range(21), u)), cc @ fx['qcon_seq']) < TOL[dt]
    g = np.cos(np.arange(len(u)))
    assert _rel(tonp(P.Qcon_sum_adjoint(g.astype(dt), range(21), u)), fx['qcon_seq'] @ g) < TOL[dt]
    gb = np.sin(np.arange(x.size)).reshape(x.shape)
    want = np.tensordot(fx['q2d_seq8'], gb)
    assert _rel(tonp(P.Q2d_sum_adjoint(gb.astype(dt), nms, x, y)), want) < TOL[dt]
    # all-zero coefficients: nothing to walk, zeros out
    assert not np.any(tonp(P.compute_z_Q2d([0.0], [], [[0.0]], r, t)))


def _grid(n, dt=np.float64):
    g = ((np.arange(n) - n // 2) / (n // 2)).astype(dt)
    x, y = np.meshgrid(g, g)
    return x, y


NMS10 = [(n, m) for n in range(11) for m in range(-10, 11)]     # 231 modes, n <= 10, |m| <= 10


def test_1024_against_the_numpy_walk():
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.qpoly_plan import evaluate, plan, Q2D, POLAR
    x, y = _grid(1024)
    x, y = 0.999 * x, 0.999 * y
    xs, ys = x[::37], y[::37]                         # the numpy walk on every 37th row
    want = evaluate(plan(NMS10, Q2D), xs, ys, len(NMS10))
    from prysm_amd.polynomials import qpoly as Q
    from prysm_amd import _lib as L
    got = Q._seq(NMS10, Q2D, x, y, L.PM_ZERNIKE_CARTESIAN)
    assert _rel_per_mode(tonp(got[:, ::37]), want) < 1e-12
    r, t = np.hypot(x, y), np.arctan2(y, x)
    gotp = P.Q2d_seq(NMS10, r, t)
    wantp = evaluate(plan(NMS10, Q2D), r[::37], t[::37], len(NMS10), POLAR)
    assert _rel_per_mode(tonp(gotp[:, ::37]), wantp) < 1e-12
    del gotp
    c = np.random.default_rng(3).standard_normal(len(NMS10))
    s = tonp(P.Q2d_sum(c, NMS10, x, y))
    assert _rel(s[::37], np.tensordot(c, want, axes=(0, 0))) < 1e-12
    # the matrix-free adjoint equals the adjoint over the stored basis
    gbar = np.random.default_rng(4).standard_normal(x.shape)
    a1 = tonp(P.Q2d_sum_adjoint(gbar, NMS10, x, y))
    a2 = tonp(P.sum_of_2d_modes_adjoint(got, gbar))
    assert _rel(a1, a2) < 1e-12
    del got
    got32 = tonp(Q._seq(NMS10, Q2D, x.astype(np.float32), y.astype(np.float32), L.PM_ZERNIKE_CARTESIAN)[:, ::37])
    assert _rel_per_mode(got32.astype(np.float64), want) < 5e-5


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_stacks_equal_single_calls(dt):
    from prysm_amd import polynomials as P
    x, y = _grid(96, dt)
    x, y = x[:, :90], y[:, :90]                       # 96 x 90 points
    nms = [(n, m) for n in range(7) for m in range(-6, 7)]
    rng = np.random.default_rng(5)
    C = rng.standard_normal((11, len(nms))).astype(dt)    # 11 = 8 + 2 + 1 vectors per walk
    S = tonp(P.Q2d_sum(C, nms, x, y))
    assert S.shape == (11, 96, 90)
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(11):
        assert _rel(S[b], tonp(P.Q2d_sum(C[b], nms, x, y))) < tol
    G = rng.standard_normal((11, 96, 90)).astype(dt)
    A = tonp(P.Q2d_sum_adjoint(G, nms, x, y))
    assert A.shape == (11, len(nms))
    for b in range(11):
        assert _rel(A[b], tonp(P.Q2d_sum_adjoint(G[b], nms, x, y))) < tol
    u = np.abs(x[0])
    Cc = rng.standard_normal((5, 9)).astype(dt)
    Sc = tonp(P.Qcon_sum(Cc, range(9), u))
    Gc = rng.standard_normal((5, u.size)).astype(dt)
    Ac = tonp(P.Qcon_sum_adjoint(Gc, range(9), u))
    for b in range(5):
        assert _rel(Sc[b], tonp(P.Qcon_sum(Cc[b], range(9), u))) < tol
        assert _rel(Ac[b], tonp(P.Qcon_sum_adjoint(Gc[b], range(9), u))) < tol


def _stack_of_15(dt, npts, nms):
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(15)
    x, y = (rng.uniform(-0.7, 0.7, npts).astype(dt) for _ in range(2))
    C = rng.standard_normal((15, len(nms))).astype(dt)
    S = tonp(P.Q2d_sum(C, nms, x, y))
    assert S.shape == (15, npts) and S.dtype == dt
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(15):
        assert _rel(S[b], tonp(P.Q2d_sum(C[b], nms, x, y))) < tol
    G = rng.standard_normal((15, npts)).astype(dt)
    A = tonp(P.Q2d_sum_adjoint(G, nms, x, y))
    assert A.shape == (15, len(nms)) and A.dtype == dt
    for b in range(15):
        assert _rel(A[b], tonp(P.Q2d_sum_adjoint(G[b], nms, x, y))) < tol


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('npts', [1024, 1027])
def test_a_stack_of_15_equals_single_calls(dt, npts):
    """15 = 8 + 4 + 2 + 1 vectors per walk, each piece at its own offset into the coefficients, the output and the partials; 1024 points
    take the 16-byte path, 1027 the element-wise one"""
    _stack_of_15(dt, npts, [(n, m) for n in range(2) for m in range(-2, 3)])


def test_a_stack_of_15_with_two_vectors_per_projection_walk():
    """625 modes in fp64: the accumulators of a projection workgroup (64 KiB) hold two vectors of them, not four, so the 15 go as seven
    pairs and a single one"""
    _stack_of_15(np.float64, 1027, [(n, m) for n in range(25) for m in range(-12, 13)])


def test_odd_point_counts_and_views():
    """point counts that are not a multiple of 4 and coordinates that start off a 16-byte boundary take the element-wise path"""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.qpoly_plan import evaluate, plan, Q2D, QCON, RADIAL
    nms = [(n, m) for n in range(6) for m in range(-4, 5)]
    x, y = _grid(64)
    xt, yt = torch.from_numpy(x).cuda().reshape(-1), torch.from_numpy(y).cuda().reshape(-1)
    for lo, hi in ((0, 4093), (1, 4001), (3, 4096)):
        xs, ys = xt[lo:hi], yt[lo:hi]
        want = evaluate(plan(nms, Q2D), tonp(xs), tonp(ys), len(nms))
        c = np.linspace(-1, 1, len(nms))
        assert _rel(tonp(P.Q2d_sum(c, nms, xs, ys)), np.tensordot(c, want, axes=(0, 0))) < 1e-12
        g = np.cos(np.arange(hi - lo))
        assert _rel(tonp(P.Q2d_sum_adjoint(g, nms, xs, ys)), want @ g) < 1e-12
        us = xs.abs()
        wantc = evaluate(plan(range(8), QCON), tonp(us), None, 8, RADIAL)
        assert _rel_per_mode(tonp(P.Qcon_seq(range(8), us)), wantc) < 1e-12
        assert _rel(tonp(P.Qcon_sum_adjoint(g, range(8), us)), wantc @ g) < 1e-12
    # a strided (non-contiguous) view
    xv, yv = torch.from_numpy(x).cuda()[:, ::3], torch.from_numpy(y).cuda()[:, ::3]
    want = evaluate(plan(nms, Q2D), tonp(xv), tonp(yv), len(nms))
    assert _rel_per_mode(tonp(P.Q2d_seq(nms, torch.hypot(xv, yv), torch.atan2(yv, xv))), want) < 1e-12


def test_dot_product_identities():
    from prysm_amd import polynomials as P
    x, y = _grid(256)
    rng = np.random.default_rng(6)
    c = rng.standard_normal(len(NMS10))
    g = rng.standard_normal(x.shape)
    lhs = float(np.vdot(tonp(P.Q2d_sum(c, NMS10, x, y)), g))
    rhs = float(np.vdot(c, tonp(P.Q2d_sum_adjoint(g, NMS10, x, y))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12
    u = np.abs(x)
    cc = rng.standard_normal(15)
    lhs = float(np.vdot(tonp(P.Qcon_sum(cc, range(15), u)), g))
    rhs = float(np.vdot(cc, tonp(P.Qcon_sum_adjoint(g, range(15), u))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12


def test_adjoints_are_bitwise_reproducible():
    from prysm_amd import polynomials as P
    x, y = _grid(512)
    g = torch.from_numpy(np.random.default_rng(7).standard_normal((3, 512, 512))).cuda()
    a = P.Q2d_sum_adjoint(g, NMS10, x, y).clone()
    b = P.Q2d_sum_adjoint(g, NMS10, x, y).clone()
    assert torch.equal(a, b)
    u = np.abs(x)
    a = P.Qcon_sum_adjoint(g, range(21), u).clone()
    b = P.Qcon_sum_adjoint(g, range(21), u).clone()
    assert torch.equal(a, b)


EFL, WVL, DX, Q = 100.0, 0.6328, 10.0 / 128, 2
NMS4 = [(n, m) for n in range(5) for m in range(-4, 5)]


def _model(amp, x, y, target):
    """loss and its gradient with respect to the Q2D coefficients, all on the device"""
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront

    def run(c):
        opd = P.Q2d_sum(c, NMS4, x, y)
        wf = Wavefront.from_amp_and_phase(amp, opd, WVL, DX)
        psf = wf.focus(EFL, Q=Q)
        I = psf.intensity.data
        diff = I - target
        loss = (diff * diff).sum()
        wbar = psf.intensity_adjoint(2 * diff).focus_adjoint(EFL, Q=Q)
        obar = wf.from_amp_and_phase_adjoint_phase(wbar).imag    # the reference's quirk: the gradient times 1j
        return loss, P.Q2d_sum_adjoint(obar, NMS4, x, y)
    return run


def _setup():
    x, y = _grid(128)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    amp = (xt * xt + yt * yt <= 1).to(torch.float64)
    rng = np.random.default_rng(8)
    c_true = torch.from_numpy(30 * rng.standard_normal(len(NMS4))).cuda()
    c0 = torch.from_numpy(30 * rng.standard_normal(len(NMS4))).cuda()
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront
    target = Wavefront.from_amp_and_phase(amp, P.Q2d_sum(c_true, NMS4, xt, yt), WVL, DX).focus(EFL, Q=Q).intensity.data.clone()
    return amp, xt, yt, target, c0


def test_psf_loss_gradient_matches_finite_differences():
    amp, x, y, target, c0 = _setup()
    run = _model(amp, x, y, target)
    loss, grad = run(c0)
    grad = tonp(grad)
    h = 1e-2
    for k in (1, 9, 22, 40):
        e = torch.zeros_like(c0)
        e[k] = h
        lp, _ = run(c0 + e)
        lm, _ = run(c0 - e)
        fd = (float(lp) - float(lm)) / (2 * h)
        assert abs(grad[k] - fd) / abs(fd) < 1e-6, (k, grad[k], fd)


def test_graph_replay_of_the_gradient_chain_is_bit_equal():
    from prysm_amd import graph
    amp, x, y, target, c0 = _setup()
    run = _model(amp, x, y, target)
    eager_loss, eager_grad = (t.clone() for t in run(c0))
    model = graph.capture(run, c0)
    loss, grad = model(c0)
    assert torch.equal(loss, eager_loss) and torch.equal(grad, eager_grad)
    # the coefficients are read on the device: an in-place update is seen by the replay
    c1 = c0.clone()
    eager1 = run(c1 * 0.5)[1].clone()
    c0.mul_(0.5)
    assert torch.equal(model(c0)[1], eager1)
    assert not torch.equal(eager1, eager_grad)
