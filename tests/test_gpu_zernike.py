"""GPU: prysm_amd.polynomials -- the Zernike basis, sum and adjoints against the reference fixture in both precisions and both
coordinate forms, against the numpy walk of the kernels' table at 1024^2, stacks, adjoint identities, bitwise reproducibility (also
under graph replay), and the gradient of a PSF loss back to the Zernike coefficients against finite differences."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_common import tonp

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 2e-5}


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'zernike.npz'))


def _nms(a):
    return [tuple(int(v) for v in row) for row in a]


def _rel_per_mode(got, ref):
    ax = tuple(range(1, ref.ndim))
    return np.max(np.max(np.abs(got - ref), axis=ax) / np.max(np.abs(ref), axis=ax))


def _rel(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def _uv(fx, polar, dt, sfx=''):
    return (fx['r' + sfx].astype(dt), fx['t' + sfx].astype(dt)) if polar else (fx['x' + sfx].astype(dt), fx['y' + sfx].astype(dt))


def _code(polar):
    from prysm_amd import _lib as L
    return L.PM_ZERNIKE_POLAR if polar else L.PM_ZERNIKE_CARTESIAN


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('polar', [True, False])
def test_basis_matches_the_reference(fx, dt, polar):
    from prysm_amd.polynomials import zernike as Z
    u, v = _uv(fx, polar, dt)
    nms = _nms(fx['nms12'])
    got = tonp(Z._seq(nms, u, v, True, _code(polar)))
    assert got.dtype == dt and got.shape == fx['seq12'].shape
    assert _rel_per_mode(got, fx['seq12']) < TOL[dt]
    u20, v20 = _uv(fx, polar, dt, '20')
    assert _rel_per_mode(tonp(Z._seq(_nms(fx['nms20']), u20, v20, True, _code(polar))), fx['seq20']) < TOL[dt]
    raw = _nms(fx['nms_raw'])
    assert _rel_per_mode(tonp(Z._seq(raw, u, v, False, _code(polar))), fx['seq_raw']) < TOL[dt]
    if polar:
        n, m = (int(a) for a in fx['odd_nm'])
        assert _rel(tonp(Z.zernike_nm(n, m, u, v)), fx['odd']) < TOL[dt]
        assert _rel_per_mode(tonp(Z.zernike_nm_seq(nms, u, v)), fx['seq12']) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('polar', [True, False])
def test_sum_and_adjoints_match_the_reference(fx, dt, polar):
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials import zernike as Z
    u, v = _uv(fx, polar, dt)
    nms = _nms(fx['nms8'])
    coefs = fx['coefs'].astype(dt)
    for c, want in zip(coefs, fx['sums']):
        got = tonp(Z._sum(c, nms, u, v, True, _code(polar)))
        assert got.dtype == dt and _rel(got, want) < TOL[dt]
    assert _rel(tonp(Z._sum(coefs, nms, u, v, True, _code(polar))), fx['sums']) < TOL[dt]
    g = fx['databar'].astype(dt)
    adj = tonp(Z._adjoint(g, nms, u, v, True, _code(polar)))
    assert adj.shape == (len(nms),) and adj.dtype == dt
    assert _rel(adj, fx['modes_adj']) < TOL[dt]
    basis = Z._seq(nms, u, v, True, _code(polar))
    madj = tonp(P.sum_of_2d_modes_adjoint(basis, g))
    assert madj.dtype == dt and _rel(madj, fx['modes_adj']) < TOL[dt]
    if not polar:
        assert _rel(tonp(P.zernike_sum(coefs[0], nms, u, v)), fx['sums'][0]) < TOL[dt]
        assert _rel(tonp(P.zernike_sum_adjoint(g, nms, u, v)), fx['modes_adj']) < TOL[dt]
        assert _rel(tonp(P.sum_of_2d_modes(basis, coefs[1])), fx['sums'][1]) < TOL[dt]


def _grid(n, dt=np.float64):
    g = ((np.arange(n) - n // 2) / (n // 2)).astype(dt)
    x, y = np.meshgrid(g, g)
    return x, y


NMS20 = [(n, m) for n in range(21) for m in range(-n, n + 1, 2)]


def test_1024_against_the_numpy_walk():
    """1024^2 points are exactly the projection's cap of 1024 workgroups of 1024 points, so every workgroup's loop runs once here; the
    strided case lives in tests/test_gpu_modal_scale.py."""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials import zernike as Z
    from prysm_amd.polynomials.zernike_plan import evaluate, plan
    x, y = _grid(1024)
    xs, ys = x[::37], y[::37]                         # the numpy walk on every 37th row (the whole basis is 1.9 GB)
    want = evaluate(plan(NMS20), xs, ys, len(NMS20))
    r, t = np.hypot(x, y), np.arctan2(y, x)
    got = Z._seq(NMS20, x, y, True, _code(False))
    assert _rel_per_mode(tonp(got[:, ::37]), want) < 1e-12
    gotp = Z._seq(NMS20, r, t, True, _code(True))
    assert _rel_per_mode(tonp(gotp[:, ::37]), want) < 1e-12
    del gotp
    c = np.random.default_rng(3).standard_normal(len(NMS20))
    s = tonp(P.zernike_sum(c, NMS20, x, y))
    assert _rel(s[::37], np.tensordot(c, want, axes=(0, 0))) < 1e-12
    # the matrix-free adjoint equals the adjoint over the stored basis
    gbar = np.random.default_rng(4).standard_normal(x.shape)
    a1 = tonp(P.zernike_sum_adjoint(gbar, NMS20, x, y))
    a2 = tonp(P.sum_of_2d_modes_adjoint(got, gbar))
    assert _rel(a1, a2) < 1e-12
    got32 = tonp(Z._seq(NMS20, x.astype(np.float32), y.astype(np.float32), True, _code(False))[:, ::37])
    assert _rel_per_mode(got32.astype(np.float64), want) < 2e-5


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_stacks_equal_single_calls(dt):
    from prysm_amd import polynomials as P
    x, y = _grid(96, dt)
    x, y = x[:, :90], y[:, :90]                       # 96 x 90 points
    nms = [(n, m) for n in range(9) for m in range(-n, n + 1, 2)]
    rng = np.random.default_rng(5)
    C = rng.standard_normal((11, len(nms))).astype(dt)    # 11 = 8 + 2 + 1 vectors per walk
    S = tonp(P.zernike_sum(C, nms, x, y))
    assert S.shape == (11, 96, 90)
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(11):
        assert _rel(S[b], tonp(P.zernike_sum(C[b], nms, x, y))) < tol
    G = rng.standard_normal((11, 96, 90)).astype(dt)
    A = tonp(P.zernike_sum_adjoint(G, nms, x, y))
    assert A.shape == (11, len(nms))
    for b in range(11):
        assert _rel(A[b], tonp(P.zernike_sum_adjoint(G[b], nms, x, y))) < tol


def _stack_of_15(dt, npts, nms):
    from prysm_amd import polynomials as P
    rng = np.random.default_rng(15)
    x, y = (rng.uniform(-0.7, 0.7, npts).astype(dt) for _ in range(2))
    C = rng.standard_normal((15, len(nms))).astype(dt)
    S = tonp(P.zernike_sum(C, nms, x, y))
    assert S.shape == (15, npts) and S.dtype == dt
    tol = 1e-14 if dt == np.float64 else 1e-6
    for b in range(15):
        assert _rel(S[b], tonp(P.zernike_sum(C[b], nms, x, y))) < tol
    G = rng.standard_normal((15, npts)).astype(dt)
    A = tonp(P.zernike_sum_adjoint(G, nms, x, y))
    assert A.shape == (15, len(nms)) and A.dtype == dt
    for b in range(15):
        assert _rel(A[b], tonp(P.zernike_sum_adjoint(G[b], nms, x, y))) < tol


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('npts', [1024, 1027])
def test_a_stack_of_15_equals_single_calls(dt, npts):
    """15 = 8 + 4 + 2 + 1 vectors per walk, each piece at its own offset into the coefficients, the output and the partials; 1024 points
    take the 16-byte path, 1027 the element-wise one"""
    _stack_of_15(dt, npts, [(n, m) for n in range(4) for m in range(-n, n + 1, 2)])


def test_a_stack_of_15_with_two_vectors_per_projection_walk():
    """630 modes in fp64: the accumulators of a projection workgroup (64 KiB) hold two vectors of them, not four, so the 15 go as seven
    pairs and a single one"""
    _stack_of_15(np.float64, 1027, [(n, m) for n in range(35) for m in range(-n, n + 1, 2)])


def test_odd_point_counts_and_views():
    """point counts that are not a multiple of 4 and coordinates that start off a 16-byte boundary take the element-wise path"""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials.zernike_plan import evaluate, plan
    nms = [(n, m) for n in range(7) for m in range(-n, n + 1, 2)]
    x, y = _grid(64)
    xt, yt = torch.from_numpy(x).cuda().reshape(-1), torch.from_numpy(y).cuda().reshape(-1)
    for lo, hi in ((0, 4093), (1, 4001), (3, 4096)):
        xs, ys = xt[lo:hi], yt[lo:hi]
        want = evaluate(plan(nms), tonp(xs), tonp(ys), len(nms))
        c = np.linspace(-1, 1, len(nms))
        assert _rel(tonp(P.zernike_sum(c, nms, xs, ys)), np.tensordot(c, want, axes=(0, 0))) < 1e-12
        g = np.cos(np.arange(hi - lo))
        assert _rel(tonp(P.zernike_sum_adjoint(g, nms, xs, ys)), want @ g) < 1e-12
        basis = torch.from_numpy(want).cuda()
        assert _rel(tonp(P.sum_of_2d_modes_adjoint(basis[:, 1:], g[1:])), want[:, 1:] @ g[1:]) < 1e-12


def test_dot_product_identities():
    from prysm_amd import polynomials as P
    x, y = _grid(256)
    nms = [(n, m) for n in range(11) for m in range(-n, n + 1, 2)]
    rng = np.random.default_rng(6)
    c = rng.standard_normal(len(nms))
    g = rng.standard_normal(x.shape)
    lhs = float(np.vdot(tonp(P.zernike_sum(c, nms, x, y)), g))
    rhs = float(np.vdot(c, tonp(P.zernike_sum_adjoint(g, nms, x, y))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12
    modes = P.zernike_nm_seq(nms, np.hypot(x, y), np.arctan2(y, x))
    lhs = float(np.vdot(tonp(P.sum_of_2d_modes(modes, c)), g))
    rhs = float(np.vdot(c, tonp(P.sum_of_2d_modes_adjoint(modes, g))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12


def test_adjoints_are_bitwise_reproducible():
    from prysm_amd import polynomials as P
    x, y = _grid(512)
    nms = [(n, m) for n in range(13) for m in range(-n, n + 1, 2)]
    g = torch.from_numpy(np.random.default_rng(7).standard_normal((3, 512, 512))).cuda()
    a = P.zernike_sum_adjoint(g, nms, x, y).clone()
    b = P.zernike_sum_adjoint(g, nms, x, y).clone()
    assert torch.equal(a, b)
    modes = P.zernike_nm_seq(nms, np.hypot(x, y), np.arctan2(y, x))
    a = P.sum_of_2d_modes_adjoint(modes, g[0]).clone()
    b = P.sum_of_2d_modes_adjoint(modes, g[0]).clone()
    assert torch.equal(a, b)


EFL, WVL, DX, Q = 100.0, 0.6328, 10.0 / 128, 2
NMS6 = [(n, m) for n in range(7) for m in range(-n, n + 1, 2)]


def _model(amp, x, y, target):
    """loss and its gradient with respect to the Zernike coefficients, all on the device"""
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront

    def run(c):
        opd = P.zernike_sum(c, NMS6, x, y)
        wf = Wavefront.from_amp_and_phase(amp, opd, WVL, DX)
        psf = wf.focus(EFL, Q=Q)
        I = psf.intensity.data
        diff = I - target
        loss = (diff * diff).sum()
        wbar = psf.intensity_adjoint(2 * diff).focus_adjoint(EFL, Q=Q)
        obar = wf.from_amp_and_phase_adjoint_phase(wbar).imag    # the reference's quirk: the gradient times 1j
        return loss, P.zernike_sum_adjoint(obar, NMS6, x, y)
    return run


def _setup():
    x, y = _grid(128)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    amp = (xt * xt + yt * yt <= 1).to(torch.float64)
    rng = np.random.default_rng(8)
    c_true = torch.from_numpy(30 * rng.standard_normal(len(NMS6))).cuda()
    c0 = torch.from_numpy(30 * rng.standard_normal(len(NMS6))).cuda()
    from prysm_amd import polynomials as P
    from prysm_amd.propagation import Wavefront
    target = Wavefront.from_amp_and_phase(amp, P.zernike_sum(c_true, NMS6, xt, yt), WVL, DX).focus(EFL, Q=Q).intensity.data.clone()
    return amp, xt, yt, target, c0


def test_psf_loss_gradient_matches_finite_differences():
    amp, x, y, target, c0 = _setup()
    run = _model(amp, x, y, target)
    loss, grad = run(c0)
    grad = tonp(grad)
    h = 1e-2
    for k in (1, 4, 12):
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
    # the coefficients are read on the device: a replay with new ones gives the eager answer for them
    c1 = c0 * 0.5
    eager1 = run(c1)[1].clone()
    assert torch.equal(model(c1)[1], eager1)
    assert not torch.equal(eager1, eager_grad)
