"""GPU: prysm_amd.segmented -- compose_opd against the reference fixture in both precisions on both routes (the Zernike table walk and
a stored basis), out= accumulation, share_grids=False against the numpy model of the plan, the two routes against each other, the
adjoint against the fixture and the dot-product identity, stacks, bitwise reproducibility, graph replay with coefficients updated in
place, and the gradient of a PSF loss back to the segment coefficients against finite differences."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_common import tonp

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 2e-5}
monomials = lambda orders, x, y: [x ** a * y ** b for a, b in orders]  # noqa: E731


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'segmented.npz'))


def _rel(got, ref):
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def build(fx, i, dtype=np.float64, share_grids=True):
    from prysm_amd import segmented as SG
    p = f'c{i}_'
    x, y = np.meshgrid(fx[p + 'xv'], fx[p + 'yv'])
    ap = SG.CompositeHexagonalAperture(x.astype(dtype), y.astype(dtype), int(fx[p + 'rings']), float(fx[p + 'sd']), float(fx[p + 'sep']),
                                       segment_angle=int(fx[p + 'angle']), exclude=tuple(int(v) for v in fx[p + 'exclude']),
                                       share_grids=share_grids)
    return ap, x


def prepared(fx, i, dtype=np.float64, share_grids=True):
    from prysm_amd.polynomials import zernike_nm_seq
    p = f'c{i}_'
    ap, x = build(fx, i, dtype, share_grids)
    if p + 'nms' in fx:
        ap.prepare_opd_bases(zernike_nm_seq, [tuple(int(v) for v in r) for r in fx[p + 'nms']])
    else:
        ap.prepare_opd_bases(monomials, [tuple(int(v) for v in r) for r in fx[p + 'orders']],
                             normalization_radius=tuple(float(v) for v in fx[p + 'nr']))
    return ap, x


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('i', [1, 2, 3, 4])
def test_compose_matches_the_reference(fx, i, dt):
    p = f'c{i}_'
    ap, x = prepared(fx, i, dt)
    sub = int(fx[p + 'sub'])
    coefs = fx[p + 'coefs']
    got = tonp(ap.compose_opd(coefs[0]))
    assert got.dtype == dt and got.shape == x.shape
    assert _rel(got[::sub, ::sub], fx[p + 'opd1']) < TOL[dt]
    base = np.random.default_rng(int(fx[p + 'seed_out'])).standard_normal(x.shape).astype(dt)
    out = torch.from_numpy(base.copy()).cuda()
    res = ap.compose_opd(torch.from_numpy(coefs[1]).cuda(), out=out)
    assert res is out
    assert _rel(tonp(out)[::sub, ::sub], fx[p + 'opd2']) < TOL[dt]
    # a numpy out is added to in place too
    hb = base.copy()
    assert ap.compose_opd(coefs[1], out=hb) is hb
    assert _rel(hb[::sub, ::sub], fx[p + 'opd2']) < TOL[dt]


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('i', [1, 2, 3, 4])
def test_adjoint_matches_the_reference(fx, i, dt):
    p = f'c{i}_'
    ap, x = prepared(fx, i, dt)
    g = np.random.default_rng(int(fx[p + 'seed_g'])).standard_normal(x.shape).astype(dt)
    got = tonp(ap.compose_opd_adjoint(g))
    assert got.dtype == dt and got.shape == fx[p + 'adj'].shape
    assert _rel(got, fx[p + 'adj']) < (1e-12 if dt == np.float64 else 1e-5)


@pytest.mark.parametrize('i', [1, 3])
def test_unshared_grids_match_the_numpy_model(fx, i):
    from prysm_amd import segmented as SG
    from prysm_amd.polynomials import zernike_plan as ZP
    p = f'c{i}_'
    ap, x = prepared(fx, i, share_grids=False)
    nms = [tuple(int(v) for v in r) for r in fx[p + 'nms']]
    table = ZP.plan(nms)
    nr = ap.vtov / 2
    bases = [ZP.evaluate(table, lx / nr, ly / nr, len(nms)) for lx, ly in ap.host_local_coords]
    coefs = fx[p + 'coefs'][0]
    ref = SG.evaluate_compose(ap.segment_plan, coefs, bases)
    assert _rel(tonp(ap.compose_opd(coefs)), ref) < 1e-12
    g = np.random.default_rng(5).standard_normal(x.shape)
    assert _rel(tonp(ap.compose_opd_adjoint(g)), SG.evaluate_project(ap.segment_plan, g, bases)) < 1e-12
    # the shared-grid result differs where a segment borrows another's local y
    shared, _ = prepared(fx, i)
    if shared.grid_sources != ap.grid_sources:
        assert not np.allclose(tonp(shared.compose_opd(coefs)), ref)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_routes_agree(fx, dt):
    ap, x = prepared(fx, 1, dt)
    nms = [tuple(int(v) for v in r) for r in fx['c1_nms']]
    from prysm_amd.polynomials import zernike_nm_seq
    twin, _ = build(fx, 1, dt)
    twin.prepare_opd_bases(lambda orders, r, t: zernike_nm_seq(orders, r, t), nms)     # not zernike_nm_seq itself: the stored route
    assert twin._route['kind'] != ap._route['kind'] and twin.grid_sources == ap.grid_sources
    # the lazily made bases of the matrix-free route are the stored ones
    for s in (0, 5, 17):
        assert _rel(tonp(ap.opd_bases[s]), tonp(twin.opd_bases[s])) < TOL[dt] * 10
    c = np.random.default_rng(9).standard_normal((3, len(ap.windows), len(nms)))
    tol = 1e-12 if dt == np.float64 else 5e-5
    assert _rel(tonp(ap.compose_opd(c)), tonp(twin.compose_opd(c))) < tol
    g = np.random.default_rng(10).standard_normal((3, *x.shape))
    assert _rel(tonp(ap.compose_opd_adjoint(g)), tonp(twin.compose_opd_adjoint(g))) < tol * 10


@pytest.mark.parametrize('i', [1, 4])
def test_dot_product_identity(fx, i):
    ap, x = prepared(fx, i)
    rng = np.random.default_rng(11)
    c = rng.standard_normal(fx[f'c{i}_coefs'][0].shape)
    g = rng.standard_normal(x.shape)
    lhs = float(np.vdot(tonp(ap.compose_opd(c)), g))
    rhs = float(np.vdot(c, tonp(ap.compose_opd_adjoint(g))))
    assert abs(lhs - rhs) / abs(lhs) < 1e-12


@pytest.mark.parametrize('i', [1, 4])
def test_stacks_equal_single_calls_and_adjoint_is_bitwise_reproducible(fx, i):
    ap, x = prepared(fx, i)
    S, K = fx[f'c{i}_coefs'].shape[1:]
    rng = np.random.default_rng(12)
    for B in (3, 11):                         # 11: a group of 8 and one of 2 and 1
        c = torch.from_numpy(rng.standard_normal((B, S, K))).cuda()
        st = ap.compose_opd(c)
        assert st.shape == (B, *x.shape)
        for b in (0, B - 1):
            assert torch.equal(st[b], ap.compose_opd(c[b]))
        g = torch.from_numpy(rng.standard_normal((B, *x.shape))).cuda()
        a = ap.compose_opd_adjoint(g).clone()
        assert a.shape == (B, S, K)
        assert torch.equal(a, ap.compose_opd_adjoint(g))
        for b in (0, B - 1):
            assert torch.allclose(a[b], ap.compose_opd_adjoint(g[b]), rtol=1e-13, atol=1e-13)


def _stack_of_15(dt, rows, cols, nms):
    from prysm_amd import segmented as SG
    from prysm_amd.polynomials import zernike_nm_seq
    x, y = np.meshgrid(np.linspace(-2.1, 2.1, cols), np.linspace(-2.1, 2.1, rows))
    ap = SG.CompositeHexagonalAperture(x.astype(dt), y.astype(dt), 1, 1.32, 0.05, segment_angle=90)
    ap.prepare_opd_bases(zernike_nm_seq, nms)
    S, K = len(ap.windows), len(nms)
    rng = np.random.default_rng(15)
    c = torch.from_numpy(rng.standard_normal((15, S, K)).astype(dt)).cuda()
    st = ap.compose_opd(c)
    assert st.shape == (15, rows, cols) and tonp(st).dtype == dt
    for b in range(15):
        assert torch.equal(st[b], ap.compose_opd(c[b]))
    g = torch.from_numpy(rng.standard_normal((15, rows, cols)).astype(dt)).cuda()
    a = ap.compose_opd_adjoint(g).clone()
    assert a.shape == (15, S, K)
    tol = 1e-13 if dt == np.float64 else 1e-5
    for b in range(15):
        assert torch.allclose(a[b], ap.compose_opd_adjoint(g[b]), rtol=tol, atol=tol)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(64, 64), (63, 65)])
def test_a_stack_of_15_equals_single_calls(dt, shape):
    """15 = 8 + 4 + 2 + 1 coefficient stacks per walk, each piece at its own offset into the coefficients, the output and the partials;
    64 x 64 points take the 16-byte path, 63 x 65 = 4095 the element-wise one"""
    _stack_of_15(dt, *shape, [(n, m) for n in range(4) for m in range(-n, n + 1, 2)])


def test_a_stack_of_15_with_two_stacks_per_projection_walk():
    """630 modes in fp64: the accumulators of a projection workgroup (64 KiB) hold two stacks' worth of them, not four, so the 15 go as
    seven pairs and a single one"""
    _stack_of_15(np.float64, 63, 65, [(n, m) for n in range(35) for m in range(-n, n + 1, 2)])


def test_graph_replay_reads_coefficients_on_the_device(fx):
    from prysm_amd import graph
    ap, x = prepared(fx, 1)
    S, K = fx['c1_coefs'].shape[1:]
    c = torch.from_numpy(fx['c1_coefs'][0]).cuda()
    eager = ap.compose_opd(c).clone()
    model = graph.capture(lambda cc: ap.compose_opd(cc), c)
    assert torch.equal(model(c), eager)
    c.mul_(-0.5).add_(0.25)                  # updated in place between replays
    eager2 = ap.compose_opd(c).clone()
    assert torch.equal(model(c), eager2) and not torch.equal(eager2, eager)


EFL, WVL, Q = 100.0, 0.6328, 2


def test_psf_loss_gradient_matches_finite_differences():
    from prysm_amd import segmented as SG
    from prysm_amd.polynomials import zernike_nm_seq, noll_to_nm
    from prysm_amd.propagation import Wavefront
    N = 256
    g1 = (np.arange(N) - N // 2) * (6.628 / N)
    x, y = np.meshgrid(g1, g1)
    ap = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
    nms = [noll_to_nm(j) for j in range(1, 7)]
    ap.prepare_opd_bases(zernike_nm_seq, nms)
    amp, dx = ap.amp, float(g1[1] - g1[0])
    rng = np.random.default_rng(13)
    S = len(ap.windows)
    c_true = torch.from_numpy(40 * rng.standard_normal((S, len(nms)))).cuda()
    c0 = torch.from_numpy(40 * rng.standard_normal((S, len(nms)))).cuda()
    target = Wavefront.from_amp_and_phase(amp, ap.compose_opd(c_true), WVL, dx).focus(EFL, Q=Q).intensity.data.clone()

    def run(c):
        wf = Wavefront.from_amp_and_phase(amp, ap.compose_opd(c), WVL, dx)
        psf = wf.focus(EFL, Q=Q)
        diff = psf.intensity.data - target
        loss = (diff * diff).sum()
        wbar = psf.intensity_adjoint(2 * diff).focus_adjoint(EFL, Q=Q)
        obar = wf.from_amp_and_phase_adjoint_phase(wbar).imag     # the reference's convention: the gradient times 1j
        return loss, ap.compose_opd_adjoint(obar)

    _, grad = run(c0)
    grad = tonp(grad)
    h = 1e-2
    for s, k in ((0, 0), (3, 1), (7, 2), (12, 4), (17, 5)):
        e = torch.zeros_like(c0)
        e[s, k] = h
        lp, _ = run(c0 + e)
        lm, _ = run(c0 - e)
        fd = (float(lp) - float(lm)) / (2 * h)
        assert abs(grad[s, k] - fd) / abs(fd) < 1e-6, (s, k, grad[s, k], fd)
