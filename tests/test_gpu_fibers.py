"""GPU: csrc/fibers.hip through prysm_amd.x.fibers, in both precisions: the modes against the reference's stored stacks
(tests/golden/fibers.npz) and the numpy model, sum and project against modes() contracted in torch, coupling and the overlap against
the fixture, and project / overlap against themselves (two runs, replays of a captured graph).  Sizes are the smallest that reach each
path: 33 x 31 = 1023 points (a wave-tile tail, not a multiple of 4), 64 x 64 (four whole workgroup tiles), a one-element-offset view
(the unaligned path), a single point at r = 0; mode sets of 1, 3 and 38 modes and the l = 25 modes of V = 30 (Miller's recurrence,
underflowing in float32).  Bounds: tests/fibers_common.py."""
import numpy as np
import pytest
import torch

import fibers_common as FC
from gpu_common import tonp
from prysm_amd.x import fibers_plan as plan

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope='module')
def FB(pa):
    from prysm_amd.x import fibers
    return fibers


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set(FB, case, gname, dt):
    r, t = FC.grid(gname, dt)
    return FB.prepare(FC.CASES[case][0], FC.mode_dict(case), FC.A, r, t), r, t


def _model(case, dt, r, t):
    table, n = plan.mode_table(FC.CASES[case][0], FC.mode_dict(case), dt)
    return plan.walk(table, n, FC.A, r, t)


def _against_model(case, dt, got, want, label):
    """the GPU kernel against the numpy model in the same precision: the mode bound"""
    V = FC.CASES[case][0]
    got, want = got.reshape(len(want), -1).astype(np.float64), want.reshape(len(want), -1).astype(np.float64)
    dev_, bound = np.max(np.abs(got - want), axis=1), FC.mode_bound(V, dt, want)
    print(f'{label} {case} {np.dtype(dt).name}: worst deviation from the model / bound {np.max(dev_ / bound):.3f}, '
          f'bit-equal {np.array_equal(got, want)}')
    assert np.all(dev_ <= bound), (case, np.argmax(dev_ / bound), np.max(dev_ / bound))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', list(FC.CASES))
def test_modes_on_1023_points(FB, case, dt):
    ms, r, t = _set(FB, case, 'g33', dt)
    got = tonp(ms.modes())
    assert got.dtype == dt and got.shape == (ms.nmodes, 33, 31)
    FC.check_modes(case, 'g33', dt, got, 'gpu ')
    _against_model(case, dt, got, _model(case, dt, r, t), 'g33')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', ['V5.5', 'V12', 'V30s'])
def test_modes_on_the_vector_path_with_a_partial_tile(FB, case, dt):
    ms, r, t = _set(FB, case, 'g48', dt)          # 1920 points: 16-byte stores, the second workgroup's last wave idle
    FC.check_modes(case, 'g48', dt, tonp(ms.modes()), 'gpu ')


@pytest.mark.parametrize('dt', DTYPES)
def test_modes_on_four_whole_tiles_and_dict_structure(FB, dt):
    yv = (np.arange(64) - 32) * 0.25
    x, y = np.meshgrid(yv, yv)
    r, t = np.sqrt(x * x + y * y).astype(dt), np.arctan2(y, x).astype(dt)
    assert (r == 0).any() and (r == FC.A).any()
    md = FC.mode_dict('V3.9')
    modes = FB.compute_LP_modes(3.9, md, FC.A, r, t)
    assert list(modes) == list(md) and [len(v) for v in modes.values()] == [len(b) for b in md.values()]
    got = np.array([tonp(m) for ms in modes.values() for m in ms])
    table, n = plan.mode_table(3.9, md, dt)
    _against_model('V3.9', dt, got, plan.walk(table, n, FC.A, r, t), '64x64')
    at_a = got.reshape(n, -1)[:, ((r == FC.A) & (y == 0)).ravel()]
    cosines = [k for k, (l, _) in enumerate(plan.mode_slots(md)) if l >= 0]
    # the core's side of r == a, J_l(U) / J_l(U) at t = 0, pi: the bound on J_l (8 eps max(1, x)) times the normaliser, and its roundings
    one = (8 * 3.9 * np.max(np.abs(table['invJ'])) + 2 + 4 * 2) * FC.eps(dt)          # ... and cos(2 pi) by two rotations
    assert np.all(np.abs(np.abs(at_a[cosines]) - 1) <= one)


@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_view_single_point_and_one_mode(FB, dt):
    r, t = FC.grid('g33', dt)
    md = FC.mode_dict('V12')
    aligned = FB.prepare(12.0, md, FC.A, r, t).modes()
    rb, tb = torch.zeros(r.size + 1, dtype=aligned.dtype, device='cuda'), torch.zeros(r.size + 1, dtype=aligned.dtype, device='cuda')
    rb[1:].copy_(dev(r.ravel()))
    tb[1:].copy_(dev(t.ravel()))
    assert rb[1:].data_ptr() % 16 != 0
    off = FB.prepare(12.0, md, FC.A, rb[1:], tb[1:])
    assert torch.equal(off.modes().reshape(aligned.shape), aligned)          # the scalar path: the same arithmetic
    g = dev(np.random.default_rng(3).standard_normal(r.size).astype(dt))
    assert torch.equal(off.project(g), FB.prepare(12.0, md, FC.A, r.ravel(), t.ravel()).project(g))
    # one point at r = 0: 1 / J_0(U) for l = 0, exactly 0 for the others
    one = tonp(FB.prepare(12.0, md, FC.A, np.zeros(1, dt), np.zeros(1, dt)).modes())[:, 0]
    table, n = plan.mode_table(12.0, md, dt)
    want = plan.walk(table, n, FC.A, np.zeros(1, dt), np.zeros(1, dt))[:, 0]
    ls = np.array([l for l, _ in plan.mode_slots(md)])
    assert np.all(one[ls != 0] == 0) and np.all(np.abs(one - want) <= 4 * FC.eps(dt) * np.abs(want))
    # a set of one mode (V = 2: single-mode)
    md1 = plan.find_all_modes(2.0)
    ms1 = FB.prepare(2.0, md1, FC.A, r, t)
    assert ms1.nmodes == 1
    table, n = plan.mode_table(2.0, md1, dt)
    want = plan.walk(table, n, FC.A, r, t).astype(np.float64)
    assert np.max(np.abs(tonp(ms1.modes()) - want)) <= 16 * 3 * FC.eps(dt) * np.max(np.abs(want))
    g2 = dev(np.stack([FC.incident('g33', dt).real, FC.incident('g33', dt).imag]).astype(dt))
    assert tuple(ms1.project(g2).shape) == (2, 1)


@pytest.mark.parametrize('dt', DTYPES)
def test_miller_branch_underflows_in_float32(FB, dt):
    """x = U r / a < 0.15 and l = 25: J_25(x) < 1e-52, far below float32's smallest denormal, on the backward recurrence and on the leading
    term; x up to 14 stays on the backward recurrence (x <= l) with values float32 holds"""
    r = np.array([1e-3, 0.01, 0.02, 0.04, 0.3, 1.0, 2.0], dtype=dt)
    t = np.full(r.shape, 0.3, dtype=dt)
    md = FC.mode_dict('V30s')
    got = tonp(FB.prepare(30.0, md, FC.A, r, t).modes())
    table, n = plan.mode_table(30.0, md, dt)
    want = plan.walk(table, n, FC.A, r, t)
    k25 = [k for k, (l, _) in enumerate(plan.mode_slots(md)) if abs(l) == 25]
    assert np.all(np.isfinite(got))
    _against_model('V30s', dt, got, want, 'small radii')
    if dt == np.float32:
        assert np.all(got[k25][:, :3] == 0) and np.all(want[k25][:, :3] == 0) and np.all(got[k25][:, 4:] != 0)
    else:
        assert np.all(got[k25] != 0) and np.all(np.abs(got[k25] - want[k25]) <= 1e-9 * np.abs(want[k25]))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', ['V2.41', 'V12'])
def test_sum_and_project_against_the_contracted_modes(FB, case, dt):
    ms, r, t = _set(FB, case, 'g33', dt)
    K, npts, e = ms.nmodes, r.size, FC.eps(dt)
    m64 = ms.modes().reshape(K, -1).double()
    rng = np.random.default_rng(11)
    for B in (1, 3, 9):                           # 1; 2 + 1; 8 + 1 vectors per launch
        c = rng.standard_normal((B, K)).astype(dt)
        got = ms.sum(dev(c)).reshape(B, -1).double()
        want = dev(c).double() @ m64
        bound = 2 * K * e * (dev(np.abs(c)).double() @ m64.abs())
        assert bool(torch.all((got - want).abs() <= bound + 1e-300)), (B, float(((got - want).abs() / (bound + 1e-300)).max()))
    single = ms.sum(dev(c[0]))
    assert single.shape == r.shape and torch.equal(single.reshape(-1), ms.sum(dev(c[:1])).reshape(-1))
    cc = (rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64 if dt == np.float32 else np.complex128)
    field = ms.sum(dev(cc))
    assert field.is_complex() and field.shape == r.shape
    assert torch.equal(field.real, ms.sum(dev(cc.real.copy()))) and torch.equal(field.imag, ms.sum(dev(cc.imag.copy())))
    # accumulate: out += the sum
    base = dev(rng.standard_normal(r.shape).astype(dt))
    out = base.clone()
    assert ms.sum(dev(c[0]), out=out, accumulate=True) is out and torch.equal(out, single + base)
    # project: real vectors, a stack of them, a complex field
    for B in (1, 3, 9):
        g = rng.standard_normal((B, *r.shape)).astype(dt)
        got = ms.project(dev(g)).double()
        gd = dev(g).reshape(B, -1).double()
        want = gd @ m64.T
        bound = 4 * npts * e * (gd.abs() @ m64.abs().T)
        assert got.shape == (B, K) and bool(torch.all((got - want).abs() <= bound)), (B, float(((got - want).abs() / bound).max()))
        for b in range(B):                        # a stack gives what its members give one at a time
            assert bool(torch.all((ms.project(dev(g[b])).double() - got[b]).abs() <= bound[b]))
    E = dev(FC.incident('g33', dt))
    pe = ms.project(E)
    assert pe.is_complex() and torch.equal(pe.real, ms.project(E.real.contiguous())) and torch.equal(pe.imag, ms.project(E.imag.contiguous()))
    norms = ms.norms().double()
    want = (m64 * m64).sum(dim=1)
    assert bool(torch.all((norms - want).abs() <= 4 * npts * e * want))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('gname', FC.GRIDS)
@pytest.mark.parametrize('case', list(FC.CASES))
def test_coupling_against_the_reference(FB, case, gname, dt):
    ms, r, t = _set(FB, case, gname, dt)
    E = FC.incident(gname, dt)
    ref = FC.golden()[f'{case}_{gname}_eta{FC.suffix(dt)}']
    bound = FC.coupling_bound(FC.CASES[case][0], dt, r.size)
    eta = ms.coupling(dev(E))
    assert eta.is_cuda and eta.dtype == ms.dtype
    d = np.max(np.abs(tonp(eta).astype(np.float64) - ref))
    print(f'coupling {case} {gname} {np.dtype(dt).name}: deviation {d:.3e}, bound {bound:.3e}')
    assert d <= bound
    as_dict = FB.multimode_coupling(dev(E), ms)
    assert list(as_dict) == list(ms.mode_dict) and torch.equal(torch.stack([v for vs in as_dict.values() for v in vs]), eta)
    if case == 'V5.5':
        stack = ms.coupling(dev(np.stack([E, 0.5j * E, E.conj()])))         # a (B, ...) stack of incident fields
        assert tuple(stack.shape) == (3, ms.nmodes)
        assert np.max(np.abs(tonp(stack[:2]).astype(np.float64) - ref)) <= bound
        assert np.max(np.abs(tonp(stack[2]) - tonp(ms.coupling(dev(E.conj().copy()))))) <= bound
        stored = FB.multimode_coupling(dev(E), FB.compute_LP_modes(5.5, ms.mode_dict, FC.A, r, t))      # the reference's stored form
        flat = np.array([float(v) for vs in stored.values() for v in vs])
        assert list(stored) == list(ms.mode_dict) and np.max(np.abs(flat - ref)) <= bound


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('gname', FC.GRIDS)
def test_overlap_and_smf_mode_field(FB, gname, dt):
    g = FC.golden()
    r, _ = FC.grid(gname, dt)
    E1, E2 = FC.incident(gname, dt), FC.second_field(gname, dt)
    ref = float(g[f'overlap_{gname}_{FC.suffix(dt)}'])
    bound = 4 * r.size * FC.eps(dt)
    res = tonp(FB.overlap(dev(E1), dev(E2))).astype(np.float64)
    want = plan.overlap(E1.astype(np.complex128), E2.astype(np.complex128))
    print(f'overlap {gname} {np.dtype(dt).name}: eta deviation {abs(res[4] - ref):.3e}, bound {bound:.3e}')
    assert abs(res[4] - ref) <= bound and np.all(np.abs(res[:4] - want[:4]) <= bound * np.sqrt(want[2] * want[3]))
    eta = FB.mode_overlap_integral(dev(E1), dev(E2))
    assert eta.is_cuda and eta.dim() == 0 and abs(float(eta) - ref) <= bound
    pre = FB.mode_overlap_integral(dev(E1), None, E2conj=dev(E2.conj().copy()), I2sum=float(want[3]))
    assert abs(float(pre) - ref) <= bound
    # a real field against a complex one, and a field against itself
    rr = tonp(FB.overlap(dev(np.abs(E1).astype(dt)), dev(E2))).astype(np.float64)
    wr = plan.overlap(np.abs(E1).astype(dt).astype(np.float64), E2.astype(np.complex128))
    assert abs(rr[4] - wr[4]) <= bound and abs(float(FB.mode_overlap_integral(dev(E1), dev(E1))) - 1) <= bound
    field = tonp(FB.smf_mode_field(FC.SMF_V, FC.A, float(g['smf_b']), r)).astype(np.float64)
    sref = g[f'smf_{gname}_field'] + (g[f'smf_{gname}_delta32'] if dt == np.float32 else 0)
    assert field.shape == r.shape and np.max(np.abs(field - sref)) <= FC.mode_bound(FC.SMF_V, dt, sref.reshape(1, -1))[0]


@pytest.mark.parametrize('dt', DTYPES)
def test_project_and_overlap_are_reproducible_and_capturable(FB, dt):
    from prysm_amd import graph
    ms, r, t = _set(FB, 'V12', 'g48', dt)
    E, E2 = dev(FC.incident('g48', dt)), dev(FC.second_field('g48', dt))

    def run(e):
        return ms.project(e), ms.coupling(e), FB.overlap(e, E2)
    first = [v.clone() for v in run(E)]
    again = run(E)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    model = graph.capture(run, E)
    for _ in range(3):
        out = model(E)
        assert all(torch.equal(a, b) for a, b in zip(first, out))
    other = [v.clone() for v in run(E2)]             # the replay reads its input on the device
    assert all(torch.equal(a, b) for a, b in zip(other, model(E2)))
    torch.cuda.synchronize()
