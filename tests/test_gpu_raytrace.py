"""GPU: pm_rt_trace through prysm_amd.x.raytracing, against the reference's stored traces (tests/golden/raytrace.npz), against the
numpy model on rays the fixture does not hold (partial wavefronts and blocks), and against itself (without history, strided rays,
repeated runs, a captured trace); the ray generators and the two analyses against the fixture.  Bounds: tests/raytrace_common.py."""
import warnings

import numpy as np
import pytest
import torch

import raytrace_common as RC
from gpu_common import tonp
from prysm_amd.x import raytrace_plan as plan

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope='module')
def RT(pa):
    from prysm_amd.x import raytracing
    return raytracing


def _surfaces(case):
    from prysm_amd.x.raytracing import surfaces as SF
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        surfs = RC.build(case, SF)
        for s in surfs:
            s.departure_band()
    return surfs


def _unpack(res):
    return tonp(res.P), tonp(res.S), tonp(res.OPL), tonp(res.status_record.surface), tonp(res.status_record.code)


@pytest.mark.parametrize('case', list(RC.CASES))
@pytest.mark.parametrize('dt', DTYPES)
def test_fixture_cases(RT, case, dt):
    g = RC.golden()
    res = RT.raytrace(_surfaces(case), g[case + '_P0'].astype(dt), g[case + '_S0'].astype(dt), RC.WVL)
    P, S, OPL, surface, code = _unpack(res)
    assert surface.dtype == np.int32 and code.dtype == np.int32
    RC.check_trace(case, dt, P, S, OPL, surface, code)
    want = RC.model(case, dt)      # informational: the model in the same precision on the whole bundle
    bit_equal = all(np.array_equal(a, b, equal_nan=True) for a, b in zip((P, S, OPL, surface, code), want))
    print(f'{case} {np.dtype(dt).name}: bit-equal to the model in the same precision: {bit_equal}')
    status = tonp(res.status)
    assert status.dtype == np.complex128 and np.array_equal(status.real, surface) and np.array_equal(status.imag, code)
    # the quirk of the NaN launch: OK by its code, rejected by valid_mask with the positions
    if case == 'C':
        assert code[-2] == plan.OK and not bool(RT.valid_mask(res.status, res.P[-1])[-2]) and bool(RT.valid_mask(res.status)[-2])


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('N', [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks_against_the_model(RT, dt, N):
    """bundles of sizes the fixture does not hold, drawn from the grids of A and D: the same statuses as the model in the same precision, and
    the fixture's bounds on the deviation from the float64 model"""
    g = RC.golden()
    rng = np.random.default_rng(N)
    for case in ('A', 'D'):
        pick = rng.choice(g[case + '_P0'].shape[0], N, replace=False)
        P0, S0 = g[case + '_P0'][pick], g[case + '_S0'][pick]
        tab, n0 = RC.table(case)
        want = plan.trace(tab, n0, plan.resolve_tol_sag(None, dt), P0.astype(dt), S0.astype(dt))
        want64 = want if dt == np.float64 else plan.trace(tab, n0, plan.resolve_tol_sag(None, np.float64), P0, S0)
        got = _unpack(RT.raytrace(_surfaces(case), P0.astype(dt), S0.astype(dt), RC.WVL))
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), (case, N, np.flatnonzero(got[4] != want[4]))
        same = (got[3] == want64[3]) & (got[4] == want64[4])      # in float32: the rays it decides as the float64 model does
        bit_equal = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[:3], want[:3]))
        print(f'{case} N={N} {np.dtype(dt).name}: bit-equal to the model in the same precision: {bit_equal}')
        for q, a, b in zip(RC.QUANTITIES, got[:3], want64[:3]):
            dev, same_nan = RC.deviations(a, b, same)
            print(f'{case} N={N} {q} {np.dtype(dt).name}: deviation {dev:.2e}, bound {RC.bound(case, q, dt):.2e}')
            assert same_nan and dev <= RC.bound(case, q, dt), (case, N, q, dev)


@pytest.mark.parametrize('dt', DTYPES)
def test_without_history_is_the_last_row(RT, dt):
    g = RC.golden()
    for case in ('A', 'D', 'E'):
        surfs = _surfaces(case)
        P0, S0 = g[case + '_P0'].astype(dt), g[case + '_S0'].astype(dt)
        full, last = RT.raytrace(surfs, P0, S0, RC.WVL), RT.raytrace(surfs, P0, S0, RC.WVL, history=False)
        assert last.P.shape == P0.shape and last.OPL.shape == P0.shape[:1]
        assert torch.equal(torch.view_as_real(last.status), torch.view_as_real(full.status))
        for a, b in ((last.P, full.P[-1]), (last.S, full.S[-1])):
            assert np.array_equal(tonp(a), tonp(b), equal_nan=True)
        total = torch.zeros_like(full.OPL[0])
        for row in full.OPL[1:]:
            total = total + row
        assert np.array_equal(tonp(last.OPL), tonp(total), equal_nan=True)


def test_no_surfaces_and_no_rays(RT):
    g = RC.golden()
    P0, S0 = g['B_P0'], g['B_S0']
    res = RT.raytrace([], P0, S0, RC.WVL)
    assert res.P.shape == (1,) + P0.shape and np.array_equal(tonp(res.P[0]), P0) and np.array_equal(tonp(res.S[0]), S0)
    assert res.OPL.shape == (1, P0.shape[0]) and not tonp(res.OPL).any() and not tonp(res.status).any() and res.status.shape == (P0.shape[0],)
    res = RT.raytrace([], P0, S0, RC.WVL, history=False)
    assert np.array_equal(tonp(res.P), P0) and res.OPL.shape == (P0.shape[0],) and not tonp(res.OPL).any()
    surfs = _surfaces('B')
    res = RT.raytrace(surfs, P0[:0], S0[:0], RC.WVL)
    assert res.P.shape == (4, 0, 3) and res.S.shape == (4, 0, 3) and res.OPL.shape == (4, 0) and res.status.shape == (0,)
    res = RT.raytrace(surfs, P0[:0].astype(np.float32), S0[:0].astype(np.float32), RC.WVL, history=False)
    assert res.P.shape == (0, 3) and res.OPL.shape == (0,) and res.P.dtype == torch.float32


def test_single_ray_integers_and_tol_sag(RT):
    surfs = _surfaces('A')
    res = RT.raytrace(surfs, [0, 1, 0], [0, 0, 1], RC.WVL)        # integers: cast to the configured precision; one ray: squeezed
    assert res.P.shape == (7, 3) and res.S.shape == (7, 3) and res.OPL.shape == (7,) and res.status.shape == (1,) and res.P.dtype == torch.float64
    assert RT.decode_status(res.status)[0] == 'OK' and res.status_record.surface.tolist() == [6]
    batch = RT.raytrace(surfs, np.array([[0.0, 1.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]), RC.WVL)
    assert torch.equal(batch.P[:, 0], res.P) and torch.equal(batch.OPL[:, 0], res.OPL)
    # a tol_sag argument overrides the default: with a coarse one Newton stops earlier and lands within it
    coarse = RT.raytrace(surfs, np.array([[0.0, 5.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]), RC.WVL, tol_sag=1e-3)
    fine = RT.raytrace(surfs, np.array([[0.0, 5.0, 0.0]]), np.array([[0.0, 0.0, 1.0]]), RC.WVL)
    d = float(torch.max(torch.abs(coarse.P[3] - fine.P[3])))
    assert 0 < d < 2e-3


def test_strided_rays_and_repeated_runs(RT):
    g = RC.golden()
    surfs = _surfaces('D')
    P0, S0 = torch.from_numpy(g['D_P0']).cuda(), torch.from_numpy(g['D_S0']).cuda()
    wide = torch.zeros((P0.shape[0], 2, 6), dtype=torch.float64, device='cuda')
    wide[:, 0, ::2], wide[:, 1, 1::2] = P0, S0
    Pv, Sv = wide[:, 0, ::2], wide[:, 1, 1::2]
    assert not Pv.is_contiguous() and not Sv.is_contiguous()
    a, b, c = RT.raytrace(surfs, P0, S0, RC.WVL), RT.raytrace(surfs, Pv, Sv, RC.WVL), RT.raytrace(surfs, P0, S0, RC.WVL)
    for other in (b, c):
        for x, y in ((a.P, other.P), (a.S, other.S), (a.OPL, other.OPL)):
            assert np.array_equal(tonp(x), tonp(y), equal_nan=True)
        assert torch.equal(torch.view_as_real(a.status), torch.view_as_real(other.status))


def test_captured_prescription_trace(RT):
    from prysm_amd import graph
    g = RC.golden()
    rx = RT.prepare(_surfaces('A'), RC.WVL, dtype=np.float64)
    assert rx.table.is_cuda and rx.table.shape == (6, plan.REC) and len(rx) == 6
    P, S = torch.from_numpy(g['A_P0']).cuda(), torch.from_numpy(g['A_S0']).cuda()

    def run():
        r = RT.raytrace(rx, P, S, RC.WVL)
        return r.P, r.S, r.OPL, r.status
    model = graph.capture(run)
    shifted = g['A_P0'] + np.array([0.5, 0.0, 0.0])
    P.copy_(torch.from_numpy(shifted))
    out = [t.clone() for t in model()]
    torch.cuda.synchronize()
    eager = RT.raytrace(rx, shifted, g['A_S0'], RC.WVL)
    for got, want in zip(out[:3], (eager.P, eager.S, eager.OPL)):
        assert np.array_equal(tonp(got), tonp(want), equal_nan=True)
    assert torch.equal(torch.view_as_real(out[3]), torch.view_as_real(eager.status))
    assert not np.array_equal(tonp(out[0][-1]), g['A_P'][-1], equal_nan=True)      # the replay traced the shifted rays, not the captured ones
    # the same prescription serves float32 rays
    r32 = RT.raytrace(rx, g['A_P0'].astype(np.float32), g['A_S0'].astype(np.float32), RC.WVL)
    assert r32.P.dtype == torch.float32


def test_ray_generators_and_analyses(RT):
    g = RC.golden()
    for case in RC.CASES:
        P, S = RC.launch(case, RT.raygen)
        assert P.is_cuda and S.is_cuda and P.dtype == torch.float64
        assert np.allclose(tonp(P), g[f'gen_{case}_P'], rtol=0, atol=1e-13) and np.allclose(tonp(S), g[f'gen_{case}_S'], rtol=0, atol=1e-15)
    fan, _ = RT.generate_collimated_ray_fan(5, 2.0, azimuth=0)
    assert np.allclose(tonp(fan), np.stack([np.linspace(-2, 2, 5), np.zeros(5), np.zeros(5)], 1), atol=1e-15)
    Pa, Sa = RC.launch('A', RT.raygen)
    Pb, Sb = RC.launch('C', RT.raygen)
    Pc, Sc = RT.concat_rayfans((Pa, Sa), (Pb, Sb))
    assert Pc.shape == (1089 + 41, 3)
    ps, ss = RT.split_rayfans(Pc, [1089, 41], Sc)
    assert torch.equal(ps[1], Pb) and torch.equal(ss[0], Sa)
    with pytest.raises(ValueError):
        RT.split_rayfans(Pc, [3, 4])
    res = RT.raytrace(_surfaces('A'), g['A_P0'], g['A_S0'], RC.WVL)
    x, y = RT.spot_positions(res.P[-1], res.status, origin='centroid')
    pupil, delta = RT.transverse_ray_aberration(res.P, axis='y', status=res.status, reference='centroid')
    b = RC.f64_bound('A', 'P')
    for got, want in ((x, g['A_spot_x']), (y, g['A_spot_y']), (pupil, g['A_tra_pupil']), (delta, g['A_tra_delta'])):
        assert got.is_cuda and got.shape == want.shape and np.max(np.abs(tonp(got) - want)) <= 2 * b
