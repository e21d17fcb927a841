"""CPU: the host side of the ray trace -- the numpy model of pm_rt_trace (prysm_amd/x/raytrace_plan.py) against the reference's stored
traces (tests/golden/raytrace.npz), the surface table, the departure band and the pose helpers against the stored numbers, the host
layer's refusals, and the argument checks of pm_rt_trace at the C ABI (no device is touched).  Bounds: tests/raytrace_common.py."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import raytrace_common as RC
from prysm_amd.x import raytrace_plan as plan

DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize('case', list(RC.CASES))
@pytest.mark.parametrize('dt', DTYPES)
def test_model_against_the_fixture(case, dt):
    RC.check_trace(case, dt, *RC.model(case, dt))


def test_the_fixture_holds_what_the_cases_are_about():
    g = RC.golden()

    def count(case, surface, code):
        return int(np.sum((g[case + '_surface'] == surface) & (g[case + '_code'] == code)))
    assert (count('A', 6, plan.OK), count('A', 1, plan.CLIP)) == (592, 497)
    assert (count('B', 3, plan.OK), count('B', 1, plan.MISS)) == (221, 220)
    assert (count('D', 3, plan.OK), count('D', 1, plan.NEWTON), count('D', 1, plan.CLIP), count('D', 2, plan.TIR)) == (280, 531, 234, 44)
    assert (count('E', 5, plan.OK), count('E', 2, plan.CLIP), count('E', 3, plan.CLIP)) == (385, 389, 315)
    # the three rays appended to C: parallel to the plane is MISS there; a NaN position stays OK with NaN positions (valid_mask is what
    # rejects it); a plain ray
    assert count('C', 2, plan.TIR) == 12
    assert g['C_surface'][-3:].tolist() == [1, 3, 3] and g['C_code'][-3:].tolist() == [plan.MISS, plan.OK, plan.OK]
    assert np.all(np.isnan(g['C_P'][1:, -2, 0])) and np.all(np.isnan(g['C_P'][-1, -2])) and np.all(np.isfinite(g['C_P'][:, -1]))
    for case in RC.CASES:
        assert g[case + '_edge32'].size <= 0.01 * g[case + '_code'].size
    # the rescue is exercised: rays go to the Lipschitz march in D and D2, and some converge there
    stats = {}
    tab, n0 = RC.table('D')
    plan.trace(tab, n0, 1e-12, g['D_P0'], g['D_S0'], stats=stats)
    assert (stats['rescued'], stats['rescue_converged']) == RC.RESCUE['D'] and stats['rescue_converged'] > 0


def test_model_without_history_is_the_last_row_and_the_ordered_sum():
    for case in ('A', 'D'):
        P, S, OPL, surface, code = RC.model(case, np.float64)
        Pf, Sf, Of, sf, cf = RC.model(case, np.float64, False)
        assert np.array_equal(Pf, P[-1], equal_nan=True) and np.array_equal(Sf, S[-1], equal_nan=True)
        total = np.zeros_like(OPL[0])
        for row in OPL[1:]:
            total = total + row
        assert np.array_equal(Of, total, equal_nan=True) and np.array_equal(sf, surface) and np.array_equal(cf, code)


def test_table_round_trip():
    from prysm_amd.x.raytracing import surfaces as SF
    tab, n0 = RC.table('E')
    assert tab.shape == (5, plan.REC) and tab.dtype == np.float64 and n0 == 1.33
    recs = plan.unpack_table(tab)
    assert [r['interaction'] for r in recs] == [plan.MEASURE, plan.REFLECT, plan.REFLECT, plan.REFRACT, plan.MEASURE]
    assert [r['shape'] for r in recs] == [plan.PLANE, plan.CONIC, plan.CONIC, plan.CONIC, plan.PLANE]
    assert recs[1]['aperture'] == (plan.AP_ANNULAR, 0.0, 0.0, 8.0, 40.0) and recs[2]['aperture'] == (plan.AP_CIRCULAR, 0.0, 0.0, 0.0, 12.0)
    assert recs[0]['aperture'][0] == plan.AP_NONE and recs[3]['n_post'] == 1.45 and recs[0]['n_post'] == 1.33
    assert (recs[3]['c'], recs[3]['k'], recs[3]['dx'], recs[3]['dy']) == (1 / 300, -1.0, 3.0, -2.0)
    assert [r['first'] for r in recs] == [True, False, False, False, False] and all(r['analytic'] and r['band'] is None and r['R'] is None for r in recs)
    assert np.array_equal(recs[1]['P'], [0, 0, 150])
    tab, n0 = RC.table('A')
    recs = plan.unpack_table(tab)
    g = RC.golden()
    assert n0 == 1.0 and recs[2]['coefs'] == (1e-6, -2e-9, 1e-12) and not recs[2]['analytic'] and recs[2]['shape'] == plan.ASPHERE
    assert np.array_equal(recs[2]['band'], g['A_band'][2]) and np.array_equal(recs[3]['R'], g['A_pose_R'][3]) and np.array_equal(recs[3]['P'], g['A_pose_P'][3])
    assert recs[4]['n_post'] == 1.0      # a mirror has no material
    with pytest.raises(NotImplementedError, match='9 coefficients'):
        SF.EvenAsphere(0.01, 0.0, [1e-9] * 9)
    # a material is anything with .n(wvl)
    class Glass:
        def n(self, wvl):
            return 1.5 + 0.01 / wvl
    s = SF.Surface(SF.Plane(), 'refract', P=3, material=Glass())
    assert plan.pack_table([s], 0.5)[0, plan.REC_NPOST] == 1.52 and plan.pack_table([s], 1.0)[0, plan.REC_NPOST] == 1.51


def test_departure_bands_and_poses_against_the_stored_numbers():
    from prysm_amd.coordinates import apply_tilt_decenter, coerce_3d_rotation, make_rotation_matrix, promote_3d_point
    from prysm_amd.x.raytracing import surfaces as SF
    g = RC.golden()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for case in RC.CASES:
            for j, s in enumerate(RC.build(case, SF)):
                b, want = s.departure_band(), g[case + '_band'][j]
                if np.isnan(want[0]):
                    assert not b.bounded
                else:
                    assert b.bounded and np.allclose([b.max_departure, b.domain_radius, b.gradient_bound, b.lipschitz], want, rtol=1e-13, atol=0)
                assert np.array_equal(s.P, g[case + '_pose_P'][j])
                assert np.allclose(np.eye(3) if s.R is None else s.R, g[case + '_pose_R'][j], rtol=0, atol=1e-15)
    assert any('departs from its conic seed' in str(w.message) for w in caught)      # D's aspheres are that steep
    assert g['D2_band'][0, 1] == 0.999 / np.sqrt((1 / 20) * (1 / 20))    # no aperture: just inside the seed conic's domain
    R = make_rotation_matrix((0, 0, 38))
    assert np.allclose(R, g['C_pose_R'][1], rtol=0, atol=1e-15) and np.allclose(R @ R.T, np.eye(3), atol=1e-15)
    assert np.allclose(make_rotation_matrix((np.pi / 2, 0, 0), radians=True), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.array_equal(promote_3d_point(5), [0, 0, 5]) and np.array_equal(promote_3d_point([1, 2]), [0, 1, 2])
    with pytest.raises(ValueError):
        promote_3d_point([1, 2, 3, 4])
    assert coerce_3d_rotation(None) is None and np.array_equal(coerce_3d_rotation([0, 0, 38]), R)
    P, R2 = apply_tilt_decenter(np.array([0.0, 0.0, 24.0]), None, tilt=[1.5, 0, 0], decenter=[0.1, -0.2, 0])
    assert np.array_equal(P, g['A_pose_P'][3]) and np.allclose(R2, g['A_pose_R'][3], rtol=0, atol=1e-15)
    assert apply_tilt_decenter(P, None)[1] is None
    with pytest.raises(ValueError):
        apply_tilt_decenter(P, None, decenter=[1, 2])


def test_shapes_on_tensors():
    """sag and sag_and_normal, for users who call them: torch operations, against the model's numpy"""
    from prysm_amd.x.raytracing import surfaces as SF
    x, y = torch.linspace(-5, 5, 11, dtype=torch.float64), torch.linspace(-3, 4, 11, dtype=torch.float64)
    sh = SF.EvenAsphere(1 / 20, -0.5, (2e-4, -3e-6))
    z, n = plan._asphere(np.float64, sh.coefs, np.float64(sh.c), np.float64(sh.k), x.numpy(), y.numpy())
    zt, nt = sh.sag_and_normal(x, y)
    assert np.allclose(zt.numpy(), z, rtol=1e-14) and np.allclose(nt.numpy(), np.stack(n, -1), rtol=1e-13, atol=1e-16) and torch.equal(sh.sag(x, y), zt)
    sh = SF.OffAxisConic(1 / 30, -1.0, dx=2.0, dy=-1.0)
    z, n = plan._conic_sag_normal(np.float64, np.float64(sh.c), np.float64(sh.k), x.numpy() + 2.0, y.numpy() - 1.0)
    zt, nt = sh.sag_and_normal(x, y)
    assert np.allclose(zt.numpy(), z, rtol=1e-14) and np.allclose(nt.numpy(), np.stack(n, -1), rtol=1e-13, atol=1e-16)
    assert torch.equal(SF.Plane().sag(x, y), torch.zeros_like(x)) and torch.equal(SF.Plane().sag_and_normal(x, y)[1][:, 2], torch.ones_like(x))
    assert torch.allclose(SF.Sphere(0.1).sag(x, y), SF.Conic(0.1, 0.0).sag(x, y))


def test_what_is_not_built_says_so():
    from prysm_amd.x import raytracing as RT
    from prysm_amd.x.raytracing import surfaces as SF
    for name in ('Q2D', 'Zernike', 'XY', 'Chebyshev', 'Jacobi', 'Toroid', 'Biconic', 'CallableShape'):
        with pytest.raises(NotImplementedError, match=name):
            getattr(SF, name)(1, 2, 3)
    with pytest.raises(NotImplementedError, match='grating'):
        SF.Surface(SF.Plane(), 'reflect', P=1, grating=object())
    with pytest.raises(NotImplementedError, match='coating'):
        SF.Surface(SF.Plane(), 'reflect', P=1, coating=object())
    with pytest.raises(NotImplementedError, match='callable clip'):
        SF.Surface(SF.Plane(), 'reflect', P=1, aperture=lambda x, y: x < 1)
    with pytest.raises(NotImplementedError, match='keep_intermediates'):
        RT.raytrace([], np.zeros((2, 3)), np.zeros((2, 3)), 0.5, keep_intermediates=True)
    # the reference's argument rules
    with pytest.raises(TypeError, match='shape'):
        SF.Surface(None, 'reflect', P=1)
    with pytest.raises(TypeError, match='interaction'):
        SF.Surface(SF.Plane(), None, P=1)
    with pytest.raises(TypeError, match='pose'):
        SF.Surface(SF.Plane(), 'reflect')
    with pytest.raises(ValueError, match='material'):
        SF.Surface(SF.Plane(), 'refract', P=1)
    with pytest.raises(ValueError, match='unknown surface type'):
        SF.Surface(SF.Plane(), 'absorb', P=1)
    s = SF.Surface(SF.Sphere(0.1), SF.STYPE_IMG, pose=([1, 2, 3], None), aperture=4.0)
    assert s.typ == SF.STYPE_IMG and np.array_equal(s.P, [1, 2, 3]) and s.aperture.clip.radius == 4.0 and s.aperture.limiting_radius() == 4.0

    class System:
        def to_surfaces(self):
            return []
    with pytest.raises(TypeError, match='compiled surface sequence'):
        RT.raytrace(System(), np.zeros((2, 3)), np.zeros((2, 3)), 0.5)
    with pytest.raises(TypeError, match='sized'):
        RT.raytrace((s for s in []), np.zeros((2, 3)), np.zeros((2, 3)), 0.5)
    for bad in ('int', np.int32, torch.float16, 'no such type'):
        with pytest.raises(TypeError, match='float32 or float64'):
            RT.prepare([s], 0.5, dtype=bad)


def test_status_helpers():
    from prysm_amd.x import raytracing as RT
    status = np.array([3 + 0j, 1 - 1j, 2 + 2j, 2 - 2j, 1 + 1j])
    assert RT.decode_status(status).tolist() == ['OK', 'MISS at surface 1', 'CLIPPED at surface 2', 'TIR at surface 2', 'NEWTON at surface 1']
    assert RT.decode_status(2 + 2j) == 'CLIPPED at surface 2' and RT.decode_status(torch.from_numpy(status))[3] == 'TIR at surface 2'
    P = np.zeros((5, 3))
    P[0, 1] = np.nan
    assert RT.valid_mask(status).tolist() == [True, False, False, False, False] and not RT.valid_mask(status, P).any()
    assert RT.valid_mask(None, P).tolist() == [False, True, True, True, True] and RT.valid_mask(None) is None
    assert RT.valid_mask(torch.from_numpy(status), torch.from_numpy(P)).tolist() == [False] * 5
    rec = RT.RayStatus.from_encoded(status)
    assert rec.surface.tolist() == [3, 1, 2, 2, 1] and rec.code.tolist() == [0, -1, 2, -2, 1] and np.array_equal(rec.encoded, status)
    assert rec.text[1] == 'MISS at surface 1'
    assert RT.resolve_tol_sag(None, np.float64) == 1e-12 and RT.resolve_tol_sag(None, np.float32) == 100 * float(np.finfo(np.float32).eps)
    assert RT.resolve_tol_sag(1e-7, np.float64) == 1e-7
    assert (RT.STATUS_OK, RT.STATUS_NEWTON, RT.STATUS_CLIP, RT.STATUS_MISS, RT.STATUS_TIR) == (plan.OK, plan.NEWTON, plan.CLIP, plan.MISS, plan.TIR)


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    return _lib.load()


def test_entry_point_argument_errors(lib):
    from prysm_amd import _lib as L
    p = ctypes.c_void_p(64)
    ok = (p, 1.0, 1e-12, 1, p, p, p, p, p, p, p, None)
    assert lib.pm_rt_trace(L.PM_C64, 8, 2, *ok) == L.PM_ERR_ARG and b'dtype' in lib.pm_last_error()
    assert lib.pm_rt_trace(9, 8, 2, *ok) == L.PM_ERR_ARG
    assert lib.pm_rt_trace(L.PM_F64, -1, 2, *ok) == L.PM_ERR_ARG and lib.pm_rt_trace(L.PM_F64, 8, -2, *ok) == L.PM_ERR_ARG
    assert lib.pm_rt_trace(L.PM_F64, 8, L.PM_RT_MAX_SURFACES + 1, *ok) == L.PM_ERR_ARG and b'table limit' in lib.pm_last_error()
    assert lib.pm_rt_trace(L.PM_F64, 8, 2, p, 1.0, 1e-12, 2, p, p, p, p, p, p, p, None) == L.PM_ERR_ARG and b'history' in lib.pm_last_error()
    assert lib.pm_rt_trace(L.PM_F64, 8, 2, p, 1.0, 0.0, 1, p, p, p, p, p, p, p, None) == L.PM_ERR_ARG and b'tol_sag' in lib.pm_last_error()
    for missing in range(8):       # table, P, S and the five outputs are all required
        ptrs = [p] * 8
        ptrs[missing] = None
        assert lib.pm_rt_trace(L.PM_F32, 8, 2, ptrs[0], 1.0, 1e-5, 0, *ptrs[1:], None) == L.PM_ERR_ARG and b'null' in lib.pm_last_error()
    q = ctypes.c_void_p(68)      # 4-byte aligned: enough for float and the status, not for double or the table
    assert lib.pm_rt_trace(L.PM_F64, 8, 2, p, 1.0, 1e-12, 1, q, p, p, p, p, p, p, None) == L.PM_ERR_ARG and b'aligned' in lib.pm_last_error()
    assert lib.pm_rt_trace(L.PM_F32, 8, 2, q, 1.0, 1e-5, 1, p, p, p, p, p, p, p, None) == L.PM_ERR_ARG and b'aligned' in lib.pm_last_error()
    assert lib.pm_rt_trace(L.PM_F32, 8, 2, p, 1.0, 1e-5, 1, p, p, p, p, p, ctypes.c_void_p(66), p, None) == L.PM_ERR_ARG
    # no rays or no surfaces: nothing to launch, nothing looked at
    assert lib.pm_rt_trace(L.PM_F64, 0, 3, *([None, 1.0, 1e-12, 1] + [None] * 8)) == 0
    assert lib.pm_rt_trace(L.PM_F32, 5, 0, *([None, 1.0, 1e-5, 0] + [None] * 8)) == 0
    assert (L.PM_RT_RECORD, L.PM_RT_MAX_SURFACES, L.PM_RT_MAX_COEFS) == (plan.REC, plan.MAX_SURFACES, plan.MAX_COEFS)


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    from prysm_amd.x import raytracing as RT
    from prysm_amd.x.raytracing import surfaces as SF
    g = RC.golden()
    surfs = [SF.Surface(SF.Plane(), 'eval', P=10)]
    with pytest.raises(RuntimeError):
        RT.raytrace(surfs, g['B_P0'], g['B_S0'], RC.WVL)
    with pytest.raises(RuntimeError):
        RT.prepare(surfs, RC.WVL)
    with pytest.raises(RuntimeError):
        RT.generate_collimated_rect_ray_grid(5, 1.0)
