"""CPU: x.polarization without a device -- the numpy model of csrc/jones.hip (prysm_amd/x/polarization_plan.py) against the reference's
golden (tests/golden/polarization.npz) within the bounds of polarization_common.py, the departures from the reference that can be
shown without a launch, the layout logic, and the argument checks of the five entry points, called with pointers that are never
dereferenced (every call is refused, or returns 0 for an empty shape, before anything is launched)."""
import ctypes
import os

import numpy as np
import pytest

import polarization_common as C
from prysm_amd import _lib as L
from prysm_amd.x import polarization_plan as PP

P = ctypes.c_void_p(64)          # never dereferenced; 16-byte aligned
ARG = L.PM_ERR_ARG


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


# ---------------------------------------------------------------- the model against the golden
@pytest.mark.parametrize('precision', C.PRECISIONS)
def test_model_generators_and_mueller_match_the_golden(precision):
    g = C.golden()
    model = C.model_cases(precision)
    for name in C.MAP_CASES + C.SCALAR_CASES:
        want = g[f'{name}_{precision}']
        assert model[name].shape == want.shape and model[name].dtype == want.dtype, name
        dev = C.dev_eps(model[name], want, precision, C.case_scale(name, precision))
        print(f'{name} precision {precision}: {dev:.3g} eps, bound {C.bound(name, precision, False):.3g}')
        assert dev <= C.bound(name, precision, False), name


@pytest.mark.parametrize('precision', C.PRECISIONS)
def test_model_products_scale_and_pauli_match_the_golden(precision):
    g, c = C.golden(), C.cdt(precision)
    mats, vec = C.jones_operands(precision)
    A, B = C.CONST_A.astype(c), C.CONST_B.astype(c)
    for name, ops, tail in (('chain6', mats, False), ('chainv', [mats[0], mats[1], vec], True), ('chainc', [A, mats[0], B, mats[1]], False)):
        got = PP.chain(ops, tail)
        want = g[f'{name}_{precision}']
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.all(np.abs(got - want) <= C.chain_bound(ops, precision)), name
    f = C.inputs(precision)['field']
    got = PP.scale(mats[0], f)
    assert got.dtype == c and np.all(np.abs(got - g[f'apply_{precision}']) <= C.scale_bound(mats[0], f, precision))
    assert np.array_equal(PP.pauli(mats[0]), g[f'pauli_{precision}'])
    assert np.array_equal(PP.chain([mats[0]]), mats[0]) and np.array_equal(PP.chain([vec], True), vec)


@pytest.mark.parametrize('precision', C.PRECISIONS)
def test_exact_structure(precision):
    g, c = C.golden(), C.cdt(precision)
    eye = np.broadcast_to(np.eye(2, dtype=c), (3, 5, 2, 2))
    assert np.array_equal(PP.mueller(eye), np.broadcast_to(np.eye(4, dtype=C.rdt(precision)), (3, 5, 4, 4)))
    for k in range(4):
        assert np.array_equal(np.array(PP.PAULI[k], dtype=c), g[f'pauli_{k}_{precision}'])
    assert np.array_equal(PP.optic(PP.RETARDER, [0.0, 0.0], (), c), np.eye(2, dtype=c))
    assert np.array_equal(PP.optic(PP.RETARDER, [0.0, 0.0], (2, 3), c), np.broadcast_to(np.eye(2, dtype=c), (2, 3, 2, 2)))
    s = 1 / np.sqrt(2)
    assert np.array_equal(g[f'cpv_left_{precision}'], np.array([s, 1j * s], dtype=c))
    assert np.array_equal(g[f'cpv_right_{precision}'], np.array([s, -1j * s], dtype=c))


def test_field_inside_the_generator_is_the_generator_then_the_scale():
    for precision in C.PRECISIONS:
        i, c = C.inputs(precision), C.cdt(precision)
        plain = PP.optic(PP.VORTEX, [i['t'], C.VVR_RETARDANCE, C.VVR_ROTATE], C.GRID, c, charge=2)
        fused = PP.optic(PP.VORTEX, [i['t'], C.VVR_RETARDANCE, C.VVR_ROTATE], C.GRID, c, charge=2, field=i['field'])
        assert np.all(np.abs(fused - PP.scale(plain, i['field'])) <= C.scale_bound(plain, i['field'], precision))


# ---------------------------------------------------------------- departures from the reference
def test_departures():
    from prysm_amd.x import polarization as pol
    g = C.golden()
    # alpha outside [0, 1]: ValueError, before any device is needed
    for alpha in (-0.1, 1.5):
        with pytest.raises(ValueError, match='alpha'):
            pol.linear_diattenuator(alpha)
    with pytest.raises(ValueError, match='alpha'):
        pol.linear_diattenuator(2.0, theta=0.1, shape=(4, 4))
    # the reference multiplies the caller's theta by the charge; the model and the wrapper leave it alone
    t = g['in_t']
    assert np.array_equal(g['vvr_theta_after_64'], t * 2) and not np.array_equal(g['vvr_theta_after_64'], t)
    t0 = t.copy()
    PP.optic(PP.VORTEX, [t, C.VVR_RETARDANCE, C.VVR_ROTATE], C.GRID, np.complex128, charge=2)
    assert np.array_equal(t, t0)
    # the leakage term: by default on element (0,0) only, as the golden has it; identity_leakage on both diagonal elements
    z = np.zeros((1, 1))
    quirk = PP.optic(PP.VORTEX, [z, 1.0, 0.0], (1, 1), np.complex128, charge=2)[0, 0]
    paper = PP.optic(PP.VORTEX, [z, 1.0, 0.0], (1, 1), np.complex128, charge=2, leak=True)[0, 0]
    jc = -1j * np.cos(0.5)
    assert quirk[0, 0] == np.sin(0.5) + jc and quirk[1, 1] == -np.sin(0.5)
    assert paper[0, 0] == np.sin(0.5) + jc and paper[1, 1] == -np.sin(0.5) + jc
    # jones_to_mueller(broadcast=False) of a single 2 x 2: the same closed form (the reference takes np.kron there)
    for precision in C.PRECISIONS:
        m = PP.mueller(C.CONST_A.astype(C.cdt(precision)))
        dev = C.dev_eps(m, g[f'mueller_nobroadcast_{precision}'], precision, C.case_scale('mueller_s', precision))
        assert dev <= C.bound('mueller_s', precision, False)      # measured: 0.327 eps, the figure of mueller_s itself
    # a map of theta in the retarder: the golden is the reference pixel by pixel, and the model reproduces a pixel called alone
    i = C.inputs(64)
    whole = PP.optic(PP.RETARDER, [i['delta'], i['theta']], C.GRID, np.complex128)
    one = PP.optic(PP.RETARDER, [i['delta'][4:5, 7:8], i['theta'][4:5, 7:8]], (1, 1), np.complex128)
    assert np.array_equal(whole[4, 7], one[0, 0])


# ---------------------------------------------------------------- layouts
def test_layout_round_trips_and_windows():
    mats, vec = C.jones_operands(64, shape=(3, 4, 5))
    m = PP.mueller(mats[0])
    for a in (mats[0], vec, m):
        p = PP.to_planes(a)
        assert p.shape == (a.shape[-2] * a.shape[-1], 3, 4, 5)
        assert np.array_equal(PP.from_planes(p), a)
        assert np.array_equal(p[1], a[..., 0, 1] if a.shape[-1] > 1 else a[..., 1, 0])
    assert PP.ncomp_of((7, 9, 2, 2), PP.AOS) == (4, (7, 9)) and PP.ncomp_of((7, 9, 2, 1), PP.AOS) == (2, (7, 9))
    assert PP.ncomp_of((4, 7, 9), PP.PLANES) == (4, (7, 9)) and PP.ncomp_of((2, 7, 9), PP.PLANES) == (2, (7, 9))
    with pytest.raises(ValueError):
        PP.ncomp_of((7, 9, 3, 2), PP.AOS)
    with pytest.raises(ValueError):
        PP.layout_code('soa')
    assert PP.rows_cols((3, 4, 5)) == (12, 5) and PP.rows_cols((5,)) == (1, 5) and PP.rows_cols(()) == (1, 1)
    # a contiguous grid, a column window of a wider one (ld = the wider row), leading dimensions that collapse, and ones that do not
    assert PP.window((6, 37), (50 * 4, 4), 4) == (6, 37, 50)
    assert PP.window((6, 37), (37, 1), 1) == (6, 37, 37)
    assert PP.window((2, 3, 5), (15, 5, 1), 1) == (6, 5, 5)
    assert PP.window((2, 3, 5), (40, 5, 1), 1) is None
    assert PP.window((6, 37), (37, 2), 1) is None and PP.window((6, 37), (30, 1), 1) is None
    assert PP.window((1, 9), (0, 1), 1) == (1, 9, 9)


# ---------------------------------------------------------------- the entry points' argument checks
def _optic(lib, dt=L.PM_C64, kind=0, rows=4, cols=4, out=P, layout=0, ld=4, ps=16, desc=True, pmap=None, pld=4, field=None, fld=4):
    d = L.pm_jones_optic_desc()
    d.kind, d.charge = kind, 1.0
    if pmap is not None:
        d.p[0].map, d.p[0].ld = pmap, pld
    return lib.pm_jones_optic(dt, ctypes.byref(d) if desc else None, rows, cols, field, fld, out, layout, ld, ps, None)


def _chain(lib, dt=L.PM_C64, count=2, rows=4, cols=4, out=P, layout=0, olayout=0, ld=4, ps=16, ops=True, mld=4, mps=16):
    recs = (L.pm_jones_operand * 6)()
    for r in recs:
        r.map, r.ld, r.pstride = 64, mld, mps
    return lib.pm_jones_chain(dt, count, recs if ops else None, layout, 0, rows, cols, out, olayout, ld, ps, None)


def _scale(lib, dt=L.PM_C64, ncomp=4, rows=4, cols=4, src=P, layout=0, ld=4, ps=16, fkind=0, field=None, fld=4, out=ctypes.c_void_p(4096),
           olayout=0, old=4, ops=16):
    return lib.pm_jones_scale(dt, ncomp, rows, cols, src, layout, ld, ps, fkind, field, fld, out, olayout, old, ops, None)


def _mueller(lib, dt=L.PM_C64, rows=4, cols=4, src=P, layout=0, ld=4, ps=16, out=P, olayout=0, old=4, ops=16):
    return lib.pm_jones_to_mueller(dt, rows, cols, src, layout, ld, ps, out, olayout, old, ops, None)


def _pauli(lib, dt=L.PM_C64, rows=4, cols=4, src=P, layout=0, ld=4, ps=16, out=P, old=4, ops=16):
    return lib.pm_pauli_coefficients(dt, rows, cols, src, layout, ld, ps, out, old, ops, None)


CALLS = {'pm_jones_optic': _optic, 'pm_jones_chain': _chain, 'pm_jones_scale': _scale, 'pm_jones_to_mueller': _mueller,
         'pm_pauli_coefficients': _pauli}


@pytest.mark.parametrize('name', sorted(CALLS))
def test_entry_points_refuse_before_they_launch(lib, name):
    call = CALLS[name]

    def refused(word, **kw):
        assert call(lib, **kw) == ARG, (name, kw)
        msg = lib.pm_last_error().decode()
        assert name in msg and word in msg, (msg, kw)

    for dt in (L.PM_F32, L.PM_F64, 99):
        refused('dtype', dt=dt)
    refused('layout', layout=2)
    refused('layout', layout=-1)
    refused('leading dimension', ld=3)
    refused('planes overlap', layout=1, ps=15, **({'olayout': 1} if name == 'pm_jones_chain' else {}))
    refused('negative', rows=-1)
    refused('aligned', **{'src' if name in ('pm_jones_scale', 'pm_jones_to_mueller') else 'out': ctypes.c_void_p(68)})
    # an empty shape returns 0 whatever the dtype and the pointers, after the mode-like arguments were looked at
    assert call(lib, rows=0) == 0 and call(lib, cols=0, dt=99) == 0
    assert call(lib, rows=0, layout=7) == ARG
    # one row takes any leading dimension
    # (never launched: the dtype is refused after the shape and before the views are looked at)
    assert call(lib, rows=1, ld=1, dt=99) == ARG and b'dtype' in lib.pm_last_error()


def test_entry_point_specific_refusals(lib):
    def word(rc, w):
        assert rc == ARG and w in lib.pm_last_error().decode(), lib.pm_last_error()

    word(_optic(lib, out=None), 'null')
    word(_optic(lib, desc=False), 'null')
    word(_optic(lib, kind=5), 'kind')
    word(_optic(lib, kind=-1), 'kind')
    word(_optic(lib, pmap=64, pld=3), 'leading dimension')
    word(_optic(lib, pmap=66), 'aligned')
    word(_optic(lib, field=ctypes.c_void_p(64), fld=2), 'leading dimension')
    word(_optic(lib, kind=L.PM_JONES_LINPOL_VECTOR, layout=1, ps=15), 'planes overlap')
    for count in (0, 7, -1):
        word(_chain(lib, count=count), 'count')
    word(_chain(lib, ops=False), 'null')
    word(_chain(lib, out=None), 'null')
    word(_chain(lib, olayout=3), 'layout')
    word(_chain(lib, mld=3), 'leading dimension')
    word(_chain(lib, layout=1, mps=15), 'planes overlap')
    for ncomp in (0, 1, 3, 16):
        word(_scale(lib, ncomp=ncomp), 'components')
    word(_scale(lib, fkind=3), 'field_kind')
    word(_scale(lib, src=None), 'null')
    word(_scale(lib, out=None), 'null')
    word(_scale(lib, old=3), 'leading dimension')
    word(_scale(lib, fkind=L.PM_JONES_FIELD_COMPLEX, field=None), 'field is missing')
    word(_scale(lib, fkind=L.PM_JONES_FIELD_REAL, field=ctypes.c_void_p(64), fld=3), 'leading dimension')
    word(_scale(lib, out=P, olayout=1, ops=16), 'in place')
    word(_scale(lib, out=P, old=5), 'in place')
    word(_mueller(lib, src=None), 'null')
    word(_mueller(lib, out=None), 'null')
    word(_mueller(lib, olayout=1, ops=15), 'planes overlap')
    word(_mueller(lib, olayout=5), 'layout')
    word(_pauli(lib, src=None), 'null')
    word(_pauli(lib, ops=15), 'planes overlap')
    word(_pauli(lib, old=3), 'leading dimension')
    assert lib.pm_version() == 107
