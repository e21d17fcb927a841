"""CPU: the host side of the fibre unit -- the special functions, the zeros, the mode solver and the numpy walk of
prysm_amd/x/fibers_plan.py against tests/golden/fibers.npz (the reference on scipy), the conventions of the mode dictionary, the table
layout, the argument checks of the entry points of csrc/fibers.hip (refused before anything is launched, so no device is needed), and
that neither the plan nor the public module imports scipy or the oracle.  Bounds: tests/fibers_common.py."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import fibers_common as FC
from prysm_amd import _lib as L
from prysm_amd.x import fibers_plan as plan

DTYPES = [np.float64, np.float32]
P = ctypes.c_void_p(64)         # never dereferenced
ODD = ctypes.c_void_p(66)
F32, F64 = L.PM_F32, L.PM_F64
BIG = 1 << 40


# --------------------------------------------------------------------------- special functions
@pytest.mark.parametrize('dt', DTYPES)
def test_besselj_against_the_tabulated_values(dt):
    g = FC.golden()
    worst = 0.0
    for l in FC.TAB_L:
        pick = g['jl_l'] == l
        x, ref, err = g['jl_x'][pick], g['jl_ref'][pick], g['jl_err'][pick]
        got = plan.besselj(l, x.astype(dt))
        assert got.dtype == dt
        xr = x.astype(dt).astype(np.float64)                 # the float32 run sees the rounded argument: |J'| <= 1
        bound = 8 * FC.eps(dt) * np.maximum(1, x) + err + np.abs(xr - x)
        dev = np.abs(got.astype(np.float64) - ref)
        worst = max(worst, np.max(dev / bound))
        assert np.all(dev <= bound), (l, x[np.argmax(dev / bound)], dev.max())
        assert plan.besselj(l, np.zeros(1, dt))[0] == (1 if l == 0 else 0)        # exact at 0
    print(f'J_l {np.dtype(dt).name}: worst deviation / bound {worst:.3f}')


@pytest.mark.parametrize('dt', DTYPES)
def test_besselke_against_the_tabulated_values(dt):
    g = FC.golden()
    worst = 0.0
    for l in FC.TAB_L:
        pick = g['ke_l'] == l
        x, ref, err = g['ke_x'][pick], g['ke_ref'][pick], g['ke_err'][pick]
        with np.errstate(over='ignore'):
            fits = np.isfinite(ref.astype(dt)) & (ref < 0.01 * np.finfo(dt).max)       # float32 cannot hold K_25(1e-3) ~ 1e106
        assert fits.sum() >= 8 and (dt == np.float32 or fits.all())
        x, ref, err = x[fits], ref[fits], err[fits]
        got = plan.besselke(l, x.astype(dt)).astype(np.float64)
        xr = x.astype(dt).astype(np.float64)                 # |d ln(e^x K_l) / dx| <= (l + 1) / x + 1 for the rounded argument
        bound = 8 * (1 + l) * FC.eps(dt) * ref + err + np.abs(xr - x) * ((l + 1) / x + 1) * ref
        dev = np.abs(got - ref)
        worst = max(worst, np.max(dev / bound))
        assert np.all(dev <= bound), (l, x[np.argmax(dev / bound)], np.max(dev / bound))
    print(f'e^x K_l {np.dtype(dt).name}: worst deviation / bound {worst:.3f}')


def test_zeros_interlace_and_are_zeros():
    prev = plan.besselj_positive_zeros(0, 40.0)
    assert abs(prev[0] - 2.404825557695773) < 1e-14 and len(prev) == 12
    for l in range(1, 30):
        z = plan.besselj_positive_zeros(l, 40.0)
        assert np.all(np.diff(z) > 0) and np.all(z < 40.0) and np.all(z > l)
        n = min(len(z), len(prev) - 1)
        assert np.all(prev[:n] < z[:n]) and np.all(z[:n] < prev[1:n + 1])
        assert np.max(np.abs(plan.besselj(l, z))) < 1e-14
        prev = z
    assert len(plan.besselj_positive_zeros(45, 40.0)) == 0


# --------------------------------------------------------------------------- the solver
@pytest.mark.parametrize('V,count', list(zip(FC.VS, FC.COUNTS)))
def test_find_all_modes_against_the_reference(V, count):
    g = FC.golden()
    tag = 'roots_' + FC.vtag(V)
    modes = plan.find_all_modes(V)
    assert sum(len(b) for b in modes.values()) == count
    ls, ns = g[tag + '_l'], g[tag + '_n']
    want_keys = [k for l in ls for k in ((0,) if l == 0 else (int(l), -int(l)))]
    assert list(modes) == want_keys                                        # 0, 1, -1, 2, -2, ...
    k, worst, bref_all = 0, 0.0, g[tag + '_b']
    for l, n in zip(ls, ns):
        b = modes[int(l)]
        # the order within a family is the reference's, checked value by value below: its roots ascend in U and are flipped once more
        # after b = 1 - (U/V)^2, so what it returns ascends in b (the comment in its source says descending)
        assert len(b) == n and np.all(np.diff(b) > 0) and np.all(np.diff(bref_all[k:k + n]) > 0) and np.all((b > 0) & (b < 1))
        if l:
            assert modes[-int(l)] is b                                     # the partners share their values
        Uref, dfref, bref = g[tag + '_U'][k:k + n], g[tag + '_df'][k:k + n], g[tag + '_b'][k:k + n]
        boundU = 2e-12 / np.abs(dfref) + 16 * FC.eps(np.float64) * V
        U = V * np.sqrt(1 - b)
        assert np.all(np.abs(U - Uref) <= boundU), (l, np.max(np.abs(U - Uref) / boundU))
        boundb = 2 * Uref / V ** 2 * boundU + 4 * FC.eps(np.float64)        # b = 1 - (U/V)^2: |db| = 2 U / V^2 |dU|, plus its own roundings
        assert np.all(np.abs(b - bref) <= boundb), (l, np.max(np.abs(b - bref) / boundb))
        worst = max(worst, np.max(np.abs(U - Uref) / boundU))
        k += n
    print(f'V = {V}: worst |U - U_ref| / bound {worst:.3f}')


def test_count_only_and_near_cutoff_modes():
    for V, count in zip(FC.VS, FC.COUNTS):
        counts = plan.find_all_modes(V, count_only=True)
        assert sum(counts.values()) == count and all(isinstance(n, int) for n in counts.values())
        assert list(counts) == list(plan.find_all_modes(V))
    assert 5e-4 < plan.find_all_modes(2.41)[1][0] < 7e-4 and 3e-5 < plan.find_all_modes(3.9)[0][0] < 5e-5       # just above cutoff


def test_public_module_carries_the_reference_names_and_conventions():
    from prysm_amd.x import fibers
    for name in ('critical_angle', 'numerical_aperture', 'V', 'find_all_modes', 'compute_LP_modes', 'smf_mode_field', 'marcuse_mfr_from_V',
                 'petermann_mfr_from_V', 'mode_overlap_integral', 'multimode_coupling', 'prepare', 'ModeSet'):
        assert callable(getattr(fibers, name)), name
    assert abs(fibers.V(4.0, 0.12, 1.55) - 2 * np.pi / 1.55 * 4.0 * 0.12) < 1e-15
    assert abs(fibers.numerical_aperture(1.45, 1.44) - np.sqrt(1.45 ** 2 - 1.44 ** 2)) < 1e-16
    assert abs(fibers.critical_angle(1.45, 1.44) - np.degrees(np.arcsin(1.44 / 1.45))) < 1e-13
    assert abs(fibers.marcuse_mfr_from_V(2.0) - (0.65 + 1.619 * 2.0 ** -1.5 + 2.879 * 2.0 ** -6)) < 1e-15
    assert abs(fibers.petermann_mfr_from_V(2.0) - (fibers.marcuse_mfr_from_V(2.0) - 0.016 - 1.567 * 2.0 ** -7)) < 1e-15
    modes = fibers.find_all_modes(5.5)
    assert list(modes) == [0, 1, -1, 2, -2, 3, -3] and sum(len(b) for b in modes.values()) == 8
    assert fibers.find_all_modes(5.5, count_only=True) == {0: 2, 1: 1, -1: 1, 2: 1, -2: 1, 3: 1, -3: 1}


# --------------------------------------------------------------------------- the table
@pytest.mark.parametrize('dt', DTYPES)
def test_table_layout(dt):
    assert plan.record_dtype(np.float32).itemsize == 32 and plan.record_dtype(np.float64).itemsize == 48
    md = FC.mode_dict('V5.5')
    table, n = plan.mode_table(5.5, md, dt)
    assert n == 8 and len(table) == 5 and table.dtype == plan.record_dtype(dt)          # 2 + 1 + 1 + 1 radial functions
    assert list(table['l']) == [0, 0, 1, 2, 3]                             # sorted by |l|
    slots = plan.mode_slots(md)
    assert [l for l, _ in slots] == [0, 0, 1, -1, 2, -2, 3, -3]
    for rec in table:
        l = int(rec['l'])
        lc, bc = slots[rec['slot_cos']]
        assert lc == l
        if l == 0:
            assert rec['slot_sin'] == -1
        else:
            ls, bs = slots[rec['slot_sin']]
            assert ls == -l and bs == bc                                   # the +- partners share the record
        U64, W64 = np.float64(rec['U']), np.float64(rec['W'])
        assert rec['U'] == dt(5.5 * np.sqrt(1 - bc)) and rec['W'] == dt(5.5 * np.sqrt(bc))
        # the normalisers are evaluated AT the rounded U, W
        assert rec['invJ'] == dt(1 / plan.besselj(l, U64)) and rec['invK'] == dt(1 / plan.besselke(l, W64))
        assert rec['flags'] == 0
    assert sorted(list(table['slot_cos']) + [s for s in table['slot_sin'] if s >= 0]) == list(range(8))
    for l, bs in md.items():                                               # each family's list is walked REVERSED
        mine = [b for ll, b in slots if ll == l]
        assert mine == list(bs[::-1])
    # a part of a dictionary: a missing partner leaves its slot out
    part, n = plan.mode_table(5.5, {-1: md[-1], 0: md[0]}, dt)
    assert n == 3 and list(part['l']) == [0, 0, 1] and list(part['slot_cos']) == [1, 2, -1] and list(part['slot_sin']) == [-1, -1, 0]
    with pytest.raises(ValueError):
        plan.mode_table(5.5, {0: [0.5], 1: [1.5]}, dt)
    smf, n = plan.smf_table(2.0, 0.4, dt)
    assert n == 1 and smf['flags'][0] == plan.FR_STRICT and smf['invJ'][0] == dt(1 / plan.besselj(1, np.float64(smf['U'][0])))


# --------------------------------------------------------------------------- the walk
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('gname', FC.GRIDS)
@pytest.mark.parametrize('case', list(FC.CASES))
def test_walk_against_the_reference_stacks(case, gname, dt):
    V = FC.CASES[case][0]
    table, n = plan.mode_table(V, FC.mode_dict(case), dt)
    r, t = FC.grid(gname, dt)
    got = plan.walk(table, n, FC.A, r, t)
    assert got.dtype == dt and got.shape == (n, *r.shape)
    FC.check_modes(case, gname, dt, got, 'model ')
    # coupling of the tilted Gaussian through the model's modes
    E = FC.incident(gname, dt)
    m = got.reshape(n, -1).astype(np.float64)
    e = E.reshape(-1).astype(np.complex128)
    eta = np.abs(m @ np.conj(e)) ** 2 / ((m * m).sum(axis=1) * (np.abs(e) ** 2).sum())
    ref = FC.golden()[f'{case}_{gname}_eta{FC.suffix(dt)}']
    dev, bound = np.max(np.abs(eta - ref)), FC.coupling_bound(V, dt, r.size)
    print(f'model coupling {case} {gname} {np.dtype(dt).name}: deviation {dev:.3e}, bound {bound:.3e}')
    assert dev <= bound


@pytest.mark.parametrize('dt', DTYPES)
def test_walk_edges(dt):
    """a single point at r = 0, the sample at r == a, and the Miller branch underflowing in float32"""
    table, n = plan.mode_table(30.0, FC.mode_dict('V30s'), dt)
    got = plan.walk(table, n, FC.A, np.zeros(1, dt), np.zeros(1, dt))
    slots = plan.mode_slots(FC.mode_dict('V30s'))
    for k, (l, _) in enumerate(slots):
        assert np.isfinite(got[k, 0]) and (got[k, 0] == 0) == (l != 0)      # J_l(0) = 0 exactly for l >= 1
    at_a = plan.walk(table, n, FC.A, np.full(1, FC.A, dt), np.zeros(1, dt))
    # J_l(U) / J_l(U) at t = 0: the bound on J_l (8 eps max(1, x)) times the normaliser, and the normaliser's own two roundings
    one = (8 * 30.0 * np.max(np.abs(table['invJ'])) + 2) * FC.eps(dt)
    for k, (l, _) in enumerate(slots):
        if l >= 0:
            assert abs(at_a[k, 0] - 1) <= one, (l, at_a[k, 0])
    near = plan.walk(table, n, FC.A, np.full(1, 0.02, dt), np.full(1, 0.3, dt))
    k25 = [k for k, (l, _) in enumerate(slots) if abs(l) == 25]
    assert np.all(np.isfinite(near)) and (dt == np.float64 or np.all(near[k25] == 0))
    assert dt == np.float32 or np.all(near[k25] != 0)


def test_smf_mode_field_and_overlap_models():
    g = FC.golden()
    b = float(g['smf_b'])
    for gname in FC.GRIDS:
        for dt in DTYPES:
            table, n = plan.smf_table(FC.SMF_V, b, dt)
            r, _ = FC.grid(gname, dt)
            got = plan.walk(table, n, FC.A, r, np.zeros_like(r))[0].astype(np.float64)
            ref = g[f'smf_{gname}_field'] + (g[f'smf_{gname}_delta32'] if dt == np.float32 else 0)
            bound = FC.mode_bound(FC.SMF_V, dt, ref.reshape(1, -1))[0]
            assert np.max(np.abs(got - ref)) <= bound
            res = plan.overlap(FC.incident(gname, dt).astype(np.complex128), FC.second_field(gname, dt).astype(np.complex128))
            assert abs(res[4] - float(g[f'overlap_{gname}_{FC.suffix(dt)}'])) <= 4 * r.size * FC.eps(np.float64)


# --------------------------------------------------------------------------- argument checks, no device
@pytest.fixture(scope='module')
def lib():
    return L.load()


def _modes(lib, dt=F32, n=8, r=P, t=P, a=4.0, table=P, nrec=3, nmodes=5, out=P):
    return lib.pm_fiber_modes(dt, n, r, t, a, table, nrec, nmodes, out, None)


def _sum(lib, dt=F32, n=8, r=P, a=4.0, nmodes=5, batch=1, coefs=P, out=P):
    return lib.pm_fiber_sum(dt, n, r, P, a, P, 3, nmodes, batch, coefs, 0, out, None)


def _project(lib, dt=F32, n=8, r=P, a=4.0, nmodes=5, batch=1, g=P, out=P, ws=P, wsb=BIG):
    return lib.pm_fiber_project(dt, n, r, P, a, P, 3, nmodes, batch, g, out, ws, wsb, None)


def _overlap(lib, dt=F32, n=8, e1=P, c1=1, e2=P, c2=1, out=P, ws=P, wsb=BIG):
    return lib.pm_overlap(dt, n, e1, c1, e2, c2, out, ws, wsb, None)


def _refused(lib, rc, code, word):
    assert rc == code, (rc, lib.pm_last_error())
    assert word.encode() in lib.pm_last_error(), lib.pm_last_error()


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib):
    ARG, UNSUP, WS = L.PM_ERR_ARG, L.PM_ERR_UNSUPPORTED, L.PM_ERR_WORKSPACE
    for call in (_modes, _sum, _project, _overlap):
        for bad in (L.PM_C64, 99):
            _refused(lib, call(lib, dt=bad, n=0), ARG, 'dtype')            # the dtype first, also for an empty shape
    for call in (_modes, _sum, _project):
        _refused(lib, call(lib, r=None), ARG, 'null')
        _refused(lib, call(lib, n=-1), ARG, 'negative')
        _refused(lib, call(lib, a=0.0), ARG, 'core radius')
        _refused(lib, call(lib, a=float('nan')), ARG, 'core radius')
        _refused(lib, call(lib, r=ODD), ARG, 'unaligned')
        _refused(lib, call(lib, out=None), ARG, 'null')
        if call is not _project:                                           # (a projection of no points still writes its zeros)
            assert call(lib, n=0) == 0                                     # the empty shape, nothing launched
    _refused(lib, _modes(lib, dt=F64, out=ctypes.c_void_p(68)), ARG, 'unaligned')
    assert _modes(lib, nmodes=0) == 0
    _refused(lib, _sum(lib, coefs=None), ARG, 'null')
    _refused(lib, _sum(lib, batch=-1), ARG, 'batch')
    assert _sum(lib, batch=0) == 0
    _refused(lib, _project(lib, batch=-1), ARG, 'batch')
    _refused(lib, _project(lib, g=None, batch=2), ARG, 'batch 1')
    _refused(lib, _project(lib, wsb=0), WS, 'workspace')
    _refused(lib, _project(lib, ws=None), WS, 'workspace')
    assert _project(lib, batch=0, wsb=0) == 0                              # no vector before the workspace
    _refused(lib, _project(lib, nmodes=4097, dt=F32), UNSUP, 'accumulators')      # 4 waves x 4097 x 4 bytes > 64 KiB
    _refused(lib, _project(lib, nmodes=2049, dt=F64), UNSUP, 'accumulators')
    with pytest.raises(NotImplementedError):
        L.check(_project(lib, nmodes=2049, dt=F64))
    _refused(lib, _overlap(lib, e1=None), ARG, 'null')
    _refused(lib, _overlap(lib, n=-1), ARG, 'negative')
    _refused(lib, _overlap(lib, e1=ctypes.c_void_p(68)), ARG, 'unaligned')        # a complex64 field wants 8 bytes
    assert lib.pm_overlap(F32, 8, ctypes.c_void_p(68), 0, P, 1, P, P, 0, None) == WS      # ... a float32 field 4; then the workspace
    _refused(lib, _overlap(lib, wsb=0), WS, 'workspace')
    with pytest.raises(ValueError):
        L.check(_overlap(lib, wsb=0))


def test_workspace_queries(lib):
    assert lib.pm_fiber_project_workspace(F64, 1023, 38, 2) == 1 * 2 * 38 * 8          # one workgroup tile of 1024 points
    assert lib.pm_fiber_project_workspace(F32, 4096 * 4096, 228, 1) == 1024 * 228 * 4  # capped at 1024 workgroups
    assert lib.pm_fiber_project_workspace(L.PM_C64, 10, 3, 1) == 0
    assert lib.pm_overlap_workspace(F32, 1023) == 16 and lib.pm_overlap_workspace(F64, 4096 * 4096) == 1024 * 32
    assert lib.pm_overlap_workspace(99, 10) == 0


def test_neither_the_plan_nor_the_module_imports_scipy_or_the_oracle():
    code = ('import sys\n'
            'import prysm_amd.x.fibers, prysm_amd.x.fibers_plan\n'
            'bad = [m for m in sys.modules if m.split(".")[0] in ("scipy", "oracle", "mpmath", "prysm")]\n'
            'assert not bad, bad\n')
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, '-c', code], check=True, cwd=root)
