"""CPU: the premise and the teeth of tests/test_gpu_modal_scale.py.  The workgroup caps read back from the workspace queries are the
ones the kernels were written with and the three sizes derived from them pass them by the margins the GPU tests rely on; the probes
sit where a mode is large; and with the numpy model of each unit summed in the kernels' order standing in for the kernel, the checks
of tests/modal_scale_common.py pass in both precisions and at least one of them fails when the second trip is skipped, the ragged
last tile is skipped, or a tile is counted twice."""
import numpy as np
import pytest

import modal_scale_common as MS

DTYPES = [np.float64, np.float32]
# the sensitivity runs: one coordinate form per kernel loop (the polar Zernike form and the 1-D families differ in the walk only)
STAND_INS = ['zernike', 'q2d', 'qcon', 'jacobi radial', 'cheby1', 'fiber']


def test_caps_and_sizes_are_the_ones_the_gpu_tests_assume():
    for unit in ('zernike', 'qpoly', 'recur', 'fiber'):
        assert MS.cap_of(unit) == 1024, unit                 # kMaxProjectGroups workgroups of 1024 points
        for dt in DTYPES:
            assert MS.groups(unit, 1024 * 1024, dt) == 1024 == MS.groups(unit, 4096 * 4096, dt)
            assert MS.groups(unit, 1023 * 1024 + 1, dt) == 1024 and MS.groups(unit, 1023 * 1024, dt) == 1023
            assert MS.groups(unit, 5003, dt, nmodes=11) == 5
    assert MS.cap_of('segment') == 256                       # kSegGroups workgroups per segment
    assert MS.groups('segment', 514 * 514) == 256 and MS.groups('segment', 100 * 100) == 10
    # the overlap launches the projection's workgroup count over one point per thread: 256 threads a workgroup, so it strides four
    # times at any size and 262144 threads are its most
    assert MS.cap_of('overlap') == 1024 and MS.groups('overlap', 262145) == 257 and MS.groups('overlap', 1920) == 2
    n_one, n_vec, n_odd = MS.sizes(1024)
    assert (n_one, n_vec, n_odd) == (1048577, 1054212, 1054215)
    assert n_vec % 4 == 0 and n_vec % MS.WAVE_TILE not in (0, MS.WAVE_TILE) and n_odd % 4 == 3
    assert MS.sizes(256) == (262145, 267780, 267783)


@pytest.mark.parametrize('n', MS.sizes(1024))
def test_coverage_model(n):
    tiles = MS.tiles_by_trip(n, 1024)
    owned = np.zeros(n, dtype=np.int32)
    for wg, wave, trip, lo, hi in tiles:
        assert lo == (wg * 4 + wave) * 256 + trip * 1024 * 1024 and 0 < hi - lo <= 256
        owned[lo:hi] += 1
    assert np.all(owned == 1)
    second = [t for t in tiles if t[2] == 1]
    assert {t[2] for t in tiles} == {0, 1}
    if n == MS.sizes(1024)[0]:
        assert second == [(0, 0, 1, n - 1, n)]               # one lane of one wave of workgroup 0
    else:
        assert {t[0] for t in second} == set(range(6)) and second[-1][4] - second[-1][3] in (4, 7)
    sets = MS.probe_sets(n, 1024)
    assert all(1 <= len(S) <= 1024 and S[-1] < n for S in sets.values())
    assert sets['last wave tile'][0] == tiles[-1][3] and sets['first tile of trip 2'][0] == second[0][3]


def stand_in(unit, dt):
    """the unit's numpy model in the precision dt at the coordinates rounded to dt, (K, n_odd)"""
    u, v = MS.unit_coords(unit, dt)
    return MS.model(unit, u, v, dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('unit', STAND_INS)
def test_checks_pass_for_the_model_and_fail_for_each_fault(unit, dt):
    cap = MS.cap_of(MS.UNITS[unit][0])
    Z = stand_in(unit, dt)
    for n in MS.sizes(cap):
        bat = MS.battery(unit, n, dt, dense=1)
        bat.placement()
        ngroups = min(-(-n // MS.TILE), cap)
        totals = [MS.tile_totals(Z[:, :n], g, dt) for g in bat.G]
        clean = np.stack([MS.combine(tt, ngroups, dt) for tt in totals])
        assert bat.verify(clean, label=f'model {unit}') == []
        twice = (cap - 1) * MS.WAVES + 1                      # a wave tile inside the last workgroup tile of the first trip
        for fault in MS.FAULTS:
            broken = np.stack([MS.combine(tt, ngroups, dt, fault, twice) for tt in totals])
            missed = bat.verify(broken)
            assert missed, (unit, n, fault)
            print(f'{unit} {np.dtype(dt).name} n={n} {fault}: noticed by {[name for name, _ in missed]}')


def test_the_polar_form_and_the_other_families_place_their_probes():
    for unit in ('zernike polar', 'jacobi', 'legendre'):
        for n in MS.sizes(1024):
            for dt in DTYPES:
                MS.battery(unit, n, dt).placement()


def test_piston_modes_of_the_models_are_exactly_one():
    for unit, (_, _, piston) in MS.UNITS.items():
        if piston is not None:
            for dt in DTYPES:
                u, v = (a[:4096] for a in MS.unit_coords(unit, dt))
                assert np.all(MS.model(unit, u, v, dt)[piston] == 1), (unit, dt)
