"""CPU: the segmented-aperture host side without a GPU -- the hex helpers and the constructor's geometry against the reference fixture,
the grid-sharing map, a numpy model of compose_opd and its adjoint driven by the segment plan (cover planes, grid sources, packed
masks) against the fixture, the C entry points' symbols and plan check, and the argument errors raised before anything is uploaded."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from prysm_amd import segmented as SG
from prysm_amd.polynomials import zernike_plan as ZP

SYMS = ('pm_segment_plan_check', 'pm_segment_compose', 'pm_segment_project', 'pm_segment_project_workspace')
MONO = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 1)]


@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'segmented.npz'))


@pytest.fixture(scope='module')
def lib():
    from prysm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def aperture(fx, i, dtype=np.float64, share_grids=True):
    p = f'c{i}_'
    x, y = np.meshgrid(fx[p + 'xv'], fx[p + 'yv'])
    ap = SG.CompositeHexagonalAperture(x.astype(dtype), y.astype(dtype), int(fx[p + 'rings']), float(fx[p + 'sd']), float(fx[p + 'sep']),
                                       segment_angle=int(fx[p + 'angle']), exclude=tuple(int(v) for v in fx[p + 'exclude']),
                                       share_grids=share_grids)
    return ap, x, y


def zernike_bases(ap, nms, polar=True):
    """the basis every segment uses, in numpy: the table walk at its grid source's local coordinates over vtov / 2"""
    table = ZP.plan(nms)
    out = []
    for s in range(len(ap.windows)):
        lx, ly = ap.host_local_coords[ap.grid_sources[s]]
        nr = ap.vtov / 2
        out.append(ZP.evaluate(table, np.hypot(lx, ly) / nr, np.arctan2(ly, lx), len(nms), polar=True))
    return out


def mono_bases(ap, nr):
    out = []
    for s in range(len(ap.windows)):
        lx, ly = ap.host_local_coords[ap.grid_sources[s]]
        xx, yy = lx / nr[0], ly / nr[1]
        out.append(np.array([xx ** a * yy ** b for a, b in MONO]))
    return out


def test_hex_helpers():
    a, b = SG.Hex(1, -2, 1), SG.Hex(0, 3, -3)
    assert SG.add_hex(a, b) == (1, 1, -2) and SG.sub_hex(a, b) == (1, -5, 4) and SG.mul_hex(a, b) == (0, -6, -3)
    assert SG.scale_hex(a, 2) == (2, -4, 2)
    assert SG.hex_dir(7) == SG.hex_dir(1) == (1, -1, 0)
    assert SG.hex_neighbor(SG.Hex(0, 0, 0), 3) == (-1, 0, 1)
    for r in (1, 2, 3):
        ring = SG.hex_ring(r)
        assert len(ring) == 6 * r and len(set(ring)) == 6 * r
        assert ring[0] == (0, r, -r)            # 'north' first
        assert all(h.q + h.r + h.s == 0 and max(abs(h.q), abs(h.r), abs(h.s)) == r for h in ring)
    x, y = SG.hex_to_xy(SG.Hex(1, 0, -1), 2.0)
    assert x == pytest.approx(3.0) and y == pytest.approx(2 * SG.VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT)
    x, y = SG.hex_to_xy(SG.Hex(0, 1, -1), 1.0, rot=0)
    assert x == pytest.approx(SG.VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT) and y == pytest.approx(1.5)
    assert SG.FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX * SG.VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT == pytest.approx(1.0, rel=1e-15)
    xg = np.zeros((10, 12))
    assert SG._local_window(5, 6, (0.0, 0.0), 1.0, 3, xg, xg) == (slice(2, 8), slice(3, 9))
    assert SG._local_window(5, 6, (-20.0, 4.0), 1.0, (3, 2), xg, xg) == (slice(7, 10), slice(0, 0))


@pytest.mark.parametrize('i', [1, 2, 3, 4])
def test_geometry_matches_the_reference(fx, i):
    p = f'c{i}_'
    ap, _, _ = aperture(fx, i)
    assert ap.vtov == pytest.approx(float(fx[p + 'vtov']), rel=1e-15)
    np.testing.assert_array_equal(np.array(ap.segment_ids), fx[p + 'ids'])
    np.testing.assert_array_equal(np.array(ap.all_centers, dtype=float).reshape(-1, 2), fx[p + 'centers'])
    np.testing.assert_array_equal(np.array([(w[0].start, w[0].stop, w[1].start, w[1].stop) for w in ap.windows]), fx[p + 'windows'])
    np.testing.assert_array_equal(np.array([(lx[0, 0], ly[0, 0]) for lx, ly in ap.host_local_coords]), fx[p + 'corners'])
    np.testing.assert_allclose([m.sum() for m in ap.host_local_masks], fx[p + 'mask_sum'], rtol=1e-13)
    np.testing.assert_allclose(np.concatenate([m[::3, ::3].ravel() for m in ap.host_local_masks]), fx[p + 'mask_sub'], atol=1e-13)
    np.testing.assert_allclose(ap.host_amp[::3, ::3], fx[p + 'amp_sub'], atol=1e-13)
    assert ap.host_amp.dtype == np.float64


@pytest.mark.parametrize('i', [1, 2, 3, 4])
def test_grid_sources_are_the_reference_groups(fx, i):
    ap, _, _ = aperture(fx, i)
    assert ap.grid_sources == [int(v) for v in fx[f'c{i}_src']]
    own, _, _ = aperture(fx, i, share_grids=False)
    assert own.grid_sources == list(range(len(own.windows)))


def test_jwst_grid_groups():
    """the reference quirk on the JWST-like layout at 512^2: 6 groups keyed on the x corner only"""
    g = (np.arange(512) - 256) * (6.628 / 512)
    x, y = np.meshgrid(g, g)
    ap = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
    groups = {}
    for s, src in enumerate(ap.grid_sources):
        groups.setdefault(src, []).append(s)
    assert sorted(groups.values()) == [[0, 3], [1, 2, 7, 11], [4, 5, 13, 17], [6, 12], [8, 9, 10], [14, 15, 16]]
    # in a group the local y differ: by about a sample where the windows are not clamped
    assert ap.host_local_coords[1][1][0, 0] != ap.host_local_coords[11][1][0, 0]


@pytest.mark.parametrize('i', [1, 2, 3, 4])
def test_plan_model_matches_the_reference(fx, i):
    p = f'c{i}_'
    ap, x, _ = aperture(fx, i)
    if i == 4:
        nr = tuple(float(v) for v in fx[p + 'nr'])
        bases = mono_bases(ap, nr)
    else:
        nms = [tuple(int(v) for v in r) for r in fx[p + 'nms']]
        bases = zernike_bases(ap, nms)
        nr = (ap.vtov / 2,) * 2
    plan = SG.SegmentPlan(x.shape, ap.windows, ap.host_local_masks, ap.all_centers, ap.grid_sources, nr[0], np.float64)
    S = len(ap.windows)
    assert plan.desc.shape == (S,) and plan.cover.dtype == np.int16 and plan.cover.shape[1] == x.size
    # every cover list is packed to the front, in segment order, and holds only segments with a non-zero mask there
    cov = plan.cover
    for a in range(1, cov.shape[0]):
        assert np.all((cov[a] < 0) | (cov[a - 1] >= 0)) and np.all((cov[a] < 0) | (cov[a] > cov[a - 1]))
    coefs = fx[p + 'coefs']
    sub = int(fx[p + 'sub'])
    got = SG.evaluate_compose(plan, coefs[0], bases)
    ref = fx[p + 'opd1']
    assert np.max(np.abs(got[::sub, ::sub] - ref)) / np.max(np.abs(ref)) < 1e-12
    base = np.random.default_rng(int(fx[p + 'seed_out'])).standard_normal(x.shape)
    got = SG.evaluate_compose(plan, coefs[1], bases, out=base)
    ref = fx[p + 'opd2']
    assert np.max(np.abs(got[::sub, ::sub] - ref)) / np.max(np.abs(ref)) < 1e-12
    g = np.random.default_rng(int(fx[p + 'seed_g'])).standard_normal(x.shape)
    adj, ref = SG.evaluate_project(plan, g, bases), fx[p + 'adj']
    assert np.max(np.abs(adj - ref)) / np.max(np.abs(ref)) < 1e-12


def test_jwst_plan_size():
    g = (np.arange(512) - 256) * (6.628 / 512)
    x, y = np.meshgrid(g, g)
    ap = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
    ap.prepare_opd_bases(SG_zernike(), [ZP.noll_to_nm(j) for j in range(1, 7)])
    plan = ap.segment_plan
    assert plan.cover.shape[0] == 2          # at most 2 non-zero masks over any pixel
    assert plan.desc.nbytes == 18 * 80


def SG_zernike():
    from prysm_amd.polynomials import zernike_nm_seq
    return zernike_nm_seq


def test_symbols_declared_exported_and_bound(lib):
    from prysm_amd import _lib
    import re
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'prysm_amd.h')).read(), flags=re.S)
    for s in SYMS:
        assert re.search(r'\b' + s + r'\s*\(', src), s
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.PM_SEGMENT_ZERNIKE == 0 and _lib.PM_SEGMENT_STORED == 1
    assert 'CompositeHexagonalAperture' in SG.__all__


def test_c_argument_errors_and_plan_check(lib):
    from prysm_amd import _lib as L
    rc = lib.pm_segment_compose(9, 0, 4, 4, None, None, 0, None, None, 0, None, None, 0, 0, None, 1, None, 0, None, None)
    assert rc == L.PM_ERR_ARG and b'dtype' in lib.pm_last_error()
    rc = lib.pm_segment_project(L.PM_F64, 5, 4, 4, None, None, 0, None, None, 0, None, 0, 0, None, 1, None, None, None, 0, None)
    assert rc == L.PM_ERR_ARG and b'source' in lib.pm_last_error()
    assert lib.pm_segment_project_workspace(L.PM_F64, 1024, 18, 6, 2) == 1 * 2 * 18 * 6 * 8
    assert lib.pm_segment_project_workspace(L.PM_F32, 10 ** 6, 18, 6, 1) == 256 * 18 * 6 * 4
    assert lib.pm_segment_project_workspace(7, 10, 1, 1, 1) == 0
    g = (np.arange(64) - 32) * (4.0 / 64)
    x, y = np.meshgrid(g, g)
    ap = SG.CompositeHexagonalAperture(x, y, 1, 1.32, 0.02)
    ap.prepare_opd_bases(SG_zernike(), [(0, 0), (1, 1)])
    plan = ap.segment_plan
    plan.check(2)
    bad = plan.desc.copy()
    bad[3]['w'] += 70
    with pytest.raises(ValueError, match='window outside'):
        L.check(lib.pm_segment_plan_check(64, 64, len(bad), bad.ctypes.data_as(ctypes.c_void_p), plan.masks.size, 2, -1))
    bad = plan.desc.copy()
    bad[2]['moff'] = plan.masks.size
    with pytest.raises(ValueError, match='mask outside'):
        L.check(lib.pm_segment_plan_check(64, 64, len(bad), bad.ctypes.data_as(ctypes.c_void_p), plan.masks.size, 2, -1))
    with pytest.raises(ValueError, match='stored basis'):
        L.check(lib.pm_segment_plan_check(64, 64, len(plan.desc), plan.desc.ctypes.data_as(ctypes.c_void_p), plan.masks.size, 2, 10))


def test_python_argument_errors_before_upload():
    g = (np.arange(64) - 32) * (4.0 / 64)
    x, y = np.meshgrid(g, g)
    with pytest.raises(ValueError, match='cartesian'):
        SG.CompositeHexagonalAperture(x, y, 1, 1.32, 0.02, segment_angle=45)
    ap = SG.CompositeHexagonalAperture(x, y, 1, 1.32, 0.02)
    S = len(ap.segment_ids)
    with pytest.raises(AttributeError):
        ap.compose_opd(np.zeros((S, 3)))
    with pytest.raises(AttributeError):
        ap.compose_opd_adjoint(np.zeros(x.shape))
    ap.prepare_opd_bases(SG_zernike(), [(0, 0), (1, 1), (1, -1)])
    assert len(ap.opd_bases) == S and len(ap.opd_grids) == S
    with pytest.raises(ValueError, match='coefs'):
        ap.compose_opd(np.zeros((S, 4)))
    with pytest.raises(ValueError, match='coefs'):
        ap.compose_opd(np.zeros((S + 1, 3)))
    with pytest.raises(ValueError, match='coefs'):
        ap.compose_opd(np.zeros(3))
    with pytest.raises(TypeError, match='real'):
        ap.compose_opd(np.zeros((S, 3), dtype=complex))
    with pytest.raises(ValueError, match='out'):
        ap.compose_opd(np.zeros((S, 3)), out=np.zeros((3, 64, 64)))
    with pytest.raises(ValueError, match='opd_bar'):
        ap.compose_opd_adjoint(np.zeros((63, 64)))
    with pytest.raises(ValueError, match='opd_bar'):
        ap.compose_opd_adjoint(np.zeros((2, 64, 63)))
    with pytest.raises(TypeError, match='real'):
        ap.compose_opd_adjoint(np.zeros((64, 64), dtype=complex))
    assert ap._dev == {}                      # nothing was uploaded
