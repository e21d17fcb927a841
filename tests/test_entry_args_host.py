"""CPU: the argument checks of every extern "C" entry point of csrc/zernike.hip, qpoly.hip, segmented.hip, geometry.hip, detector.hip,
dm.hip, ee.hip and bayer.hip -- what each refuses, under which word, and which of two simultaneous faults it reports, i.e. the ORDER of
its checks.  Every call here is refused, or returns 0 for an empty shape, before anything is launched, so the pointers are never
dereferenced and no device is needed.  tests/test_pointwise_args_host.py does the same for csrc/pointwise.hip.

Most of these units look at the dtype FIRST (an empty call with a bad dtype is refused, not 0); pm_bindown and pm_lattice look at their
mode / op before it, pm_tile at its scale, and the two encircled-energy entry points at everything else before it.  The table states
which."""
import ctypes
import os
import types

import pytest

from prysm_amd import _lib as L

P = ctypes.c_void_p(16)         # never dereferenced
D9 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
C = 4                           # columns of every shape here (even: the Bayer entry points ask for that)
ARG, UNSUP, WS = L.PM_ERR_ARG, L.PM_ERR_UNSUPPORTED, L.PM_ERR_WORKSPACE
F32, F64 = L.PM_F32, L.PM_F64
REAL_BAD = (L.PM_C64, 99)
BIG = 1 << 40                   # a workspace size no check finds short


def A(**kw):
    """The knobs of one call: dt the dtype, P a pointer or None, n the rows (0: the empty shape, -1: a bad one), dld / dbs what is added
    to a good leading dimension / batch stride (-1: a bad one), b the batch, sel / sel2 the mode-like arguments (0 is valid for all of
    them), ws the workspace bytes, x a free extra"""
    a = dict(dt=F32, P=P, n=4, dld=0, dbs=0, b=1, sel=0, sel2=0, ws=BIG, x=None)
    a.update(kw)
    return types.SimpleNamespace(**a)


def E(call, bad=REAL_BAD, word='dtype', null='dtype', ld=None, sel=None, ws=None, empty=(ARG, 'dtype'), extra=()):
    """One row.  call(lib, a) -> rc.  bad: the dtypes refused, under `word`.  What is reported (a word of pm_last_error) when a bad dtype
    meets a null pointer (null), a leading dimension below the row (ld) or a short workspace (ws), and when a bad mode-like argument
    meets a bad shape (sel); None where the entry point has no such argument.  empty: (rc, word) of an empty shape with a bad dtype.
    extra: further pins, (label, knobs, rc, word)."""
    return types.SimpleNamespace(call=call, bad=bad, word=word, null=null, ld=ld, sel=sel, ws=ws, empty=empty, extra=tuple(extra))


def _walk(fn, project=False, sums=False):
    def call(lib, a):
        head = (a.dt, a.sel, a.n, a.P, a.P, a.P, 3, 10)
        if project:
            return getattr(lib, fn)(*head, a.b, a.P, a.P, a.P, a.ws, None)
        if sums:
            return getattr(lib, fn)(*head, a.b, a.P, 0, a.P, None)
        return getattr(lib, fn)(*head, a.P, None)
    return call


def _segment(fn, project=False):
    def call(lib, a):
        head = (a.dt, a.sel, a.n, C, a.P, a.P, 3, a.P, a.P)
        if project:
            return getattr(lib, fn)(*head, 8, a.P, 3, 10, a.P, a.b, a.P, a.P, a.P, a.ws, None)
        return getattr(lib, fn)(*head, 2, a.P, a.P, 3, 10, a.P, a.b, a.P, 0, a.P, None)
    return call


def _planes(a):
    return (a.P, C, 1, a.n * C) * 4


ENTRIES = {
    # ---- zernike.hip: the dtype, the coordinates, then pointers and sizes
    'pm_zernike_basis': E(_walk('pm_zernike_basis'), sel='coords'),
    'pm_zernike_sum': E(_walk('pm_zernike_sum', sums=True), sel='coords'),
    'pm_zernike_project': E(_walk('pm_zernike_project', project=True), sel='coords', ws='dtype', extra=[
        ('short workspace', dict(ws=0), WS, 'workspace'), ('no vector before the workspace', dict(b=0, ws=0), 0, None)]),
    'pm_modes_dot': E(lambda lib, a: lib.pm_modes_dot(a.dt, 10, a.n, a.P, a.n + a.dld, a.P, a.P, a.P, a.ws, None), ld='dtype', ws='dtype',
                      extra=[('stride below npts', dict(dld=-1), ARG, 'mode_stride'), ('short workspace', dict(ws=0), WS, 'workspace')]),
    # ---- qpoly.hip: as zernike.hip
    'pm_qpoly_basis': E(_walk('pm_qpoly_basis'), sel='coords'),
    'pm_qpoly_sum': E(_walk('pm_qpoly_sum', sums=True), sel='coords'),
    'pm_qpoly_project': E(_walk('pm_qpoly_project', project=True), sel='coords', ws='dtype',
                          extra=[('short workspace', dict(ws=0), WS, 'workspace')]),
    # ---- segmented.hip: the dtype, the source, then sizes, then pointers
    'pm_segment_plan_check': E(lambda lib, a: lib.pm_segment_plan_check(a.n, C, 0 if a.P else 1, a.P, 16, 10, -1), bad=(), null=None, empty=None,
                               extra=[('null plan', dict(P=None), ARG, 'null plan'), ('no segment', dict(), 0, None)]),
    'pm_segment_compose': E(_segment('pm_segment_compose'), sel='source'),
    'pm_segment_project': E(_segment('pm_segment_project', project=True), sel='source', ws='dtype',
                            extra=[('short workspace', dict(ws=0), WS, 'workspace')]),
    # ---- geometry.hip: the dtype first
    'pm_xy_grid': E(lambda lib, a: lib.pm_xy_grid(a.dt, a.n, a.n and C, 0.1, 1, a.P, a.P, None)),
    'pm_cart_to_polar': E(lambda lib, a: lib.pm_cart_to_polar(a.dt, a.n, C, 0, a.P, a.P, a.P, a.P, None)),
    'pm_polar_to_cart': E(lambda lib, a: lib.pm_polar_to_cart(a.dt, a.n, a.P, a.P, a.P, a.P, None)),
    'pm_sdf_render': E(lambda lib, a: lib.pm_sdf_render(a.dt, a.sel, a.n, C, a.P, a.P, 0, 0, 0.1, 0.1, a.P, 3, a.b, a.sel2, 0.1, a.P, C + a.dld,
                                                        a.n * C + a.dbs, None), ld='dtype', sel='coords', extra=[
        ('out_kind after coords', dict(sel=77, sel2=77), ARG, 'coords'), ('out_kind before the shape', dict(sel2=77, n=-1), ARG, 'out_kind'),
        ('ld below the row', dict(dld=-1), ARG, 'out_ld'), ('overlapping stack', dict(b=2, dbs=-1), ARG, 'out_bstride'),
        ('one program may have any stride, and no row is no work', dict(dbs=-1, n=0), 0, None)]),
    # ---- detector.hip
    'pm_bindown': E(lambda lib, a: lib.pm_bindown(a.dt, a.b, a.n, C, 2, 2, a.sel, a.P, 2 * C + a.dld, 4 * a.n * C + a.dbs, a.P, C, a.n * C, None),
                    ld='dtype', sel='mode', extra=[
        ('the mode before the dtype', dict(dt=99, sel=77), ARG, 'mode'), ('ld below the row', dict(dld=-1), ARG, 'leading dimension'),
        ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride')]),
    'pm_tile': E(lambda lib, a: lib.pm_tile(a.dt, a.b, a.n, C, 2, 2, a.x or 1.0, a.P, C, a.n * C, a.P, 2 * C + a.dld, 4 * a.n * C + a.dbs, None),
                 ld='dtype', extra=[
        ('the scale before the dtype', dict(dt=99, x=float('inf')), ARG, 'scale'), ('ld below the row', dict(dld=-1), ARG, 'leading dimension'),
        ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride')]),
    'pm_detector_digitize': E(lambda lib, a: lib.pm_detector_digitize(a.dt, a.b, a.n, C, a.P, C + a.dld, a.n * C + a.dbs, 0.0, 1e5, 1.0,
                                                                      a.x or 12, None, 0, a.sel or 2, a.P, None), ld='dtype', extra=[
        ('bits before the shape', dict(x=40, n=-1), ARG, 'bits'), ('ld below the row', dict(dld=-1), ARG, 'smaller than the row'),
        ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride'), ('ld before the width', dict(dld=-1, sel=3), ARG, 'smaller than the row'),
        ('a width of 3 bytes', dict(sel=3), ARG, 'out_bytes'), ('12 bits in one byte', dict(sel=1), ARG, 'do not fit')]),
    'pm_detector_expose': E(lambda lib, a: lib.pm_detector_expose(a.dt, a.b, a.n, C, a.P, C + a.dld, a.n * C + a.dbs, None, None, 1.0, 0.0, 0.0,
                                                                  0.0, 1e5, 1.0, a.x or 12, None, 0, a.sel or 2, 1, 7, 0, a.P, a.P, None),
                            ld='dtype', extra=[
        ('bits before the shape', dict(x=40, n=-1), ARG, 'bits'), ('ld below the row', dict(dld=-1), ARG, 'smaller than the row'),
        ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride'), ('a width of 3 bytes', dict(sel=3), ARG, 'out_bytes')]),
    'pm_detector_words': E(lambda lib, a: lib.pm_detector_words(7, 0, a.n, 0, 0, a.P, None), bad=(), null=None, empty=None,
                           extra=[('null out', dict(P=None), ARG, 'null pointer'), ('no pixel', dict(n=0), 0, None)]),
    # ---- dm.hip: pm_lattice looks at its op first, pm_warp at its dtype and then at the order
    'pm_lattice': E(lambda lib, a: lib.pm_lattice(a.dt, a.sel, a.b if a.n else 0, a.n or 4, C, 2, 2, 0, 0, 2, 2, 1.0, a.P, 2 + a.dld, 4, a.P, C, 4 * C,
                                                  None), ld='dtype', sel=None, extra=[
        ('the op before the dtype', dict(dt=99, sel=77), ARG, 'op'), ('in_ld below the row', dict(dld=-1), ARG, 'in_ld')]),
    'pm_lattice (gather)': E(lambda lib, a: lib.pm_lattice(a.dt, L.PM_LATTICE_GATHER, a.b if a.n else 0, a.n or 4, C, 2, 2, 0, 0, 2, 2, 1.0, a.P,
                                                           C + a.dld, 4 * C, a.P, 2, 4, None), bad=(99, L.PM_BOOL), ld='dtype'),
    'pm_warp': E(lambda lib, a: lib.pm_warp(a.dt, a.x or 3, a.b if a.n else 0, a.n or 4, C, a.P, C + a.dld, 4 * C, D9, 1.0, 4, C, 0, 0, a.P, C,
                                            4 * C, a.P, a.ws, None), bad=(99, L.PM_BOOL), ld='dtype', ws='dtype', extra=[
        ('the dtype before the order', dict(dt=99, x=1), ARG, 'dtype'), ('order 1', dict(x=1), UNSUP, 'order'),
        ('the order before the pointers', dict(x=1, P=None), UNSUP, 'order'), ('short workspace', dict(ws=0), WS, 'workspace')]),
    # ---- ee.hip: everything else first ("bad argument"), then the dtype, then the workspace; no empty return
    'pm_encircled_energy': E(lambda lib, a: lib.pm_encircled_energy(a.dt, a.n, C, a.P, C + a.dld, 0.1, 1, D9, a.P, a.P, a.ws, None),
                             bad=(F32, F64, 99), null='bad argument', ld='bad argument', ws='dtype', empty=(ARG, 'bad argument'),
                             extra=[('short workspace', dict(dt=L.PM_C64, ws=0), WS, 'workspace')]),
    'pm_encircled_energy_adjoint': E(lambda lib, a: lib.pm_encircled_energy_adjoint(a.dt, a.n, C, 0.1, 1, D9, D9, a.P, C + a.dld, None),
                                     bad=(F32, F64, 99), null='bad argument', ld='bad argument', empty=(ARG, 'bad argument')),
    # ---- bayer.hip: the dtype, the mode-like arguments, the shape, the strides, then the pointers; no empty return
    'pm_bayer_demosaic': E(lambda lib, a: lib.pm_bayer_demosaic(a.x if a.x is not None else a.dt, a.dt, a.sel, 0, a.b, a.n, C, a.P, C + a.dld,
                                                                a.n * C + a.dbs, a.P, None), ld='dtype', sel='cfa', extra=[
        ('a float mosaic of the other precision', dict(x=F64), ARG, 'in dtype'), ('the empty shape', dict(n=0), ARG, 'at least 1'),
        ('ld below the row', dict(dld=-1), ARG, 'row stride'), ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride'),
        ('the strides before the pointers', dict(dld=-1, P=None), ARG, 'row stride'), ('null', dict(P=None), ARG, 'null pointer')]),
    'pm_bayer_weave': E(lambda lib, a: lib.pm_bayer_weave(a.dt, a.sel, a.sel2, a.b, a.n, C, *_planes(a), a.P, C + a.dld, a.n * C + a.dbs, None),
                        ld='dtype', sel='mode', extra=[
        ('cfa after the mode', dict(sel=77, sel2=77), ARG, 'mode'), ('cfa before the shape', dict(sel2=77, n=-1), ARG, 'cfa'),
        ('ld below the row', dict(dld=-1), ARG, 'row stride'), ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride')]),
    'pm_bayer_deinterlace': E(lambda lib, a: lib.pm_bayer_deinterlace(a.dt, a.sel, a.b, a.n, C, a.P, C + a.dld, a.n * C + a.dbs, a.P, None),
                              ld='dtype', sel='cfa', extra=[('odd rows after the strides', dict(n=3, dld=-1), ARG, 'row stride'),
                                                            ('odd rows', dict(n=3), ARG, 'even')]),
    'pm_bayer_assemble': E(lambda lib, a: lib.pm_bayer_assemble(a.dt, a.b, a.n, C, *_planes(a), a.P, None),
                           extra=[('the empty shape', dict(n=0), ARG, 'at least 1')]),
    'pm_bayer_class_max': E(lambda lib, a: lib.pm_bayer_class_max(a.dt, a.sel, a.b, a.n, C, a.P, C + a.dld, a.n * C + a.dbs, a.P, a.P, a.ws, None),
                            ld='dtype', sel='classes', ws='dtype', extra=[
        ('short workspace', dict(ws=0), WS, 'workspace'), ('the pointers before the workspace', dict(ws=0, P=None), ARG, 'null pointer'),
        ('an RGB row is 3 n long', dict(sel=L.PM_BAYER_RGB), ARG, 'row stride')]),
    'pm_bayer_scale': E(lambda lib, a: lib.pm_bayer_scale(a.dt, a.sel, a.sel2, a.b, a.n, C, a.P, C + a.dld, a.n * C + a.dbs, D9 if a.P else None, 0,
                                                          None, None, None), ld='dtype', sel='classes', extra=[
        ('cfa after the classes', dict(sel=77, sel2=77), ARG, 'classes'), ('cfa before the shape', dict(sel2=77, n=-1), ARG, 'cfa'),
        ('overlapping stack', dict(b=2, dbs=-1), ARG, 'bstride')]),
}

# name: (call(lib, dtype), the dtypes that give 0, {dtype: the bytes of a good call})
WORKSPACES = {
    'pm_zernike_project_workspace': (lambda lib, dt: lib.pm_zernike_project_workspace(dt, 1027, 10, 15), REAL_BAD, {F32: 2 * 15 * 10 * 4, F64: 2400}),
    'pm_modes_dot_workspace': (lambda lib, dt: lib.pm_modes_dot_workspace(dt, 10, 2049), REAL_BAD, {F32: 2 * 10 * 4, F64: 160}),
    'pm_qpoly_project_workspace': (lambda lib, dt: lib.pm_qpoly_project_workspace(dt, 1 << 21, 10, 15), REAL_BAD,
                                   {F32: 1024 * 15 * 10 * 4, F64: 1024 * 15 * 10 * 8}),
    'pm_segment_project_workspace': (lambda lib, dt: lib.pm_segment_project_workspace(dt, 5000, 3, 10, 15), REAL_BAD,
                                     {F32: 5 * 15 * 3 * 10 * 4, F64: 5 * 15 * 3 * 10 * 8}),
    'pm_segment_project_workspace (group cap)': (lambda lib, dt: lib.pm_segment_project_workspace(dt, 1 << 20, 1, 1, 1), REAL_BAD,
                                                 {F32: 256 * 4, F64: 256 * 8}),
    'pm_warp_workspace': (lambda lib, dt: lib.pm_warp_workspace(dt, 2, 3, 4), (99, L.PM_BOOL),
                          {F32: 96, L.PM_C64: 96, F64: 192, L.PM_C128: 192}),
    'pm_encircled_energy_workspace': (lambda lib, dt: lib.pm_encircled_energy_workspace(), (), {F32: 1024 * 8 * 8}),
    'pm_bayer_class_max_workspace': (lambda lib, dt: lib.pm_bayer_class_max_workspace(), (), {F32: 4096 * 4 * 8}),
}


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _expect(lib, rc, name, want_rc, word, what):
    msg = lib.pm_last_error().decode()
    assert rc == want_rc, (name, what, rc, msg)
    if want_rc:
        assert name.split(' ')[0] in msg and word in msg, (name, what, msg)


def _with(kind):
    return [n for n, e in ENTRIES.items() if getattr(e, kind) is not None and e.bad]


def test_every_entry_point_of_the_eight_units_has_a_row():
    """the extern "C" functions of the eight units, read from their sources, against the two tables"""
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), 'csrc')
    names = set()
    for unit in ('zernike', 'qpoly', 'segmented', 'geometry', 'detector', 'dm', 'ee', 'bayer'):
        with open(os.path.join(src, unit + '.hip')) as f:
            text = f.read()
        names |= set(re.findall(r'^(?:int|size_t) (pm_\w+)\(', text[text.index('extern "C"'):], re.M))
    assert len(names) == 36
    assert names == {n.split(' ')[0] for n in list(ENTRIES) + list(WORKSPACES)}


@pytest.mark.parametrize('name', [n for n, e in ENTRIES.items() if e.bad])
def test_bad_dtype_is_refused(lib, name):
    e = ENTRIES[name]
    for dt in e.bad:
        _expect(lib, e.call(lib, A(dt=dt)), name, ARG, e.word, dt)


@pytest.mark.parametrize('name', _with('null'))
def test_bad_dtype_and_null_pointer(lib, name):
    e = ENTRIES[name]
    for dt in e.bad:
        _expect(lib, e.call(lib, A(dt=dt, P=None)), name, ARG, e.null, dt)


@pytest.mark.parametrize('name', _with('ld'))
def test_bad_dtype_and_bad_leading_dimension(lib, name):
    e = ENTRIES[name]
    for dt in e.bad:
        _expect(lib, e.call(lib, A(dt=dt, dld=-1)), name, ARG, e.ld, dt)


@pytest.mark.parametrize('name', _with('sel'))
def test_bad_mode_and_bad_shape(lib, name):
    """cfa / coords / mode / source / classes = 77 with a negative row count: the mode-like argument is reported"""
    e = ENTRIES[name]
    _expect(lib, e.call(lib, A(sel=77, n=-1)), name, ARG, e.sel, 'sel')


@pytest.mark.parametrize('name', _with('ws'))
def test_short_workspace_and_bad_dtype(lib, name):
    e = ENTRIES[name]
    for dt in e.bad:
        _expect(lib, e.call(lib, A(dt=dt, ws=0)), name, ARG, e.ws, dt)


@pytest.mark.parametrize('name', _with('empty'))
def test_empty_shape_with_bad_dtype(lib, name):
    e = ENTRIES[name]
    for dt in e.bad:
        _expect(lib, e.call(lib, A(dt=dt, n=0)), name, e.empty[0], e.empty[1], dt)


@pytest.mark.parametrize('name,label', [(n, x[0]) for n, e in ENTRIES.items() for x in e.extra])
def test_further_pins(lib, name, label):
    _, knobs, rc, word = next(x for x in ENTRIES[name].extra if x[0] == label)
    _expect(lib, ENTRIES[name].call(lib, A(**knobs)), name, rc, word, label)


@pytest.mark.parametrize('name', list(WORKSPACES))
def test_workspace_sizes(lib, name):
    call, bad, good = WORKSPACES[name]
    for dt in bad:
        assert call(lib, dt) == 0, (name, dt)
    for dt, nbytes in good.items():
        assert call(lib, dt) == nbytes, (name, dt)
