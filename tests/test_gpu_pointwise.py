"""The pointwise, synthesis and resampling kernels (csrc/pointwise.hip, csrc/ee.hip) called at the C ABI: leading dimensions above the
width, bases that are not 16-byte aligned, guard bands of sentinels around every output, more than 262140 rows (the grid-stride step
of the row loop), phases of up to 1e6 rad against an exact reference, and np.pad / scipy / mpmath for the rest.

Bounds that were MEASURED on an MI355X (the project states no error for the device atan2, sqrt and j1); everything else is derived
next to its constant.

    quantity                         measured (largest)   bound in the test   margin
    -------------------------------  -------------------  ------------------  -----------------------------------------
    pm_abs_arg |z|,   fp32  (sqrt)   1.030 ulp            3 ulp               2x, rounded up to a whole ulp (8 at most)
    pm_abs_arg |z|,   fp64  (sqrt)   0.958 ulp            2 ulp               2x, rounded up to a whole ulp (8 at most)
    pm_abs_arg arg z, fp32  (atan2)  2.037 ulp            5 ulp               2x, rounded up to a whole ulp (8 at most)
    pm_abs_arg arg z, fp64  (atan2)  1.350 ulp            3 ulp               2x, rounded up to a whole ulp (8 at most)
    pm_encircled_energy     (j1)     4.74e-16 relative    1.9e-15 relative    4x (1e-10 at most)

|z| and arg z: against mpmath at 40 digits, in units in the last place of the result type, over the inputs of
test_abs_arg_layouts.  Encircled energy: |EE - ref| / |ref| against the mpmath / fsum reference over the shapes, precisions and radii
of test_encircled_energy (the same figure for a float32 and a float64 MTF: the values are float32 numbers and the sums are fp64).
"""
import ctypes
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import pointwise_common as PC
from conftest import rel_max
from pointwise_common import LD, window

pytestmark = pytest.mark.gpu

# measured bounds (the table above): ulps of the result type
ABS_ULP_BOUND = {'complex64': 3.0, 'complex128': 2.0}
ARG_ULP_BOUND = {'complex64': 5.0, 'complex128': 3.0}
EE_REL_BOUND = 1.9e-15

CDTYPES = ['complex64', 'complex128']
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope='module')
def env():
    from prysm_amd import _lib as L
    lib = L.load()
    assert torch.cuda.is_available()
    return L, lib


def code_of(L, cdtype):
    return L.PM_C64 if np.dtype(cdtype) == np.dtype('complex64') else L.PM_C128


def ok(L, rc):
    assert rc == 0, (rc, L.load().pm_last_error())
    torch.cuda.synchronize()


def within(got, ref, S, c, rdtype, what=''):
    """|got - ref| <= c eps_T S element by element (longdouble reference)"""
    eps = LD(np.finfo(rdtype).eps)
    err = np.abs(np.asarray(got).astype(LD) - ref)
    lim = c * eps * S
    bad = err > lim
    if bad.any():
        i = np.unravel_index(np.argmax(err - lim), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} elements beyond {c} eps S; worst at {i}: err {float(err[i]):.3e}, limit {float(lim[i]):.3e}')


def within_complex(got, rr, ri, sr, si, c, rdtype, what=''):
    within(got.real, rr, sr, c, rdtype, what + ' (real)')
    within(got.imag, ri, si, c, rdtype, what + ' (imag)')


# =========================================================================== layout sweep: arithmetic kernels
# c = (roundings of one output component, counted in csrc/pointwise.hip and csrc/pm_common.h) + 1.  Every rounding is at most
# eps_T / 2 relative to a partial result that S bounds, so k roundings give at most ~ k eps_T S / 2: the bounds hold with a factor 2
# to spare, and a dropped conjugation, a wrong index or a missing term is an error of order S, 1e6 times the bound.
C_CMUL = 4          # cmul / cmulc: two products and one sum (3)
C_RMUL = 3          # scale * r (1), times a component of a (1)
C_SCALE_SEP = 8     # cscale(cx, scale) (1), cmul with ry (3), cmul with in (3)
C_ABS2 = 4          # two squares and a sum (3)
C_ABS2_ACC = 6      # ... times the weight (1), added to out (1)
C_OUTER = 4         # one cmul (3)


def c_sum_modes(nmodes):
    return nmodes + 2   # SumModes: one multiply-add per mode (nmodes), the accumulated start value and the final store (2)


@pytest.mark.parametrize('cdtype', CDTYPES)
@pytest.mark.parametrize('op', [0, 1])
def test_cmul_layouts(env, cdtype, op):
    L, lib = env
    rng = np.random.default_rng(100 + op)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    for shape, pad, off in PC.layouts():
        a = window(shape, cdtype, *PC.other_layout(pad, off, 1), rng=rng)
        b = window(shape, cdtype, *PC.other_layout(pad, off, 2), rng=rng)
        o = window(shape, cdtype, pad, off)
        ok(L, lib.pm_cmul(code_of(L, cdtype), op, shape[0], shape[1], a.ptr, a.ld, b.ptr, b.ld, o.ptr, o.ld, L.stream_ptr()))
        within_complex(o.data(), *PC.ref_cmul(a.data(), b.data(), conj_b=bool(op)), C_CMUL, rd, f'pm_cmul op {op} {shape} {pad} {off}')
        o.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_rmul_layouts(env, cdtype):
    L, lib = env
    rng = np.random.default_rng(101)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    scale = 0.3
    for shape, pad, off in PC.layouts():
        r = window(shape, rd, *PC.other_layout(pad, off, 1), rng=rng)
        a = window(shape, cdtype, *PC.other_layout(pad, off, 2), rng=rng)
        o = window(shape, cdtype, pad, off)
        ok(L, lib.pm_rmul(code_of(L, cdtype), shape[0], shape[1], r.ptr, r.ld, a.ptr, a.ld, scale, o.ptr, o.ld, L.stream_ptr()))
        f = LD(rd.type(scale)) * r.data().astype(LD)        # the scale as the kernel holds it: converted to T
        ar, ai = a.data().real.astype(LD), a.data().imag.astype(LD)
        within_complex(o.data(), f * ar, f * ai, np.abs(f * ar), np.abs(f * ai), C_RMUL, rd, f'pm_rmul {shape} {pad} {off}')
        o.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_scale_sep_layouts(env, cdtype):
    L, lib = env
    rng = np.random.default_rng(102)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    scale = -1.7
    flags = [(ry, cx) for ry in (None, 0, 1) for cx in (None, 0, 1)]     # absent, present, conjugated
    for n, (shape, pad, off) in enumerate(PC.layouts()):
        rows, cols = shape
        x = window(shape, cdtype, *PC.other_layout(pad, off, 1), rng=rng)
        ry = window((1, rows), cdtype, 0, off, rng=rng)
        cx = window((1, cols), cdtype, 0, 1 - off, rng=rng)
        tall = rows > 1000
        for ryf, cxf in ([flags[n % 9]] if tall else flags):
            o = window(shape, cdtype, pad, off)
            ok(L, lib.pm_scale_sep(code_of(L, cdtype), rows, cols, x.ptr, x.ld, NULL if ryf is None else ry.ptr, ryf or 0,
                                   NULL if cxf is None else cx.ptr, cxf or 0, scale, o.ptr, o.ld, L.stream_ptr()))
            s = LD(rd.type(scale))
            fr, fi = np.full((1, cols), s), np.zeros((1, cols), LD)
            sr, si = np.abs(fr), np.zeros((1, cols), LD)
            if cxf is not None:
                w = cx.data()
                fr, fi = s * w.real.astype(LD), s * (-w.imag if cxf else w.imag).astype(LD)
                sr, si = np.abs(fr), np.abs(fi)
            if ryf is not None:
                fr, fi, sr, si = PC.ref_cmul_parts(fr, fi, sr, si, ry.data().reshape(rows, 1), conj_b=bool(ryf))
            fr, fi, sr, si = PC.ref_cmul_parts(fr, fi, sr, si, x.data())
            within_complex(o.data(), fr, fi, sr, si, C_SCALE_SEP, rd, f'pm_scale_sep ry {ryf} cx {cxf} {shape} {pad} {off}')
            o.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_abs2_layouts(env, cdtype):
    L, lib = env
    rng = np.random.default_rng(103)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    weight = 0.6
    for shape, pad, off in PC.layouts():
        x = window(shape, cdtype, *PC.other_layout(pad, off, 1), rng=rng)
        o = window(shape, rd, pad, off, rng=rng)
        before = o.data()
        i2 = PC.ref_abs2(x.data())
        ok(L, lib.pm_abs2(code_of(L, cdtype), shape[0], shape[1], x.ptr, x.ld, o.ptr, o.ld, 1, weight, L.stream_ptr()))
        term = LD(rd.type(weight)) * i2
        within(o.data(), before.astype(LD) + term, np.abs(before.astype(LD)) + term, C_ABS2_ACC, rd, f'pm_abs2 accumulate {shape} {pad} {off}')
        o.check_guards()
        ok(L, lib.pm_abs2(code_of(L, cdtype), shape[0], shape[1], x.ptr, x.ld, o.ptr, o.ld, 0, weight, L.stream_ptr()))   # the weight is not applied
        within(o.data(), i2, i2, C_ABS2, rd, f'pm_abs2 store {shape} {pad} {off}')
        o.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_outer_layouts(env, cdtype):
    L, lib = env
    rng = np.random.default_rng(104)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    for shape, pad, off in PC.layouts():
        rows, cols = shape
        hy = window((1, rows), cdtype, 0, off, rng=rng)
        hx = window((1, cols), cdtype, 0, 1 - off, rng=rng)
        o = window(shape, cdtype, pad, off)
        ok(L, lib.pm_outer(code_of(L, cdtype), rows, cols, hy.ptr, hx.ptr, o.ptr, o.ld, L.stream_ptr()))
        within_complex(o.data(), *PC.ref_cmul(hy.data().reshape(rows, 1), hx.data()), C_OUTER, rd, f'pm_outer {shape} {pad} {off}')
        o.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_sum_modes_layouts(env, cdtype, accumulate):
    L, lib = env
    rng = np.random.default_rng(105 + accumulate)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    counts = (0, 1, 32, 33, 70)         # none, one, a full launch of 32, one more, three launches
    for n, (shape, pad, off) in enumerate(PC.layouts()):
        rows, cols = shape
        tall = rows > 1000
        for nmodes in ([3] if tall else counts if n % 6 == 0 else [counts[n % 5]]):
            ipad, ioff = PC.other_layout(pad, off, 1)
            m = window((max(nmodes, 1) * rows, cols), rd, ipad, ioff, rng=rng)       # the modes stacked: mode b starts rows * ld further on
            o = window(shape, rd, pad, off, rng=rng)
            before = o.data()
            w = rng.standard_normal(max(nmodes, 1))
            arr = (ctypes.c_double * len(w))(*w)
            ok(L, lib.pm_sum_modes(code_of(L, cdtype), nmodes, rows, cols, m.ptr, rows * m.ld, m.ld, arr, accumulate, o.ptr, o.ld,
                                   L.stream_ptr()))
            got = o.data()
            what = f'pm_sum_modes {nmodes} modes acc {accumulate} {shape} {pad} {off}'
            if nmodes == 0 and accumulate:
                assert np.array_equal(got.view(np.uint8), before.view(np.uint8)), what + ': out must stay untouched'
            else:
                modes = m.data().reshape(max(nmodes, 1), rows, cols)[:nmodes]
                ref, S = PC.ref_sum_modes(modes, w.astype(rd), before if accumulate else None)
                if nmodes == 0:
                    assert np.all(got == 0), what
                within(got, ref, S, c_sum_modes(nmodes), rd, what)
            o.check_guards()


# =========================================================================== modulus and phase
def _abs_arg_inputs(rng, shape, cdtype):
    """all four quadrants, the axes, zero, signed zeros on the negative and the positive real axis, and magnitudes over the range
    whose squares stay normal numbers: 1e-30 .. 1e30 in fp64, 1e-15 .. 1e15 in fp32"""
    rd = PC.REAL_OF[np.dtype(cdtype)]
    n = shape[0] * shape[1]
    span = 30 if rd == np.dtype('float64') else 15
    mag = 10.0 ** rng.uniform(-span, span, n)
    ang = rng.uniform(-np.pi, np.pi, n)
    z = (mag * np.exp(1j * ang)).astype(cdtype)
    special = [complex(0.0, 0.0), complex(-1.0, 0.0), complex(-1.0, -0.0), complex(1.0, 0.0), complex(1.0, -0.0), complex(0.0, 2.0),
               complex(0.0, -2.0), complex(-3.0, 4.0), complex(10.0 ** span, 10.0 ** span), complex(10.0 ** -span, -10.0 ** -span)]
    k = min(n, len(special))
    z[:k] = np.array(special[:k], dtype=cdtype)
    return z.reshape(shape)


def _ulp_errors(got_abs, got_arg, z, rd, idx):
    worst_abs = worst_arg = 0.0
    zf = z.ravel()
    with mpmath.workdps(40):
        for i in idx:
            x, y = mpmath.mpf(float(zf[i].real)), mpmath.mpf(float(zf[i].imag))
            if got_abs is not None:
                worst_abs = max(worst_abs, PC.ulps(got_abs.ravel()[i], mpmath.sqrt(x * x + y * y), rd))
            if got_arg is not None:
                want = mpmath.atan2(y, x)
                if float(zf[i].imag) == 0.0 and float(zf[i].real) < 0 and math.copysign(1.0, float(zf[i].imag)) < 0:
                    want = -mpmath.pi           # atan2(-0, x < 0) = -pi: mpmath has no signed zero
                worst_arg = max(worst_arg, PC.ulps(got_arg.ravel()[i], want, rd))
    return worst_abs, worst_arg


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_abs_arg_layouts(env, cdtype):
    L, lib = env
    rng = np.random.default_rng(106)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    worst = [0.0, 0.0]
    for shape, pad, off in PC.layouts():
        z = _abs_arg_inputs(rng, shape, cdtype)
        x = window(shape, cdtype, *PC.other_layout(pad, off, 1), data=z)
        idx = PC.sample_indices(rng, shape, 1024)
        for which in ('both', 'abs', 'arg'):
            oa = window(shape, rd, pad, off)
            og = window(shape, rd, *PC.other_layout(pad, off, 2))
            ok(L, lib.pm_abs_arg(code_of(L, cdtype), shape[0], shape[1], x.ptr, x.ld, NULL if which == 'arg' else oa.ptr, oa.ld,
                                 NULL if which == 'abs' else og.ptr, og.ld, L.stream_ptr()))
            oa.check_guards()
            og.check_guards()
            ga = None if which == 'arg' else oa.data()
            gg = None if which == 'abs' else og.data()
            if which == 'both':
                first_a, first_g = ga, gg
                ua, ug = _ulp_errors(ga, gg, z, rd, idx)
                worst = [max(worst[0], ua), max(worst[1], ug)]
                # every element, against numpy in the same precision (itself good to an ulp): an indexing error is not a matter of ulps
                z64 = z.astype(np.complex128)
                assert np.all(np.abs(ga - np.abs(z64)) <= (ABS_ULP_BOUND[cdtype] + 1) * np.spacing(np.abs(z64).astype(rd)).astype(np.float64))
                assert np.all(np.abs(gg - np.angle(z64)) <= (ARG_ULP_BOUND[cdtype] + 1) * np.spacing(np.abs(np.angle(z64)).astype(rd)).astype(np.float64) + 0.0)
                # signs of the zeros: atan2(+-0, -1) = +-pi, atan2(+-0, 1) = +-0, |0| = 0
                flat = z.ravel()
                for i in range(min(flat.size, 5)):
                    if flat[i].imag == 0:
                        assert math.copysign(1.0, float(gg.ravel()[i])) == math.copysign(1.0, float(flat[i].imag)), (i, flat[i], gg.ravel()[i])
                assert ga.ravel()[0] == 0 and gg.ravel()[0] == 0
            else:       # a NULL output leaves its buffer alone (its window still holds its zeros) and the other output is the same, bit for bit
                if ga is not None:
                    assert np.array_equal(ga.view(np.uint8), first_a.view(np.uint8)) and not og.data().any()
                if gg is not None:
                    assert np.array_equal(gg.view(np.uint8), first_g.view(np.uint8)) and not oa.data().any()
    print(f'MEASURED pm_abs_arg {cdtype}: |z| {worst[0]:.3f} ulp, arg z {worst[1]:.3f} ulp')
    assert worst[0] <= ABS_ULP_BOUND[cdtype] and worst[1] <= ARG_ULP_BOUND[cdtype], worst


# =========================================================================== embed / pad: bit-exact against numpy
ELEM_DTYPE = {1: np.dtype('uint8'), 4: np.dtype('uint32'), 8: np.dtype('uint64'), 16: np.dtype('complex128')}
# irows, icols, orows, ocols, off_y, off_x
EMBED_CASES = [
    (3, 5, 7, 9, 2, 3),          # pad
    (7, 9, 3, 5, -2, -3),        # crop (negative offsets)
    (3, 9, 7, 5, 2, -3),         # pad the rows, crop the columns
    (9, 3, 5, 70, -3, 66),       # crop the rows, pad the columns; more than one block of columns
    (3, 5, 4, 4, 10, 0),         # the input entirely below the output
    (3, 5, 4, 4, 0, -5),         # ... entirely to its left
    (1, 1, 1, 1, 0, 0),
    (1, 65, 1, 65, 0, 1),
    (4, 3, 262145, 3, 262140, 0),     # tall: rows past 4 * 65535 are reached only by the grid-stride step
]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize('elem', [1, 4, 8, 16])
def test_embed_bit_exact(env, elem):
    L, lib = env
    rng = np.random.default_rng(107 + elem)
    dt = ELEM_DTYPE[elem]
    for case in EMBED_CASES:
        ir, ic, orows, ocols, oy, ox = case
        layouts = [(1, 1)] if orows > 1000 else [(p, o) for p in PC.LD_PADS for o in PC.BASE_OFFS]
        for pad, off in layouts:
            x = window((ir, ic), dt, *PC.other_layout(pad, off, 1), rng=rng)
            o = window((orows, ocols), dt, pad, off, rng=rng)
            fill = PC.random_values(rng, (1,), dt)          # non-zero, every byte of it random
            ok(L, lib.pm_embed(elem, ir, ic, x.ptr, x.ld, orows, ocols, oy, ox, ctypes.c_void_p(fill.ctypes.data), o.ptr, o.ld,
                               L.stream_ptr()))
            want = PC.ref_embed(x.data(), (orows, ocols), (oy, ox), fill[0])
            assert np.array_equal(_bits(o.data()), _bits(want)), (case, pad, off)
            o.check_guards()
    # fill NULL: zeros
    x = window((2, 2), dt, rng=rng)
    o = window((4, 4), dt, 1, 1, rng=rng)
    ok(L, lib.pm_embed(elem, 2, 2, x.ptr, x.ld, 4, 4, 1, 1, NULL, o.ptr, o.ld, L.stream_ptr()))
    assert np.array_equal(_bits(o.data()), _bits(PC.ref_embed(x.data(), (4, 4), (1, 1), 0)))
    o.check_guards()


@pytest.mark.parametrize('elem', [1, 4, 8, 16])
def test_embed_layouts(env, elem):
    """the layout sweep with the named shapes as OUTPUT windows: an input of the same shape shifted one row down and two columns to
    the left, so that every case pads on one side and crops on the other"""
    L, lib = env
    rng = np.random.default_rng(123 + elem)
    dt = ELEM_DTYPE[elem]
    for shape, pad, off in PC.layouts():
        rows, cols = shape
        oy, ox = (1 if rows > 1 else 0), (-2 if cols > 2 else 0)
        x = window(shape, dt, *PC.other_layout(pad, off, 1), rng=rng)
        o = window(shape, dt, pad, off, rng=rng)
        fill = PC.random_values(rng, (1,), dt)
        ok(L, lib.pm_embed(elem, rows, cols, x.ptr, x.ld, rows, cols, oy, ox, ctypes.c_void_p(fill.ctypes.data), o.ptr, o.ld, L.stream_ptr()))
        assert np.array_equal(_bits(o.data()), _bits(PC.ref_embed(x.data(), shape, (oy, ox), fill[0]))), (shape, pad, off)
        o.check_guards()


@pytest.mark.parametrize('elem', [1, 4, 8, 16])
@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_pad_index_bit_exact(env, elem, mode):
    L, lib = env
    rng = np.random.default_rng(108 + 4 * elem + mode)
    dt = ELEM_DTYPE[elem]
    n = 0
    for m_, n_ in ((1, 1), (1, 5), (4, 1), (3, 5), (2, 66)):
        x0 = PC.random_values(rng, (m_, n_), dt)
        widths = lambda k: (0, 1, k - 1, k, 3 * k + 2)      # noqa: E731
        for i in range(5):
            before = (widths(m_)[i], widths(n_)[(i + 1) % 5])
            after = (widths(m_)[(i + 2) % 5], widths(n_)[(i + 3) % 5])
            pad, off = PC.LD_PADS[n % 3], PC.BASE_OFFS[(n // 3) % 2]
            n += 1
            x = window((m_, n_), dt, *PC.other_layout(pad, off, 1), data=x0)
            orows, ocols = m_ + before[0] + after[0], n_ + before[1] + after[1]
            o = window((orows, ocols), dt, pad, off, rng=rng)
            ok(L, lib.pm_pad_index(elem, mode, m_, n_, x.ptr, x.ld, orows, ocols, before[0], before[1], o.ptr, o.ld, L.stream_ptr()))
            want = np.pad(x0, ((before[0], after[0]), (before[1], after[1])), mode=PC.PAD_MODES[mode])
            assert np.array_equal(_bits(o.data()), _bits(want)), (mode, (m_, n_), before, after)
            o.check_guards()
    # tall: 262145 rows from 5
    x0 = PC.random_values(rng, (5, 3), dt)
    x = window((5, 3), dt, 7, 1, data=x0)
    o = window(PC.TALL_SHAPE, dt, 1, 1)
    ok(L, lib.pm_pad_index(elem, mode, 5, 3, x.ptr, x.ld, PC.TALL_SHAPE[0], 3, 100, 0, o.ptr, o.ld, L.stream_ptr()))
    want = np.pad(x0, ((100, PC.TALL_SHAPE[0] - 105), (0, 0)), mode=PC.PAD_MODES[mode])
    assert np.array_equal(_bits(o.data()), _bits(want))
    o.check_guards()


@pytest.mark.parametrize('elem', [1, 4, 8, 16])
@pytest.mark.parametrize('mode', [1, 2, 3, 4])
def test_pad_index_layouts(env, elem, mode):
    """the layout sweep with the named shapes as OUTPUT windows, filled from a small input placed inside them (64 rows for the tall
    shape, so that np.pad gets there in a few thousand steps)"""
    L, lib = env
    rng = np.random.default_rng(140 + 4 * elem + mode)
    dt = ELEM_DTYPE[elem]
    for shape, pad, off in PC.layouts():
        rows, cols = shape
        ir, ic = (64 if rows > 1000 else min(rows, 2)), min(cols, 5)
        oy, ox = (rows - ir) // 2, (cols - ic) // 3
        x0 = PC.random_values(rng, (ir, ic), dt)
        x = window((ir, ic), dt, *PC.other_layout(pad, off, 1), data=x0)
        o = window(shape, dt, pad, off, rng=rng)
        ok(L, lib.pm_pad_index(elem, mode, ir, ic, x.ptr, x.ld, rows, cols, oy, ox, o.ptr, o.ld, L.stream_ptr()))
        want = np.pad(x0, ((oy, rows - ir - oy), (ox, cols - ic - ox)), mode=PC.PAD_MODES[mode])
        assert np.array_equal(_bits(o.data()), _bits(want)), (mode, shape, pad, off)
        o.check_guards()


# =========================================================================== argument checks
def test_leading_dimension_below_cols_is_refused(env):
    """rows > 1 and a leading dimension below cols: PM_ERR_ARG and a message, nothing launched (every output keeps its bytes);
    one row takes any leading dimension."""
    L, lib = env
    rng = np.random.default_rng(109)
    cd, rd = np.dtype('complex64'), np.dtype('float32')
    R, C = 2, 8
    code = L.PM_C64
    a, b = window((R, C), cd, rng=rng), window((R, C), cd, rng=rng)
    r = window((R, C), rd, rng=rng)
    v = window((1, C), cd, rng=rng)
    o, o2 = window((R, C), cd, rng=rng), window((R, C), rd, rng=rng)
    coeff = window((R + 24, C + 24), np.complex128, rng=rng)
    w1 = (ctypes.c_double * 1)(1.0)
    s = L.stream_ptr()
    ld, bad = C, C - 1

    def calls():        # name -> (number of leading dimensions, the call given all of them)
        return {
            'pm_cmul': (3, lambda d: lib.pm_cmul(code, 0, R, C, a.ptr, d[0], b.ptr, d[1], o.ptr, d[2], s)),
            'pm_rmul': (3, lambda d: lib.pm_rmul(code, R, C, r.ptr, d[0], a.ptr, d[1], 1.0, o.ptr, d[2], s)),
            'pm_scale_sep': (2, lambda d: lib.pm_scale_sep(code, R, C, a.ptr, d[0], NULL, 0, v.ptr, 0, 1.0, o.ptr, d[1], s)),
            'pm_abs2': (2, lambda d: lib.pm_abs2(code, R, C, a.ptr, d[0], o2.ptr, d[1], 0, 1.0, s)),
            'pm_abs_arg': (3, lambda d: lib.pm_abs_arg(code, R, C, a.ptr, d[0], o2.ptr, d[1], r.ptr, d[2], s)),
            'pm_sum_modes': (2, lambda d: lib.pm_sum_modes(code, 1, R, C, r.ptr, R * C, d[0], w1, 0, o2.ptr, d[1], s)),
            'pm_pupil_synth': (3, lambda d: lib.pm_pupil_synth(code, R, C, r.ptr, L.PM_F32, d[0], r.ptr, d[1], 1.0, o.ptr, d[2], s)),
            'pm_quadratic_phase': (3, lambda d: lib.pm_quadratic_phase(code, R, C, r.ptr, d[0], r.ptr, d[1], 1.0, o.ptr, d[2], s)),
            'pm_outer': (1, lambda d: lib.pm_outer(code, R, C, v.ptr, v.ptr, o.ptr, d[0], s)),
            'pm_embed': (2, lambda d: lib.pm_embed(8, R, C, a.ptr, d[0], R, C, 0, 0, NULL, o.ptr, d[1], s)),
            'pm_pad_index': (2, lambda d: lib.pm_pad_index(8, 1, R, C, a.ptr, d[0], R, C, 0, 0, o.ptr, d[1], s)),
            'pm_mdft_basis': (1, lambda d: lib.pm_mdft_basis(code, R, C, r.ptr, r.ptr, 1, o.ptr, d[0], s)),
            'pm_mdft_basis_grid': (1, lambda d: lib.pm_mdft_basis_grid(code, R, C, 1.0, 0.0, 1.0, 1.0, 1, o.ptr, d[0], s)),
            'pm_sample_map': (3, lambda d: lib.pm_sample_map(code, 1, R, C, a.ptr, d[0], 1.0, 0.0, 0.0, R, C, r.ptr, C, 1, r.ptr, C, 1, b.ptr,
                                                             d[1], 0.0, 0.0, o.ptr, d[2], s)),
            'pm_sample_spline': (2, lambda d: lib.pm_sample_spline(code, 3, R, C, coeff.ptr, coeff.ld, 1.0, 0.0, 0.0, R, C, r.ptr, C, 1, r.ptr, C,
                                                                   1, b.ptr, d[0], 0.0, 0.0, o.ptr, d[1], s)),
        }
    table = calls()
    for name, (nld, fn) in table.items():
        for k in range(nld):
            d = [ld] * nld
            d[k] = bad
            rc = fn(d)
            assert rc == L.PM_ERR_ARG, (name, k, rc)
            msg = lib.pm_last_error().decode()
            assert name in msg and 'leading dimension' in msg, (name, msg)
    torch.cuda.synchronize()
    for w in (o, o2, r, a, b):
        assert np.array_equal(_bits(w.host()), _bits(w.initial)), 'an output changed although the call was refused'
    # one row: any leading dimension
    o1 = window((1, C), cd)
    ok(L, lib.pm_cmul(code, 0, 1, C, a.ptr, 0, b.ptr, 1, o1.ptr, 3, s))
    within_complex(o1.data(), *PC.ref_cmul(a.data()[:1], b.data()[:1]), C_CMUL, rd, 'pm_cmul, one row')
    o1.check_guards()


# =========================================================================== phase kernels against the exact reference
def check_phase(got, t64, turn_of, rd, rng, amp=None, product_roundings=2, extra_rel=0.0, limit=4096, what=''):
    """Every element against numpy (exp(2 pi i frac(t)) from the fp64 turns `t64`, itself off by one more fp64 rounding of t), and up
    to `limit` seeded samples against the exact reference under phase_bound (pointwise_common.phase_bound holds the derivation).
    turn_of(flat index) returns the exact turns as a Fraction."""
    shape = got.shape
    a64 = np.ones(shape) if amp is None else np.asarray(amp, dtype=np.float64)
    approx = a64 * np.exp(2j * np.pi * (t64 - np.rint(t64)))
    full = PC.phase_bound(rd, np.abs(t64).ravel(), a64.ravel(), product_roundings + 1, extra_rel).reshape(shape) + 4e-16 * np.abs(a64)
    err = np.maximum(np.abs(got.real - approx.real), np.abs(got.imag - approx.imag))
    assert np.all(err <= full), f'{what}: element {np.unravel_index(np.argmax(err - full), shape)} off by {err.max():.3e}'
    idx = PC.sample_indices(rng, shape, limit)
    turns = [turn_of(int(i)) for i in idx]
    amps = a64.ravel()[idx]
    e = PC.phase_errors(got.ravel()[idx], turns, amps)
    bound = PC.phase_bound(rd, turns, amps, product_roundings, extra_rel)
    ratio = float(np.max(e / bound))
    assert ratio <= 1.0, f'{what}: error / bound = {ratio:.3f} at sample {int(idx[np.argmax(e / bound)])} ({e.max():.3e})'
    return ratio


K_PUPIL = 9929.180537     # 2 pi / (0.6328 um) in rad / um, roughly: the value is arbitrary, the kernel sees k / (2 pi)
AMP_KINDS = ['none', 'f32', 'f64', 'bool']


def _run_pupil(env, cdtype, amp_kind, shape, pad, off, reach, rng, limit=4096):
    L, lib = env
    rd = PC.REAL_OF[np.dtype(cdtype)]
    rows, cols = shape
    opd0 = (rng.uniform(-1, 1, shape) * reach / K_PUPIL).astype(rd)
    opd0.ravel()[0] = rd.type(reach / K_PUPIL)           # |k opd| reaches `reach` rad
    opd0.ravel()[-1] = rd.type(-reach / K_PUPIL)
    opd = window(shape, rd, *PC.other_layout(pad, off, 1), data=opd0)
    adt = {'none': None, 'f32': np.dtype('float32'), 'f64': np.dtype('float64'), 'bool': np.dtype('uint8')}[amp_kind]
    acode = {'none': L.PM_F32, 'f32': L.PM_F32, 'f64': L.PM_F64, 'bool': L.PM_BOOL}[amp_kind]
    amp = amp0 = None
    if adt is not None:
        amp0 = (rng.random(shape) > 0.3).astype(adt) if amp_kind == 'bool' else (rng.uniform(-2, 2, shape)).astype(adt)
        amp = window(shape, adt, *PC.other_layout(pad, off, 2), data=amp0)
    o = window(shape, cdtype, pad, off)
    ok(L, lib.pm_pupil_synth(code_of(L, cdtype), rows, cols, NULL if amp is None else amp.ptr, acode, cols if amp is None else amp.ld,
                             opd.ptr, opd.ld, K_PUPIL, o.ptr, o.ld, L.stream_ptr()))
    o.check_guards()
    k2 = K_PUPIL / (2.0 * math.pi)                       # the host's division, the value the kernel receives
    fk2 = Fraction(k2)
    flat = opd0.ravel()
    return check_phase(o.data(), opd0.astype(np.float64) * k2, lambda i: Fraction(float(flat[i])) * fk2, rd, rng,
                       amp=None if amp0 is None else amp0.astype(np.float64), limit=limit,
                       what=f'pm_pupil_synth {cdtype} amp {amp_kind} {shape} {pad} {off} reach {reach:g}')


@pytest.mark.parametrize('cdtype', CDTYPES)
@pytest.mark.parametrize('amp_kind', AMP_KINDS)
def test_pupil_synth_phase_accuracy(env, cdtype, amp_kind):
    """|k opd| up to 1e3, 1e5 and 1e6 rad: at 1e6 rad the fp32 bound is still 6e-8 + 2e-10; a phase formed in fp32 has lost
    1e6 * 2^-24 = 0.06 rad there"""
    rng = np.random.default_rng(110)
    worst = max(_run_pupil(env, cdtype, amp_kind, (13, 67), 1, 1, reach, rng) for reach in (1e3, 1e5, 1e6))
    print(f'pm_pupil_synth {cdtype} amp {amp_kind}: error / bound = {worst:.3f}')


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_pupil_synth_layouts(env, cdtype):
    rng = np.random.default_rng(111)
    for n, (shape, pad, off) in enumerate(PC.layouts()):
        _run_pupil(env, cdtype, AMP_KINDS[n % 4], shape, pad, off, 1e3, rng, limit=128 if shape[0] < 1000 else 1024)


def _run_quadratic(env, cdtype, shape, pad, off, reach, rng, limit=4096):
    L, lib = env
    rd = PC.REAL_OF[np.dtype(cdtype)]
    c = 0.731 * reach                                    # x^2 + y^2 <= 1.37: the phase c (x^2 + y^2) reaches `reach` rad
    x0, y0 = rng.uniform(-0.82, 0.82, shape).astype(rd), rng.uniform(-0.82, 0.82, shape).astype(rd)
    x0.ravel()[0] = y0.ravel()[0] = rd.type(0.827)
    x = window(shape, rd, *PC.other_layout(pad, off, 1), data=x0)
    y = window(shape, rd, *PC.other_layout(pad, off, 2), data=y0)
    o = window(shape, cdtype, pad, off)
    ok(L, lib.pm_quadratic_phase(code_of(L, cdtype), shape[0], shape[1], x.ptr, x.ld, y.ptr, y.ld, c, o.ptr, o.ld, L.stream_ptr()))
    o.check_guards()
    c2 = c / (2.0 * math.pi)
    fc2 = Fraction(c2)
    xf, yf = x0.ravel(), y0.ravel()
    x64, y64 = x0.astype(np.float64), y0.astype(np.float64)
    return check_phase(o.data(), (x64 * x64 + y64 * y64) * c2, lambda i: (Fraction(float(xf[i])) ** 2 + Fraction(float(yf[i])) ** 2) * fc2,
                       rd, rng, limit=limit, what=f'pm_quadratic_phase {cdtype} {shape} {pad} {off} reach {reach:g}')


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_quadratic_phase_accuracy(env, cdtype):
    rng = np.random.default_rng(112)
    worst = max(_run_quadratic(env, cdtype, (13, 67), 7, 1, reach, rng) for reach in (1e3, 1e5, 1e6))
    print(f'pm_quadratic_phase {cdtype}: error / bound = {worst:.3f}')


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_quadratic_phase_layouts(env, cdtype):
    rng = np.random.default_rng(113)
    for shape, pad, off in PC.layouts():
        _run_quadratic(env, cdtype, shape, pad, off, 1e3, rng, limit=128 if shape[0] < 1000 else 1024)


def _run_mdft(env, cdtype, M, N, pad, off, sign, reach_turns, rng, limit=4096):
    L, lib = env
    rd = PC.REAL_OF[np.dtype(cdtype)]
    f0 = (rng.uniform(-1, 1, M) * reach_turns / 8).astype(rd)
    x0 = (rng.uniform(-1, 1, N) * 8).astype(rd)
    f0[0], x0[0] = rd.type(reach_turns / 8), rd.type(-8)
    f = window((1, M), rd, 0, off, data=f0)
    x = window((1, N), rd, 0, 1 - off, data=x0)
    E = window((M, N), cdtype, pad, off)
    ok(L, lib.pm_mdft_basis(code_of(L, cdtype), M, N, f.ptr, x.ptr, sign, E.ptr, E.ld, L.stream_ptr()))
    E.check_guards()
    t64 = sign * np.outer(f0.astype(np.float64), x0.astype(np.float64))
    return check_phase(E.data(), t64, lambda i: sign * Fraction(float(f0[i // N])) * Fraction(float(x0[i % N])), rd, rng, limit=limit,
                       what=f'pm_mdft_basis {cdtype} {M} x {N} {pad} {off} sign {sign}')


@pytest.mark.parametrize('cdtype', CDTYPES)
@pytest.mark.parametrize('sign', [1, -1])
def test_mdft_basis_accuracy(env, cdtype, sign):
    rng = np.random.default_rng(114)
    worst = max(_run_mdft(env, cdtype, 13, 67, 1, 1, sign, reach, rng) for reach in (1e2, 1e4, 1e5))
    print(f'pm_mdft_basis {cdtype} sign {sign}: error / bound = {worst:.3f}')


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_mdft_basis_layouts(env, cdtype):
    rng = np.random.default_rng(115)
    for n, ((M, N), pad, off) in enumerate(PC.layouts()):
        _run_mdft(env, cdtype, M, N, pad, off, 1 if n % 2 else -1, 1e2, rng, limit=128 if M < 1000 else 1024)


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_mdft_basis_grid_bit_equal_to_numpy_vectors(env, cdtype):
    """the grid variant equals pm_mdft_basis fed with the vectors numpy builds operation by operation in the real type"""
    L, lib = env
    rd = PC.REAL_OF[np.dtype(cdtype)]
    T = rd.type
    cases = [(5, 7, 0.0), (6, 8, 0.0), (5, 8, 0.37), (64, 33, -1.25), (1, 1, 0.5), (3, 129, 0.1)]
    for n, (M, N, f_shift) in enumerate(cases):
        f_step, f_scale, x_step = 0.0123, 1 / 0.6328, 0.0417
        x = (np.arange(-(N // 2), -(N // 2) + N).astype(rd) * T(x_step)).astype(rd)
        f = ((np.arange(-(M // 2), -(M // 2) + M).astype(rd) * T(f_step) + T(f_shift)) * T(f_scale)).astype(rd)
        assert x.dtype == rd and f.dtype == rd
        for sign in (1, -1):
            pad = PC.LD_PADS[n % 3]
            fw, xw = window((1, M), rd, data=f), window((1, N), rd, data=x)
            A = window((M, N), cdtype, pad, n % 2)
            B = window((M, N), cdtype, pad + 1, 1 - n % 2)        # E_ld > N in every case
            ok(L, lib.pm_mdft_basis(code_of(L, cdtype), M, N, fw.ptr, xw.ptr, sign, A.ptr, A.ld, L.stream_ptr()))
            ok(L, lib.pm_mdft_basis_grid(code_of(L, cdtype), M, N, f_step, f_shift, f_scale, x_step, sign, B.ptr, B.ld, L.stream_ptr()))
            assert np.array_equal(_bits(A.data()), _bits(B.data())), (M, N, f_shift, sign)
            B.check_guards()


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_as_tf_vectors_against_fftfreq(env, cdtype):
    """k = np.fft.fftfreq(n, dx).astype(real), then exp(2 pi i coef k^2) exactly.  The kernel forms k as i / (n d), numpy as
    i * (1 / (n d)): two fp64 values at most one ulp apart (each is within half an ulp plus 2^-53 relative of the quotient), which
    the square doubles -- extra_rel = 2^-51 on top of the two fp64 roundings of k * k * coef."""
    L, lib = env
    rng = np.random.default_rng(116)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    wvl, dx, z = 0.6328, 0.01, 1000.0
    coef = -(wvl / 1e3) * z * 0.5
    sizes = [1, 2, 5, 256, 257, 1000]
    worst = 0.0
    for i, rows in enumerate(sizes):
        cols = sizes[(i + 1 + i % 2 * 2) % len(sizes)]
        assert rows != cols
        hy, hx = window((1, rows), cdtype, 0, i % 2), window((1, cols), cdtype, 0, 1 - i % 2)
        ok(L, lib.pm_as_tf_vectors(code_of(L, cdtype), rows, cols, wvl, dx, z, hy.ptr, hx.ptr, L.stream_ptr()))
        hy.check_guards()
        hx.check_guards()
        for n, h in ((rows, hy), (cols, hx)):
            k = np.fft.fftfreq(n, dx).astype(rd)
            k64 = k.astype(np.float64)
            worst = max(worst, check_phase(h.data(), (k64 * k64 * coef).reshape(1, n), lambda j: Fraction(float(k[j])) ** 2 * Fraction(coef), rd,
                                           rng, extra_rel=2.0 ** -51, what=f'pm_as_tf_vectors {cdtype} n {n}'))
    print(f'pm_as_tf_vectors {cdtype}: error / bound = {worst:.3f}')


@pytest.mark.parametrize('cdtype', CDTYPES)
def test_czt_vectors(env, cdtype):
    """b[j] = e(half n^2), a[i] = e(half q^2), h[t] = e(-half (d + shift)^2) with exact turns.  Roundings of t in the kernel: the sum
    q = integer + shift (one, counted twice because q is squared) and the two products half * q * q: four."""
    L, lib = env
    rng = np.random.default_rng(117)
    rd = PC.REAL_OF[np.dtype(cdtype)]
    shift, half = 0.3, 0.5 * 0.0123 * 0.417
    fs, fh = Fraction(shift), Fraction(half)
    for N, M, K in ((16, 9, 24), (15, 10, 40), (7, 7, 13), (8, 8, 16), (1, 1, 1)):
        b, a, h = window((1, N), cdtype, 0, 1), window((1, M), cdtype, 0, 0), window((1, K), cdtype, 0, 1, rng=rng)
        ok(L, lib.pm_czt_vectors(code_of(L, cdtype), N, M, K, shift, half, b.ptr, a.ptr, h.ptr, L.stream_ptr()))
        for w in (b, a, h):
            w.check_guards()
        tb = [fh * Fraction(j - N // 2) ** 2 for j in range(N)]
        ta = [fh * (Fraction(i - M // 2) + fs) ** 2 for i in range(M)]
        th = [-fh * (Fraction(t - M // 2 - (N - 1 - N // 2)) + fs) ** 2 for t in range(N + M - 1)]
        for got, turns in ((b.data().ravel(), tb), (a.data().ravel(), ta), (h.data().ravel()[:N + M - 1], th)):
            t64 = np.array([float(t) for t in turns]).reshape(1, -1)
            check_phase(got.reshape(1, -1), t64, lambda i: turns[i], rd, rng, product_roundings=4, what=f'pm_czt_vectors {cdtype} {N} {M} {K}')
        assert not _bits(h.data().ravel()[N + M - 1:]).any(), 'the tail of h must be exactly zero'
        if N + M - 1 > 1:
            keep = _bits(h.host()).copy()
            assert lib.pm_czt_vectors(code_of(L, cdtype), N, M, N + M - 2, shift, half, b.ptr, a.ptr, h.ptr, L.stream_ptr()) == L.PM_ERR_ARG
            assert b'pm_czt_vectors' in lib.pm_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(h.host()), keep)


# =========================================================================== encircled energy
EE_SHAPES = [(1, 1), (7, 9), (64, 64), (33, 128)]
EE_DF = 1.0
_ee_cache = {}


def _ee_case(shape):
    """a seeded MTF whose values float32 holds exactly (both precisions read the same numbers), the centre bin 1, zero outside a
    seeded subset for the two larger shapes; 17 radii from 0 up to 2 pi r nu = 1e3 at the corner; the mpmath reference, once"""
    if shape not in _ee_cache:
        rng = np.random.default_rng(118 + shape[0])
        rows, cols = shape
        n = rows * cols
        support = np.arange(n) if n <= 64 else np.sort(rng.choice(n, size=96, replace=False))
        centre = (rows // 2) * cols + cols // 2
        support = np.union1d(support, [centre])
        mtf = np.zeros(n, np.float32)
        mtf[support] = rng.random(support.size).astype(np.float32)
        mtf[centre] = 1.0
        nu_max = max(EE_DF * math.hypot(rows // 2, cols // 2), 1.0)
        radii = np.linspace(0.0, 1e3 / (2 * math.pi * nu_max), 17)
        ref = PC.ref_encircled_energy(mtf.reshape(shape).astype(np.float64), EE_DF, radii, support)
        _ee_cache[shape] = (mtf.reshape(shape), radii, ref)
    return _ee_cache[shape]


def _ee_call(env, rd, mtfw, shape, radii, out):
    L, lib = env
    code = L.PM_C64 if rd == np.dtype('float32') else L.PM_C128
    nb = lib.pm_encircled_energy_workspace()
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    arr = (ctypes.c_double * max(len(radii), 1))(*radii)
    ok(L, lib.pm_encircled_energy(code, shape[0], shape[1], mtfw.ptr, mtfw.ld, EE_DF, len(radii), arr, out.ptr, L.ptr(ws), nb, L.stream_ptr()))


@pytest.mark.parametrize('rdtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', EE_SHAPES)
def test_encircled_energy(env, rdtype, shape):
    rd = np.dtype(rdtype)
    mtf, radii, ref = _ee_case(shape)
    mtfw = window(shape, rd, 3, 1, data=mtf)
    worst = 0.0
    for nr in (0, 1, 7, 8, 9, 17):          # the pass boundary at 8 radii: none, part of a pass, a full pass, one more, three passes
        out = window((1, max(nr, 1)), np.float64, 0, 1)
        keep = out.data()
        _ee_call(env, rd, mtfw, shape, radii[:nr], out)
        got = out.data().ravel()
        out.check_guards()
        if nr == 0:
            assert np.array_equal(got, keep.ravel())
            continue
        assert got[0] == 0.0                                    # r = 0
        if nr > 1:
            rel = np.abs(got[1:nr] - ref[1:nr]) / np.abs(ref[1:nr])
            worst = max(worst, float(rel.max()))
        again = window((1, nr), np.float64, 0, 0)
        _ee_call(env, rd, mtfw, shape, radii[:nr], again)
        assert np.array_equal(_bits(again.data()), _bits(out.data())), 'two runs must be bit-equal'
    print(f'MEASURED pm_encircled_energy {rdtype} {shape}: relative error {worst:.3e}')
    assert worst <= EE_REL_BOUND


def _ee_adjoint(env, rd, shape, radii, w, out):
    L, lib = env
    code = L.PM_C64 if rd == np.dtype('float32') else L.PM_C128
    ra = (ctypes.c_double * max(len(radii), 1))(*radii)
    wa = (ctypes.c_double * max(len(w), 1))(*w)
    ok(L, lib.pm_encircled_energy_adjoint(code, shape[0], shape[1], EE_DF, len(radii), ra, wa, out.ptr, out.ld, L.stream_ptr()))


@pytest.mark.parametrize('rdtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', EE_SHAPES)
def test_encircled_energy_adjoint(env, rdtype, shape):
    """values against mpmath (small shapes) or scipy's fp64 j1 (large ones); 9 and 17 radii accumulate across passes of 8.
    Tolerance: fp64 J1 carries an ABSOLUTE error of a few 1e-16 (so relative to the largest bin, not to each), 17 terms: 1e-12 of the
    largest bin; float32 output is rounded once per pass of 8 radii, at most three times: 2 eps_32."""
    from scipy.special import j1
    rd = np.dtype(rdtype)
    _, radii, _ = _ee_case(shape)
    rng = np.random.default_rng(119)
    w17 = rng.uniform(0.2, 1.0, 17)
    for nr in (0, 1, 8, 9, 17):
        out = window(shape, rd, 3, 1, rng=rng)
        _ee_adjoint(env, rd, shape, radii[:nr], w17[:nr], out)
        out.check_guards()
        got = out.data()
        if nr == 0:
            assert not got.any(), 'an empty radius list writes zeros'
            continue
        if shape[0] * shape[1] <= 64:
            ref = PC.ref_encircled_energy_adjoint(shape, EE_DF, radii[:nr], w17[:nr])
        else:
            x, y = PC.ee_grid(shape, EE_DF)
            nu = np.hypot(*np.meshgrid(x, y))
            nu[nu == 0] = 1e-16
            ref = sum(wk * rk * j1(2 * np.pi * rk * nu) / nu for rk, wk in zip(radii[:nr], w17[:nr])) * EE_DF ** 2
        tol = 1e-12 if rd == np.dtype('float64') else 2 * float(np.finfo(np.float32).eps)
        assert np.max(np.abs(got - ref)) <= tol * max(np.max(np.abs(ref)), 1e-300), (nr, np.max(np.abs(got - ref)), np.max(np.abs(ref)))
        again = window(shape, rd, 0, 0, rng=rng)
        _ee_adjoint(env, rd, shape, radii[:nr], w17[:nr], again)
        assert np.array_equal(_bits(again.data()), _bits(got)), 'two runs must be bit-equal'


@pytest.mark.parametrize('shape', EE_SHAPES)
def test_encircled_energy_dot_product_identity(env, shape):
    """<EE(m), w> = <m, adj(w)> to 1e-13 relative in fp64, 17 radii (three passes on both sides), ld > cols"""
    rd = np.dtype('float64')
    _, radii, _ = _ee_case(shape)
    rng = np.random.default_rng(120)
    m = rng.random(shape)
    m[shape[0] // 2, shape[1] // 2] = 1.0
    w = rng.uniform(0.2, 1.0, 17)
    mw = window(shape, rd, 3, 1, data=m)
    ee = window((1, 17), np.float64, 0, 1)
    _ee_call(env, rd, mw, shape, radii, ee)
    adj = window(shape, rd, 3, 0)
    _ee_adjoint(env, rd, shape, radii, w, adj)
    lhs = math.fsum(ee.data().ravel() * w)
    rhs = math.fsum((m * adj.data()).ravel())
    print(f'pm_encircled_energy dot-product identity {shape}: {abs(lhs - rhs) / abs(lhs):.3e}')
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


# =========================================================================== map sampling against scipy (tests/golden/pointwise.npz)
SAMPLE_DX, SAMPLE_CENTER = 0.5, (0.25, -0.5)      # powers of two and dyadic: the kernel's coordinate arithmetic is exact in fp32 too


@pytest.mark.parametrize('cdtype', CDTYPES)
@pytest.mark.parametrize('name', ['small', 'square'])
def test_sample_map_against_scipy(env, golden, cdtype, name):
    """orders 0 .. 5; coordinates as full grids, as a row vector (strides 0, 1) with a column vector (strides 1, 0), and as grids with
    ld > cols: three bit-equal results that match scipy.  Tolerance: the one test_measured_fpm_golden uses for complex128 (1e-12,
    1e-11 from order 4); for complex64 the coordinates are exact here, so what remains is the rounding of the fp64 result to
    float32, eps_32 / 2 = 6e-8 of each value: 1e-6 of the largest (that test allows 2e-4 / 5e-4 for its fp32 coordinates)."""
    L, lib = env
    g = golden('pointwise')
    rd = PC.REAL_OF[np.dtype(cdtype)]
    rng = np.random.default_rng(121)
    m0 = g[f'{name}_map']
    ny, nx = m0.shape
    row, col = g[f'{name}_row'], g[f'{name}_col']
    R, C = len(row), len(col)
    cxo, cyo = SAMPLE_CENTER
    xv = (cxo + SAMPLE_DX * (col - nx // 2)).astype(rd)
    yv = (cyo + SAMPLE_DX * (row - ny // 2)).astype(rd)
    assert np.array_equal((xv.astype(np.float64) - cxo) / SAMPLE_DX + nx // 2, col)      # exact in the real type
    assert np.array_equal((yv.astype(np.float64) - cyo) / SAMPLE_DX + ny // 2, row)
    inside = ((row >= 0) & (row <= ny - 1))[:, None] & ((col >= 0) & (col <= nx - 1))[None, :]
    assert inside.any() and (~inside).any() and (row == 0).any() and (col == nx - 1).any()
    X, Y = np.broadcast_to(xv, (R, C)), np.broadcast_to(yv[:, None], (R, C))
    mapw = window((ny, nx), cdtype, 7, 1, data=m0)
    junk = rng.uniform(-8, 8, R * C).astype(rd)
    ways = {
        'grids': (window((R, C), rd, data=X), C, 1, window((R, C), rd, data=Y), C, 1),
        # the vectors lead R * C elements (the rest is other data): a kernel that took them for grids would still read inside the buffer
        'vectors': (window((1, R * C), rd, 0, 1, data=np.concatenate([xv, junk[C:]])), 0, 1,
                    window((1, R * C), rd, 0, 1, data=np.concatenate([yv, junk[R:]])), 1, 0),
        'wide grids': (window((R, C), rd, 7, 1, data=X), C + 7, 1, window((R, C), rd, 1, 0, data=Y), C + 1, 1),
    }
    fill_scalar = 0.25 - 0.5j
    fill0 = PC.random_values(rng, (R, C), cdtype)
    fillw = window((R, C), cdtype, 3, 1, data=fill0)
    for order in range(6):
        want = g[f'{name}_o{order}']
        coeff = None
        if order >= 2:
            coeff = window((ny + 24, nx + 24), np.complex128, 1, 1)
            ok(L, lib.pm_spline_prefilter(code_of(L, cdtype), order, ny, nx, mapw.ptr, mapw.ld, coeff.ptr, coeff.ld, L.stream_ptr()))
            coeff.check_guards()
        for fill_kind in ('scalar', 'array'):
            expect = np.where(inside, want, fill_scalar if fill_kind == 'scalar' else fill0.astype(np.complex128))
            results = {}
            for way, (xw, xsy, xsx, yw, ysy, ysx) in ways.items():
                o = window((R, C), cdtype, 7, 1)
                fptr, fld = (NULL, 0) if fill_kind == 'scalar' else (fillw.ptr, fillw.ld)
                if order < 2:
                    rc = lib.pm_sample_map(code_of(L, cdtype), order, ny, nx, mapw.ptr, mapw.ld, SAMPLE_DX, cxo, cyo, R, C, xw.ptr, xsy, xsx,
                                           yw.ptr, ysy, ysx, fptr, fld, fill_scalar.real, fill_scalar.imag, o.ptr, o.ld, L.stream_ptr())
                else:
                    rc = lib.pm_sample_spline(code_of(L, cdtype), order, ny, nx, coeff.ptr, coeff.ld, SAMPLE_DX, cxo, cyo, R, C, xw.ptr, xsy,
                                              xsx, yw.ptr, ysy, ysx, fptr, fld, fill_scalar.real, fill_scalar.imag, o.ptr, o.ld,
                                              L.stream_ptr())
                ok(L, rc)
                o.check_guards()
                results[way] = o.data()
            first = results['grids']
            for way, got in results.items():
                assert np.array_equal(_bits(got), _bits(first)), f'{name} order {order} fill {fill_kind}: "{way}" differs from "grids"'
            tol = (1e-12 if order < 4 else 1e-11) if cdtype == 'complex128' else 1e-6
            assert rel_max(first, expect) < tol, (name, order, fill_kind, rel_max(first, expect))
            assert np.array_equal(first[~inside], expect[~inside].astype(cdtype)), 'outside the map the fill is copied, not computed'


# =========================================================================== the Python wrappers on strided views
def test_ops_wrappers_accept_strided_views(env):
    """_ops.cmul / rmul / scale_sep / abs2 / abs_arg take one leading dimension per array: a transposed or column-strided view is
    copied first (it used to be read as if its rows were contiguous, silently)."""
    from prysm_amd import _ops
    rng = np.random.default_rng(122)
    for cdtype in CDTYPES:
        rd = PC.REAL_OF[np.dtype(cdtype)]
        tol = 8 * float(np.finfo(rd).eps)
        close = lambda got, want: np.max(np.abs(got.cpu().numpy() - want)) <= tol * np.max(np.abs(want))      # noqa: E731
        base = PC.random_values(rng, (6, 10), cdtype)
        other = PC.random_values(rng, (10, 6), cdtype)
        real = PC.random_values(rng, (6, 10), rd)
        tb, to, tr = (torch.from_numpy(v).cuda() for v in (base, other, real))
        views = [(tb.T, base.T, to, other, tr.T, real.T), (tb[:, ::2], base[:, ::2], to.T[:, ::2], other.T[:, ::2], tr[:, ::2], real[:, ::2])]
        for x, xn, y, yn, r, rn in views:
            assert x.stride(-1) != 1
            rows, cols = xn.shape
            xn128 = xn.astype(np.complex128)
            assert close(_ops.cmul(x, y), xn128 * yn)
            assert close(_ops.cmul(x, y, conj_b=True), xn128 * np.conj(yn))
            assert close(_ops.rmul(r, x, 2.0), 2.0 * rn * xn128)
            rv, cv = PC.random_values(rng, (rows,), cdtype), PC.random_values(rng, (cols,), cdtype)
            got = _ops.scale_sep(x, row_vec=torch.from_numpy(rv).cuda(), col_vec=torch.from_numpy(cv).cuda(), scale=0.5)
            assert close(got, 0.5 * xn128 * rv[:, None] * cv[None, :])
            assert close(_ops.abs2(x), np.abs(xn128) ** 2)
            a, p = _ops.abs_arg(x)
            assert close(a, np.abs(xn128)) and close(p, np.angle(xn128))
            for t in (_ops.cmul(x, y), _ops.abs2(x), a, p):
                assert tuple(t.shape) == (rows, cols) and t.is_contiguous()
            out = torch.zeros((cols, rows), dtype=tr.dtype, device='cuda').T
            with pytest.raises(ValueError):
                _ops.abs2(x, out=out)
            with pytest.raises(ValueError):
                _ops.abs2(x, out=torch.zeros((rows, 2 * cols), dtype=tr.dtype, device='cuda')[:, ::2], weight=1.0)
        # one row broadcast over six (strides (0, 1)): rows that overlap are copied too, not passed on with a leading dimension of 0
        xb, rb = tb[:1].expand(6, 10), tr[:1].expand(6, 10)
        assert xb.stride(0) == 0 and xb.stride(1) == 1
        bn, rn = np.broadcast_to(base[:1], (6, 10)).astype(np.complex128), np.broadcast_to(real[:1], (6, 10))
        full = base.astype(np.complex128)
        assert close(_ops.cmul(xb, tb), bn * full) and close(_ops.cmul(tb, xb, conj_b=True), full * np.conj(bn))
        assert close(_ops.rmul(rb, tb), rn * full) and close(_ops.rmul(tr, xb), real * bn)
        assert close(_ops.scale_sep(xb, scale=2.0), 2.0 * bn) and close(_ops.abs2(xb), np.abs(bn) ** 2)
        a, p = _ops.abs_arg(xb)
        assert close(a, np.abs(bn)) and close(p, np.angle(bn))
        with pytest.raises(ValueError):
            _ops.abs2(tb, out=rb)
