"""GPU: the wavefront-sensor unit (csrc/sensors.hip) behind prysm_amd.x.psi, x.shack_hartmann, x.pdi and x.sri, against the reference's
outputs in tests/golden/sensors.npz, against the truth (integer PSI frames) and against the numpy model (x/sensors_plan.py).  Bounds
and cases: tests/sensors_common.py."""
import ctypes

import numpy as np
import pytest
import torch

import sensors_common as C
from gpu_common import TOL64, tonp

pytestmark = pytest.mark.gpu

TDT = {np.float64: torch.float64, np.float32: torch.float32, np.uint8: torch.uint8, np.uint16: torch.uint16}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def G():
    return C.golden()


@pytest.fixture(scope='module')
def M():
    from prysm_amd.x import psi, shack_hartmann, pdi, sri, sensors_plan
    from prysm_amd import _lib, _ops
    return dict(psi=psi, sh=shack_hartmann, pdi=pdi, sri=sri, SP=sensors_plan, L=_lib, ops=_ops)


@pytest.fixture
def precision32():
    from prysm_amd.conf import config
    config.precision = 32
    yield
    config.precision = 64


# ----------------------------------------------------------------------------- PSI against the reference and the truth
@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('name', C.PSI_SCHEMES)
def test_psi_against_golden(G, M, name, dt):
    psi = M['psi']
    sch = C.scheme(psi, name)
    fr = [dev(f) for f in C.frames(G['psi_phi'], sch.shifts, dt)]
    w = psi.degroot_formalism_psi(fr, sch)
    assert w.dtype == TDT[dt]
    d = C.wrapped_diff(tonp(w), G[f'psi_{name}_{"f64" if dt == np.float64 else "f32"}']).max()
    print(f'psi {name} {np.dtype(dt).name}: {d / C.eps(dt):.2f} eps (bound {C.PSI_EPS_MULT[dt]})')
    assert d <= C.PSI_EPS_MULT[dt] * C.eps(dt)
    num, den = psi.psi_accumulate(fr, sch)
    mn, md, _ = M['SP'].psi([tonp(f) for f in fr], sch.s, sch.c, dt)
    assert np.array_equal(tonp(num), mn) and np.array_equal(tonp(den), md)


@pytest.mark.parametrize('idt', [np.uint16, np.uint8])
@pytest.mark.parametrize('name', ['schwider', 'zygo13'])
def test_psi_integer_frames_against_the_truth(G, M, name, idt):
    psi = M['psi']
    sch = C.scheme(psi, name)
    phi = G['psi_phi']
    fr = [dev(f) for f in C.frames(phi, sch.shifts, idt, C.INT_AMPL[idt])]
    w = psi.degroot_formalism_psi(fr, sch)
    assert w.dtype == torch.float64
    d = C.wrapped_diff(tonp(w), phi).max()
    print(f'psi {name} {np.dtype(idt).name}: {d:.3e} rad (bound {C.int_bound(sch, C.INT_AMPL[idt], np.float64):.3e})')
    assert d <= C.int_bound(sch, C.INT_AMPL[idt], np.float64)


def test_psi_integer_frames_give_config_precision(G, M, precision32):
    psi = M['psi']
    sch = psi.SCHWIDER
    fr = [dev(f) for f in C.frames(G['psi_phi'], sch.shifts, np.uint16, C.INT_AMPL[np.uint16])]
    w = psi.degroot_formalism_psi(fr, sch)
    assert w.dtype == torch.float32
    assert C.wrapped_diff(tonp(w), G['psi_phi']).max() <= C.int_bound(sch, C.INT_AMPL[np.uint16], np.float32)


def test_psi_richdata_in_richdata_out(G, M):
    from prysm_amd._richdata import RichData
    psi = M['psi']
    sch = psi.SCHWIDER
    fr = [RichData(dev(f), 0.1, 0.6328) for f in C.frames(G['psi_phi'], sch.shifts)]
    w = psi.degroot_formalism_psi(fr, sch)
    num, den = psi.psi_accumulate(fr, sch)
    assert isinstance(w, RichData) and isinstance(num, RichData) and (w.dx, w.wavelength) == (0.1, 0.6328)
    assert np.array_equal(tonp(w.data), tonp(psi.degroot_formalism_psi([f.data for f in fr], sch)))


# ----------------------------------------------------------------------------- PSI kernel coverage, against the model
def _check_model(M, frames_dev, s, c, odt, want=(True, True, True)):
    got = M['ops'].psi(frames_dev, s, c, TDT[odt], want)
    model = M['SP'].psi([tonp(f) for f in frames_dev], s, c, odt)
    for g, m, w in zip(got, model[:2], want[:2]):       # the sums: the same operations in the same order, to the bit
        assert (g is None) == (not w)
        if w:
            assert np.array_equal(tonp(g), m)
    if want[2]:
        assert C.wrapped_diff(tonp(got[2]), model[2]).max() <= 4 * C.eps(odt)        # atan2 of equal pairs: two implementations
    else:
        assert got[2] is None
    return got


@pytest.mark.parametrize('fdt,odt', [(np.float32, np.float32), (np.float64, np.float64), (np.uint8, np.float64), (np.uint16, np.float32)])
@pytest.mark.parametrize('cols', C.PSI_COLS)
def test_psi_column_counts(M, fdt, odt, cols):
    K = 5
    fr = [dev(f) for f in C.random_frames(K, (7, cols), fdt)]
    s, c = C.random_weights(K)
    _check_model(M, fr, s, c, odt)


@pytest.mark.parametrize('want', [(True, False, False), (False, True, False), (True, True, True)])
def test_psi_output_subsets(M, want):
    fr = [dev(f) for f in C.random_frames(4, (9, 70), np.float32)]
    _check_model(M, fr, *C.random_weights(4), np.float32, want)


@pytest.mark.parametrize('K', [1, 32])
def test_psi_fewest_and_most_frames(M, K):
    fr = [dev(f) for f in C.random_frames(K, (5, 65), np.float64)]
    _check_model(M, fr, *C.random_weights(K), np.float64)


def test_psi_refuses_33_frames(M):
    fr = [dev(f) for f in C.random_frames(33, (4, 8), np.float32)]
    sch = M['psi'].Scheme(np.zeros(33), np.ones(33), np.ones(33))
    with pytest.raises(ValueError, match='between 1 and 32'):
        M['psi'].degroot_formalism_psi(fr, sch)


def test_psi_separate_frames_equal_a_stack_to_the_bit(M):
    host = C.random_frames(5, (33, 70), np.float32)
    s, c = C.random_weights(5)
    sch = M['psi'].Scheme(np.zeros(5), s, c)
    pads = [torch.empty(1000 + 16 * k, device='cuda') for k in range(5)]       # so that the separate frames do not lie side by side
    sep = [dev(f) for f in host]
    stack = dev(np.stack(host))
    a = M['psi'].degroot_formalism_psi(sep, sch)
    b = M['psi'].degroot_formalism_psi(stack, sch)
    assert torch.equal(a, b)
    na, da = M['psi'].psi_accumulate(sep, sch)
    nb, db = M['psi'].psi_accumulate(stack, sch)
    assert torch.equal(na, nb) and torch.equal(da, db)
    del pads


@pytest.mark.parametrize('fdt,odt', [(np.float32, np.float32), (np.uint16, np.float64)])
def test_psi_strided_rows(M, fdt, odt):
    """ld > cols: views of wider buffers, with a row stride that keeps (72) and one that breaks (71) the 16-byte rule"""
    for ld in (72, 71):
        host = C.random_frames(3, (6, ld), fdt)
        fr = [dev(f)[:, :65] for f in host]
        assert fr[0].stride(0) == ld
        _check_model(M, fr, *C.random_weights(3), odt)


@pytest.mark.parametrize('fdt,odt', [(np.float32, np.float32), (np.float64, np.float64), (np.uint8, np.float32)])
def test_psi_base_offset_by_one_element(M, fdt, odt):
    """every frame one element past a 16-byte boundary: a scalar head per row, then wide loads; and one frame alone offset: element loads"""
    cols, ld, rows = 64, 80, 5
    host = C.random_frames(3, (1, rows * ld + 1), fdt)
    bases = [dev(f).reshape(-1) for f in host]
    views = [torch.as_strided(b, (rows, cols), (ld, 1), 1) for b in bases]
    assert views[0].data_ptr() % 16 == np.dtype(fdt).itemsize and views[0].stride(0) == ld
    _check_model(M, views, *C.random_weights(3), odt)
    mixed = [views[0], torch.as_strided(bases[1], (rows, cols), (ld, 1), 0), views[2]]
    _check_model(M, mixed, *C.random_weights(3), odt)


def test_psi_second_trip_of_the_row_loop(M):
    rows, cols, K = C.PSI_TALL
    rng = np.random.default_rng(11)
    host = [rng.uniform(0, 4000, (rows, cols)).astype(np.float32) for _ in range(K)]
    s, c = C.random_weights(K)
    got = M['ops'].psi([dev(f) for f in host], s, c, torch.float32, (True, True, True))
    mn, md, mw = M['SP'].psi(host, s, c, np.float32)
    assert np.array_equal(tonp(got[0]), mn) and np.array_equal(tonp(got[1]), md)
    assert C.wrapped_diff(tonp(got[2])[-8:], mw[-8:]).max() <= 4 * C.eps(np.float32)


# ----------------------------------------------------------------------------- Shack-Hartmann
def _sh(M, name, dt, form='arrays'):
    from prysm_amd import geometry
    n, shape, shift, pitch, ap, kw = C.SH_CASES[name]
    aperture = geometry.circle if ap == 'circle' else geometry.rectangle
    if form == 'grid':
        return M['sh'].shack_hartmann(pitch, n, C.SH_EFL, C.SH_WVL, aperture=aperture, aperture_kwargs=dict(kw), shift=shift, shape=shape, dx=C.SH_DX)
    if form == 'vectors':
        x, y = (dev(v) for v in C.sh_vectors(shape, dt))
    else:
        x, y = (dev(v) for v in C.sh_xy(shape, dt))
    return M['sh'].shack_hartmann(pitch, n, C.SH_EFL, C.SH_WVL, x, y, aperture=aperture, aperture_kwargs=dict(kw), shift=shift)


@pytest.mark.parametrize('dt', [np.float64, np.float32])
@pytest.mark.parametrize('name', list(C.SH_CASES))
def test_shack_hartmann_against_golden(G, M, name, dt):
    got = tonp(_sh(M, name, dt))
    assert got.dtype == (np.complex128 if dt == np.float64 else np.complex64)
    idx = G[f'sh_{name}_idx']
    maxarg = C.sh_max_arg(float(G[f'sh_{name}_maxtotal']))
    n, shape, shift, pitch, ap, kw = C.SH_CASES[name]
    par = M['SP'].lenslet_params(pitch, n, C.SH_EFL, C.SH_WVL, M['SP'].LENSLET_CIRCLE if ap == 'circle' else M['SP'].LENSLET_RECTANGLE, kw, shift)
    model, count = M['SP'].lenslet_screen(*C.sh_xy(shape, dt), par, dt)
    if dt == np.float64:
        # membership: the model's count map is the golden's, and a sample whose membership differed from the model's would be off by
        # the whole term of a lenslet (up to max|arg| rad), not by roundings: the set of such samples must be empty
        assert np.array_equal(count, G[f'sh_{name}_count'])
        assert np.flatnonzero(np.abs(got - model) > 1e-9 * max(1.0, maxarg)).size == 0
    keep = (G[f'sh_{name}_count'] == G[f'sh_{name}_count32']).ravel()[idx]
    d = np.abs(got.ravel()[idx] - G[f'sh_{name}_{"f64" if dt == np.float64 else "f32"}'])[keep].max()
    print(f'sh {name} {np.dtype(dt).name}: {d:.3e} = {d / (C.eps(dt) * maxarg):.3f} eps max|arg| (c = {C.SH_C[dt]})')
    assert d <= C.SH_C[dt] * C.eps(dt) * maxarg


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_shack_hartmann_coordinate_forms_agree_to_the_bit(M, dt, request):
    if dt == np.float32:
        request.getfixturevalue('precision32')
    a = _sh(M, C.SH_FORMS_CASE, dt, 'arrays')
    b = _sh(M, C.SH_FORMS_CASE, dt, 'vectors')
    c = _sh(M, C.SH_FORMS_CASE, dt, 'grid')
    assert a.dtype == b.dtype == c.dtype and torch.equal(a, b) and torch.equal(a, c)


def test_shack_hartmann_fallback_loop_on_the_device(G, M):
    """a rotated rectangle is not the kernel's: the loop runs, with this library's geometry.rectangle on device windows; angle 90 of a
    square is the square"""
    from prysm_amd import geometry
    name = 'n4_64_shift'
    n, shape, shift, pitch, ap, kw = C.SH_CASES[name]
    x, y = (dev(v) for v in C.sh_xy(shape))
    got = tonp(M['sh'].shack_hartmann(pitch, n, C.SH_EFL, C.SH_WVL, x, y, aperture=geometry.rectangle, aperture_kwargs={'angle': 90}, shift=shift))
    maxarg = C.sh_max_arg(float(G[f'sh_{name}_maxtotal']))
    # the loop's tensor operations do not round as the reference's do (on the device a division by a scalar is a multiplication by its
    # reciprocal), so each of the at most four terms of a sample may be one unit in the last place off: 4 eps max|arg| (measured: 0.26)
    d = np.abs(got.ravel()[G[f'sh_{name}_idx']] - G[f'sh_{name}_f64']).max()
    print(f'sh fallback loop: {d / (C.eps(np.float64) * maxarg):.3f} eps max|arg| (bound 4)')
    assert d <= 4 * C.eps(np.float64) * maxarg


# ----------------------------------------------------------------------------- PS/PDI
def _field():
    x, y, amp, opd = C.pupil()
    return x, y, C.pupil_field(amp, opd)


@pytest.mark.parametrize('gt,ax,ps', C.PDI_CASES)
def test_pspdi_against_golden(G, M, gt, ax, ps):
    x, y, field = _field()
    p = M['pdi'].PSPDI(dev(x), dev(y), C.IF_EFL, C.IF_EPD, C.IF_WVL, grating_type=gt, grating_axis=ax, **C.PDI_KW)
    f = dev(field)
    inten = p.forward_model(f, phase_shift=ps)
    dbg = p.forward_model(f, phase_shift=ps, debug=True)
    key = C.pdi_key(gt, ax, ps)
    for fname, v in zip(C.PDI_FIELDS, C.pdi_fields(inten, dbg)):
        a = tonp(v)
        ref = G[f'{key}_{fname}']
        d = np.abs(a.ravel()[C.sample_idx(a.shape, C.pdi_stride(fname))] - ref).max() / float(G[f'{key}_{fname}_peak'])
        assert d < TOL64, (fname, d)
    ratio, I1, I2 = M['pdi'].evaluate_test_ref_arm_matching(dbg)
    assert isinstance(ratio, torch.Tensor) and ratio.dim() == 0 and ratio.is_cuda
    r = tonp(dbg['at_camera']['ref'])
    t = tonp(dbg['at_camera']['test'])
    assert abs(float(ratio) - (np.abs(r) ** 2).mean() / (np.abs(t) ** 2).mean()) <= 1e-9 * float(ratio)


def test_pspdi_transmissivity_goes_through_the_combination(M):
    x, y, field = _field()
    kw = dict(C.PDI_KW, test_arm_transmissivity=0.7)
    p = M['pdi'].PSPDI(dev(x), dev(y), C.IF_EFL, C.IF_EPD, C.IF_WVL, **kw)
    inten = tonp(p.forward_model(dev(field)))
    want = np.abs(tonp(p.ref_beam) + tonp(p.test_beam)) ** 2
    assert np.abs(inten - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_rectangle_pulse(G, M, dt):
    got = tonp(M['pdi'].rectangle_pulse(dev(C.PULSE_X.astype(dt)), **C.PULSE_KW))
    assert got.dtype == dt
    model = M['SP'].grating(M['SP'].GRATING_PULSE, C.PULSE_X.astype(dt), M['SP'].pulse_params(**C.PULSE_KW), dt)
    assert np.array_equal(got, model)
    if dt == np.float64:
        assert np.array_equal(got, G['pulse'])
    x2 = np.linspace(-7, 9, 3 * 70).reshape(3, 70).astype(dt)
    got2 = tonp(M['pdi'].rectangle_pulse(dev(x2)))
    assert got2.shape == x2.shape and np.array_equal(got2, M['SP'].grating(M['SP'].GRATING_PULSE, x2, M['SP'].pulse_params(), dt))


# ----------------------------------------------------------------------------- SRI
@pytest.mark.parametrize('ps', C.SRI_SHIFTS)
def test_sri_against_golden(G, M, ps):
    x, y, field = _field()
    s = M['sri'].SelfReferencedInterferometer(dev(x), dev(y), C.IF_EFL, C.IF_EPD, C.IF_WVL, fiber_samples=C.SRI_FIBER_SAMPLES)
    a = tonp(s.forward_model(dev(field), phase_shift=ps))
    tag = '0' if ps == 0 else '0p3'
    d = np.abs(a.ravel()[C.sample_idx(a.shape, C.PDI_STRIDE['pupil'])] - G[f'sri_{tag}_intensity']).max() / float(G[f'sri_{tag}_intensity_peak'])
    assert d < TOL64, d
    dbg = s.forward_model(dev(field), phase_shift=ps, debug=True)
    tot = tonp(dbg['at_camera']['ref']) + tonp(dbg['at_camera']['test'])
    assert np.abs(np.abs(tot) ** 2 - a).max() <= 1e-12 * a.max()


def test_to_photonic_fiber_and_back_return_more(G, M):
    from prysm_amd.propagation import Wavefront
    x, y, field = _field()
    s = M['sri'].SelfReferencedInterferometer(dev(x), dev(y), C.IF_EFL, C.IF_EPD, C.IF_WVL, fiber_samples=C.SRI_FIBER_SAMPLES)
    assert np.abs(tonp(s.Efib) - G['sri_efib']).max() <= 1e-12 * G['sri_efib'].max()
    wf = Wavefront(dev(field), C.IF_WVL, s.dx)
    nxt, at, emitted, coupling = M['sri'].to_photonic_fiber_and_back(wf, C.IF_EFL, s.Efib, s.dxfib, s.Ifibsum, phase_shift=0.3, return_more=True)
    assert isinstance(coupling, torch.Tensor) and coupling.dim() == 0 and coupling.is_cuda
    assert abs(float(coupling) - float(G['sri_more_coupling'])) <= 1e-10 * float(G['sri_more_coupling'])
    for got, key in ((at, 'sri_more_at'), (emitted, 'sri_more_emitted')):
        assert np.abs(tonp(got) - G[key]).max() / np.abs(G[key]).max() < TOL64, key
    n = tonp(nxt)
    assert np.abs(n.ravel()[C.sample_idx(n.shape, C.PDI_STRIDE['pupil'])] - G['sri_more_next']).max() / float(G['sri_more_next_peak']) < TOL64
    eta = M['sri'].overlap_integral(at.data, s.Efib, (torch.abs(at.data) ** 2).sum(), s.Ifibsum)
    assert abs(float(eta) - float(G['sri_more_coupling'])) <= 1e-10 * float(G['sri_more_coupling'])


# ----------------------------------------------------------------------------- C ABI: refusals launch nothing
def test_c_abi_argument_checks(M):
    L = M['L']
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.float64, device='cuda')
    before = buf.clone()
    p = ctypes.c_void_p(buf.data_ptr())
    st = L.stream_ptr()
    tab = L.pm_psi_frames()
    tab.frame[0] = buf.data_ptr()
    tab.s[0] = tab.c[0] = 1.0
    bad = []
    # pm_psi: dtype codes, ld < cols, K range, null everything
    bad.append(lib.pm_psi(L.PM_C64, L.PM_F32, 1, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F32, L.PM_U8, 1, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F32, L.PM_F64, 1, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 1, 2, 4, ctypes.byref(tab), 3, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 1, 2, 4, ctypes.byref(tab), 4, p, p, p, 3, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 0, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 33, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 2, 2, 4, ctypes.byref(tab), 4, p, p, p, 4, st))       # frame 1 is null
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 1, 2, 4, ctypes.byref(tab), 4, None, None, None, 4, st))
    bad.append(lib.pm_psi(L.PM_F64, L.PM_F64, 1, 2, 4, None, 4, p, p, p, 4, st))
    # pm_lenslet_screen
    lens = L.pm_lenslets()
    lens.kind, lens.nx, lens.ny, lens.pitch, lens.half_width, lens.half_height, lens.efl, lens.k = 0, 2, 2, 1.0, 0.5, 0.5, 50.0, -1.0
    ok = ctypes.byref(lens)
    bad.append(lib.pm_lenslet_screen(L.PM_C64, L.PM_COORDS_GRID, 2, 4, None, 0, None, 0, 0.1, ok, p, 4, st))
    bad.append(lib.pm_lenslet_screen(L.PM_F64, 7, 2, 4, None, 0, None, 0, 0.1, ok, p, 4, st))
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_GRID, 2, 4, None, 0, None, 0, 0.1, ok, p, 3, st))
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_POINTWISE, 2, 4, p, 3, p, 4, 0.1, ok, p, 4, st))
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_POINTWISE, 2, 4, None, 4, None, 4, 0.1, ok, p, 4, st))
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_GRID, 2, 4, None, 0, None, 0, 0.1, None, None, 4, st))
    lens.kind = 5
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_GRID, 2, 4, None, 0, None, 0, 0.1, ok, p, 4, st))
    lens.kind, lens.half_height = 0, 1.5
    bad.append(lib.pm_lenslet_screen(L.PM_F64, L.PM_COORDS_GRID, 2, 4, None, 0, None, 0, 0.1, ok, p, 4, st))
    # pm_grating
    par = (ctypes.c_double * 5)(1.5, 0.45, 1.0, 0.2, 0.6)
    bad.append(lib.pm_grating(L.PM_C128, L.PM_GRATING_PULSE, L.PM_COORDS_POINTWISE, 2, 4, p, 4, 0.0, 0.0, par, None, 0, p, 4, st))
    bad.append(lib.pm_grating(L.PM_F64, 9, L.PM_COORDS_POINTWISE, 2, 4, p, 4, 0.0, 0.0, par, None, 0, p, 4, st))
    bad.append(lib.pm_grating(L.PM_F64, L.PM_GRATING_PULSE, L.PM_COORDS_POINTWISE, 2, 4, p, 3, 0.0, 0.0, par, None, 0, p, 4, st))
    bad.append(lib.pm_grating(L.PM_F64, L.PM_GRATING_PULSE, L.PM_COORDS_POINTWISE, 2, 4, p, 4, 0.0, 0.0, par, p, 3, p, 4, st))
    bad.append(lib.pm_grating(L.PM_F64, L.PM_GRATING_PULSE, L.PM_COORDS_POINTWISE, 2, 4, None, 4, 0.0, 0.0, None, None, 0, None, 4, st))
    # pm_beam_combine
    bad.append(lib.pm_beam_combine(L.PM_F64, 2, 4, p, 4, 1.0, p, 4, 1.0, p, 4, None, 0, st))
    bad.append(lib.pm_beam_combine(L.PM_C128, 2, 4, p, 3, 1.0, p, 4, 1.0, p, 4, None, 0, st))
    bad.append(lib.pm_beam_combine(L.PM_C128, 2, 4, p, 4, 1.0, p, 4, 1.0, p, 3, None, 0, st))
    bad.append(lib.pm_beam_combine(L.PM_C128, 2, 4, p, 4, 1.0, p, 4, 1.0, None, 0, None, 0, st))
    bad.append(lib.pm_beam_combine(L.PM_C128, 2, 4, None, 4, 1.0, None, 4, 1.0, None, 0, None, 0, st))
    # pm_fiber_scale
    bad.append(lib.pm_fiber_scale(L.PM_C64, 2, 4, p, 4, p, p, 1.0, 0.0, p, 4, st))
    bad.append(lib.pm_fiber_scale(L.PM_F64, 2, 4, p, 3, p, p, 1.0, 0.0, p, 4, st))
    bad.append(lib.pm_fiber_scale(L.PM_F64, 2, 4, p, 4, p, p, 1.0, 0.0, p, 3, st))
    bad.append(lib.pm_fiber_scale(L.PM_F64, 2, 4, None, 4, None, None, 1.0, 0.0, None, 4, st))
    assert bad == [L.PM_ERR_ARG] * len(bad), bad
    torch.cuda.synchronize()
    assert torch.equal(buf, before)        # nothing was launched: the buffer every call pointed at is untouched
