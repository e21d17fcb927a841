"""GPU: x.polarization on the kernels of csrc/jones.hip -- both precisions and both layouts, against the reference's golden
(tests/golden/polarization.npz) and against the numpy model (prysm_amd/x/polarization_plan.py).  Cases and bounds:
tests/polarization_common.py.

Shapes: the golden's (19, 35); (1, 1); (3, 129), odd and across wavefront column boundaries; a [:, 3:40] window of a 50-column array
(leading dimension != cols) with every output inside a NaN frame that must survive; and (262145, 2), whose rows 262140 ... 262144 are
on the second trip of the row loop (pm_sweep.h: 65535 workgroups of 4 rows per trip).  Every base above is 16-byte aligned;
test_unaligned_views_take_the_scalar_path covers the 8-byte accesses of a complex64 aos view and the scalar Mueller store.

Away from the golden's grid a generator is compared with the model; the bound there is the sum of the two constants, since
|kernel - model| <= |kernel - reference| + |reference - model|."""
import numpy as np
import pytest
import torch

import polarization_common as C
from gpu_common import tonp
from prysm_amd.x import polarization_plan as PP

pytestmark = pytest.mark.gpu

SHAPES = {'grid': (19, 35), 'one': (1, 1), 'odd': (3, 129), 'window': (6, 37), 'tall': (262145, 2)}
PAD = (3, 10)       # columns of the wider array left and right of the window
TCD = {64: torch.complex128, 32: torch.complex64}
TRD = {64: torch.float64, 32: torch.float32}


@pytest.fixture(scope='module')
def pol():
    from prysm_amd.x import polarization
    return polarization


@pytest.fixture
def at(request):
    from prysm_amd.conf import config
    config.precision = request.param
    yield request.param
    config.precision = 64


both = pytest.mark.parametrize('at', C.PRECISIONS, indirect=True)
layouts = pytest.mark.parametrize('layout', ['aos', 'planes'])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def put(a, layout, wide=False):
    """an aos numpy Jones / Mueller array on the device in `layout`; wide: as the [:, 3:-10] window of a wider array"""
    t = dev(PP.to_planes(a) if layout == 'planes' else np.asarray(a))
    if not wide:
        return t
    ax = 2 if layout == 'planes' else 1
    shape = list(t.shape)
    shape[ax] += sum(PAD)
    win = torch.full(shape, float('nan'), dtype=t.dtype, device='cuda').narrow(ax, PAD[0], t.shape[ax])
    win.copy_(t)
    return win


def put_map(a, wide=False):
    t = dev(a)
    if not wide:
        return t
    win = torch.full((t.shape[0], t.shape[1] + sum(PAD)), float('nan'), dtype=t.dtype, device='cuda')[:, PAD[0]:PAD[0] + t.shape[1]]
    win.copy_(t)
    return win


def _isnan(t):
    return torch.isnan(t)      # of a complex element: either part


class Frame:
    """an output inside a NaN frame: .win goes to out=, check() asserts that nothing outside the window was written"""

    def __init__(self, pix, ncomp, layout, dtype, wide):
        rows, cols = pix
        full = (rows + 2, cols + sum(PAD)) if wide else (rows, cols)
        self.planes = layout == 'planes'
        shape = (ncomp, *full) if self.planes else (*full, *PP.tail_of(ncomp))
        self.big = torch.full(shape, float('nan'), dtype=dtype, device='cuda')
        self.win, self.mask = self.big, None
        if wide:
            self.win = self.big[:, 1:1 + rows, PAD[0]:PAD[0] + cols] if self.planes else self.big[1:1 + rows, PAD[0]:PAD[0] + cols]
            self.mask = torch.ones(full, dtype=torch.bool, device='cuda')
            self.mask[1:1 + rows, PAD[0]:PAD[0] + cols] = False

    def check(self):
        if self.mask is not None:
            outside = self.big[:, self.mask] if self.planes else self.big[self.mask]
            assert bool(_isnan(outside).all()), 'the frame was written'
        assert not bool(_isnan(self.win).any()), 'a pixel was not written'


def get(t, layout):
    a = tonp(t)
    return PP.from_planes(a) if layout == 'planes' else a


def rand_inputs(precision, pix, seed=5):
    rng = np.random.default_rng(seed)
    r, c = C.rdt(precision), C.cdt(precision)
    mats, vec = C.jones_operands(precision, shape=pix, count=2 if pix[0] > 1000 else 6, seed=seed)
    return dict(mats=mats, vec=vec, theta=rng.uniform(-3.1, 3.1, pix).astype(r), delta=rng.uniform(-3.1, 3.1, pix).astype(r),
                field=(rng.standard_normal(pix) + 1j * rng.standard_normal(pix)).astype(c), rfield=rng.uniform(-2, 2, pix).astype(r))


# ---------------------------------------------------------------- against the golden
def golden_calls(pol, i, layout):
    """case -> the device result in `layout`, on the golden's inputs (device tensors)"""
    kw = dict(out_layout=layout)
    mats, _ = C.jones_operands(32 if i['theta'].dtype == torch.float32 else 64)
    ret = pol.linear_retarder(i['delta'], i['theta'], **kw)
    vvr2 = pol.vector_vortex_retarder(2, i['t'], C.VVR_RETARDANCE, C.VVR_ROTATE, **kw)
    return {
        'rot': pol.jones_rotation_matrix(i['theta'], **kw), 'ret': ret,
        'diat': pol.linear_diattenuator(i['alpha'], i['theta'], **kw),
        'hwp': pol.half_wave_plate(i['theta'], **kw), 'pol': pol.linear_polarizer(i['theta'], **kw),
        'vvr2': vvr2, 'vvr6': pol.vector_vortex_retarder(6, i['t'], C.VVR_RETARDANCE, C.VVR_ROTATE, **kw),
        'vvr2_leak': pol.vector_vortex_retarder(2, i['t'], C.VVR_RETARDANCE, C.VVR_ROTATE, identity_leakage=True, **kw),
        'lpv': pol.linear_pol_vector(i['angle'], **kw),
        'mueller': pol.jones_to_mueller(put(mats[0], layout), layout=layout),
        'mueller_ret': pol.jones_to_mueller(ret, layout=layout), 'mueller_vvr2': pol.jones_to_mueller(vvr2, layout=layout),
    }


@both
@layouts
def test_generators_and_mueller_against_the_golden(pol, at, layout):
    g = C.golden()
    i = {k: dev(v) for k, v in C.inputs(at).items()}
    t0 = i['t'].clone()
    got = golden_calls(pol, i, layout)
    assert torch.equal(i['t'], t0), 'vector_vortex_retarder changed the caller\'s theta'
    failed = []
    for name in C.MAP_CASES:
        a = get(got[name], layout)
        if name in ('mueller_ret', 'mueller_vvr2'):
            a = C.mueller_samples(a)
        want = g[f'{name}_{at}']
        assert a.shape == want.shape and a.dtype == want.dtype, name
        d = C.dev_eps(a, want, at, C.case_scale(name, at))
        print(f'GPU_DEV {name} precision {at} {layout}: {d:.4g} eps (bound {C.bound(name, at, True):.4g})')
        if not d <= C.bound(name, at, True):
            failed.append((name, d))
    assert not failed, failed


@both
def test_scalar_forms_are_built_on_the_host_and_match_the_golden(pol, at):
    g = C.golden()
    got = {'rot_s': pol.jones_rotation_matrix(0.3), 'ret_s': pol.linear_retarder(1.1, 0.4), 'diat_s': pol.linear_diattenuator(0.3, 0.4),
           'hwp_s': pol.half_wave_plate(0.7), 'qwp_s': pol.quarter_wave_plate(0.7), 'pol_s': pol.linear_polarizer(0.7),
           'lpv_s': pol.linear_pol_vector(30.0), 'mueller_s': pol.jones_to_mueller(C.CONST_A.astype(C.cdt(at)))}
    for name, t in got.items():
        want = g[f'{name}_{at}']
        a = tonp(t)
        assert a.shape == want.shape and a.dtype == want.dtype, name
        assert C.dev_eps(a, want, at, C.case_scale(name, at)) <= C.bound(name, at, False), name
    m = tonp(pol.jones_to_mueller(C.CONST_A.astype(C.cdt(at)), broadcast=False))
    assert C.dev_eps(m, g[f'mueller_nobroadcast_{at}'], at, C.case_scale('mueller_s', at)) <= C.bound('mueller_s', at, False)
    for k in range(4):
        assert np.array_equal(tonp(pol.pauli_spin_matrix(k)), g[f'pauli_{k}_{at}'])
        assert np.array_equal(tonp(pol.pauli_spin_matrix(k, shape=(3, 5))), np.broadcast_to(g[f'pauli_{k}_{at}'], (3, 5, 2, 2)))
    for hand in ('left', 'right'):
        assert np.array_equal(tonp(pol.circular_pol_vector(hand)), g[f'cpv_{hand}_{at}'])
        # departure: the reference raises IndexError for any shape
        v = tonp(pol.circular_pol_vector(hand, shape=(4, 7)))
        assert v.shape == (4, 7, 2, 1) and np.array_equal(v, np.broadcast_to(g[f'cpv_{hand}_{at}'].reshape(2, 1), (4, 7, 2, 1)))
    with pytest.raises(ValueError):
        pol.circular_pol_vector('up')
    c = pol.pauli_coefficients(C.CONST_A.astype(C.cdt(at)))
    assert np.array_equal(np.array(c, dtype=C.cdt(at)), PP.pauli(C.CONST_A.astype(C.cdt(at))))
    kron = tonp(pol.broadcast_kron(C.CONST_A.astype(C.cdt(at)), C.CONST_B.astype(C.cdt(at))))
    # one complex product per element: sqrt(5) / 2 eps |a| |b| each side
    assert np.all(np.abs(kron - g[f'kron_{at}']) <= C.SCALE_C * C.eps(at) * np.kron(np.abs(C.CONST_A), np.abs(C.CONST_B)))


@both
@layouts
def test_products_scale_and_pauli_against_the_golden(pol, at, layout):
    g, c = C.golden(), C.cdt(at)
    mats, vec = C.jones_operands(at)
    A, B = C.CONST_A.astype(c), C.CONST_B.astype(c)
    d = [put(m, layout) for m in mats]
    for name, ops, dops in (('chain6', mats, d), ('chainv', [mats[0], mats[1], vec], [d[0], d[1], put(vec, layout)]),
                            ('chainc', [A, mats[0], B, mats[1]], [A, d[0], B, d[1]])):
        got = get(pol.jones_product(*dops, layout=layout), layout)
        want = g[f'{name}_{at}']
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.all(np.abs(got - want) <= C.chain_bound(ops, at)), name
    f = C.inputs(at)['field']
    got = get(pol.apply_polarization_optic(dev(f), d[0], layout=layout), layout)
    assert np.all(np.abs(got - g[f'apply_{at}']) <= C.scale_bound(mats[0], f, at))
    cs = pol.pauli_coefficients(d[0], layout=layout)
    assert np.array_equal(np.stack([tonp(x) for x in cs]), g[f'pauli_{at}'])


# ---------------------------------------------------------------- every shape, against the model
@both
@layouts
@pytest.mark.parametrize('case', sorted(SHAPES))
def test_every_kernel_on_every_shape(pol, at, layout, case):
    pix, wide, tall = SHAPES[case], case == 'window', case == 'tall'
    other = 'planes' if layout == 'aos' else 'aos'
    c, cd, rd = C.cdt(at), TCD[at], TRD[at]
    x = rand_inputs(at, pix)
    J, J2, V = x['mats'][0], x['mats'][1], x['vec']
    dJ, dJ2, dV = put(J, layout, wide), put(J2, layout, wide), put(V, layout, wide)
    dfield, drfield = put_map(x['field'], wide), put_map(x['rfield'], wide)

    # relayout, bit for bit, matrices and vectors
    for a, da, nc in ((J, dJ, 4), (V, dV, 2)):
        fr = Frame(pix, nc, other, cd, wide)
        (pol.to_planes if layout == 'aos' else pol.from_planes)(da, out=fr.win)
        fr.check()
        assert np.array_equal(get(fr.win, other), a)
        back = (pol.from_planes if layout == 'aos' else pol.to_planes)(fr.win)
        assert np.array_equal(get(back, layout), a)

    # field x J: complex and real fields, across layouts, and in place
    for f, df in ((x['field'], dfield), (x['rfield'], drfield)):
        for ol in (layout, other):
            fr = Frame(pix, 4, ol, cd, wide)
            pol.apply_polarization_optic(df, dJ, layout=layout, out_layout=ol, out=fr.win)
            fr.check()
            assert np.all(np.abs(get(fr.win, ol) - PP.scale(J, f)) <= C.scale_bound(J, f, at))
    apart = pol.apply_polarization_optic(dfield, dJ, layout=layout)
    work = dJ.clone() if not wide else put(J, layout, wide)
    same = pol.apply_polarization_optic(dfield, work, layout=layout, out=work)
    assert same.data_ptr() == work.data_ptr() and torch.equal(same, apart)
    fr = Frame(pix, 2, layout, cd, wide)
    pol.apply_polarization_optic(dfield, dV, layout=layout, out=fr.win)
    fr.check()
    assert np.all(np.abs(get(fr.win, layout) - PP.scale(V, x['field'])) <= C.scale_bound(V, x['field'], at))

    # the chain: K = 1 ... 6, constants among the maps, a vector tail
    A, B, CV = C.CONST_A.astype(c), C.CONST_B.astype(c), C.CONST_V.astype(c)
    if tall:
        chains = [([A, J, J2], [A, dJ, dJ2], False), ([J, B, V], [dJ, B, dV], True)]
    else:
        m, dm = x['mats'], [dJ, dJ2] + [put(a, layout, wide) for a in x['mats'][2:]]
        chains = [(m[:k], dm[:k], False) for k in range(1, 7)]
        chains += [([A, m[0], B, m[1]], [A, dm[0], B, dm[1]], False), ([m[0], A], [dm[0], A], False), ([A], [A], False),
                   ([V], [dV], True), ([m[0], V], [dm[0], dV], True), ([m[0], A, m[1], m[2], B, V], [dm[0], A, dm[1], dm[2], B, dV], True),
                   ([m[0], m[1], CV], [dm[0], dm[1], CV], True)]
    for ops, dops, tail in chains:
        for ol in (layout, other):
            fr = Frame(pix, 2 if tail else 4, ol, cd, wide)
            pol.jones_product(*dops, layout=layout, out_layout=ol, out=fr.win)
            fr.check()
            full = [np.broadcast_to(o, (*pix, *o.shape)) if o.ndim == 2 else o for o in ops]
            assert np.all(np.abs(get(fr.win, ol) - PP.chain(ops, tail)) <= C.chain_bound(full, at)), (len(ops), tail, ol)

    # Mueller, to both layouts, and Pauli
    want = PP.mueller(J)
    for ol in (layout, other):
        fr = Frame(pix, 16, ol, rd, wide)
        pol.jones_to_mueller(dJ, layout=layout, out_layout=ol, out=fr.win)
        fr.check()
        d = C.dev_eps(get(fr.win, ol), want, at, C.mueller_scale(J))
        assert d <= C.bound('mueller', at, True) + C.bound('mueller', at, False), d
    fr = Frame(pix, 4, 'planes', cd, wide)
    pol.pauli_coefficients(dJ, layout=layout, out=fr.win)
    fr.check()
    assert np.array_equal(tonp(fr.win), PP.pauli(J))

    # generators on maps, with and without the field inside
    dth, dde = put_map(x['theta'], wide), put_map(x['delta'], wide)
    for name, kind, call, params, charge in (
            ('ret', PP.RETARDER, lambda **kw: pol.linear_retarder(dde, dth, **kw), [x['delta'], x['theta']], 1.0),
            ('vvr6', PP.VORTEX, lambda **kw: pol.vector_vortex_retarder(6, dth, C.VVR_RETARDANCE, C.VVR_ROTATE, **kw),
             [x['theta'], C.VVR_RETARDANCE, C.VVR_ROTATE], 6)):
        fr = Frame(pix, 4, layout, cd, wide)
        call(out_layout=layout, out=fr.win)
        fr.check()
        plain = get(fr.win, layout)
        lim = C.bound(name, at, True) + C.bound(name, at, False)
        assert C.dev_eps(plain, PP.optic(kind, params, pix, c, charge=charge), at) <= lim, name
        fr2 = Frame(pix, 4, other, cd, wide)
        call(out_layout=other, out=fr2.win, field=dfield)
        fr2.check()
        assert np.all(np.abs(get(fr2.win, other) - PP.scale(plain, x['field'])) <= C.scale_bound(plain, x['field'], at)), name
    rot = get(pol.jones_rotation_matrix(0.3, shape=pix, out_layout=layout), layout)
    assert np.array_equal(rot, np.broadcast_to(PP.optic(PP.ROTATION, [0.3], (), c), (*pix, 2, 2)))


# ---------------------------------------------------------------- structure, precision rules
@both
def test_exact_structure_and_dtypes(pol, at):
    c, pix = C.cdt(at), (5, 67)
    eye = dev(np.broadcast_to(np.eye(2, dtype=c), (*pix, 2, 2)))
    assert np.array_equal(tonp(pol.jones_to_mueller(eye)), np.broadcast_to(np.eye(4, dtype=C.rdt(at)), (*pix, 4, 4)))
    assert np.array_equal(tonp(pol.linear_retarder(0)), np.eye(2, dtype=c))
    assert np.array_equal(tonp(pol.linear_retarder(0, shape=pix)), np.broadcast_to(np.eye(2, dtype=c), (*pix, 2, 2)))
    th = dev(np.random.default_rng(2).uniform(-3, 3, pix).astype(C.rdt(at)))
    assert torch.equal(pol.half_wave_plate(th), pol.linear_retarder(np.pi, th))
    assert torch.equal(pol.quarter_wave_plate(th), pol.linear_retarder(np.pi / 2, th))
    # scalars alone: the config's precision; maps: the maps' precision, whatever the config says
    assert pol.linear_retarder(0.2, 0.1, shape=pix).dtype == TCD[at]
    for p in (64, 32):
        m = th.to(TRD[p])
        assert pol.linear_retarder(m).dtype == TCD[p] and pol.vector_vortex_retarder(2, m).dtype == TCD[p]
        assert pol.jones_to_mueller(pol.linear_retarder(m)).dtype == TRD[p]
    with pytest.raises(ValueError):
        pol.jones_product(*[eye] * 7)
    with pytest.raises(ValueError):
        pol.jones_to_mueller(eye, out=torch.empty((5, 66, 4, 4), dtype=TRD[at], device='cuda'))


# ---------------------------------------------------------------- end to end: a vortex field through the FFT as a stack
@both
def test_vortex_field_through_focus_as_a_stack(pol, at):
    from prysm_amd import propagation
    n = 32
    rng = np.random.default_rng(9)
    y, x = np.mgrid[-n // 2:n // 2, -n // 2:n // 2].astype(C.rdt(at))
    t = dev(np.arctan2(y, x))
    E = dev((rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))).astype(C.cdt(at)))
    stack = pol.vector_vortex_retarder(2, t, field=E, out_layout='planes')
    assert stack.shape == (4, n, n)
    got = pol.from_planes(propagation.focus(stack, 2))
    aos = pol.vector_vortex_retarder(2, t, field=E)
    want = pol.jones_adapter(propagation.focus)(aos, 2)
    assert got.shape == want.shape and torch.equal(got, want)


def test_capture_replays_the_same_bits(pol):
    from prysm_amd import graph
    i = C.inputs(32)
    t, f = dev(i['t']), dev(i['field'])
    A = C.CONST_A.astype(np.complex64)

    def model(t, f):
        v = pol.vector_vortex_retarder(2, t, C.VVR_RETARDANCE, C.VVR_ROTATE, field=f)
        q = pol.quarter_wave_plate(t)
        return pol.jones_to_mueller(pol.jones_product(q, v, A))

    eager = model(t, f).clone()
    cap = graph.capture(model, t, f)
    assert torch.equal(cap(t, f), eager)
    assert torch.equal(cap(t, f), eager)


@layouts
def test_unaligned_views_take_the_scalar_path(pol, layout):
    """an aos complex64 view one complex element into its buffer is 8-byte, not 16-byte, aligned, and an aos float32 Mueller output one
    real into its buffer 4-byte aligned: the kernels then use one access per component, with the same bits as the 16-byte path"""
    pix, n = (5, 67), 5 * 67
    x = rand_inputs(32, pix)
    J, J2, V = x['mats'][0], x['mats'][1], x['vec']

    def off(a):         # the aos array at an odd element of a NaN-framed buffer
        t = dev(a)
        buf = torch.full((t.numel() + 2,), float('nan'), dtype=t.dtype, device='cuda')
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        return buf, view

    def out(shape, dtype):
        buf = torch.full((int(np.prod(shape)) + 2,), float('nan'), dtype=dtype, device='cuda')
        return buf, buf[1:-1].view(shape)

    def framed(buf):
        return bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1])) and not bool(torch.isnan(buf[1:-1]).any())

    _, dJ = off(J)
    _, dJ2 = off(J2)
    _, dV = off(V)
    assert dJ.data_ptr() % 16 == 8 and dV.data_ptr() % 16 == 8
    ol = PP.layout_code(layout)
    # loads from unaligned aos, stores to `layout`; then loads from `layout`, stores to unaligned aos
    assert np.array_equal(get(pol.apply_polarization_optic(dev(x['field']), dJ, out_layout=layout), layout),
                          get(pol.apply_polarization_optic(dev(x['field']), dev(J), out_layout=layout), layout))
    mid = pol.to_planes(dJ) if ol == PP.PLANES else dev(J)
    for a, da, src in ((J, dJ, mid), (V, dV, pol.to_planes(dV) if ol == PP.PLANES else dev(V))):
        buf, o = out(a.shape, torch.complex64)
        if ol == PP.PLANES:
            pol.from_planes(src, out=o)
        else:
            pol.apply_polarization_optic(dev(np.ones(pix, np.float32)), src, out=o)      # times 1: exact
        assert framed(buf) and np.array_equal(tonp(o), a)
    buf, o = out((*pix, 2, 2), torch.complex64)
    pol.jones_product(dJ, dJ2, out=o)
    assert framed(buf) and torch.equal(o, pol.jones_product(dev(J), dev(J2)))
    buf, o = out((*pix, 2, 1), torch.complex64)
    pol.jones_product(dJ, dV, out=o)
    assert framed(buf) and torch.equal(o, pol.jones_product(dev(J), dev(V)))
    buf, o = out((*pix, 2, 2), torch.complex64)
    th = dev(x['theta'])
    pol.vector_vortex_retarder(2, th, 2.5, 0.3, out=o)
    assert framed(buf) and torch.equal(o, pol.vector_vortex_retarder(2, th, 2.5, 0.3))
    # the Mueller record one real into its buffer
    buf, o = out((*pix, 4, 4), torch.float32)
    assert o.data_ptr() % 16 == 4
    pol.jones_to_mueller(dJ if ol == PP.AOS else mid, layout=layout, out_layout='aos', out=o)
    assert framed(buf) and torch.equal(o, pol.jones_to_mueller(dev(J)))
    cs = pol.pauli_coefficients(dJ)
    assert np.array_equal(np.stack([tonp(c) for c in cs]), PP.pauli(J))
