"""GPU: every modal reduction on the second trip of its grid-stride loop -- the Zernike, Q, recurrence and fibre projections past
their 1024 workgroups of 1024 points, the stored-basis dot product past 256 chunks in its second stage, the segmented projection past
256 workgroups per window, the separable adjoint past 1024 columns, the fibre overlap at and past its 262144 threads, and the Bayer
class maxima past 4096 workgroups.  Sizes, references and the three checks (exact count, probes, dense) with their bounds are
tests/modal_scale_common.py's, none of which grows with the point count; tests/test_modal_scale_host.py shows on the CPU that each
check passes for the numpy models summed in the kernels' order and that a skipped trip, a skipped ragged tile and a doubled tile are
each noticed.  Every case runs twice and must give the same bits; one Zernike case replays under graph capture.

A stack of 3 (a piece of 2 vectors and one of 1) must equal its members taken one at a time, bit for bit.

Segmented: the window of a segment is a square about the hexagon and the mask weighs the input, so on a symmetric grid the second
trip and the last tile of the largest window lie outside the hexagon and a kernel that skipped them would be right.  The grid here
ends on the row through the centre of the middle segment: its window is clipped to 511 rows of 514 columns, the trip past
256 x 1024 points is the row through the widest part of the hexagon (510 points, two waves of workgroup 0), and the last points
are its vertex.

Bayer: the issue's 1370 x 43 x 3 image has 343 row groups of 4, below 4096 / 3 workgroup rows, so it does not stride; it is kept
and a 5466 x 43 x 3 image, which does, stands beside it.
"""
import numpy as np
import pytest
import torch

import modal_scale_common as MS
from gpu_common import tonp

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
CAP = 1024
SIZES = MS.sizes(CAP)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _devcoords(unit, n, dt):
    return tuple(dev(a[:n]) for a in MS.unit_coords(unit, dt))


def _run(label, bat, project, stack=True):
    """project((B, n) device tensor) -> (B, K): the battery's checks, two runs bit for bit, the dense rows as a stack of 3 against
    its members"""
    G = dev(bat.G)
    first = project(G).clone()
    assert torch.equal(first, project(G)), label
    assert bat.verify(tonp(first), label) == []
    if stack:
        D = G[bat.dense0:]
        assert D.shape[0] == 3
        st = tonp(project(D).clone()).astype(np.float64)
        one = np.stack([tonp(project(D[b:b + 1]))[0] for b in range(3)]).astype(np.float64)
        print(f'{label} {np.dtype(bat.dt).name} n={bat.n} stack of 3 against its members: {np.max(np.abs(st - one)) / np.max(np.abs(st)):.3e}')
        assert np.array_equal(st, one)
    return first


def _e0(K, dt):
    c = np.zeros(K, dtype=dt)
    c[0] = 1
    return c


# ----------------------------------------------------------------------------- Zernike

@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('unit', ['zernike', 'zernike polar'])
def test_zernike_adjoint(unit, n, dt):
    from prysm_amd import _lib as L, polynomials as P
    from prysm_amd.polynomials import zernike as Z
    assert MS.cap_of('zernike') == CAP and MS.groups('zernike', n, dt) == CAP and n > CAP * MS.TILE
    u, v = _devcoords(unit, n, dt)
    code = L.PM_ZERNIKE_POLAR if unit == 'zernike polar' else L.PM_ZERNIKE_CARTESIAN
    # the device's piston is 1 to the bit on a tile, which the exact count relies on
    assert bool(torch.all(Z._sum(_e0(len(MS.ZERNIKE_NMS), dt), MS.ZERNIKE_NMS, u[:1024], v[:1024], True, code) == 1))
    if unit == 'zernike':
        project = lambda G: P.zernike_sum_adjoint(G, MS.ZERNIKE_NMS, u, v)                   # noqa: E731
    else:
        project = lambda G: Z._adjoint(G, MS.ZERNIKE_NMS, u, v, True, code)                  # noqa: E731
    _run(unit, MS.battery(unit, n, dt), project)


@pytest.mark.parametrize('dt', DTYPES)
def test_stored_basis_adjoint_past_256_chunks(dt):
    """pm_modes_dot at n_vec: 515 chunks of 2048 points, so reduce_partials_kernel's threads take up to three partials each"""
    from prysm_amd import _lib as L, polynomials as P
    n = SIZES[1]
    code = L.PM_F32 if dt == np.float32 else L.PM_F64
    K = len(MS.ZERNIKE_NMS)
    chunks = L.load().pm_modes_dot_workspace(code, K, n) // (K * np.dtype(dt).itemsize)
    assert chunks == -(-n // 2048) > 256
    stored = MS.reference('zernike', dt)[:, :n].astype(dt)
    basis = dev(stored)
    bat = MS.Battery(stored.astype(np.float64), n, CAP, dt, MS.TOL_ZERNIKE[dt], piston=0)
    _run('zernike', bat, lambda G: torch.stack([P.sum_of_2d_modes_adjoint(basis, g) for g in G]), stack=False)


def test_zernike_adjoint_replays_under_capture():
    from prysm_amd import graph, polynomials as P
    n, dt = SIZES[1], np.float32
    x, y = _devcoords('zernike', n, dt)
    bat = MS.battery('zernike', n, dt)
    G = dev(bat.G)

    def run(g):
        return P.zernike_sum_adjoint(g, MS.ZERNIKE_NMS, x, y)
    eager = run(G).clone()
    model = graph.capture(run, G)
    for _ in range(2):
        assert torch.equal(model(G), eager)
    other = G.flip(0).contiguous()                       # the replay reads its input on the device
    want = run(other).clone()
    assert torch.equal(model(other), want) and not torch.equal(want, eager)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- Q polynomials

@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('unit', ['q2d', 'qcon'])
def test_q_adjoints(unit, n, dt):
    """no mode of the Q families is constant: probes and the dense check"""
    from prysm_amd import polynomials as P
    assert MS.cap_of('qpoly') == CAP and MS.groups('qpoly', n, dt) == CAP
    u, v = _devcoords(unit, n, dt)
    if unit == 'q2d':
        project = lambda G: P.Q2d_sum_adjoint(G, MS.Q2D_NMS, u, v)                           # noqa: E731
    else:
        project = lambda G: P.Qcon_sum_adjoint(G, MS.QCON_NS, u)                             # noqa: E731
    _run(unit, MS.battery(unit, n, dt), project)


# ----------------------------------------------------------------------------- the recurrence families

@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('unit', ['jacobi', 'jacobi radial', 'cheby1', 'legendre'])
def test_recurrence_adjoints(unit, n, dt):
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials import _recur as R
    assert MS.cap_of('recur') == CAP and MS.groups('recur', n, dt) == CAP
    u, v = _devcoords(unit, n, dt)
    if unit == 'jacobi radial':
        K = len(MS.JACOBI_NS)
        one = P.jacobi_radial_sum(_e0(K, dt), MS.JACOBI_NS, *MS.JACOBI, u[:1024], v[:1024], MS.RADIUS)
        project = lambda G: P.jacobi_radial_sum_adjoint(G, MS.JACOBI_NS, *MS.JACOBI, u, v, MS.RADIUS)        # noqa: E731
    else:
        fam, params, ns = ('jacobi', MS.JACOBI, MS.JACOBI_NS) if unit == 'jacobi' else (unit, (), MS.FAMILY_NS)
        one = R.sum1d(fam, params, _e0(len(ns), dt), ns, u[:1024])[0]
        project = lambda G: R.project1d(fam, params, ns, u, databar=G)                                       # noqa: E731
    assert bool(torch.all(one == 1))                     # order 0 on the device is 1 to the bit
    _run(unit, MS.battery(unit, n, dt), project)


SEP_MNS = [(m, n) for m in range(5) for n in range(4)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('fam,shape', [('cheby1', (70, 1100)), ('cheby1', (67, 1027)), ('legendre', (67, 1027))])
def test_separable_adjoint_past_1024_columns(fam, shape, dt):
    """recur2_project_rows_kernel's 1024 threads take a second column each, raggedly: 76 of them at 1100 columns, 3 at 1027.  The
    probes are whole columns (a column is `rows` points): 1023, 1024, 1026 and the last."""
    from prysm_amd import polynomials as P
    from prysm_amd.polynomials import recur_plan as RP
    rows, cols = shape
    assert cols > 1024 and cols % 64
    adj = P.cheby1_2d_sum_adjoint if fam == 'cheby1' else P.legendre_2d_sum_adjoint
    x, y = np.linspace(-1, 1, cols).astype(dt), np.linspace(-1, 0.8, rows).astype(dt)
    px = RP.evaluate(RP.plan(fam, nmax=4), x.astype(np.float64))[0]
    py = RP.evaluate(RP.plan(fam, nmax=3), y.astype(np.float64))[0]
    fmax = np.max(np.abs(py), axis=1)[:, None] * np.max(np.abs(px), axis=1)[None, :]
    xd, yd = dev(x), dev(y)
    order = lambda W: np.array([W[n, m] for m, n in SEP_MNS])                                # noqa: E731
    e, tol = MS.eps(dt), MS.TOL_ZERNIKE[dt]
    rng = np.random.default_rng(61)
    gs = []
    for j in sorted({1023, 1024, 1026, cols - 1}):
        g = np.zeros(shape, dtype=dt)
        g[:, j] = 1
        gs.append((f'column {j}', 'probe', g))
    gs += [(f'dense {i}', 'dense', rng.standard_normal(shape).astype(dt)) for i in range(3)]
    G = dev(np.stack([g for _, _, g in gs]))
    first = adj(G, SEP_MNS, xd, yd).clone()
    assert torch.equal(first, adj(G, SEP_MNS, xd, yd))
    got = tonp(first).astype(np.float64)
    for (name, kind, g), a in zip(gs, got):
        g64 = g.astype(np.float64)
        want, mag = py @ g64 @ px.T, np.abs(py) @ np.abs(g64) @ np.abs(px).T
        if kind == 'probe':
            bound = rows * tol * fmax + 16 * e * mag
        else:
            bound = tol * fmax * np.abs(g64).sum() + 32 * e * mag
        ratio = np.max(np.abs(a - order(want)) / order(bound))
        print(f'separable {fam} {rows} x {cols} {np.dtype(dt).name} {name}: deviation / bound {ratio:.3e}')
        if kind == 'probe':
            assert np.max(np.abs(order(want)) / order(rows * fmax)) > 0.1                    # the column weighs in some mode
        if kind == 'probe' or dt == np.float64:
            assert ratio <= 1, name
    st = got[-3:]
    one = np.stack([tonp(adj(G[b], SEP_MNS, xd, yd)) for b in range(len(gs) - 3, len(gs))]).astype(np.float64)
    print(f'separable {fam} {rows} x {cols} {np.dtype(dt).name} stack against its members: {np.max(np.abs(st - one)) / np.max(np.abs(st)):.3e}')
    assert np.array_equal(st, one)


# ----------------------------------------------------------------------------- fibres

@pytest.fixture(scope='module')
def FB(pa):
    from prysm_amd.x import fibers
    return fibers


def _mode_set(FB, n, dt):
    import fibers_common as FC
    r, t = _devcoords('fiber', n, dt)
    return FB.prepare(MS.FIBER_V, MS.fiber_mode_dict(), FC.A, r, t)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', SIZES)
def test_fibre_project_norms_and_coupling(FB, n, dt):
    assert MS.cap_of('fiber') == CAP and MS.groups('fiber', n, dt) == CAP
    ms = _mode_set(FB, n, dt)
    bat = MS.battery('fiber', n, dt)
    assert ms.nmodes == bat.ref.shape[0] == 8
    _run('fiber', bat, ms.project)
    # the modes against themselves: values off by at most TOL max|Z_k| move a square by 2 |Z_k| of that
    e, tol = MS.eps(dt), MS.tol_fiber(dt)
    norms = ms.norms().clone()
    ms._norm = None
    assert torch.equal(norms, ms.norms())
    want = (bat.ref * bat.ref).sum(axis=1)
    bound = 2 * tol * bat.zmax * np.abs(bat.ref).sum(axis=1) + 32 * e * want
    ratio = np.max(np.abs(tonp(norms).astype(np.float64) - want) / bound)
    print(f'fiber {np.dtype(dt).name} n={n} norms: deviation / bound {ratio:.3e}')
    assert ratio <= 1
    # coupling is |project|^2 / (norms * sum |E|^2) of three quantities that are each held to a reference at this size
    r, t = (a[:n].astype(np.float64) for a in MS.unit_coords('fiber', dt))
    E = (np.exp(-(r / 3.5) ** 2) * np.exp(0.3j * r * np.cos(t))).astype(np.complex64 if dt == np.float32 else np.complex128)
    Ed = dev(E)
    eta = ms.coupling(Ed).clone()
    assert torch.equal(eta, ms.coupling(Ed))
    p = tonp(ms.project(Ed)).astype(np.complex128)
    power = float(FB.overlap(Ed, Ed)[2])
    made = np.abs(p) ** 2 / (tonp(norms).astype(np.float64) * power)
    assert np.max(np.abs(tonp(eta).astype(np.float64) - made)) <= 8 * e * np.max(made)
    # and the complex projection is its two real ones, against the reference
    for part, got in ((E.real, p.real), (E.imag, p.imag)):
        g64 = part.astype(np.float64)
        bound = tol * bat.zmax * np.abs(g64).sum() + 32 * e * (np.abs(bat.ref) @ np.abs(g64))
        ratio = np.max(np.abs(got - bat.ref @ g64) / bound)
        print(f'fiber {np.dtype(dt).name} n={n} project of a complex field: deviation / bound {ratio:.3e}')
        assert dt == np.float32 or ratio <= 1


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', SIZES + (262144 + 1, 262144 + 5 * 256 + 133))
def test_overlap_counts_every_point(FB, n, dt):
    """integer-valued fields: S, I1 and I2 are integers below 2^24 whatever the order, so they are exact in float32 too.  262145 and
    263557 are one point and a ragged stretch past 262144, the most threads the overlap launches (1024 workgroups of 256)."""
    assert MS.groups('overlap', n, dt) == min(-(-n // 1024), CAP)
    p = np.arange(n)
    ar, ai, br, bi = 1 + p % 2, (p // 3) % 2, 1 + (p // 2) % 2, p % 5 % 3 - 1
    want = np.array([np.sum(ar * br + ai * bi), np.sum(ai * br - ar * bi), np.sum(ar * ar + ai * ai), np.sum(br * br + bi * bi)],
                    dtype=np.float64)
    assert np.max(np.abs(want)) < 2 ** 24 and 5 * n < 2 ** 24
    ct = np.complex64 if dt == np.float32 else np.complex128
    E1, E2 = dev((ar + 1j * ai).astype(ct)), dev((br + 1j * bi).astype(ct))
    res = FB.overlap(E1, E2).clone()
    assert torch.equal(res, FB.overlap(E1, E2))
    got = tonp(res).astype(np.float64)
    assert np.array_equal(got[:4], want), (got[:4], want)
    eta = (want[0] ** 2 + want[1] ** 2) / (want[2] * want[3])
    assert abs(got[4] - eta) <= 8 * MS.eps(dt) * eta
    assert torch.equal(FB.mode_overlap_integral(E1, E2), res[4])
    # a real field against a complex one: the kernel's other instantiations
    R1 = dev(ar.astype(dt))
    got = tonp(FB.overlap(R1, E2)).astype(np.float64)
    assert np.array_equal(got[:4], [np.sum(ar * br), np.sum(-ar * bi), np.sum(ar * ar), want[3]])
    got = tonp(FB.overlap(E1, R1)).astype(np.float64)
    assert np.array_equal(got[:4], [np.sum(ar * ar), np.sum(ai * ar), want[2], np.sum(ar * ar)])


# ----------------------------------------------------------------------------- segmented

SEG_NMS = [(0, 0), (1, 1), (1, -1), (2, 0), (2, 2), (2, -2)]
SEG_COLS = 1415


def _segment_grid(cap):
    """(x, y, window points): 1415 columns at a pitch that gives windows 514 wide, and the fewest rows whose 514-wide window has more
    than cap * 1024 points and no multiple of 1024; the last row runs through the centre of the middle segment"""
    from prysm_amd import segmented as SG
    dx = 4.2 / (SEG_COLS - 1)
    w = 2 * int(1.32 * SG.FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX / 2 / dx + 1)
    rows = next(r for r in range(1, w) if r * w > cap * MS.TILE and (r * w) % MS.TILE)
    xv = (np.arange(SEG_COLS) - (SEG_COLS + 1) // 2) * dx
    yv = (np.arange(rows) - (rows - 1)) * dx
    x, y = np.meshgrid(xv, yv)
    return x, y, rows * w


@pytest.fixture(scope='module')
def seg_cache():
    return {}


def _aperture(cache, dt, route):
    from prysm_amd import segmented as SG
    from prysm_amd.polynomials import zernike_nm_seq, zernike_plan as ZP
    if (dt, route) not in cache:
        cap = MS.cap_of('segment')
        x, y, wpts = _segment_grid(cap)
        ap = SG.CompositeHexagonalAperture(x.astype(dt), y.astype(dt), 1, 1.32, 0.05, segment_angle=90, share_grids=False)
        if route == 'walk':
            ap.prepare_opd_bases(zernike_nm_seq, SEG_NMS)
        else:
            ap.prepare_opd_bases(lambda orders, r, t: zernike_nm_seq(orders, r, t), SEG_NMS)
        plan = ap.segment_plan
        s0 = int(np.argmax([int(d['h']) * int(d['w']) for d in plan.desc]))
        # the size the test is about, from the plan itself
        assert plan.window_pts == int(plan.desc[s0]['h']) * int(plan.desc[s0]['w']) == wpts == 511 * 514
        assert wpts > cap * MS.TILE and wpts % MS.TILE and MS.groups('segment', wpts, dt, len(SEG_NMS)) == cap == 256
        if (dt, 'bases') not in cache:
            table, nr = ZP.plan(SEG_NMS), ap.vtov / 2
            cache[dt, 'bases'] = [ZP.evaluate(table, lx.astype(np.float64) / nr, ly.astype(np.float64) / nr, len(SEG_NMS))
                                  for lx, ly in ap.host_local_coords]
        cache[dt, route] = ap, plan, s0
    return cache[dt, route] + (cache[dt, 'bases'],)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('route', ['walk', 'stored'])
def test_segmented_adjoint_past_256_workgroups_a_window(seg_cache, route, dt):
    from prysm_amd import _lib as L, segmented as SG
    ap, plan, s0, bases = _aperture(seg_cache, dt, route)
    assert ap._route['kind'] == (L.PM_SEGMENT_ZERNIKE if route == 'walk' else L.PM_SEGMENT_STORED)
    cap, K, S = 256, len(SEG_NMS), len(plan.desc)
    y0, x0, h, w, mask = plan._seg(s0)
    mask = mask.astype(np.float64)
    n = h * w
    # the modes of the largest window as the kernel weighs them: mask * Z
    bat = MS.Battery(bases[s0].reshape(K, n) * mask, n, cap, dt, MS.TOL_ZERNIKE[dt])
    bat.placement()                                      # the trip past the cap and the last tile lie inside the hexagon
    exact = ((1 + np.arange(n) % 3) * (mask == 1)).astype(dt)
    assert np.count_nonzero(exact[cap * MS.TILE:]) > 500 and exact.sum() < 2 ** 24
    rows_g = np.concatenate([exact[None], bat.G])
    G = np.zeros((len(rows_g), *plan.shape), dtype=dt)
    G[:, y0:y0 + h, x0:x0 + w] = rows_g.reshape(-1, h, w)
    # piston times a mask of 1 is 1 to the bit on the device
    c = np.zeros((S, K), dtype=dt)
    c[s0, 0] = 1
    opd = tonp(ap.compose_opd(c))[y0:y0 + h, x0:x0 + w].ravel()
    assert np.all(opd[mask == 1] == 1)
    Gd = dev(G)
    first = ap.compose_opd_adjoint(Gd).clone()
    assert first.shape == (len(G), S, K) and torch.equal(first, ap.compose_opd_adjoint(Gd))
    got = tonp(first).astype(np.float64)
    label = f'segment {route}'
    print(f'{label} {np.dtype(dt).name} n={n} exact: got {got[0, s0, 0]:.1f} want {float(exact.sum()):.1f}')
    assert got[0, s0, 0] == float(exact.sum())
    assert bat.verify(got[1:, s0, :], label) == []
    # every segment, the neighbours whose windows overlap this one included, against the numpy model of the plan
    e, tol = MS.eps(dt), MS.TOL_ZERNIKE[dt]
    absb = [np.abs(b) for b in bases]
    zmax = np.array([np.max(np.abs(b.reshape(K, -1)), axis=1) if b.size else np.zeros(K) for b in bases])
    for i in range(len(G)):
        if dt == np.float32 and i > len(G) - 4:
            continue                                     # the dense rows are printed above, asserted in float64
        g64 = G[i].astype(np.float64)
        want, mag = SG.evaluate_project(plan, g64, bases), SG.evaluate_project(plan, np.abs(g64), absb)
        weight = SG.evaluate_project(plan, np.abs(g64), [np.ones_like(b[:1]) for b in bases])
        bound = tol * zmax * weight + 32 * e * mag
        assert np.all(np.abs(got[i] - want) <= bound), (i, float(np.max(np.abs(got[i] - want) / (bound + 1e-300))))
    D = Gd[-3:]
    st = tonp(ap.compose_opd_adjoint(D)).astype(np.float64)
    one = np.stack([tonp(ap.compose_opd_adjoint(D[b])) for b in range(3)]).astype(np.float64)
    print(f'{label} {np.dtype(dt).name} stack of 3 against its members: {np.max(np.abs(st - one)) / np.max(np.abs(st)):.3e}')
    assert np.array_equal(st, one)


# ----------------------------------------------------------------------------- Bayer class maxima

def _class_max(a, classes, n):
    from prysm_amd import _lib as L
    lib = L.load()
    t = dev(a)
    m = a.shape[0]
    ld = t.numel() // m
    out = torch.empty(4, dtype=torch.float64, device='cuda')
    ws = L.workspace(int(lib.pm_bayer_class_max_workspace()))
    code = L.PM_F32 if a.dtype == np.float32 else L.PM_F64
    L.check(lib.pm_bayer_class_max(code, classes, 1, m, n, L.ptr(t), ld, m * ld, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()))
    return out


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('nan', [False, True])
def test_mosaic_class_maxima_past_4096_workgroups(dt, nan):
    """5466 x 130: 3 workgroup columns leave 1365 workgroup rows of 4 rows, so rows 5460 .. 5465 are read on a second trip.  Every
    class has its one maximum there, class 3 in the last row."""
    from prysm_amd import _lib as L
    m, n = 5466, 130
    gy = min((m + 3) // 4, 4096 // ((n + 63) // 64))
    assert L.load().pm_bayer_class_max_workspace() == 4096 * 4 * 8 and m > 4 * gy
    a = np.random.default_rng(71).random((m, n)).astype(dt)
    spots = [(4 * gy, 64), (4 * gy + 2, 129), (4 * gy + 1, 0), (m - 1, 127)]
    for k, (r, c) in enumerate(spots):
        assert 2 * (r & 1) + (c & 1) == k and r >= 4 * gy
        a[r, c] = 2 + k
    if nan:
        a[spots[2]] = np.nan
    want = np.array([a[0::2, 0::2].max(), a[0::2, 1::2].max(), a[1::2, 0::2].max(), a[1::2, 1::2].max()], dtype=np.float64)
    assert np.array_equal(want, [2, 3, np.nan if nan else 4, 5], equal_nan=True)
    got = _class_max(a, L.PM_BAYER_MOSAIC, n).clone()
    assert np.array_equal(tonp(got), want, equal_nan=True), (tonp(got), want)
    assert np.array_equal(tonp(_class_max(a, L.PM_BAYER_MOSAIC, n)), tonp(got), equal_nan=True)
    # through the package: the gains divided by the largest max * gain / saturation
    from prysm_amd import bayer
    if not nan:
        scaled = tonp(bayer.wb_prescale(dev(a.copy()), 1.0, 1.0, 1.0, 1.0, safe=True, saturation=1.0))
        ref = a.astype(np.float64) / 5
        assert np.max(np.abs(scaled - ref)) <= 4 * MS.eps(dt) * np.max(ref)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('nan', [False, True])
@pytest.mark.parametrize('m', [1370, 5466])
def test_rgb_class_maxima(m, dt, nan):
    """rows of 3 x 43 values.  1370 rows are 343 workgroup rows, one trip; 5466 rows go past the 1365 there are, and each channel has
    its one maximum in rows 5460 .. 5465, channel 2 in the last row"""
    from prysm_amd import _lib as L
    a = np.random.default_rng(72).random((m, 43, 3)).astype(dt)
    lo = 4 * min((m + 3) // 4, 4096 // 3)
    assert (m > lo) == (m == 5466)
    first = lo if m > lo else m - 6
    spots = [(first + 1, 10, 0), (first + 3, 42, 1), (m - 1, 0, 2)]
    for k, s in enumerate(spots):
        a[s] = 2 + k
    if nan:
        a[spots[1]] = np.nan
    want = np.array([a[..., 0].max(), a[..., 1].max(), a[..., 2].max()], dtype=np.float64)
    assert np.array_equal(want, [2, np.nan if nan else 3, 4], equal_nan=True)
    got = tonp(_class_max(a, L.PM_BAYER_RGB, 43))
    assert np.array_equal(got[:3], want, equal_nan=True), (got, want)
    assert np.array_equal(tonp(_class_max(a, L.PM_BAYER_RGB, 43))[:3], got[:3], equal_nan=True)
