"""GPU: csrc/cgemm.hip on every kernel form, edge and operand layout (the frames, data, references and checks are tests/cgemm_common.py;
tests/test_cgemm_host.py shows on the CPU that those checks notice faults).

Exact integer data compared with np.array_equal carries the coverage: the register-staged kernel in its four instantiations and both
precisions on ragged, tiny and empty shapes, its slab split-K with short last slabs and without a workspace; the LDS-DMA kernel's
four-wave 64 x 64, 128 x 128 and eight-wave forms from one K-tile up, its XCD remap on and off, its slabs, and the |.|^2 epilogue of
each; operands with leading dimensions above the row and the layouts that must leave the LDS-DMA route.  Rounded data then checks the
accuracy of one shape per form.  Every shape's route and slab count is asserted as it is observed through the ABI
(cgemm_common.dma_accepts, planned_slabs); a knob the library refuses raises in _lib.tuning_local and fails the test.
"""
import numpy as np
import pytest
import torch

import cgemm_common as G
from cgemm_common import C64, C128
from prysm_amd import _lib

pytestmark = pytest.mark.gpu

FEW_OPS = [(0, 0), (3, 1), (2, 2), (1, 3)]
DTYPES = [pytest.param(C64, id='c64'), pytest.param(C128, id='c128')]


@pytest.fixture(scope='module')
def lib(pa):
    return _lib.load()


def _alpha(i):
    return G.ALPHAS[i % len(G.ALPHAS)]


def _seed(*v):
    return [int(x) + 7 for x in v]


def _all_ops_exact(lib, dt, M, N, K, dma, ops=G.OPS, **kw):
    """exact data for every op pair; the route must be `dma` (complex64).  Returns the planned slab count."""
    S = None
    for i, (opA, opB) in enumerate(ops):
        r = G.run_exact(lib, dt, opA, opB, M, N, K, _alpha(i), _seed(dt, opA, opB, M, N, K), **kw)
        if dt == C64:
            assert r.dma == dma, f'op ({opA}, {opB}) {M} x {N} x {K}: the LDS-DMA kernel {"refused" if dma else "took"} this call'
        S = r.S
    return S


# ------------------------------------------------------------------------------------------------ the register-staged kernel

STAGED_SHAPES = [(64, 64, 16), (128, 64, 32), (65, 127, 17), (130, 63, 33), (1, 1, 1), (1, 130, 7), (130, 1, 8), (31, 65, 15), (63, 33, 1),
                 (65, 65, 0)]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('M,N,K', STAGED_SHAPES)
def test_staged_every_instantiation(lib, dt, M, N, K):
    """cgemm_kernel<T, BK, AKF, BKF> for both T and all four (AKF, BKF), with and without each conjugation, on whole tiles (complex64:
    gemm_dma = 0 sends the multiples of 64 here), ragged edges on both sides over several tiles, K tails shorter than a K-tile, K < BK,
    K = 1 and K = 0 (exact zeros over the whole interior), in wide frames"""
    knobs = G.STAGED if dt == C64 and (M, N, K) in STAGED_SHAPES[:2] else {}
    with _lib.tuning_local(**knobs):
        assert _all_ops_exact(lib, dt, M, N, K, dma=False) == 1
        if K == 0:
            r = G.run_exact(lib, dt, 0, 0, M, N, K, 2.0, _seed(0))
            assert not r.got.any() and r.got.shape == (M, N)


SPLIT_SHAPES = {(65, 65, 1000): 4, (65, 65, 1030): 8, (65, 65, 257): 2, (65, 65, 255): 1, (65, 65, 256): 2, (65, 33, 300): 2, (64, 64, 8200): 32}


SPLIT_CASES = [pytest.param(dt, *shape, id=f'{name}-{"x".join(map(str, shape))}') for shape in SPLIT_SHAPES for dt, name in ((C64, 'c64'), (C128, 'c128'))
               if not (shape[2] == 8200 and dt == C128)]


@pytest.mark.parametrize('dt,M,N,K', SPLIT_CASES)
def test_staged_slab_split_k(lib, dt, M, N, K):
    """the slabs of cgemm_ws_staged + splitk_reduce_kernel<T>: 4 slabs with a last one of 232, 8 with a last one of 22 (complex64) or 78
    (complex128), either side of the first split, a query of 32 slabs of which the launch runs 31 (complex64 under gemm_dma = 0); with
    exactly the queried bytes between guards, twice (bit-equal), without a workspace and with one byte too few (the unsplit fallback)"""
    with _lib.tuning_local(**(G.STAGED if K == 8200 else {})):
        assert G.planned_slabs(lib, dt, M, N, K)[0] == SPLIT_SHAPES[(M, N, K)]
        for i, (opA, opB) in enumerate(FEW_OPS):
            seed = _seed(dt, opA, opB, K)
            first = G.run_exact(lib, dt, opA, opB, M, N, K, _alpha(i), seed)
            assert not first.dma and first.S == SPLIT_SHAPES[(M, N, K)]
            assert np.array_equal(G.run_exact(lib, dt, opA, opB, M, N, K, _alpha(i), seed).got, first.got)
            for ws in ('null', 'short'):
                assert np.array_equal(G.run_exact(lib, dt, opA, opB, M, N, K, _alpha(i), seed, ws=ws).got, first.got)


@pytest.mark.parametrize('M,N,K', [(64, 64, 64), (128, 128, 48)])
def test_leaving_the_dma_route(lib, M, N, K):
    """complex64 multiples of 64 x 64 x 16: packed and wide-aligned operands are the LDS-DMA kernel's; a base at 8 mod 16 or an odd
    leading dimension, on A alone or on B alone, is refused by pm_cgemm_abs2 and exact through pm_cgemm (the staged kernel)"""
    _all_ops_exact(lib, C64, M, N, K, dma=True, kindA='packed', kindB='packed')
    _all_ops_exact(lib, C64, M, N, K, dma=True)
    for kindA, kindB in [('unaligned-base', 'wide-aligned'), ('wide-aligned', 'unaligned-base'), ('unaligned-ld', 'wide-aligned'),
                         ('wide-aligned', 'unaligned-ld')]:
        _all_ops_exact(lib, C64, M, N, K, dma=False, kindA=kindA, kindB=kindB)


# ------------------------------------------------------------------------------------------------ the LDS-DMA kernel

@pytest.mark.parametrize('M,N,K', [(64, 64, 16), (64, 64, 32), (64, 64, 48), (64, 64, 64), (64, 64, 80), (192, 64, 32), (256, 128, 48),
                                   (128, 256, 48)])
def test_dma_four_waves(lib, M, N, K):
    """64 x 64 tiles, four waves: 1 to 5 K-tiles (the ring's short prologue, its first turn), three workgroups (no XCD remap) and eight
    with ntm != ntn under the remap; wide-aligned frames (ld > row)"""
    with _lib.tuning_local(**G.FOUR):
        assert _all_ops_exact(lib, C64, M, N, K, dma=True) == 1


@pytest.mark.parametrize('M,N,K', [(128, 128, 16), (256, 128, 32), (512, 256, 48)])
def test_dma_128(lib, M, N, K):
    """128 x 128 tiles: one, two and eight workgroups (the remap on, ntm != ntn)"""
    with _lib.tuning_local(**G.BIG):
        assert _all_ops_exact(lib, C64, M, N, K, dma=True) == 1


@pytest.mark.parametrize('wgs,M,N,K', [(2, 64, 64, 32), (2, 64, 64, 64), (2, 64, 64, 96), (2, 64, 64, 160), (2, 64, 64, 48), (4, 128, 64, 96)])
def test_dma_eight_waves(lib, wgs, M, N, K):
    """64 x 64 tiles with two K-groups of four waves that run 1, 2, 3 and 5 K-tiles each and meet through LDS; K = 48 is no multiple of
    32 and takes the four-wave form again"""
    with _lib.tuning_local(**dict(G.EIGHT, gemm_dma_wgs=wgs)):
        assert _all_ops_exact(lib, C64, M, N, K, dma=True) == 1


DMA_SLAB_OPS = [(0, 0), (0, 2), (3, 0), (2, 3)]


@pytest.mark.parametrize('knobs,M,N,K,S', [(G.SLABS, 64, 64, 192, 2), (G.SLABS, 64, 64, 256, 4), (G.SLABS, 64, 64, 320, 4), (G.SLABS, 64, 64, 272, 1),
                                            (dict(G.SLABS, gemm_dma_wgs=8), 192, 64, 256, 4), ({}, 64, 64, 1024, 16)])
def test_dma_slabs(lib, knobs, M, N, K, S):
    """K split across workgroups and splitk_reduce_kernel<float>: 2 and 4 slabs, 4 of 80 (five K-tiles), none where half of K is no
    multiple of 16, 12 workgroups (no remap), and the default knobs' 16; twice (bit-equal) and without a workspace"""
    with _lib.tuning_local(**knobs):
        for i, (opA, opB) in enumerate(DMA_SLAB_OPS):
            seed = _seed(opA, opB, M, K)
            first = G.run_exact(lib, C64, opA, opB, M, N, K, _alpha(i), seed)
            assert first.dma and first.S == S, (first.dma, first.S)
            assert np.array_equal(G.run_exact(lib, C64, opA, opB, M, N, K, _alpha(i), seed).got, first.got)
            assert np.array_equal(G.run_exact(lib, C64, opA, opB, M, N, K, _alpha(i), seed, ws='null').got, first.got)


# K = 128 is the shortest K the slab form takes (two slabs of 64); cgemm_common's docstring has the bound that keeps it exact
ABS2_FORMS = [('four', G.FOUR, (64, 64, 16), 1), ('four', G.FOUR, (192, 64, 64), 1), ('four', G.FOUR, (128, 256, 48), 1),
              ('128', G.BIG, (128, 128, 16), 1), ('128', G.BIG, (256, 128, 64), 1),
              ('eight', G.EIGHT, (64, 64, 32), 1), ('eight', G.EIGHT, (64, 64, 64), 1), ('eight', dict(G.EIGHT, gemm_dma_wgs=4), (128, 64, 64), 1),
              ('slabs', G.SLABS, (64, 64, 128), 2), ('slabs', dict(G.SLABS, gemm_dma_wgs=8), (192, 64, 128), 2)]


@pytest.mark.parametrize('form,knobs,shape,S', ABS2_FORMS, ids=[f'{f[0]}-{"x".join(map(str, f[2]))}' for f in ABS2_FORMS])
def test_abs2_epilogue_every_form(lib, form, knobs, shape, S):
    """weight |alpha op(A) @ op(B)|^2 stored into a framed real image with ldr > N, then accumulated onto a preset one, exact; in the
    epilogue of the three unsplit forms and in splitk_reduce_abs2_kernel for the slabs"""
    with _lib.tuning_local(**knobs):
        for i, (opA, opB) in enumerate([(0, 0), (0, 2), (2, 2), (3, 1)]):
            got = G.run_abs2_exact(lib, opA, opB, *shape, (1.0, 0.5)[i % 2], (1.0, 2.0)[(i // 2) % 2], _seed(opA, opB, *shape))
            assert got == S, (form, got)


# ------------------------------------------------------------------------------------------------ accuracy

ACCURACY = [('staged c64', C64, {}, (65, 127, 17), False, 1), ('staged c128', C128, {}, (65, 127, 17), False, 1),
            ('staged c64', C64, dict(gemm_min_wgs=4096), (65, 65, 64), False, 1), ('staged c128', C128, dict(gemm_min_wgs=4096), (65, 65, 64), False, 1),
            ('dma four', C64, G.FOUR, (64, 64, 64), True, 1), ('dma 128', C64, G.BIG, (128, 128, 64), True, 1),
            ('dma eight', C64, G.EIGHT, (64, 64, 64), True, 2), ('dma slabs', C64, G.SLABS, (64, 64, 128), True, 2)]
_worst = {}


@pytest.mark.parametrize('route,dt,knobs,shape,dma,S', ACCURACY, ids=[f'{a[0]}-{"x".join(map(str, a[3]))}'.replace(' ', '-') for a in ACCURACY])
def test_accuracy(lib, route, dt, knobs, shape, dma, S):
    """normal operands, alpha = 0.37, against numpy complex128 within cgemm_common's derived bound, real and imaginary parts apart.  S is
    the number of partial sums that meet: the planned slabs (gemm_min_wgs = 4096 does not split K = 64: a slab keeps 128 of K), or the two
    K-groups of the eight-wave form"""
    M, N, K = shape
    with _lib.tuning_local(**knobs):
        planned = G.planned_slabs(lib, dt, M, N, K)[0]
        assert planned == (1 if route == 'dma eight' else S)
        for opA, opB in FEW_OPS + [(0, 2), (2, 0)]:
            rng = np.random.default_rng(_seed(dt, opA, opB, K))
            sa, sb = G.stored_shapes(opA, opB, M, N, K)
            A, B = G.crandn(rng, sa, G.NP_OF[dt]), G.crandn(rng, sb, G.NP_OF[dt])
            r = G.run_cgemm(lib, dt, opA, opB, M, N, K, 0.37, A, B)
            assert r.dma == dma
            ratio = G.rounded_ratio(r.got, A, B, opA, opB, 0.37, S, G.EPS[dt])
            _worst[route] = max(_worst.get(route, 0.0), ratio)
            assert ratio <= 1.0, (route, opA, opB, ratio)
    print(f'cgemm accuracy: {route} {M} x {N} x {K}: worst |err| / bound so far {_worst[route]:.3g}')


# ------------------------------------------------------------------------------------------------ the np facade

def test_facade_sliced_views_are_operand_flags(pa, lib, monkeypatch):
    """``@`` of sliced, transposed and conjugated views: each reaches pm_cgemm as the view's own storage with an op code and a leading
    dimension above the row -- no .contiguous() copy -- and is exact against numpy"""
    from prysm_amd import _ops, npfacade
    xp = npfacade.NumpyFacade()
    rng = np.random.default_rng(5)
    for cdt in (np.complex64, np.complex128):
        a, b = G.exact_operand(rng, (60, 44), cdt), G.exact_operand(rng, (44, 36), cdt)
        da, db = xp.asarray(a), xp.asarray(b)
        seen = []
        real = _ops.cgemm

        def spy(A, B, opA=0, opB=0, alpha=1.0):
            seen.append((A.data_ptr(), A.stride(0), opA, B.data_ptr(), B.stride(0), opB))
            return real(A, B, opA, opB, alpha)
        monkeypatch.setattr(_ops, 'cgemm', spy)
        item = np.dtype(cdt).itemsize
        pa_, pb_ = da.data_ptr(), db.data_ptr()

        got = da[2:50, 3:40] @ db[3:40, 1:30].conj()
        G.assert_exact(got.get(), a[2:50, 3:40].astype(np.complex128) @ b[3:40, 1:30].conj().astype(np.complex128), 'sliced @ sliced.conj()')
        assert seen.pop() == (pa_ + (2 * 44 + 3) * item, 44, 0, pb_ + (3 * 36 + 1) * item, 36, 1)

        got = da.T[3:40, 2:46].conj() @ db[:, 1:30]
        G.assert_exact(got.get(), a.T[3:40, 2:46].conj().astype(np.complex128) @ b[:, 1:30].astype(np.complex128), 'a.T[...].conj() @ ...')
        assert seen.pop() == (pa_ + (2 * 44 + 3) * item, 44, 3, pb_ + item, 36, 0)

        got = db[3:40, 1:30].T @ da[2:50, 3:40].T
        G.assert_exact(got.get(), b[3:40, 1:30].T.astype(np.complex128) @ a[2:50, 3:40].T.astype(np.complex128), 'b.T @ a.T')
        assert seen.pop() == (pb_ + (3 * 36 + 1) * item, 36, 2, pa_ + (2 * 44 + 3) * item, 44, 2)

        got = da[5:6, 3:40] @ db[3:40, 7:8]           # (1, K) by (K, 1)
        G.assert_exact(got.get(), a[5:6, 3:40].astype(np.complex128) @ b[3:40, 7:8].astype(np.complex128), '(1, K) @ (K, 1)')
        assert tuple(got.shape) == (1, 1) and seen.pop()[::3] == (pa_ + (5 * 44 + 3) * item, pb_ + (3 * 36 + 7) * item)
        assert not seen
        monkeypatch.setattr(_ops, 'cgemm', real)


def test_ops_cgemm_refuses_mismatched_operands_on_the_device(pa, lib):
    """the operand checks of _ops.cgemm on device tensors (tests/test_cgemm_host.py has them on the CPU)"""
    from prysm_amd import _ops
    a = torch.zeros((64, 64), dtype=torch.complex64, device='cuda')
    with pytest.raises(ValueError, match='same dtype'):
        _ops.cgemm(a, a.to(torch.complex128))
    with pytest.raises(ValueError, match='same device'):
        _ops.cgemm(a, a.cpu())
    with pytest.raises(ValueError, match='unit inner stride'):
        _ops.cgemm(a, a.T)
    assert _ops.cgemm_abs2(a, a) is not None
