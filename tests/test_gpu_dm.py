"""GPU: the deformable mirror (prysm_amd.x.dm) -- every reference fixture case (render, render_adjoint), known answers at user
sizes (a single poke is a rolled influence function; a 90 degree clocking is np.rot90), the dot-product identity where render_adjoint
is an exact adjoint, stacks, hipGraph capture and the surface feeding a propagation on the device."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from gpu_common import TOL32, TOL64, tonp
from oracle import prysm_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    d = np.load(os.path.join(GOLDEN, 'dm.npz'))
    return d, json.loads(bytes(d['meta']).decode())


def _kw(m):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in m.items()
            if k in ('Nout', 'Nact', 'sep', 'shift', 'rot', 'upsample')}


def _keep(shape_in, Nout_shape, M, off=(0, 0)):
    """pixels whose pull coordinate lies more than 1e-9 from 0 or n - 1 (the constant-mode cutoff makes those last-bit sensitive)"""
    from prysm_amd.x.dm import apply_homography
    r, c = np.meshgrid(np.arange(Nout_shape[0]) + off[0], np.arange(Nout_shape[1]) + off[1], indexing='ij')
    x, y = apply_homography(M, c.astype(float), r.astype(float))
    edge = np.zeros(r.shape, bool)
    for v, n in ((x, shape_in[1]), (y, shape_in[0])):
        edge |= (np.abs(v) < 1e-9) | (np.abs(v - (n - 1)) < 1e-9)
    return ~edge


def _rel(got, ref, mask=None):
    d = np.abs(got - ref)
    if mask is not None:
        d = d[mask]
    return np.max(d) / np.max(np.abs(ref))


CASES = ['plain', 'shift', 'clock', 'tilt', 'rot3', 'up064', 'up125', 'small', 'large', 'odd', 'f32']


@pytest.mark.parametrize('name', CASES)
def test_fixture_render_and_adjoint(fx, name):
    from prysm_amd.x.dm import DM, _window
    d, meta = fx
    m = meta[name]
    ifn = d[f"ifn_{m['ifn']}"].astype(m['dtype'])
    dm = DM(ifn, **_kw(m))
    dm.actuators[:] = torch.from_numpy(d[f'{name}_acts']).to(dm.actuators.device)
    tol = TOL32 if ifn.dtype == np.float32 else TOL64
    got = tonp(dm.render(wfe=True))
    sfe = tonp(dm.render(wfe=False))
    assert got.dtype == ifn.dtype
    # the fixture holds the renders on every step-th row and column (render(wfe=False) only where the obliquity is not 1)
    mask = np.ones(got.shape, bool)
    if dm.needs_rot and m.get('upsample', 1) == 1:
        win = _window(tuple(ifn.shape), dm.Nout)
        mask = _keep(ifn.shape, got.shape, dm.Mifwd, win[1] if win else (0, 0))
    st = m['render_step']
    ref = d[f'{name}_wfe']
    assert got[::st, ::st].shape == ref.shape
    assert _rel(got[::st, ::st], ref, mask[::st, ::st]) < tol
    ss = m['sfe_step']
    ref_sfe = d[f'{name}_sfe'] if f'{name}_sfe' in d else ref[::ss // st, ::ss // st] / 2
    assert _rel(sfe[::ss, ::ss], ref_sfe, mask[::ss, ::ss]) < tol
    assert tuple(dm.Nintermediate) == tuple(m['Nintermediate'])
    pg = np.random.default_rng(m['pg_seed']).standard_normal(got.shape).astype(got.dtype)
    adj = tonp(dm.render_adjoint(pg, wfe=True))
    aref = d[f'{name}_adj']
    assert adj.shape == aref.shape
    assert _rel(adj, aref) < tol


def _gauss(N, sigma, dtype=np.float64):
    y = np.arange(N) - N // 2
    return np.exp(-(y[:, None] ** 2 + y[None, :] ** 2) / (2 * sigma ** 2)).astype(dtype)


@pytest.mark.parametrize('N, nact', [(512, 50), (1024, 64)])
def test_single_poke_is_rolled_ifn(N, nact):
    from prysm_amd.x.dm import DM
    sep = N // nact - 2
    ifn = _gauss(N, 3.0)
    dm = DM(ifn, N, Nact=nact, sep=sep)
    y0, x0, sy, sx, ny, nx = dm.lattice
    for i, j in ((nact // 2, nact // 2), (3, nact - 5)):
        dm.actuators.zero_()
        dm.actuators[i, j] = 1
        got = tonp(dm.render())
        ref = 2 * dm.obliquity * np.roll(ifn, (y0 + i * sy, x0 + j * sx), axis=(0, 1))
        assert _rel(got, ref) < TOL64


@pytest.mark.parametrize('N, nact', [(512, 50), (1024, 64)])
def test_rot90_is_np_rot90(N, nact):
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(N)
    ifn = _gauss(N, 4.0)
    acts = rng.standard_normal((nact, nact))
    flat = DM(ifn, N, Nact=nact, sep=N // nact - 2)
    flat.update(acts)
    ref = np.rot90(tonp(flat.render()), -1)
    dm = DM(ifn, N, Nact=nact, sep=N // nact - 2, rot=(90, 0, 0))
    dm.update(acts)
    got = tonp(dm.render())
    mask = _keep(ifn.shape, ref.shape, dm.Mifwd)
    assert mask.sum() >= (N - 2) ** 2
    assert _rel(got, ref, mask) < TOL64


@pytest.mark.parametrize('shift', [(0, 0), (2.7, -1.2)])
@pytest.mark.parametrize('Nout', [256, 300, 200])
def test_dot_product_identity(shift, Nout):
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(Nout)
    dm = DM(_gauss(256, 3.0), Nout, Nact=24, sep=9, shift=shift)
    a = rng.standard_normal((24, 24))
    dm.update(a)
    r = tonp(dm.render())
    g = rng.standard_normal(r.shape)
    adj = tonp(dm.render_adjoint(g))
    lhs, rhs = float(np.vdot(r, g)), float(np.vdot(a, adj))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(r) * np.linalg.norm(g) * 1e-3)


@pytest.mark.parametrize('kw', [dict(), dict(rot=(5, 10, 0)), dict(Nout=600), dict(Nout=448), dict(upsample=0.64, Nout=512)])
def test_render_stack_equals_single_renders(kw):
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(8)
    kw = dict(dict(Nout=512), **kw)
    dm = DM(_gauss(512, 3.0), Nact=50, sep=8, **kw)
    acts = torch.from_numpy(rng.standard_normal((8, 50, 50))).to(dm.actuators.device)
    st = tonp(dm.render_stack(acts))
    assert float(dm.actuators.abs().max()) == 0.0
    for b in range(8):
        dm.update(acts[b])
        one = tonp(dm.render())
        assert st.shape[1:] == one.shape
        assert _rel(st[b], one) < TOL64
    # and the stacked adjoint
    g = rng.standard_normal(st.shape)
    ga = tonp(dm.render_adjoint(g))
    for b in (0, 7):
        assert _rel(ga[b], tonp(dm.render_adjoint(g[b]))) < TOL64


@pytest.mark.parametrize('kw', [dict(), dict(rot=(5, 10, 0))])
def test_captured_render_stack_is_bit_equal(kw):
    from prysm_amd import graph
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(3)
    dm = DM(_gauss(512, 3.0), 512, Nact=50, sep=8, **kw)
    dev = dm.actuators.device
    acts = torch.from_numpy(rng.standard_normal((4, 50, 50))).to(dev)
    model = graph.capture(lambda a: dm.render_stack(a), acts)
    new = torch.from_numpy(rng.standard_normal((4, 50, 50))).to(dev)
    replay = model(new).clone()
    eager = dm.render_stack(new)
    torch.cuda.synchronize()
    assert torch.equal(replay, eager)


def test_surface_feeds_focus_on_device():
    from prysm_amd import propagation as P
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(11)
    dm = DM(_gauss(256, 3.0), 256, Nact=24, sep=9, rot=(3, 0, 0))
    dm.update(rng.standard_normal((24, 24)) * 50)
    surf = dm.render()                       # a device tensor, nm
    assert surf.is_cuda
    amp = (rng.random((256, 256)) > 0.2).astype(np.float64)
    psf = tonp(P.Wavefront.from_amp_and_phase(amp, surf, 0.6328, 0.04).focus(100.0, Q=2).data)
    ref = O.focus(O.from_amp_and_phase(amp, tonp(surf), 0.6328), 2)
    assert _rel(psf, ref) < TOL64


@pytest.mark.parametrize('rot', [(0, 0, 0), (5, 10, 0)])
def test_float32_upsample_stays_float32(rot):
    """the Fourier resample works in config precision; the DM brings its result back to the influence function's precision (the
    adjoint's convolution reads its multiplier in the precision of its input)"""
    from prysm_amd.x.dm import DM
    rng = np.random.default_rng(5)
    acts = rng.standard_normal((24, 24))
    out = {}
    for dt in (np.float32, np.float64):
        dm = DM(_gauss(256, 3.0, dt), 256, Nact=24, sep=9, rot=rot, upsample=0.64)
        dm.update(acts)
        r = dm.render()
        g = dm.render_adjoint(np.random.default_rng(6).standard_normal(tuple(r.shape)))
        assert r.dtype == g.dtype == dm.ifn.dtype
        out[dt] = (tonp(r), tonp(g))
    for k in range(2):
        assert _rel(out[np.float32][k], out[np.float64][k]) < 2e-5
