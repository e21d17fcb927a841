"""Generate the deformable-mirror fixture (tests/golden/dm.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists):

    python tests/golden/make_golden_dm.py

Imports brandondube/prysm from PRYSM_REFERENCE, builds prysm.x.dm.DM for each case below on small seeded inputs and stores the
inputs, the lattice geometry, render(wfe=True) (and render(wfe=False) where the obliquity is not 1 -- elsewhere it is exactly
half of it), and render_adjoint(wfe=True) of a protograd drawn from np.random.default_rng(seed).standard_normal(Nout) (the test
draws the same one).  Rotated cases also store the projection coordinates.

Kept small (well under a megabyte): the influence functions are Gaussians cut to 0 below 1e-20 (stored once per shape, they
compress to almost nothing); render(wfe=True) is stored whole for `plain` and `rot3` and on every RENDER_STEP-th row and column
elsewhere, render(wfe=False) always on every RENDER_STEP-th (an off-by-one window or lattice still shows there); the projection
coordinates on every PROJ_STEP-th row and column, as float32 (the tests check the homographies with them and compute the fp64
coordinates themselves).
"""
import json
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm.x.dm import DM  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


RENDER_STEP = 2
PROJ_STEP = 4
FULL = ('plain', 'rot3')


def gaussian_ifn(shape, sigma):
    y, x = [np.arange(n) - n // 2 for n in shape]
    g = np.exp(-(y[:, None] ** 2 + x[None, :] ** 2) / (2 * sigma ** 2))
    g[g < 1e-20] = 0
    return g


# name: (ifn shape, ifn dtype, sigma, kwargs of DM)
CASES = {
    'plain': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6)),
    'shift': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, shift=(3.3, -2))),
    'clock': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, rot=(10, 0, 0))),
    'tilt': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, rot=(0, 20, 0))),
    'rot3': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, rot=(5, 10, 15))),
    'up064': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, upsample=0.64)),
    'up125': ((128, 128), 'f8', 3.0, dict(Nout=128, Nact=16, sep=6, upsample=1.25)),
    'small': ((128, 128), 'f8', 3.0, dict(Nout=100, Nact=14, sep=6)),
    'large': ((128, 128), 'f8', 3.0, dict(Nout=160, Nact=16, sep=6)),
    'odd': ((96, 120), 'f8', 2.5, dict(Nout=(96, 120), Nact=(13, 9), sep=(7, 8), shift=(1.5, 0.5))),
    'f32': ((128, 128), 'f4', 3.0, dict(Nout=128, Nact=16, sep=6)),
}


def main():
    out = {}
    meta = {}
    for k, (name, (shape, dt, sigma, kw)) in enumerate(CASES.items()):
        rng = np.random.default_rng(1000 + k)
        ifn_key = f'{shape[0]}x{shape[1]}_s{sigma}'
        if f'ifn_{ifn_key}' not in out:
            out[f'ifn_{ifn_key}'] = gaussian_ifn(shape, sigma)
        ifn = out[f'ifn_{ifn_key}'].astype(dt)
        dm = DM(ifn, **kw)
        acts = rng.standard_normal(dm.actuators.shape).astype(dt)
        dm.actuators[:] = acts
        sfe = dm.render(wfe=False)
        wfe = dm.render(wfe=True)
        pg = np.random.default_rng(2000 + k).standard_normal(wfe.shape).astype(wfe.dtype)
        adj = dm.render_adjoint(pg.copy(), wfe=True)
        iyy, ixx = dm.iyy, dm.ixx
        step = 1 if name in FULL else RENDER_STEP
        meta[name] = dict(kw, shape=list(shape), dtype=dt, sigma=sigma, ifn=ifn_key, pg_seed=2000 + k, render_step=step, sfe_step=RENDER_STEP,
                          proj_step=PROJ_STEP,
                          obliquity=dm.obliquity, Nintermediate=list(dm.Nintermediate),
                          lattice=[iyy.start, ixx.start, iyy.step, ixx.step, *dm.actuators.shape])
        out[f'{name}_acts'] = acts
        out[f'{name}_wfe'] = wfe[::step, ::step]
        out[f'{name}_adj'] = adj
        if dm.obliquity != 1.0:
            out[f'{name}_sfe'] = sfe[::RENDER_STEP, ::RENDER_STEP]
        else:
            assert np.array_equal(sfe * 2, wfe)
        if dm.needs_rot:
            for a in ('projx', 'projy', 'invprojx', 'invprojy'):
                out[f'{name}_{a}'] = getattr(dm, a)[::PROJ_STEP, ::PROJ_STEP].astype(np.float32)
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'dm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
