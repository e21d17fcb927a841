"""Generate the coatings fixture (tests/golden/coatings.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists), on the CPU:

    python tests/golden/make_golden_coatings.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores data only.  Materials 1.38, 2.1588, 1.6290 + 0.0034836j, 1.46.  Cases:
- `c1_L1`, `c1_L5`, `c1_L40`: layers cycling the materials, seeded thicknesses in 0.05 .. 0.25 um, ambient 1, substrate 1.458461,
  wavelengths 0.45 .. 0.75 um (67) x angles 0, 23, 60 degrees;
- `c2_tir`: indices 1.38, 2.3, thicknesses 0.1, 0.07 um, ambient 1.5, substrate 1.0, 0.55 um, angles 0, 30, 41, 42, 60 degrees
  (|r| = 1 beyond the critical angle, 41.81 degrees);
- `c3_map`: the reference's own 3 x 4, 5-layer per-sample case of tests/test_thinfilm.py, 23 degrees.
Per case the operands `<case>_n`, `_d`, `_wvl`, `_aoi` (degrees), `_nsub`, `_n0`, the seeds `_dR`, `_dT` (seeded normal), and per
polarisation `<case>_<s|p>_`: `r`, `t` (stack_rt), `r_tf`, `t_tf` (multilayer_stack_rt), `R`, `T`, `A` (RTA), `E`, `H`
(internal_fields), `grad_RT`, `grad_R`, `grad_T` (thickness_gradient with both seeds, dR alone, dT alone).
The refinement trajectory: 6 layers cycling the materials from d0 = 0.09, 0.06, 0.11, 0.08, 0.05, 0.10, the term
Reflectance(wavelengths x (0, 23, 45) degrees, 'avg', target 0, weight 1), the reference's Adam with alpha 0.002, 20 steps:
`traj_x` (21, 6) and `traj_f` (21,), row 0 the start and row k the iterate after step k with the merit there.

The numpy model (prysm_amd/thinfilm_plan.py) is run on every case: its float64 deviations are asserted against
tests/coatings_common.py's bound and its complex64 deviations printed, for the table of tolerances there.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from prysm import thinfilm as RT  # noqa: E402
from prysm.x.coatings import diff as RD  # noqa: E402
from prysm.x.coatings import merit as RM  # noqa: E402
from prysm.x.coatings import stack as RS  # noqa: E402
from prysm.x.optym import optimizers as ROPT  # noqa: E402

import coatings_common as CC  # noqa: E402


def case_operands(rng):
    wv = np.linspace(0.45, 0.75, 67)
    cases = {}
    for L in (1, 5, 40):
        cases[f'c1_L{L}'] = dict(n=np.array([CC.MATERIALS[i % 4] for i in range(L)]), d=rng.uniform(0.05, 0.25, L), wvl=wv.reshape(1, 67),
                                 aoi=np.array([0.0, 23.0, 60.0]).reshape(3, 1), nsub=np.float64(1.458461), n0=np.float64(1.0))
    cases['c2_tir'] = dict(n=np.array([1.38, 2.3]), d=np.array([0.1, 0.07]), wvl=np.float64(0.55), aoi=np.array([0.0, 30.0, 41.0, 42.0, 60.0]),
                           nsub=np.float64(1.0), n0=np.float64(1.5))
    wvl = .587725
    x = np.linspace(0, 1, 12).reshape(3, 4)
    n = np.array([1.35 + 0.12 * layer + 0.01j * layer + 1e-3 * x for layer in range(5)])
    d = np.array([wvl / (4 + layer) * (1 + 0.05 * x) for layer in range(5)])
    cases['c3_map'] = dict(n=n, d=d, wvl=np.float64(wvl), aoi=np.float64(23.0), nsub=1.458461 + 0.02 * x, n0=np.float64(1.0))
    return cases


def reference_case(op, dR, dT):
    out = {}
    n, d = op['n'], op['d']
    theta = np.radians(op['aoi'])
    scalar = lambda v: v.item() if np.ndim(v) == 0 else v  # noqa: E731
    stack = RS.Stack(list(n), d, scalar(op['nsub']), scalar(op['n0']))
    shape = np.broadcast(op['wvl'], op['aoi'], op['nsub'], n[0], d[0]).shape
    for pol in CC.POLS:
        r, t = RS.stack_rt(stack, op['wvl'], theta, pol)
        R, T, A = RS.RTA(stack, op['wvl'], theta, pol)
        E, H = RS.internal_fields(stack, op['wvl'], theta, pol)
        if n.ndim == 1 and len(shape):      # scalar layers over a grid: the grid rides on wavelength and aoi
            rtf, ttf = RT.multilayer_stack_rt(n, d, op['wvl'], pol, scalar(op['nsub']), aoi=op['aoi'], ambient_index=scalar(op['n0']))
        else:
            rtf, ttf = RT.multilayer_stack_rt(n, d, op['wvl'], pol, scalar(op['nsub']), aoi=scalar(op['aoi']), ambient_index=scalar(op['n0']))
        fwd = RD.forward_eval(stack, op['wvl'], theta, pol)
        full = lambda a, lead=(): np.broadcast_to(a, lead + shape).astype(a.dtype)  # noqa: E731
        L = len(d)
        out.update({f'{pol}_r': full(r + 0j), f'{pol}_t': full(t + 0j), f'{pol}_r_tf': full(rtf + 0j), f'{pol}_t_tf': full(ttf + 0j),
                    f'{pol}_R': full(R), f'{pol}_T': full(T), f'{pol}_A': full(A, (L,)), f'{pol}_E': full(E + 0j, (L + 1,)),
                    f'{pol}_H': full(H + 0j, (L + 1,)),
                    f'{pol}_grad_RT': RD.thickness_gradient(fwd, dR=dR, dT=dT), f'{pol}_grad_R': RD.thickness_gradient(fwd, dR=dR),
                    f'{pol}_grad_T': RD.thickness_gradient(fwd, dT=dT)})
    return out, shape


def main():
    rng = np.random.default_rng(20261019)
    out = {'materials': np.array(CC.MATERIALS)}
    cases = case_operands(rng)
    for name, op in cases.items():
        shape = np.broadcast(op['wvl'], op['aoi'], op['nsub'], op['n'][0], op['d'][0]).shape
        dR, dT = rng.standard_normal(shape), rng.standard_normal(shape)
        res, _ = reference_case(op, dR, dT)
        for k, v in op.items():
            out[f'{name}_{k}'] = np.asarray(v)
        out[f'{name}_dR'], out[f'{name}_dT'] = dR, dT
        for k, v in res.items():
            out[f'{name}_{k}'] = np.asarray(v)
    # ---- the refinement trajectory
    n6, W, A, nsub = CC.traj_operands({'c1_L1_wvl': cases['c1_L1']['wvl']})
    term = RM.Reflectance(W, A, 'avg', 0.0, 1.0)

    def fg(x):
        return term.value_and_grad(RS.Stack(list(n6), x, nsub))

    opt = ROPT.Adam(fg, np.array(CC.TRAJ_D0), CC.TRAJ_ALPHA)
    xs, fs = [np.array(CC.TRAJ_D0)], [fg(np.array(CC.TRAJ_D0))[0]]
    for _ in range(CC.TRAJ_STEPS):
        opt.step()
        xs.append(np.asarray(opt.x, dtype=np.float64).copy())
        fs.append(fg(opt.x)[0])
    out['traj_x'], out['traj_f'] = np.array(xs), np.array(fs)
    print('trajectory: f %.5g -> %.5g' % (fs[0], fs[-1]))
    path = os.path.join(HERE, 'coatings.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, 'bytes,', len(out), 'arrays')
    assert size < 1 << 20, size
    # ---- the model on every case
    CC.golden.cache_clear()
    g = CC.golden()
    table = {}
    for name in CC.CASES:
        table[name] = {}
        for dt in (np.complex128, np.complex64):
            for quantity in CC.QUANTITIES + CC.GRADS:
                dev = 0.0
                for pol in CC.POLS:
                    got = CC.model_grad(name, pol, quantity[5:], dt, g) if quantity in CC.GRADS else CC.model(name, pol, dt, g)[quantity]
                    dev = max(dev, CC.deviation(got, name, pol, quantity, g))
                if dt == np.complex128:
                    assert dev <= CC.F64_TOL, (name, quantity, dev)
                    print(f'{name:7s} {quantity:8s} float64 {dev:.2e}')
                else:
                    table[name][quantity] = dev
        for pol in CC.POLS:      # multilayer_stack_rt's r is stack_rt's
            assert np.max(np.abs(g[f'{name}_{pol}_r_tf'] - g[f'{name}_{pol}_r'])) <= 1e-13 * np.max(np.abs(g[f'{name}_{pol}_r'])), name
    print('C64_DEV = {')
    for name, row in table.items():
        print(f"    '{name}': {{" + ', '.join(f"'{k}': {v:.1e}" for k, v in row.items()) + '},')
    print('}')
    xs = CC.adam_numpy(lambda x: CC.model_fg(x, g=g), CC.TRAJ_D0, CC.TRAJ_ALPHA, CC.TRAJ_STEPS)
    fm = np.array([CC.model_fg(x, g=g)[0] for x in xs])
    dx = np.max(np.abs(xs - g['traj_x']) / np.abs(g['traj_x']))
    df = np.max(np.abs(fm - g['traj_f']) / np.abs(g['traj_f']))
    print(f'trajectory: model float64 deviation x {dx:.2e} f {df:.2e}')
    assert max(dx, df) <= CC.TRAJ_TOL


if __name__ == '__main__':
    main()
