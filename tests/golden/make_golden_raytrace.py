"""Generate the ray-trace fixture (tests/golden/raytrace.npz) from the REFERENCE itself.

Run where the reference exists, on the CPU, with PRYSM_REFERENCE naming its checkout:

    PRYSM_REFERENCE=/path/to/prysm python tests/golden/make_golden_raytrace.py

Imports brandondube/prysm and stores data only.  The reference's prysm/x/raytracing/__init__.py wants a `_first_order` module its
tree does not hold, so an empty stand-in package with that directory as its __path__ is registered and surfaces, spencer_and_murty,
raygen, intersections and analysis are imported from it as submodules.  Indices are prysm.x.materials.core.ConstantMaterial.

The cases are tests/raytrace_common.py CASES (float64, wavelength 0.55 um, lengths in mm), and what is stored is listed in that
module's docstring.  The numpy model (prysm_amd/x/raytrace_plan.py) is run on every case in float64 and in float32: its float64
statuses are asserted equal to the reference's on every ray, its float64 deviations asserted within 1e-9, the rays its float32
walk decides differently stored as `<case>_edge32` and asserted to be at most 1 % of the case, and the tables F64_DEV, F32_DEV,
EDGE32_SHARE and RESCUE of tests/raytrace_common.py printed.
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE')
if not REF:
    sys.exit('set PRYSM_REFERENCE to a checkout of the reference')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import prysm.x  # noqa: E402, F401
from prysm.x.materials.core import ConstantMaterial  # noqa: E402

_pkg = types.ModuleType('prysm.x.raytracing')
_pkg.__path__ = [os.path.join(REF, 'prysm', 'x', 'raytracing')]
sys.modules['prysm.x.raytracing'] = _pkg
# analysis imports paraxial, which imports the two names of the missing module; nothing stored here calls them
_first_order = types.ModuleType('prysm.x.raytracing._first_order')
_first_order.format_first_order = _first_order.initialize_slots = None
sys.modules['prysm.x.raytracing._first_order'] = _first_order
RSM = importlib.import_module('prysm.x.raytracing.spencer_and_murty')
RI = importlib.import_module('prysm.x.raytracing.intersections')
RSF = importlib.import_module('prysm.x.raytracing.surfaces')
RG = importlib.import_module('prysm.x.raytracing.raygen')
RA = importlib.import_module('prysm.x.raytracing.analysis')

import raytrace_common as RC  # noqa: E402
from prysm_amd.x import raytrace_plan as plan  # noqa: E402
from prysm_amd.x.raytracing import surfaces as SF  # noqa: E402


def main():
    out = {}
    f64_dev, f32_dev, edge_share, rescue = {}, {}, {}, {}
    warnings.simplefilter('ignore')
    for case, spec in RC.CASES.items():
        surfs = RC.build(case, RSF, material=ConstantMaterial)
        P0, S0 = RC.launch(case, RG)
        P0, S0 = np.array(P0, dtype=np.float64), np.array(S0, dtype=np.float64)
        out[f'gen_{case}_P'], out[f'gen_{case}_S'] = P0, S0
        if 'extra' in spec:
            P0, S0 = np.vstack([P0, np.array(spec['extra'][0])]), np.vstack([S0, np.array(spec['extra'][1])])
        with np.errstate(all='ignore'):
            res = RSM.raytrace(surfs, P0, S0, RC.WVL)
        J, N = len(surfs), P0.shape[0]
        surface, code = res.status.real.astype(np.int32), res.status.imag.astype(np.int32)
        out[case + '_P0'], out[case + '_S0'] = P0, S0
        out[case + '_P'], out[case + '_S'], out[case + '_OPL'] = res.P, res.S, res.OPL
        out[case + '_surface'], out[case + '_code'] = surface, code
        out[case + '_pose_P'] = np.array([s.P for s in surfs])
        out[case + '_pose_R'] = np.array([np.eye(3) if s.R is None else s.R for s in surfs])
        bands = np.full((J, 4), np.nan)
        for j, s in enumerate(surfs):
            b = s.departure_band()
            if b.bounded:
                bands[j] = b.max_departure, b.domain_radius, b.gradient_bound, b.lipschitz
        out[case + '_band'] = bands
        counts = {RSM.decode_status(complex(a, b)): int(np.sum((surface == a) & (code == b))) for a, b in sorted(set(zip(surface.tolist(), code.tolist())))}
        print(case, N, 'rays', counts)

        # the model, float64: statuses equal, deviations within 1e-9
        mine = RC.build(case, SF)
        tab, n0 = plan.pack_table(mine, RC.WVL), plan.launch_index(mine, RC.WVL)
        stats = {}
        m64 = plan.trace(tab, n0, plan.resolve_tol_sag(None, np.float64), P0, S0, stats=stats)
        assert np.array_equal(m64[3], surface) and np.array_equal(m64[4], code), (case, np.flatnonzero(m64[4] != code))
        rescue[case] = (stats.get('rescued', 0), stats.get('rescue_converged', 0))
        keep = np.ones(N, dtype=bool)
        f64_dev[case] = {}
        for q, got in zip(RC.QUANTITIES, m64[:3]):
            dev, same_nan = RC.deviations(got, out[f'{case}_{q}'], keep)
            assert same_nan and dev <= 1e-9, (case, q, dev)
            f64_dev[case][q] = dev
        # float32: the rays it decides differently, the deviations of the others
        m32 = plan.trace(tab, n0, plan.resolve_tol_sag(None, np.float32), P0.astype(np.float32), S0.astype(np.float32))
        edge = np.flatnonzero((m32[3] != surface) | (m32[4] != code))
        out[case + '_edge32'] = edge.astype(np.int64)
        edge_share[case] = edge.size / N
        assert edge.size <= 0.01 * N, (case, edge.size, N)
        keep[edge] = False
        f32_dev[case] = {}
        for q, got in zip(RC.QUANTITIES, m32[:3]):
            dev, same_nan = RC.deviations(got, out[f'{case}_{q}'], keep)
            assert same_nan, (case, q)
            f32_dev[case][q] = dev
        if case == 'A':
            x, y = RA.spot_positions(res.P[-1], res.status, origin='centroid')
            pupil, delta = RA.transverse_ray_aberration(res.P, axis='y', status=res.status, reference='centroid')
            out['A_spot_x'], out['A_spot_y'], out['A_tra_pupil'], out['A_tra_delta'] = x, y, pupil, delta

    def table(name, d, fmt):
        print(name + ' = {')
        for case, v in d.items():
            print(f"    '{case}': " + fmt(v) + ',')
        print('}')
    table('F64_DEV', f64_dev, lambda v: '{' + ', '.join(f"'{q}': {x:.1e}" for q, x in v.items()) + '}')
    table('F32_DEV', f32_dev, lambda v: '{' + ', '.join(f"'{q}': {x:.1e}" for q, x in v.items()) + '}')
    table('EDGE32_SHARE', edge_share, lambda v: f'{v:.4f}')
    table('RESCUE', rescue, repr)
    np.savez_compressed(RC.PATH, **out)
    print('wrote', RC.PATH, os.path.getsize(RC.PATH), 'bytes')


if __name__ == '__main__':
    main()
