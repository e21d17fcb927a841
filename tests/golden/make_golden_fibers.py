"""Writes tests/golden/fibers.npz from the reference (prysm/x/fibers.py, which runs on scipy).  Run by hand, with the reference's
directory given; the file holds data only:

    python tests/golden/make_golden_fibers.py /path/to/prysm

  roots_<V>_{l,n,b,U,df}   find_all_modes(V) for V in fibers_common.VS: the families l >= 0, their counts, b (descending per family),
                           U = V sqrt(1 - b) and the reference's df/dU at U
  jl_l, jl_x, jl_ref, jl_err   J_l(x) from scipy for l in TAB_L (flat), and |scipy - 40-digit value|
  ke_l, ke_x, ke_ref, ke_err   e^x K_l(x) likewise
  <case>_{keys,counts,b}   the mode dictionary of a case (fibers_common.CASES)
  <case>_<grid>_idx        flat indices of the points stored: every point where modes x points <= 20000, else every 4th plus the
                           points with r = 0 and r == a -- the whole stacks would be 2.4 MB
  <case>_<grid>_stack      compute_LP_modes on the float64 grid there, (nmodes, len(idx)) float64
  <case>_<grid>_delta32    (the same on the grid rounded to float32, evaluated in float64) - stack, float32
  <case>_<grid>_eta{64,32} multimode_coupling of fibers_common.incident, flat in mode order
  smf_<grid>_{field,delta32}, smf_b   smf_mode_field for V = 2
  overlap_<grid>_{64,32}   mode_overlap_integral(incident, second_field)
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1])

import fibers_common as FC  # noqa: E402
from prysm.x import fibers as R  # noqa: E402
from scipy import special  # noqa: E402

mp.mp.dps = 40


def flat(d):
    return [m for ms in d.values() for m in ms]


def tab_points(l):
    xj = sorted({0.0, 1e-3, 0.5, 1.0, 2.0, 3.0, 5.0, 7.5, 8.0, 8.5, 12.0, 20.0, 33.3, 47.1, 60.0, max(l - 0.5, 0.25), float(l), l + 0.5,
                 0.5 * l + 0.1, 0.1 * l + 0.01, 2.0 * l + 1})
    xk = sorted({1e-3, 1e-2, 0.1, 0.5, 0.99, 1.0, 1.01, 1.5, 1.97, 2.0, 2.5, 4.0, 9.0, 30.0, 100.0, 700.0})
    return np.array(xj), np.array(xk)


def main():
    out = {}
    for V in FC.VS:
        modes = R.find_all_modes(V)
        ls = [l for l in modes if l >= 0]
        b = np.concatenate([modes[l] for l in ls])
        U = V * np.sqrt(1 - b)
        df = np.concatenate([R._ghatak_u_with_derivative(V * np.sqrt(1 - modes[l]), V, l)[1] for l in ls])
        tag = 'roots_' + FC.vtag(V)
        out[tag + '_l'], out[tag + '_n'] = np.array(ls, np.int32), np.array([len(modes[l]) for l in ls], np.int32)
        out[tag + '_b'], out[tag + '_U'], out[tag + '_df'] = b, U, df
        assert sum(len(v) for v in modes.values()) == FC.COUNTS[FC.VS.index(V)]
    jl, jx, jr, je, kl, kx, kr, ke = [], [], [], [], [], [], [], []
    for l in FC.TAB_L:
        xj, xk = tab_points(l)
        for must in (0, 1e-3, max(l - 0.5, 0.25), l, l + 0.5, 60):
            assert must in xj, (l, must)
        vj, vk = special.jv(l, xj), special.kve(l, xk)
        jl.append(np.full(len(xj), l, np.int32)), jx.append(xj), jr.append(vj)
        je.append([abs(float(mp.besselj(l, mp.mpf(float(x))) - mp.mpf(float(v)))) for x, v in zip(xj, vj)])
        kl.append(np.full(len(xk), l, np.int32)), kx.append(xk), kr.append(vk)
        ke.append([abs(float(mp.besselk(l, mp.mpf(float(x))) * mp.exp(mp.mpf(float(x))) - mp.mpf(float(v)))) for x, v in zip(xk, vk)])
    for name, parts in (('jl_l', jl), ('jl_x', jx), ('jl_ref', jr), ('jl_err', je), ('ke_l', kl), ('ke_x', kx), ('ke_ref', kr), ('ke_err', ke)):
        out[name] = np.concatenate([np.asarray(p) for p in parts])

    for case, (V, keep) in FC.CASES.items():
        modes = R.find_all_modes(V)
        if keep is not None:
            modes = {l: modes[l] for l in modes if l in keep}
        out[case + '_keys'] = np.array(list(modes), np.int32)
        out[case + '_counts'] = np.array([len(v) for v in modes.values()], np.int32)
        out[case + '_b'] = np.concatenate(list(modes.values()))
        nmodes = int(out[case + '_counts'].sum())
        for gname in FC.GRIDS:
            r, t = FC.grid(gname)
            r32, t32 = (a.astype(np.float64) for a in FC.grid(gname, np.float32))
            npts = r.size
            if nmodes * npts <= 20000:
                idx = np.arange(npts)
            else:
                idx = np.union1d(np.arange(0, npts, 4), np.flatnonzero((r.ravel() == 0) | (r.ravel() == FC.A)))
            full64 = np.array(flat(R.compute_LP_modes(V, modes, FC.A, r, t))).reshape(nmodes, -1)
            full32 = np.array(flat(R.compute_LP_modes(V, modes, FC.A, r32, t32))).reshape(nmodes, -1)
            key = f'{case}_{gname}_'
            out[key + 'idx'] = idx.astype(np.int32)
            out[key + 'stack'] = full64[:, idx]
            out[key + 'delta32'] = (full32 - full64)[:, idx].astype(np.float32)
            for sfx, full, dt in (('64', full64, np.float64), ('32', full32, np.float32)):
                E = FC.incident(gname, dt).astype(np.complex128)
                fields = {0: [m.reshape(r.shape) for m in full]}
                out[key + 'eta' + sfx] = np.array(R.multimode_coupling(E, fields)[0])

    b = R.find_all_modes(FC.SMF_V)[0][0]
    out['smf_b'] = np.float64(b)
    for gname in FC.GRIDS:
        r, _ = FC.grid(gname)
        r32 = FC.grid(gname, np.float32)[0].astype(np.float64)
        f64, f32 = R.smf_mode_field(FC.SMF_V, FC.A, b, r), R.smf_mode_field(FC.SMF_V, FC.A, b, r32)
        out[f'smf_{gname}_field'], out[f'smf_{gname}_delta32'] = f64, (f32 - f64).astype(np.float32)
        for sfx, dt in (('64', np.float64), ('32', np.float32)):
            E1, E2 = FC.incident(gname, dt).astype(np.complex128), FC.second_field(gname, dt).astype(np.complex128)
            out[f'overlap_{gname}_{sfx}'] = np.float64(R.mode_overlap_integral(E1, E2))
    np.savez_compressed(FC.GOLDEN, **out)
    print(FC.GOLDEN, os.path.getsize(FC.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
