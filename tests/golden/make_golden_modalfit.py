"""Writes tests/golden/modalfit.npz from the reference (prysm/polynomials/fitting.py and Interferogram.pvr, on numpy and scipy).
Run by hand, with the reference's directory given; the file holds data only -- coordinates, (n, m) indices, the measured maps and
the reference's outputs, not the bases:

    python tests/golden/make_golden_modalfit.py /path/to/prysm

Cases and bounds: tests/modalfit_common.py.  Keys:

  z37_r, _t, _nms, _data, _coef_f64, _coef_f32, _kappa, _nvalid      lstsq; _f32: the reference in float64 on float32-rounded inputs
  z11a_r, _t, _nms, _mask, _kappa, _Q_f64, _Q_f32 (the orthogonalised modes inside the mask, (K, count)), _ortho_f64, _ortho_f32 (the
        reference's own max|Q Q^T - I|), _rdiag (the raw diag(R) of its QR)
  z11a_norm_<to>_3d_<f>, z11a_norm_<to>_piston_<f>, z11a_norm_<to>_m4_<f>     normalize_modes of the stack, of piston (the loophole) and
        of mode 4 as 2-D inputs, on the rows NORM_ROWS; <f> = f32 is stored as float32
  hopkins_<i>      the three (a, b, c) of HOPKINS on the z37 grid with H = HOPKINS_H
  pvr_<name>_data, _f64, _f32      the map and the reference's pvr

Asserts what the cases rely on: kappa < 100, an invalid pixel inside the disc, a sign flip in the raw diag(R).  Prints the float64
numpy model's deviation from the reference for every compared value.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, sys.argv[1])

import modalfit_common as C  # noqa: E402
from prysm import polynomials as ref  # noqa: E402
from prysm.interferogram import Interferogram  # noqa: E402
from prysm_amd.polynomials import fit_plan as FP  # noqa: E402

warnings.simplefilter('ignore')
f32 = np.float32


def r32(a):
    return np.asarray(a).astype(f32).astype(np.float64)


def kappa(A, mask):
    return float(np.linalg.cond(A[:, mask].T))


def main():
    out = {}
    # ---- z37
    x, y, r, t = C.grid(C.Z37_SHAPE, diameter=2)
    nms = C.nms_of('z37')
    B = np.asarray(ref.zernike_nm_seq(nms, r, t, norm=False))
    data, _ = C.z37_data(B, r)
    ok = np.isfinite(data)
    assert np.any(~ok & (r <= 1)), 'no invalid pixel inside the disc'
    out.update(z37_r=r, z37_t=t, z37_nms=np.array(nms), z37_data=data, z37_kappa=kappa(B, ok), z37_nvalid=int(ok.sum()))
    assert out['z37_kappa'] < 100
    out['z37_coef_f64'] = ref.lstsq(B, data)
    out['z37_coef_f32'] = ref.lstsq(r32(B), r32(data))
    print(f"z37: kappa {out['z37_kappa']:.2f}, {out['z37_nvalid']} valid pixels")

    # ---- z11a
    x, y, r, t = C.grid(C.Z11A_SHAPE, diameter=2)
    nms = C.nms_of('z11a')
    A = np.asarray(ref.zernike_nm_seq(nms, r, t, norm=False))
    mask = C.annulus(r)
    out.update(z11a_r=r, z11a_t=t, z11a_nms=np.array(nms), z11a_mask=mask, z11a_kappa=kappa(A, mask))
    assert out['z11a_kappa'] < 100
    _, R = np.linalg.qr(A[:, mask].T)
    out['z11a_rdiag'] = np.diag(R)
    assert np.any(np.diag(R) < 0) and np.any(np.diag(R) > 0), 'no sign flip in diag(R): the sign convention is not tested'
    for f, conv in (('f64', np.asarray), ('f32', r32)):
        Q = ref.orthogonalize_modes(conv(A), mask)
        assert not Q[:, ~mask].any()
        out[f'z11a_Q_{f}'] = Q[:, mask].astype(f32 if f == 'f32' else np.float64)
        out[f'z11a_ortho_{f}'] = C.orthogonality(Q, mask)
        for to in ('std', 'ptp'):
            keep = (lambda a: a.astype(f32)) if f == 'f32' else (lambda a: a)
            out[f'z11a_norm_{to}_3d_{f}'] = keep(ref.normalize_modes(conv(A), mask, to=to)[:, C.NORM_ROWS])
            out[f'z11a_norm_{to}_piston_{f}'] = keep(ref.normalize_modes(conv(A[0]), mask, to=to)[C.NORM_ROWS])
            out[f'z11a_norm_{to}_m4_{f}'] = keep(ref.normalize_modes(conv(A[4]), mask, to=to)[C.NORM_ROWS])
    print(f"z11a: kappa {out['z11a_kappa']:.2f}, {int(mask.sum())} points, reference orthogonality {out['z11a_ortho_f64'] / C.eps(np.float64):.1f} eps64")

    # ---- hopkins
    H = C.HOPKINS_H
    for i, (a, b, c) in enumerate(C.HOPKINS):
        out[f'hopkins_{i}'] = ref.hopkins(a, b, c, out['z37_r'], out['z37_t'], H)

    # ---- pvr
    for name, (shape, dx, radius, _) in C.PVR_CASES.items():
        z = C.pvr_map(name)
        out[f'pvr_{name}_data'] = z
        out[f'pvr_{name}_f64'] = Interferogram(z.copy(), dx=dx).pvr(radius)
        out[f'pvr_{name}_f32'] = Interferogram(r32(z), dx=dx).pvr(radius)
        print(f"pvr {name}: {out[f'pvr_{name}_f64']:.6f}")
    try:
        Interferogram(C.pvr_map('rect'), dx=0.25).pvr()
        raise AssertionError('the reference accepted a non-square map without a radius')
    except ValueError:
        pass

    np.savez_compressed(C.GOLDEN, **out)
    C._golden = None
    print(f'wrote {C.GOLDEN}: {os.path.getsize(C.GOLDEN)} bytes')

    # ---- the float64 model against what was just written
    G = C.golden()
    Bm = C.basis('z37')
    print('model basis vs reference basis (eps64):', C.deviation(Bm, B, np.float64))
    print('model lstsq vs reference (eps64 max|c|):', C.deviation(FP.lstsq(Bm, G['z37_data']), G['z37_coef_f64'], np.float64))
    print('model lstsq f32 vs reference (eps32 max|c|):', C.deviation(FP.lstsq(Bm.astype(f32), G['z37_data'].astype(f32)), G['z37_coef_f32'], f32))
    Am = C.basis('z11a')
    Qm = FP.orthogonalize_modes(Am, mask)
    print('model Q vs reference (eps64 max|Q|):', C.deviation(Qm[:, mask], G['z11a_Q_f64'], np.float64),
          ' orthogonality (eps64):', C.orthogonality(Qm, mask) / C.eps(np.float64))
    for to in ('std', 'ptp'):
        print(f'model normalize {to} vs reference (eps64):', C.deviation(FP.normalize_modes(Am, mask, to)[:, C.NORM_ROWS], G[f'z11a_norm_{to}_3d_f64'], np.float64))


if __name__ == '__main__':
    main()
