"""Time prysm_amd.segmented on the device with HIP events after warm-up, on the JWST-like layout (rings 2, centre excluded, aperture
6.628 across the grid, segment_diameter 1.32, segment_separation 0.007):

- compose_opd and compose_opd_adjoint on the matrix-free route (zernike_nm_seq: the table walk per point) and on the stored route
  (the same Zernike bases through a lambda, kept on the device);
- the reference's algorithm run on the device with existing ops: per segment sum_of_2d_modes over the stored (K, h, w) basis, the
  mask multiply and the window add; for the adjoint, sum_of_2d_modes_adjoint per segment of mask * g[window];
- a full-grid zernike_sum / zernike_sum_adjoint of the same K, as a yardstick.

    python tools/exp_segmented.py [--reps 20] [--quick]

One JSON line per configuration (N in 1024, 2048; float32, float64; K in 3, 12, 36 (Noll 1..K); B in 1, 8), times in microseconds.
--quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run, where the launch sequence is wanted).
--launches makes one compose_opd and one compose_opd_adjoint call per precision at 2048^2, K = 12, B = 1, and nothing else on the
device but the uploads: under rocprofv3 --kernel-trace --stats it shows how many launches each call is.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd import polynomials as P  # noqa: E402
from prysm_amd import segmented as SG  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def launches():
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        g1 = ((np.arange(2048) - 1024) * (6.628 / 2048)).astype(dt)
        x, y = np.meshgrid(g1, g1)
        ap = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
        ap.prepare_opd_bases(P.zernike_nm_seq, [P.noll_to_nm(j) for j in range(1, 13)])
        c = torch.from_numpy(rng.standard_normal((len(ap.windows), 12)).astype(dt)).cuda()
        g = torch.from_numpy(rng.standard_normal(x.shape).astype(dt)).cuda()
        ap.compose_opd(c)
        ap.compose_opd_adjoint(g)
        torch.cuda.synchronize()
        print(np.dtype(dt).name, 'one compose_opd and one compose_opd_adjoint', flush=True)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument('--reps', type=int, default=20)
    ap_.add_argument('--warmup', type=int, default=3)
    ap_.add_argument('--quick', action='store_true')
    ap_.add_argument('--launches', action='store_true')
    a = ap_.parse_args()
    if a.launches:
        return launches()
    if a.quick:
        a.reps, a.warmup = 2, 1
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for N in (1024, 2048):
        for dt in (np.float32, np.float64):
            tdt = torch.float32 if dt == np.float32 else torch.float64
            g1 = ((np.arange(N) - N // 2) * (6.628 / N)).astype(dt)
            x, y = np.meshgrid(g1, g1)
            mf = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
            st = SG.CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
            S = len(mf.windows)
            masks = mf.local_masks
            xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            xn, yn = xd / (mf.vtov / 2), yd / (mf.vtov / 2)
            for K in (3, 12, 36):
                nms = [P.noll_to_nm(j) for j in range(1, K + 1)]
                mf.prepare_opd_bases(P.zernike_nm_seq, nms)
                st.prepare_opd_bases(lambda orders, r, t: P.zernike_nm_seq(orders, r, t), nms)
                bases = st.opd_bases
                c1 = torch.from_numpy(rng.standard_normal((S, K))).to('cuda', tdt)
                c8 = torch.from_numpy(rng.standard_normal((8, S, K))).to('cuda', tdt)
                w1, w8 = c1.cpu().numpy(), c8.cpu().numpy()
                z1 = torch.from_numpy(rng.standard_normal(K)).to('cuda', tdt)
                z8 = torch.from_numpy(rng.standard_normal((8, K))).to('cuda', tdt)
                gg1 = torch.from_numpy(rng.standard_normal((N, N))).to('cuda', tdt)
                gg8 = torch.from_numpy(rng.standard_normal((8, N, N))).to('cuda', tdt)

                def loop_compose(w):
                    out = torch.zeros((N, N), dtype=tdt, device='cuda')
                    for win, m, b, c in zip(mf.windows, masks, bases, w):
                        tile = P.sum_of_2d_modes(b, c)
                        tile *= m
                        out[win] += tile
                    return out

                def loop_adjoint(g):
                    return torch.stack([P.sum_of_2d_modes_adjoint(b, m * g[win]) for win, m, b in zip(mf.windows, masks, bases)])

                fns = dict(
                    compose1=lambda: mf.compose_opd(c1),
                    compose8=lambda: mf.compose_opd(c8),
                    stored_compose1=lambda: st.compose_opd(c1),
                    stored_compose8=lambda: st.compose_opd(c8),
                    loop_compose1=lambda: loop_compose(w1),
                    loop_compose8=lambda: [loop_compose(w) for w in w8],
                    zsum1=lambda: P.zernike_sum(z1, nms, xn, yn),
                    zsum8=lambda: P.zernike_sum(z8, nms, xn, yn),
                    adjoint1=lambda: mf.compose_opd_adjoint(gg1),
                    adjoint8=lambda: mf.compose_opd_adjoint(gg8),
                    stored_adjoint1=lambda: st.compose_opd_adjoint(gg1),
                    stored_adjoint8=lambda: st.compose_opd_adjoint(gg8),
                    loop_adjoint1=lambda: loop_adjoint(gg1),
                    loop_adjoint8=lambda: [loop_adjoint(gg8[b]) for b in range(8)],
                    zadj1=lambda: P.zernike_sum_adjoint(gg1, nms, xn, yn),
                    zadj8=lambda: P.zernike_sum_adjoint(gg8, nms, xn, yn),
                )
                for fn in fns.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                us = {k: timed(fn, max(1, a.reps // 4) if k.startswith('loop') and k.endswith('8') else a.reps) for k, fn in fns.items()}
                rec = dict(N=N, dtype=np.dtype(dt).name, K=K, S=S, P=int(mf.segment_plan.cover.shape[0]),
                           plan_bytes=int(mf.segment_plan.nbytes), us={k: round(v, 1) for k, v in us.items()})
                for b in ('1', '8'):
                    rec[f'compose{b}_vs_loop'] = round(us['loop_compose' + b] / us['compose' + b], 2)
                    rec[f'compose{b}_vs_zsum'] = round(us['compose' + b] / us['zsum' + b], 2)
                    rec[f'adjoint{b}_vs_loop'] = round(us['loop_adjoint' + b] / us['adjoint' + b], 2)
                    rec[f'adjoint{b}_vs_zadj'] = round(us['adjoint' + b] / us['zadj' + b], 2)
                print(json.dumps(rec), flush=True)
                del gg8, bases
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
