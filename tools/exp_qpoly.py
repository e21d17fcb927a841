"""Time the Forbes Q polynomials of prysm_amd.polynomials on the device with HIP events after warm-up: Q2d_seq against a
device-to-device copy of the same output bytes, Q2d_sum and Q2d_sum_adjoint (B = 1 and B = 8) against sum_of_2d_modes /
sum_of_2d_modes_adjoint over the materialised basis, and sum_of_2d_modes_adjoint against the copy.

    python tools/exp_qpoly.py [--reps 20] [--quick]

One JSON line per configuration (size, precision, K = 36 for n <= 3, |m| <= 4 or 231 for n <= 10, |m| <= 10).  Rates are bytes moved over time: a copy
moves 2x its bytes (read + write), the basis writes K planes, the modes dot reads K + 1 planes.  --quick runs each configuration a
few times only (for a rocprofv3 --kernel-trace --stats run, where the launch sequence, not the time, is wanted).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd import polynomials as P  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    if a.quick:
        a.reps, a.warmup = 2, 1
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for N in (1024, 2048):
        for dt in (torch.float32, torch.float64):
            g = ((torch.arange(N, dtype=dt, device='cuda') - N // 2) / (N // 2))
            y, x = torch.meshgrid(g, g, indexing='ij')
            x, y = x.contiguous(), y.contiguous()
            r, t = torch.hypot(x, y), torch.atan2(y, x)
            es = 4 if dt == torch.float32 else 8
            for nmax, mmax in ((3, 4), (10, 10)):
                nms = [(n, m) for n in range(nmax + 1) for m in range(-mmax, mmax + 1)]
                K = len(nms)
                c1 = torch.from_numpy(rng.standard_normal(K)).to('cuda', dt)
                c8 = torch.from_numpy(rng.standard_normal((8, K))).to('cuda', dt)
                g1 = torch.from_numpy(rng.standard_normal((N, N))).to('cuda', dt)
                g8 = torch.from_numpy(rng.standard_normal((8, N, N))).to('cuda', dt)
                basis = P.Q2d_seq(nms, r, t)
                src = torch.empty_like(basis)
                w1 = c1.cpu().numpy()
                w8 = c8.cpu().numpy()
                fns = dict(
                    seq=lambda: P.Q2d_seq(nms, r, t),
                    copy=lambda: src.copy_(basis),
                    sum1=lambda: P.Q2d_sum(c1, nms, x, y),
                    sum8=lambda: P.Q2d_sum(c8, nms, x, y),
                    modes_sum1=lambda: P.sum_of_2d_modes(basis, w1),
                    modes_sum8=lambda: [P.sum_of_2d_modes(basis, w) for w in w8],
                    adj1=lambda: P.Q2d_sum_adjoint(g1, nms, x, y),
                    adj8=lambda: P.Q2d_sum_adjoint(g8, nms, x, y),
                    modes_adj1=lambda: P.sum_of_2d_modes_adjoint(basis, g1),
                    modes_adj8=lambda: [P.sum_of_2d_modes_adjoint(basis, g8[b]) for b in range(8)],
                )
                for fn in fns.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                us = {k: timed(fn, max(1, a.reps // 8) if k.endswith('8') else a.reps) for k, fn in fns.items()}
                out_b = K * N * N * es
                rec = dict(N=N, dtype=str(dt).split('.')[-1], K=K, nmax=nmax, mmax=mmax, us={k: round(v, 1) for k, v in us.items()})
                rec['copy_GBps'] = round(2 * out_b / us['copy'] / 1e3, 1)
                rec['seq_GBps'] = round(out_b / us['seq'] / 1e3, 1)
                rec['seq_over_copy_rate'] = round(rec['seq_GBps'] / rec['copy_GBps'], 3)
                rec['modes_adj_GBps'] = round((K + 1) * N * N * es / us['modes_adj1'] / 1e3, 1)
                rec['modes_adj_over_copy_rate'] = round(rec['modes_adj_GBps'] / rec['copy_GBps'], 3)
                for b in ('1', '8'):
                    rec[f'sum{b}_speedup'] = round(us['modes_sum' + b] / us['sum' + b], 2)
                    rec[f'adj{b}_speedup'] = round(us['modes_adj' + b] / us['adj' + b], 2)
                print(json.dumps(rec), flush=True)
                del basis, src, g8
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
