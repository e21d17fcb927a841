"""Time the recurrence families of prysm_amd.polynomials on the device with HIP events after warm-up, each against the reference's own
formulation written as torch operations on the same device:

- cheby1_2d_sum_der_xy and xy_sum_der_xy with 16 x 16 modes at 1024^2 and 4096^2, fp32 and fp64, against stored axis tables and
  Ty.T @ C @ Tx three times (the tables are built outside the timed window, which favours the reference);
- cheby1_2d_sum_adjoint (z, dz/dx and dz/dy adjoints into one gradient) at the same sizes against Ty @ g @ Tx.T three times;
- legendre_seq of 31 orders on 2^20 points against the recurrence as one torch expression per order, and against a device copy of the
  same output bytes.

    python tools/exp_recur.py [--reps 50] [--rounds 5] [--out profiles/recur/exp_recur.log]

One JSON line per configuration, printed and appended to --out.  The kernel and the torch formulation alternate within a round; a time
is the median over the rounds of the mean over --reps calls, with the spread (min, max) beside it.  store_GBps is the bytes of the three
outputs over the kernel's time (the sum is store-bound: nothing else of that size moves).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prysm_amd import polynomials as P  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def bracket(fns, reps, rounds, warmup=3):
    """{name: (median, min, max) microseconds}: the functions alternate within each round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn, reps))
    return {k: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in got.items()}


def legendre_torch(nmax, x, out):
    """legendre_seq as the reference walks it (legendre.py:34-57): one expression per order"""
    out[0] = 1
    out[1] = x
    for k in range(2, nmax + 1):
        torch.sub((2 * k - 1) / k * x * out[k - 1], (k - 1) / k * out[k - 2], out=out[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recur', 'exp_recur.log'))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    log = open(a.out, 'w')

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    emit(dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, time='us: [median, min, max] over the rounds'))
    rng = np.random.default_rng(0)
    mns = [(m, n) for m in range(16) for n in range(16)]
    for N in (1024, 4096):
        for dt in (torch.float32, torch.float64):
            es = 4 if dt == torch.float32 else 8
            x = torch.linspace(-1, 1, N, dtype=dt, device='cuda')
            c = torch.from_numpy(rng.standard_normal(256)).to('cuda', dt)
            C = c.reshape(16, 16).T.contiguous()               # C[n][m] of mns' order (m outer)
            g = torch.from_numpy(rng.standard_normal((3, N, N))).to('cuda', dt)
            reps = a.reps if N <= 1024 else max(5, a.reps // 4)
            for fam, fwd in (('cheby1', P.cheby1_2d_sum_der_xy), ('xy', P.xy_sum_der_xy)):
                if fam == 'cheby1':
                    T, Td = P.cheby1_seq(range(16), x), P.cheby1_der_seq(range(16), x)
                else:
                    T = torch.stack([x ** k for k in range(16)])
                    Td = torch.stack([k * x ** max(k - 1, 0) for k in range(16)])
                fns = {'kernel': lambda: fwd(c, mns, x, x),
                       'torch': lambda: (T.T @ C @ T, T.T @ C @ Td, Td.T @ C @ T)}
                # how far the two are apart, relative to the largest value, before they are timed
                err = max(float((got - want).abs().max() / want.abs().max()) for got, want in zip(fns['kernel'](), fns['torch']()))
                us = bracket(fns, reps, a.rounds)
                emit(dict(what=fam + '_2d_sum_der_xy', N=N, dtype=str(dt).split('.')[-1], modes='16x16', us=us, kernel_vs_torch=err,
                          speedup=round(us['torch'][0] / us['kernel'][0], 2), store_GBps=round(3 * N * N * es / us['kernel'][0] / 1e3, 1)))
            T, Td = P.cheby1_seq(range(16), x), P.cheby1_der_seq(range(16), x)
            fns = {'kernel': lambda: P.cheby1_2d_sum_adjoint(g[0], mns, x, x, dx_bar=g[1], dy_bar=g[2]),
                   'torch': lambda: T @ g[0] @ T.T + T @ g[1] @ Td.T + Td @ g[2] @ T.T}
            got, want = fns['kernel']().reshape(16, 16).T, fns['torch']()
            err = float((got - want).abs().max() / want.abs().max())
            us = bracket(fns, reps, a.rounds)
            emit(dict(what='cheby1_2d_sum_adjoint', N=N, dtype=str(dt).split('.')[-1], modes='16x16', maps=3, us=us, kernel_vs_torch=err,
                      speedup=round(us['torch'][0] / us['kernel'][0], 2), read_GBps=round(3 * N * N * es / us['kernel'][0] / 1e3, 1)))
            del g, T, Td
            torch.cuda.empty_cache()
    npts = 1 << 20
    for dt in (torch.float32, torch.float64):
        es = 4 if dt == torch.float32 else 8
        x = torch.linspace(-1, 1, npts, dtype=dt, device='cuda')
        out = torch.empty((31, npts), dtype=dt, device='cuda')
        src = P.legendre_seq(range(31), x)
        fns = {'kernel': lambda: P.legendre_seq(range(31), x), 'torch': lambda: legendre_torch(30, x, out), 'copy': lambda: out.copy_(src)}
        err = float((legendre_torch(30, x, out) - src).abs().max())
        us = bracket(fns, a.reps, a.rounds)
        emit(dict(what='legendre_seq', npts=npts, orders=31, dtype=str(dt).split('.')[-1], us=us, kernel_vs_torch=err,
                  speedup=round(us['torch'][0] / us['kernel'][0], 2), store_GBps=round(31 * npts * es / us['kernel'][0] / 1e3, 1),
                  copy_GBps=round(2 * 31 * npts * es / us['copy'][0] / 1e3, 1)))
    log.close()


if __name__ == '__main__':
    main()
