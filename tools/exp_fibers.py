"""Time prysm_amd.x.fibers on the device with HIP events.

    python tools/exp_fibers.py [--window 0.25] [--quick] [--sides 1024 4096] [--budget 900] [--log profiles/fibers/exp_fibers.log]

One JSON line per measurement, printed and written to the log.  Grids of side^2 points over a diameter of 30 around a core of radius
4, float32 and float64, V = 5.5 (8 modes) and V = 30 (228 modes), through a prepared ModeSet:
- `modes`: ModeSet.modes(), every mode in one launch; `store_gbs` is the rate of its stores and `store_share` that rate over
  `--hbm-gbs` (default 6290 GB/s, what the ray trace's log measured for stores).  torch has no J_n or K_n, so there is no torch
  formulation of this one.
- `sum`: ModeSet.sum of one real coefficient vector, against `coefs @ stored` over the stored basis (the basis is formed before the
  clock starts; its bytes are `stored_gb`).
- `coupling1`, `coupling8`: ModeSet.coupling of one complex field and of a stack of 8, against the same formula over the stored basis:
  `view_as_real(E) (B, npts, 2)` contracted with the stored modes by tensordot, sum |E|^2, and the division, the modes' own sums formed
  before the clock starts as ModeSet caches them.
- `overlap`: fibers.overlap of two complex fields, against the three reductions (E1 * E2.conj()).sum(), (|E1|^2).sum(), (|E2|^2).sum().
`us` brackets the whole Python call; `torch_us` the torch formulation; `torch_over_call` > 1 means the unit's call wins.  A timed batch
is as many calls as fill `--window` seconds (at least 2); batches repeat until two agree within 3 % (at most 5), and the median of three
more is reported with the count as `reps`.  Configurations are visited smallest first; when `--budget` seconds have passed the rest
are logged as skipped.  --quick runs each measurement twice only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prysm_amd.x import fibers as FB  # noqa: E402

A = 4.0


def batch_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def timed(fn, quick, window):
    fn()
    torch.cuda.synchronize()
    if quick:
        return batch_ms(fn, 2) * 1e3, 2
    reps = max(2, int(window * 1e3 / batch_ms(fn, 2)) + 1)
    prev = batch_ms(fn, reps)
    for _ in range(5):
        cur = batch_ms(fn, reps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return sorted(batch_ms(fn, reps) for _ in range(3))[1] * 1e3, reps


def grid(side, dt):
    v = (torch.arange(side, dtype=torch.float64, device='cuda') - side // 2) * (30.0 / side)
    y, x = torch.meshgrid(v, v, indexing='ij')
    E1 = torch.exp(-(x * x + y * y) / 3.5 ** 2) * torch.exp(2j * np.pi * (0.021 * x - 0.013 * y))
    E2 = torch.exp(-((x - 0.7) ** 2 / 9 + (y + 0.4) ** 2 / 5)) * torch.exp(1j * (0.05 * (x * x + y * y) + 0.3))
    ct = torch.complex64 if dt == torch.float32 else torch.complex128
    return torch.sqrt(x * x + y * y).to(dt), torch.atan2(y, x).to(dt), E1.to(ct), E2.to(ct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sides', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--budget', type=float, default=900.0)
    ap.add_argument('--hbm-gbs', type=float, default=6290.0)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'fibers', 'exp_fibers.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    log = open(a.log, 'w')
    t0 = time.time()

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    assert torch.cuda.is_available(), 'exp_fibers.py needs an MI355X'
    dicts = {V: FB.find_all_modes(V) for V in (5.5, 30.0)}
    for side in sorted(a.sides):
        for dt in (torch.float32, torch.float64):
            name = str(dt).split('.')[1]
            r, t, E1, E2 = grid(side, dt)
            npts, el = r.numel(), r.element_size()
            head = dict(side=side, dtype=name)
            if time.time() - t0 > a.budget:
                emit(**head, skipped='budget')
                continue
            us, reps = timed(lambda: FB.overlap(E1, E2), a.quick, a.window)
            tus, treps = timed(lambda: ((E1 * E2.conj()).sum(), (E1.abs() ** 2).sum(), (E2.abs() ** 2).sum()), a.quick, a.window)
            emit(**head, op='overlap', us=round(us, 1), reps=reps, torch_us=round(tus, 1), torch_reps=treps, torch_over_call=round(tus / us, 2),
                 read_gbs=round(4 * npts * el / us / 1e3, 1))
            E8 = torch.stack([E1 * (1 + 0.1 * k) for k in range(8)])
            for V, md in dicts.items():
                head = dict(side=side, dtype=name, V=V)
                if time.time() - t0 > a.budget:
                    emit(**head, skipped='budget')
                    continue
                ms = FB.prepare(V, md, A, r, t)
                K = ms.nmodes
                head['modes'] = K
                us, reps = timed(ms.modes, a.quick, a.window)
                gbs = K * npts * el / us / 1e3
                emit(**head, op='modes', us=round(us, 1), reps=reps, store_gbs=round(gbs, 1), store_share=round(gbs / a.hbm_gbs, 3))
                coefs = torch.linspace(-1, 1, K, dtype=dt, device='cuda')
                ms.norms()
                rows = [('sum', lambda: ms.sum(coefs)), ('coupling1', lambda: ms.coupling(E1)), ('coupling8', lambda: ms.coupling(E8))]
                mine = {op: timed(fn, a.quick, a.window) for op, fn in rows}
                stored = ms.modes().reshape(K, -1)
                norms = (stored * stored).sum(dim=1)

                def t_coupling(E):
                    e = torch.view_as_real(E.reshape(-1, npts))
                    p = torch.tensordot(e, stored, dims=([1], [1]))
                    return (p * p).sum(dim=1) / (norms[None, :] * (e * e).sum(dim=(1, 2))[:, None])
                theirs = {'sum': lambda: coefs @ stored, 'coupling1': lambda: t_coupling(E1), 'coupling8': lambda: t_coupling(E8)}
                close = float((t_coupling(E1)[0] - ms.coupling(E1)).abs().max())
                for op, _ in rows:
                    (us, reps), (tus, treps) = mine[op], timed(theirs[op], a.quick, a.window)
                    emit(**head, op=op, us=round(us, 1), reps=reps, torch_us=round(tus, 1), torch_reps=treps,
                         torch_over_call=round(tus / us, 2), stored_gb=round(K * npts * el / 1e9, 2), coupling_max_diff=close)
                del stored, norms, ms
            del r, t, E1, E2, E8
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
