"""Time prysm_amd.x.optym.PrysmLBFGSB on the device, after a run-in until batch times stop drifting.

    python tools/exp_lbfgsb.py [--reps 5] [--quick] [--sizes 1024,4096] [--log profiles/lbfgsb/exp_lbfgsb.log]

One JSON line per configuration, printed and appended to the log; n = size^2, memory 10, float32 and float64.
- `step`: microseconds of one whole step EXCLUDING fg, wall clock around step() with a synchronize, minus the time of the fg calls
  it made (fg is the quadratic f = 1/2 sum w (x - t)^2, timed by itself the same way).  A step reads records on the host, so HIP
  events around it would not see its stalls.  `unbounded`, and `bounded` with bounds that hold about 30 % of the variables.
  `floor_us` is (2 m + 6) n s bytes over 6.29 TB/s, the store / copy rate measured for this part, for the unbounded step.
- `torch_step`: the unbounded step of the reference in torch operations (the two-loop recursion, the trial point, the pair and its
  products, lines 933-977 and 1086-1107) with its scalars on the device and no host read, HIP events; the line search is taken as
  accepted at alpha = 1, which favours it.  The bounded step of the reference (the Cauchy sweep, the subspace solve) has NO torch
  baseline here.
- `pass`: one pass by itself, including its fold launch and its host read where it has one, with the bytes it must move (every
  history row once) and their share of 6.29 TB/s.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd.x.optym import PrysmLBFGSB  # noqa: E402

RATE = 6.29e12      # bytes per second, the store / copy rate measured for this part
MEMORY = 10


def wall_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def settled(fn, reps, quick):
    """us per call: batches of `reps` until two successive batches agree within 3 % (at most 8), then the median of three more"""
    fn()
    if quick:
        return wall_us(fn, 2)
    prev = wall_us(fn, reps)
    for _ in range(8):
        cur = wall_us(fn, reps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return sorted(wall_us(fn, reps) for _ in range(3))[1]


def problem(n, dtype, seed=3):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    t = torch.randn(n, generator=gen, device='cuda', dtype=dtype)
    w = torch.rand(n, generator=gen, device='cuda', dtype=dtype) * 19.5 + 0.5
    x0 = torch.randn(n, generator=gen, device='cuda', dtype=dtype)
    calls = [0]

    def fg(x):
        calls[0] += 1
        d = x - t
        g = w * d
        return 0.5 * torch.dot(g, d), g
    return fg, x0, calls


def torch_step(S, Y, rho, x, g, g_new, k):
    """-H g by the two-loop recursion, the trial point at alpha = 1, the new pair and its products; nothing read on the host"""
    q = g.clone()
    alphas = [None] * k
    for i in range(k - 1, -1, -1):
        alphas[i] = torch.dot(S[i], q) * rho[i]
        q -= Y[i] * alphas[i]
    q *= 1 / (rho[k - 1] * torch.dot(Y[k - 1], Y[k - 1]))
    for i in range(k):
        beta = torch.dot(Y[i], q) * rho[i]
        q += S[i] * (alphas[i] - beta)
    p = -q
    x_new = x + 1.0 * p
    phi1 = torch.dot(g_new, p)
    s = p * 1.0
    y = g_new - g
    sy, yy = torch.dot(s, y), torch.dot(y, y)
    S[0].copy_(s)
    Y[0].copy_(y)
    return x_new, phi1, sy, yy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sizes', default='1024,4096')
    ap.add_argument('--log', default=os.path.join('profiles', 'lbfgsb', 'exp_lbfgsb.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    out = open(a.log, 'a')

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()

    for size in (int(s) for s in a.sizes.split(',')):
        n = size * size
        for dtype in (torch.float32, torch.float64):
            s = 4 if dtype == torch.float32 else 8
            name = 'float32' if s == 4 else 'float64'
            for case in ('unbounded', 'bounded'):
                fg, x0, calls = problem(n, dtype)
                kw = {} if case == 'unbounded' else dict(lower_bounds=torch.full((n,), -1.04, dtype=dtype), upper_bounds=torch.full((n,), 1.04, dtype=dtype))
                opt = PrysmLBFGSB(fg, x0, memory=MEMORY, **kw)
                fg_us = settled(lambda: fg(opt.x), a.reps, a.quick)

                def warm():      # the timed steps run on a full history: memory steps from a fresh start first
                    opt.reset()
                    for _ in range(MEMORY):
                        opt.step()
                rounds, per = (1 if a.quick else 3), 4
                total, ncalls, reads = 0.0, 0, 0
                for _ in range(rounds):
                    warm()
                    torch.cuda.synchronize()
                    calls[0], reads0 = 0, opt.host_reads
                    t0 = time.perf_counter()
                    for _ in range(per):
                        opt.step()
                    torch.cuda.synchronize()
                    total += (time.perf_counter() - t0) * 1e6
                    ncalls += calls[0]
                    reads += opt.host_reads - reads0
                md = dict(opt.last_step_metadata)
                steps = rounds * per
                step_us = (total - ncalls * fg_us) / steps
                floor = (2 * MEMORY + 6) * n * s / RATE * 1e6
                emit(what='step', case=case, size=size, dtype=name, memory=MEMORY, step_us=round(step_us, 1), fg_us=round(fg_us, 1),
                     fg_calls_per_step=round(ncalls / steps, 2), host_reads_per_step=round(reads / steps, 2),
                     floor_us=round(floor, 1) if case == 'unbounded' else None,
                     floor_fraction=round(floor / step_us, 3) if case == 'unbounded' else None, last_step=md)
                # ---- the passes by themselves, on the full history
                P, k = opt._passes, opt._core.H.k
                rows = 2 * k
                passes = [('W^T g + small algebra + direction', P.direction_unbounded, (2 * rows + 3) * n * s),
                          ('trial', lambda: L_trial(P), 3 * n * s)]
                if case == 'bounded':
                    P.breakpoints()
                    P.cauchy_point(0.0, 0.01)
                    passes += [('breakpoints', P.breakpoints, (rows + 6) * n * s),
                               ('cauchy point', lambda: P.cauchy_point(0.0, 0.01), 4 * n * s + n),
                               ('small algebra + residual', lambda: P.residual_from(np.full(rows, 1e-3)), (rows + 4) * n * s),
                               ('free dots + gram + small algebra + subspace', lambda: P.subspace_step(n - 1),
                                (3 * rows + 9) * n * s + 3 * n)]
                for label, fn, nbytes in passes:
                    us = settled(fn, a.reps, a.quick)
                    emit(what='pass', name=label, case=case, size=size, dtype=name, rows=rows, us=round(us, 1), mbytes=round(nbytes / 1e6, 1),
                         rate_fraction=round(nbytes / (us * 1e-6) / RATE, 3))
                if case == 'unbounded':
                    S, Y = P.S[:MEMORY].clone(), P.Y[:MEMORY].clone()
                    rho = 1 / (S * Y).sum(dim=1)
                    g = fg(opt.x)[1]
                    g_new = g * 0.5
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                    def events(reps):
                        start.record()
                        for _ in range(reps):
                            torch_step(S, Y, rho, opt.x, g, g_new, MEMORY)
                        stop.record()
                        torch.cuda.synchronize()
                        return start.elapsed_time(stop) / reps * 1e3
                    events(2)
                    tus = sorted(events(a.reps) for _ in range(3))[1]
                    emit(what='torch_step', case=case, size=size, dtype=name, memory=MEMORY, torch_us=round(tus, 1),
                         torch_over_fused=round(tus / step_us, 2))
                del opt, P
                torch.cuda.empty_cache()


def L_trial(P):
    from prysm_amd import _lib as L
    L.check(P.lib.pm_lbfgsb_trial(P.code, P.n, L.ptr(P.x), L.ptr(P.p), 0.5, L.ptr(P.lo), L.ptr(P.hi), L.ptr(P.xt), L.stream_ptr()))


if __name__ == '__main__':
    main()
