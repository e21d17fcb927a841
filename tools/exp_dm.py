"""Time the deformable mirror (prysm_amd.x.dm) on the device: render, render_adjoint and render_stack(B) with HIP events after
warm-up, per configuration (size / actuators / samples per actuator, precision, rotation, upsample).

    python tools/exp_dm.py [--reps 50] [--stack 64] [--quick]

One JSON line per configuration: us per render, per adjoint, per field of a B-stack.  --quick runs each configuration a few times
only (for a rocprofv3 --kernel-trace --stats run, where the launch sequence, not the time, is wanted).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd.x.dm import DM  # noqa: E402


def gauss(N, sigma, dtype):
    y = np.arange(N) - N // 2
    return np.exp(-(y[:, None] ** 2 + y[None, :] ** 2) / (2 * sigma ** 2)).astype(dtype)


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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--stack', type=int, default=64)
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    if a.quick:
        a.reps, a.warmup = 2, 1
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for N, nact, per in ((512, 50, 8), (1024, 64, 16)):
        for dt in (np.float32, np.float64):
            for rot in ((0, 0, 0), (5, 10, 0)):
                for up in (1, 0.64):
                    dm = DM(gauss(N, per * 0.6, dt), N, Nact=nact, sep=per, rot=rot, upsample=up)
                    dm.update(rng.standard_normal((nact, nact)))
                    acts = torch.from_numpy(rng.standard_normal((a.stack, nact, nact)).astype(dt)).cuda()
                    g = torch.from_numpy(rng.standard_normal((N, N)).astype(dt)).cuda()
                    for _ in range(a.warmup):
                        dm.render()
                        dm.render_adjoint(g)
                    dm.render_stack(acts)
                    torch.cuda.synchronize()
                    r = timed(dm.render, a.reps)
                    adj = timed(lambda: dm.render_adjoint(g), a.reps)
                    st = timed(lambda: dm.render_stack(acts), max(1, a.reps // 10)) / a.stack
                    print(json.dumps(dict(N=N, nact=nact, per_act=per, dtype=np.dtype(dt).name, rot=list(rot), upsample=up,
                                          render_us=round(r, 1), adjoint_us=round(adj, 1), stack_B=a.stack,
                                          stack_us_per_field=round(st, 2))), flush=True)


if __name__ == '__main__':
    main()
