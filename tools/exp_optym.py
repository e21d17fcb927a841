"""Time prysm_amd.x.optym on the device with HIP events, after a run-in until batch times stop drifting.

    python tools/exp_optym.py [--reps 10] [--quick] [--log profiles/optym/exp_optym.log]

One JSON line per configuration, printed and appended to the log: a step of each optimizer and each cost at 1024^2 and 4096^2 in
float32 and float64, against the SAME formulas written as torch operations on the same device (`torch_us`; the parent of this
feature has nothing to time).  gb_per_s is the bytes the algorithm needs (what the fused kernels read and write once) over the fused
time; torch_over_fused > 1 means the fused form wins.
- step: fg is a stored gradient (the model is not what is timed); advance + step, two launches.  Bytes: x, g and the state read,
  x, x_prev and the state written.
- cost: masked (a byte mask), three launches (four for the bias-and-gain-invariant cost).  Bytes: two passes over M, D and the mask
  and one store of the gradient.  The torch form uses the mask as a weight (no compaction, no host read), the cheapest torch can do.
--quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd.x import optym as O  # noqa: E402


def batch_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def timed(fn, reps, quick):
    """us per call: batches of `reps` until two successive batches agree within 3 % (at most 8), then the median of three more"""
    fn()
    torch.cuda.synchronize()
    if quick:
        return batch_ms(fn, 2) * 1e3
    prev = batch_ms(fn, reps)
    for _ in range(8):
        cur = batch_ms(fn, reps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return sorted(batch_ms(fn, reps) for _ in range(3))[1] * 1e3


class TorchStep:
    """the reference's step() of each optimizer in torch operations, unbounded, with the host's beta ** iter"""

    def __init__(self, name, x, g, alpha=0.05, beta1=0.9, beta2=0.999):
        self.name, self.x, self.g, self.alpha, self.b1, self.b2 = name, x.clone(), g, alpha, beta1, beta2
        self.m, self.v = torch.zeros_like(x), torch.zeros_like(x)
        self.eps = float(torch.finfo(x.dtype).eps)
        self.iter = 0

    def __call__(self):
        self.iter += 1
        k, g, a, b1, b2, eps = self.iter, self.g, self.alpha, self.b1, self.b2, self.eps
        n = self.name
        if n == 'GradientDescent':
            self.x = self.x - a * g
        elif n == 'AdaGrad':
            self.m += g * g
            self.x = self.x - a * g / (torch.sqrt(self.m) + eps)
        elif n == 'RMSProp':
            self.m = b1 * self.m + (1 - b1) * (g * g)
            self.x = self.x - a * g / (torch.sqrt(self.m) + eps)
        elif n in ('Adam', 'AdaMomentum'):
            self.m = b1 * self.m + (1 - b1) * g
            if n == 'Adam':
                self.v = b2 * self.v + (1 - b2) * (g * g)
            else:
                self.v = b2 * self.v + (1 - b2) * (self.m * self.m) + eps
            mhat, vhat = self.m / (1 - b1 ** k), self.v / (1 - b2 ** k)
            self.x = self.x - a * mhat / (torch.sqrt(vhat) + eps if n == 'Adam' else torch.sqrt(vhat))
        elif n == 'RAdam':
            self.m = b1 * self.m + (1 - b1) * g
            self.v = b2 * self.v + (1 - b2) * (g * g)
            rhoinf = 2 / (1 - b2) - 1
            rho = rhoinf - (2 * k * b2 ** k) / (1 - b2 ** k)
            if rho >= 5:
                r = float(np.sqrt((rho - 4) * (rho - 2) * rhoinf / ((rhoinf - 4) * (rhoinf - 2) * rho)))
                self.x = self.x - a * r * (self.m / (1 - b1 ** k)) * (float(np.sqrt(1 - b2 ** k)) / (torch.sqrt(self.v) + eps))
            else:
                self.x = self.x - a * g
        else:      # Yogi
            gsq = g * g
            self.m = b1 * self.m + (1 - b1) * g
            self.v = self.v - (1 - b2) * torch.sign(self.v - gsq) * gsq
            self.x = self.x - a * self.m / (torch.sqrt(torch.sqrt(self.v + eps)) + eps)


def torch_cost(name, M, D, w):
    """the masked costs with the mask as a float weight: no compaction and no host read"""
    N = w.sum()
    if name == 'mean_square_error':
        diff = (M - D) * w
        return (diff * diff).sum() / N, 2 * diff / N
    if name == 'negative_loglikelihood':
        c = -((D * torch.log(M) + (1 - D) * torch.log(1 - M)) * w).sum() / N
        return c, ((-D / M) + ((1 - D) / (1 - M))) * w / N
    Imean, Dmean = (M * w).sum() / N, (D * w).sum() / N
    Ihat, Dhat = (M - Imean) * w, (D - Dmean) * w
    alpha = (Ihat * Dhat).sum() / (Ihat * Ihat).sum()
    beta = Dmean - alpha * Imean
    R = 1 / (D * D * w).sum()
    raw = ((alpha * M + beta) - D) * w
    return R * (raw * raw).sum(), 2 * R * alpha * raw


STATE = dict(GradientDescent=0, AdaGrad=1, RMSProp=1, Adam=2, RAdam=2, AdaMomentum=2, Yogi=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--log', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'optym', 'exp_optym.log'))
    a = ap.parse_args()
    dev = torch.device('cuda')
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    log = open(a.log, 'w')

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    for n in (1024, 4096):
        for dt in (torch.float32, torch.float64):
            es = 4 if dt == torch.float32 else 8
            x0 = torch.randn(n * n, device=dev, dtype=dt)
            grad = torch.randn(n * n, device=dev, dtype=dt)
            for name, ns in STATE.items():
                opt = getattr(O, name)(lambda x: (None, grad), x0, 0.05)
                fused = timed(opt.step, a.reps, a.quick)
                ref = TorchStep(name, x0, grad)
                comp = timed(ref, a.reps, a.quick)
                nbytes = (2 + ns + 2 + ns) * n * n * es
                emit(op='step', optimizer=name, n=n, dtype=str(dt).split('.')[1], fused_us=round(fused, 1), torch_us=round(comp, 1),
                     gb_per_s=round(nbytes / fused / 1e3, 1), torch_over_fused=round(comp / fused, 2))
                del opt, ref
            M = torch.rand(n * n, device=dev, dtype=dt) * 0.9 + 0.05
            D = torch.rand(n * n, device=dev, dtype=dt) * 0.9 + 0.05
            mask = torch.rand(n * n, device=dev) < 0.7
            w = mask.to(dt)
            for name in ('mean_square_error', 'bias_and_gain_invariant_error', 'negative_loglikelihood'):
                fn = getattr(O, name)
                fused = timed(lambda: fn(M, D, mask=mask), a.reps, a.quick)
                comp = timed(lambda: torch_cost(name, M, D, w), a.reps, a.quick)
                nbytes = (2 * (2 * es + 1) + es) * n * n
                emit(op='cost', cost=name, n=n, dtype=str(dt).split('.')[1], fused_us=round(fused, 1), torch_us=round(comp, 1),
                     gb_per_s=round(nbytes / fused / 1e3, 1), torch_over_fused=round(comp / fused, 2))


if __name__ == '__main__':
    main()
