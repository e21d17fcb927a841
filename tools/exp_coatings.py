"""Time prysm_amd.x.coatings on the device with HIP events, after a run-in until batch times stop drifting.

    python tools/exp_coatings.py [--reps 10] [--quick] [--log profiles/coatings/exp_coatings.log]

One JSON line per configuration, printed and appended to the log.  Two shapes, both precisions:
- `spectral`: 40 layers over 1024 wavelengths x 3 angles (3072 samples, shared layer tables);
- `map`: 8 layers over a 1024 x 1024 angle-of-incidence map at one wavelength (1048576 samples).
Operations: `stack_rt` and `RTA` for s, and `value_and_grad` of Reflectance(target 0.1) for 'avg', each against the SAME formulas
written as torch operations on the same device (`torch_us`: the characteristic-matrix sweep in complex tensors, both polarisations
for 'avg', its gradient by torch.autograd; the parent of this feature has nothing to time).  `avg_us` against `s_plus_p_us` is the
both-polarisations sweep against an s term and a p term evaluated one after the other.  torch_over_fused > 1 means the kernels win.
--quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd.x import coatings as C  # noqa: E402

MATERIALS = (1.38, 2.1588, 1.6290 + 0.0034836j, 1.46)


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


def torch_cos_snell(n0, n1, sin0):
    sint = n0 / n1 * sin0
    cost = torch.sqrt(1 - sint * sint)
    return torch.where((sint.imag == 0) & (sint.real > 1), -cost, cost)


def torch_sweep(n, d, wvl, theta, nsub, n0, pol, fields=False):
    """the sweep from the substrate in complex tensors: r, t, R, T and (with `fields`) the per-layer absorptance.  n: complex
    scalars per layer, d: a real tensor of L thicknesses, wvl and theta real tensors over the samples"""
    cd = torch.complex64 if d.dtype == torch.float32 else torch.complex128
    sin0, cos0 = torch.sin(theta).to(cd), torch.cos(theta).to(cd)
    n0, nsub = torch.tensor(n0, dtype=cd, device=d.device), torch.tensor(nsub, dtype=cd, device=d.device)
    cs = torch_cos_snell(n0, nsub, sin0)
    eta0, etas = (n0 / cos0, nsub / cs) if pol == 'p' else (n0 * cos0, nsub * cs)
    B, Cc = torch.ones_like(etas), etas
    flux = [(B * Cc.conj()).real]
    for j in range(len(n) - 1, -1, -1):
        nj = torch.tensor(n[j], dtype=cd, device=d.device)
        cost = torch_cos_snell(n0, nj, sin0)
        beta = (2 * math.pi * nj * d[j] * cost) / wvl
        sinb, cosb = torch.sin(beta), torch.cos(beta)
        eta = nj / cost if pol == 'p' else nj * cost
        B, Cc = cosb * B + (-1j * sinb / eta) * Cc, (-1j * eta * sinb) * B + cosb * Cc
        if fields:
            flux.append((B * Cc.conj()).real)
    den = eta0 * B + Cc
    r, t = (eta0 * B - Cc) / den, 2 * eta0 / den
    R, T = r.real ** 2 + r.imag ** 2, etas.real / eta0.real * (t.real ** 2 + t.imag ** 2)
    if not fields:
        return r, t, R, T
    scale = (t.real ** 2 + t.imag ** 2) / eta0.real
    f = torch.stack(flux[::-1]) * scale
    return R, T, f[:-1] - f[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--log', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'coatings', 'exp_coatings.log'))
    a = ap.parse_args()
    dev = torch.device('cuda')
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    log = open(a.log, 'w')

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    rng = np.random.default_rng(3)
    for shape_name, L in (('spectral', 40), ('map', 8)):
        n = [MATERIALS[j % 4] for j in range(L)]
        d0 = rng.uniform(0.05, 0.25, L)
        if shape_name == 'spectral':
            W, A = np.meshgrid(np.linspace(0.45, 0.75, 1024), np.radians([0.0, 23.0, 45.0]))
        else:
            y, x = np.mgrid[-1:1:1024j, -1:1:1024j]
            W, A = np.float64(0.55), np.radians(40.0) * np.hypot(x, y) / math.sqrt(2)
        for dt in (torch.float32, torch.float64):
            d = torch.from_numpy(d0).to(dev, dt)
            stack = C.Stack(n, d, 1.458461)
            wv, th = torch.from_numpy(np.broadcast_to(W, A.shape).copy()).to(dev, dt), torch.from_numpy(A).to(dev, dt)
            Wf, Af = (W, A) if shape_name == 'spectral' else (0.55, th)      # the map stays on the device: no 8 MB upload per call
            base = dict(shape=shape_name, layers=L, samples=int(A.size), dtype=str(dt).split('.')[1])
            for op, fused_fn, torch_fn in (
                    ('stack_rt', lambda: C.stack_rt(stack, Wf, Af, 's'), lambda: torch_sweep(n, d, wv, th, 1.458461, 1.0, 's')),
                    ('RTA', lambda: C.RTA(stack, Wf, Af, 's'), lambda: torch_sweep(n, d, wv, th, 1.458461, 1.0, 's', fields=True))):
                fused, comp = timed(fused_fn, a.reps, a.quick), timed(torch_fn, a.reps, a.quick)
                emit(op=op, pol='s', **base, fused_us=round(fused, 1), torch_us=round(comp, 1), torch_over_fused=round(comp / fused, 2))
            # the public call resolves the grid on the host every time; a merit term keeps its device operands, as an optimizer's fg does
            avg = C.Reflectance(W, A, 'avg', 0.1)
            sp = C.MeritFunction([C.Reflectance(W, A, 's', 0.1, 0.5), C.Reflectance(W, A, 'p', 0.1, 0.5)])

            def torch_fg():
                dd = d.clone().requires_grad_(True)
                q = (torch_sweep(n, dd, wv, th, 1.458461, 1.0, 's')[2] + torch_sweep(n, dd, wv, th, 1.458461, 1.0, 'p')[2]) / 2
                f = torch.sum((q - 0.1) ** 2)
                f.backward()
                return f, dd.grad
            fused = timed(lambda: avg.value_and_grad(stack), a.reps, a.quick)
            split = timed(lambda: sp.value_and_grad(stack), a.reps, a.quick)
            comp = timed(torch_fg, a.reps, a.quick)
            emit(op='value_and_grad', pol='avg', **base, avg_us=round(fused, 1), s_plus_p_us=round(split, 1), torch_us=round(comp, 1),
                 s_plus_p_over_avg=round(split / fused, 2), torch_over_fused=round(comp / fused, 2))
            del stack, avg, sp


if __name__ == '__main__':
    main()
