"""Time prysm_amd.detector on the device with HIP events, after a run-in until batch times stop drifting.

    python tools/exp_detector.py [--reps 10] [--quick]

One JSON line per configuration.
- expose: 1024^2 x 1, x 16, x 64 frames and 4096^2 x 1, uint16, at means 5, 100 and 1e4 (inversion, PTRS near its start, PTRS far
  in), with and without prnu / dcnu maps, against (a) `composed`: the same exposure from torch calls on the same device
  (torch.poisson, torch.normal, adds, clamps, scale, cast) -- the stand-in for the reference on this device -- and (b) `fill`: a
  fill_ of the same output bytes, the store-rate floor.  samples_per_s, composed_over_fused (> 1: the fused kernel wins),
  fill_over_fused (the fraction of the floor reached).
- reuse: 64 frames in one call against 64 calls of one frame (what computing the per-pixel constants once is worth, launches included).
- bindown: 4096^2 fp32 by 2, 4, 8 against a copy of the same bytes read + written (torch copy_ of the input, scaled) and against
  torch's reshape(...).mean(...).
--quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd import detector as D  # noqa: E402


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


def composed_expose(img, t, dark_t, prnu, dcnu, read_noise, bias, fwc, inv_gain, cap, frames):
    e = img * t
    if prnu is not None:
        e = e * prnu
    d = dark_t * dcnu if dcnu is not None else dark_t
    mean = (e + d).to(torch.float64).expand(frames, *img.shape)
    shot = torch.poisson(mean)
    x = shot + torch.normal(0.0, read_noise, shot.shape, device=img.device, dtype=torch.float64) + bias
    x = torch.clamp(x, max=fwc) * inv_gain
    return torch.clamp(x, 0, cap).to(torch.int32).to(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda')
    par = dict(dark_current=1.0, read_noise=3.0, bias=100.0, fwc=6e4, conversion_gain=1.0, bits=16, exposure_time=1.0)
    for n, frames in ((1024, 1), (1024, 16), (1024, 64), (4096, 1)):
        for mean in (5.0, 100.0, 1e4):
            for maps in (False, True):
                img = (mean - 1.0) * (0.9 + 0.2 * torch.rand((n, n), device=dev, dtype=torch.float32))
                prnu = 1 + 0.01 * torch.randn((n, n), device=dev, dtype=torch.float64) if maps else None
                dcnu = 1 + 0.01 * torch.randn((n, n), device=dev, dtype=torch.float64).abs() if maps else None
                det = D.Detector(**par, prnu=prnu, dcnu=dcnu, seed=1)
                out = torch.empty((frames, n, n), dtype=torch.uint16, device=dev)
                fused = timed(lambda: det.expose(img, frames=frames, validate=False), a.reps, a.quick)
                comp = timed(lambda: composed_expose(img, 1.0, 1.0, prnu, dcnu, 3.0, 100.0, 6e4, 1.0, 65535.0, frames), max(2, a.reps // 3), a.quick)
                fill = timed(lambda: out.view(torch.int16).fill_(7), a.reps, a.quick)
                print(json.dumps(dict(op='expose', n=n, frames=frames, mean=mean, maps=maps, fused_us=round(fused, 1), composed_us=round(comp, 1),
                                      fill_us=round(fill, 1), samples_per_s=round(frames * n * n / fused * 1e6, 0),
                                      composed_over_fused=round(comp / fused, 2), fill_over_fused=round(fill / fused, 3))), flush=True)
    for mean in (5.0, 100.0, 1e4):
        img = torch.full((1024, 1024), mean - 1.0, device=dev, dtype=torch.float32)
        det = D.Detector(**par, seed=1)
        one = timed(lambda: det.expose(img, frames=64, validate=False), a.reps, a.quick)

        def loop():
            for _ in range(64):
                det.expose(img, validate=False)
        many = timed(loop, max(2, a.reps // 3), a.quick)
        print(json.dumps(dict(op='reuse', n=1024, frames=64, mean=mean, one_call_us=round(one, 1), calls_64_us=round(many, 1),
                              ratio=round(many / one, 2))), flush=True)
    x = torch.rand((4096, 4096), device=dev, dtype=torch.float32)
    for f in (2, 4, 8):
        small = torch.empty((4096 // f, 4096 // f), device=dev, dtype=torch.float32)
        nbytes = x.numel() * 4 + small.numel() * 4
        half = torch.empty(nbytes // 8, device=dev, dtype=torch.float32)
        src = torch.empty_like(half)
        ours = timed(lambda: D.bindown(x, f), a.reps, a.quick)
        copy = timed(lambda: half.copy_(src), a.reps, a.quick)           # reads nbytes / 2 and writes nbytes / 2: the same traffic
        ref = timed(lambda: x.reshape(4096 // f, f, 4096 // f, f).mean(dim=(1, 3)), a.reps, a.quick)
        print(json.dumps(dict(op='bindown', n=4096, factor=f, bindown_us=round(ours, 1), copy_same_bytes_us=round(copy, 1), torch_mean_us=round(ref, 1),
                              gb_per_s=round(nbytes / ours / 1e3, 1), copy_over_bindown=round(copy / ours, 3),
                              torch_over_bindown=round(ref / ours, 2))), flush=True)


if __name__ == '__main__':
    main()
