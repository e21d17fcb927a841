"""Time prysm_amd.bayer on the device with HIP events, after a run-in until batch times stop drifting.

    python tools/exp_bayer.py [--reps 10] [--quick]

One JSON line per configuration.
- demosaic: demosaic_malvar at 1024^2, 2048^2 and 4096^2, from a float32 mosaic and from uint16 DN (float32 out), against (a) `copy`:
  a torch copy_ that moves the same bytes read + written (half of them each way), the rate floor, and (b) `composed`: the reference's
  algorithm from torch calls on the same device (reflect padding, four conv2d, the strided assignments, the stack).  gb_per_s counts
  the bytes the algorithm needs (one read of the mosaic, one store of the image); copy_over_fused is the fraction of the floor
  reached, composed_over_fused > 1 means the fused kernel wins.  layout 'chw' is timed too: it stores without the LDS staging, so
  the pair separates the store form from the rest.
- prescale: wb_prescale(safe=True) at 4096^2 float32 (two reads, one store) against a copy of the same bytes.
--quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd import bayer as B  # noqa: E402
from prysm_amd import bayer_plan as BP  # noqa: E402


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


def composed_malvar(img, weights):
    """demosaic_malvar (rggb) as the reference writes it, on the device: integer input promoted, four reflect-padded convolutions,
    ten strided assignments, a stack"""
    if not img.is_floating_point():
        img = img.to(torch.float32)
    pad = F.pad(img[None, None], (2, 2, 2, 2), mode='reflect')       # torch's 'reflect' omits the edge sample: the same traffic
    g, c1, c2, c3 = (F.conv2d(pad, w)[0, 0] for w in weights)
    red, blue = torch.empty_like(img), torch.empty_like(img)
    g[B.top_right] = img[B.top_right]
    g[B.bottom_left] = img[B.bottom_left]
    red[B.top_left] = img[B.top_left]
    red[B.top_right] = c1[B.top_right]
    red[B.bottom_left] = c2[B.bottom_left]
    red[B.bottom_right] = c3[B.bottom_right]
    blue[B.top_left] = c3[B.top_left]
    blue[B.top_right] = c2[B.top_right]
    blue[B.bottom_left] = c1[B.bottom_left]
    blue[B.bottom_right] = img[B.bottom_right]
    return torch.stack((red, g, blue), dim=2)


def same_bytes_copy(nbytes, dev):
    """a copy_ that reads nbytes / 2 and writes nbytes / 2"""
    dst = torch.empty(nbytes // 8, device=dev, dtype=torch.float32)
    src = torch.empty_like(dst)
    return lambda: dst.copy_(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda')
    weights = [torch.tensor(np.array(t) / 8., dtype=torch.float32, device=dev)[None, None]
               for t in (BP.kernel_G_at_R_or_B, BP.kernel_R_at_G_in_RB, BP.kernel_R_at_G_in_BR, BP.kernel_R_at_B_in_BB)]
    from prysm_amd.conf import config
    config.precision = 32          # uint16 DN -> float32
    for n in (1024, 2048, 4096):
        for src in ('float32', 'uint16'):
            if src == 'float32':
                img = torch.rand((n, n), device=dev, dtype=torch.float32) * 4095
            else:
                img = torch.randint(0, 4096, (n, n), device=dev, dtype=torch.int32).to(torch.uint16)
            nbytes = img.numel() * img.element_size() + 3 * n * n * 4
            fused = timed(lambda: B.demosaic_malvar(img), a.reps, a.quick)
            planar = timed(lambda: B.demosaic_malvar(img, layout='chw'), a.reps, a.quick)
            copy = timed(same_bytes_copy(nbytes, dev), a.reps, a.quick)
            comp = timed(lambda: composed_malvar(img, weights), max(2, a.reps // 3), a.quick)
            print(json.dumps(dict(op='demosaic', n=n, input=src, fused_us=round(fused, 1), fused_chw_us=round(planar, 1),
                                  copy_same_bytes_us=round(copy, 1), composed_us=round(comp, 1), gb_per_s=round(nbytes / fused / 1e3, 1),
                                  copy_over_fused=round(copy / fused, 3), copy_over_fused_chw=round(copy / planar, 3),
                                  composed_over_fused=round(comp / fused, 2))), flush=True)
    n = 4096
    mos = torch.rand((n, n), device=dev, dtype=torch.float32) * 4095
    nbytes = 3 * n * n * 4
    ours = timed(lambda: B.wb_prescale(mos, 1.0001, 1.0, 1.0, 0.9999, safe=True, saturation=4000.0), a.reps, a.quick)
    copy = timed(same_bytes_copy(nbytes, dev), a.reps, a.quick)
    print(json.dumps(dict(op='prescale_safe', n=n, prescale_us=round(ours, 1), copy_same_bytes_us=round(copy, 1),
                          gb_per_s=round(nbytes / ours / 1e3, 1), copy_over_prescale=round(copy / ours, 3))), flush=True)


if __name__ == '__main__':
    main()
