"""Time the PSD surface synthesis (csrc/psdsynth.hip and the two transforms around it) on the device with HIP events (DESIGN.md
section 5), by the protocol of tools/exp_interferogram.py.

    python tools/exp_psdsynth.py [--window 0.15] [--quick] [--budget 400] [--log profiles/psdsynth/exp_psdsynth.log]

One JSON line per measurement, printed and written to the log; float32 and float64 (config.precision follows), 1024^2 and 4096^2, a
single surface and batch = 8.  The first line holds `store_gbs`, the rate of a zero fill of 1 GiB in this run.
- `render`: render_synthetic_surface(size 100, abc_psd a = 1e4, b = 1/100, c = 2, 'circle', rms = 5, a seed), no host read, against the
  same formulas as torch operations on the device (`torch_us`: torch.rand, fft2, angle, exp, the PSD from generated frequencies,
  ifft2, the masked rms; `torch_over_call` > 1 means the unit's call wins).
- `uniform`, `signal`, `finish`, `scale`: each launch of the unit alone on the arrays of that render (`finish` is the pass and its
  fold), with `floor_us`, the time its bytes take at the store rate -- uniform writes N^2 s, signal reads and writes N^2 2s, finish
  reads N^2 2s and writes N^2 s, scale reads and writes N^2 s (s the bytes of a real) -- and `floor_share` = floor_us / us;
  `transforms`: the forward and the inverse transform of that render together.
A timed batch is as many calls as fill `--window` seconds (at least 2); batches repeat until two agree within 3 % (at most 5), and the
median of three more is reported with the count as `reps`.  When `--budget` seconds have passed the remaining cases are logged as
skipped.  --quick runs each twice only.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prysm_amd import _ops, interferogram  # noqa: E402
from prysm_amd import psdsynth_plan as PP  # noqa: E402
from prysm_amd.conf import config  # noqa: E402

SIZE, RMS, A, B, C = 100.0, 5.0, 1e4, 1 / 100, 2.0


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


def t_render(side, batch, rdt):
    """the same formulas as torch operations on the device"""
    dxg = SIZE / (side - 1)
    nu = torch.fft.fftshift(torch.fft.fftfreq(side, dxg, dtype=torch.float64, device='cuda'))
    nu[side // 2] = nu[side // 2 + 1] / 10
    psd = (A / (1 + (torch.hypot(nu[None, :], nu[:, None]) / B) ** C)).to(rdt)
    fs = -2 * float(PP.freq_vector(side, dxg)[0])
    dx = 1 / fs
    area = ((side - 1) * dx) ** 2
    phase = torch.angle(torch.fft.fft2(torch.rand((batch, side, side), dtype=rdt, device='cuda')))
    signal = torch.exp(1j * phase) * torch.sqrt(area * psd)
    z = torch.fft.ifftshift(torch.fft.ifft2(torch.fft.fftshift(signal, dim=(-2, -1))), dim=(-2, -1)).real / (dx * dx)
    g = (torch.arange(side, dtype=rdt, device='cuda') - side // 2) * (SIZE / side)
    z = torch.where(torch.hypot(g[None, :], g[:, None]) <= SIZE / 2, z, torch.full((), math.nan, dtype=rdt, device='cuda'))
    ms = torch.nansum(z * z, dim=(-2, -1)) / torch.isfinite(z).sum(dim=(-2, -1))
    return z * (RMS / torch.sqrt(ms))[:, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.15)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--budget', type=float, default=400)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'psdsynth', 'exp_psdsynth.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    t0 = time.time()
    log = open(a.log, 'w')

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    buf = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    us, _ = timed(buf.zero_, a.quick, a.window)
    store_gbs = buf.numel() / us / 1e3
    del buf
    emit({'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'store_gbs': round(store_gbs, 1)})
    for prec, rdt in ((32, torch.float32), (64, torch.float64)):
        config.precision = prec
        for side in (1024, 4096):
            for batch in (1, 8):
                es = 4 if prec == 32 else 8
                shape = (side, side)
                dxg = SIZE / (side - 1)
                model = (PP.ABC, A, B, C, dxg)
                dx, area, scale = PP.window(PP.freq_vector(side, dxg)[0], shape)
                shift = PP.shifts(shape)
                u = _ops.psd_uniform((batch,) + shape, rdt, 7)
                spectrum = interferogram._forward_spectrum(u)
                field = _ops.fft2(spectrum, direction=1, scale=scale, in_shift=shift, out_shift=shift)
                z, sums = _ops.psd_finish(field, circle=(SIZE / 2, SIZE / side))

                def transforms():
                    _ops.fft2(interferogram._forward_spectrum(u), direction=1, scale=scale, in_shift=shift, out_shift=shift)

                def case(name, fn, ref=None, nbytes=None):
                    rec = {'case': name, 'side': side, 'batch': batch, 'dtype': str(rdt)}
                    if time.time() - t0 > a.budget:
                        emit(dict(rec, skipped='budget'))
                        return
                    us, reps = timed(fn, a.quick, a.window)
                    rec.update(us=round(us, 2), reps=reps)
                    if ref is not None:
                        tus, _ = timed(ref, a.quick, a.window)
                        rec.update(torch_us=round(tus, 2), torch_over_call=round(tus / us, 2))
                    if nbytes is not None:
                        floor = nbytes / (store_gbs * 1e9) * 1e6
                        rec.update(floor_us=round(floor, 2), floor_share=round(floor / us, 3))
                    emit(rec)
                n = batch * side * side
                case('render', lambda: interferogram.render_synthetic_surface(SIZE, side, rms=RMS, mask='circle', seed=7, batch=batch, a=A, b=B, c=C),
                     lambda: t_render(side, batch, rdt))
                case('uniform', lambda: _ops.psd_uniform((batch,) + shape, rdt, 7, out=u), nbytes=n * es)
                case('signal', lambda: _ops.psd_signal(spectrum, area, model=model), nbytes=n * 4 * es)
                case('finish', lambda: _ops.psd_finish(field, circle=(SIZE / 2, SIZE / side), out=z), nbytes=n * 3 * es)
                case('scale', lambda: _ops.psd_scale(z, sums, RMS), nbytes=n * 2 * es)
                case('transforms', transforms)
                del u, spectrum, field, z, sums
                torch.cuda.empty_cache()
    config.precision = 64
    log.close()


if __name__ == '__main__':
    main()
