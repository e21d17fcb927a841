"""Time the interferogram unit (csrc/interferogram.hip) on the device with HIP events.

    python tools/exp_interferogram.py [--window 0.15] [--quick] [--budget 400] [--log profiles/interferogram/exp_interferogram.log]

One JSON line per measurement, printed and written to the log; float32 and float64 (config.precision follows), 1024^2 and 4096^2.  The
data is the golden case scaled up: noise on a tilted, curved surface with a piston of 1000, NaN outside a disc and in a frame.  Every
case is timed against the same formulas as torch operations on the device (`torch_us`; `torch_over_call` > 1 means the unit's call
wins), host reads included on both sides:
- `stats`: pm_ifg_stats alone, no host read.  `floor_us` is ONE read of the N^2 s bytes at the store rate this run measures (the first
  line of the log: `store_gbs`, a zero fill of 1 GiB); the call reads the data twice (the variance is two-pass), so `floor_share` =
  2 floor_us / us.
- `rms`, `std`: the util call with its host read of the record.
- `clean`: crop + remove_piston + remove_tiptilt + remove_power on a fresh Interferogram of the same tensor.
- `spike_clip`, `psd`, `bandlimited_rms`, `filter_lp`: the methods, on the cleaned and filled data.
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

from prysm_amd import _ops, util  # noqa: E402
from prysm_amd.conf import config  # noqa: E402
from prysm_amd.interferogram import Interferogram  # noqa: E402


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


def surface(side, dtype):
    """the golden case at `side` samples: (data with NaN, dx)"""
    dx = 4.0 / side
    v = (torch.arange(side, dtype=torch.float64, device='cuda') - side // 2) * dx
    x, y = v[None, :], v[:, None]
    g = torch.Generator(device='cuda').manual_seed(3)
    z = 5 * torch.randn((side, side), dtype=torch.float64, device='cuda', generator=g) + 30 * x - 20 * y + 8 * (x * x + y * y) + 1000
    z[torch.rand((side, side), device='cuda', generator=g) < 1e-5] += 200
    z[torch.hypot(x, y).expand(side, side) > 1.7] = math.nan
    z[:, :side // 16] = math.nan
    z[-side // 20:, :] = math.nan
    return z.to(dtype), dx


# ---------------------------------------------------------------- the same formulas as torch operations
def t_rms(z):
    return torch.sqrt((z[torch.isfinite(z)] ** 2).mean()).item()


def t_std(z):
    return z[torch.isfinite(z)].std(unbiased=False).item()


def t_clean(z, dx):
    fin = torch.isfinite(z)
    rows, cols = fin.any(dim=1).nonzero(), fin.any(dim=0).nonzero()
    r0, r1, c0, c1 = (int(v) for v in torch.stack((rows[0, 0], rows[-1, 0], cols[0, 0], cols[-1, 0])).tolist())
    z = z[r0:r1 + 1, c0:c1 + 1]
    fin = fin[r0:r1 + 1, c0:c1 + 1]
    m, n = z.shape
    z = z - z[fin].mean()
    x = ((torch.arange(n, dtype=z.dtype, device=z.device) - n // 2) * dx).expand(m, n)
    y = ((torch.arange(m, dtype=z.dtype, device=z.device) - m // 2) * dx)[:, None].expand(m, n)
    c = torch.linalg.lstsq(torch.stack((x[fin], y[fin]), dim=1), z[fin][:, None]).solution
    z = z - (c[0] * x + c[1] * y)
    xx = torch.linspace(-1, 1, n, dtype=z.dtype, device=z.device).expand(m, n)
    yy = torch.linspace(-1, 1, m, dtype=z.dtype, device=z.device)[:, None].expand(m, n)
    rho2 = xx * xx + yy * yy
    c = torch.linalg.lstsq(torch.stack((rho2[fin], torch.ones_like(rho2[fin])), dim=1), z[fin][:, None]).solution
    return torch.where(fin, z - c[0] * rho2, z)


def t_spike_clip(z):
    std = z[torch.isfinite(z)].std(unbiased=False)
    z[z.abs() > 3 * std] = math.nan
    return z


def t_psd(z, dx):
    m, n = z.shape
    w = torch.outer(torch.hann_window(m, periodic=False, dtype=z.dtype, device=z.device), torch.hann_window(n, periodic=False, dtype=z.dtype, device=z.device))
    ft = torch.fft.ifftshift(torch.fft.fft2(torch.fft.fftshift(z * w)))
    return (ft.real ** 2 + ft.imag ** 2) / ((w * w).sum() * (1 / dx) ** 2)


def t_band(z, dx, flow, fhigh):
    p = t_psd(z, dx)
    m, n = p.shape
    ux = torch.fft.fftshift(torch.fft.fftfreq(n, dx, dtype=torch.float64, device=z.device))
    uy = torch.fft.fftshift(torch.fft.fftfreq(m, dx, dtype=torch.float64, device=z.device))
    r = torch.hypot(ux[None, :], uy[:, None])
    work = torch.where((r < flow) | (r > fhigh), torch.zeros_like(p), p)
    d = 1 / (m * dx)
    return torch.sqrt(torch.trapezoid(torch.trapezoid(work, dx=d, dim=0), dx=d, dim=0)).item()


def t_filter_lp(z, dx, fc):
    m, n = z.shape
    x = (torch.arange(n, dtype=z.dtype, device=z.device) - n // 2) * dx
    y = (torch.arange(m, dtype=z.dtype, device=z.device) - m // 2) * dx
    r = torch.hypot(x[None, :], y[:, None])
    nn = torch.hypot((torch.arange(n, dtype=z.dtype, device=z.device) - n // 2)[None, :], (torch.arange(m, dtype=z.dtype, device=z.device) - m // 2)[:, None])
    k = min(m, n)
    w = torch.cos(math.pi / k * nn) ** 2
    w[nn > k // 2] = 0
    fcn = fc / (1 / (2 * dx))
    a = r * (math.pi * fcn / dx)
    h = torch.where(a.abs() < 1e-8, torch.full_like(a, 0.5), torch.special.bessel_j1(a) / a) * (fcn ** 2 * math.pi / 2)
    H = torch.fft.fft2(w * h).abs()
    return torch.fft.ifft2(torch.fft.fft2(z) * H).real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.15)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--budget', type=float, default=400)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'interferogram', 'exp_interferogram.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    t0 = time.time()
    log = open(a.log, 'w')

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    def over():
        return time.time() - t0 > a.budget

    buf = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    us, _ = timed(buf.zero_, a.quick, a.window)
    store_gbs = buf.numel() / us / 1e3
    del buf
    emit({'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'store_gbs': round(store_gbs, 1)})
    for prec, rdt in ((32, torch.float32), (64, torch.float64)):
        config.precision = prec
        for side in (1024, 4096):
            z, dx = surface(side, rdt)
            es = z.element_size()

            def case(name, fn, ref, **more):
                if over():
                    emit({'case': name, 'side': side, 'dtype': str(rdt), 'skipped': 'budget'})
                    return
                us, reps = timed(fn, a.quick, a.window)
                tus, _ = timed(ref, a.quick, a.window)
                rec = {'case': name, 'side': side, 'dtype': str(rdt), 'us': round(us, 2), 'torch_us': round(tus, 2), 'torch_over_call': round(tus / us, 2),
                       'reps': reps}
                rec.update({k: (v(us) if callable(v) else v) for k, v in more.items()})
                emit(rec)
            floor = side * side * es / (store_gbs * 1e9) * 1e6
            case('stats', lambda: _ops.ifg_stats(z), lambda: (t_rms(z), t_std(z)), floor_us=round(floor, 2), floor_share=lambda us: round(2 * floor / us, 3))
            case('rms', lambda: util.rms(z), lambda: t_rms(z))
            case('std', lambda: util.std(z), lambda: t_std(z))
            work, twork = z.clone(), z.clone()
            case('clean', lambda: Interferogram(work, dx=dx).crop().remove_piston().remove_tiptilt().remove_power(), lambda: t_clean(twork, dx))
            I = Interferogram(work, dx=dx).crop().remove_piston().remove_tiptilt().remove_power()
            flat = t_clean(twork, dx).contiguous()
            case('spike_clip', lambda: I.spike_clip(3), lambda: t_spike_clip(flat))
            # the spectra on the whole side x side array (the cropped disc has whatever size its bounding box has), piston taken off, NaN as 0
            flat = torch.nan_to_num(z, nan=1000.0) - 1000
            I = Interferogram(flat.clone(), dx=dx)
            case('psd', lambda: I.psd(), lambda: t_psd(flat, dx), shape=list(I.shape))
            case('bandlimited_rms', lambda: I.bandlimited_rms(flow=1.0, fhigh=20.0), lambda: t_band(flat, dx, 1.0, 20.0))
            keep = I.data.clone()

            def filt():
                I.data = keep
                I.filter(10.0, 'lp')
            case('filter_lp', filt, lambda: t_filter_lp(flat, dx, 10.0))
            del z, work, twork, flat, keep, I
            torch.cuda.empty_cache()
    config.precision = 64
    log.close()


if __name__ == '__main__':
    main()
