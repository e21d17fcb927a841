"""Time the wavefront-sensor unit (csrc/sensors.hip) on the device with HIP events.

    python tools/exp_sensors.py [--window 0.25] [--quick] [--budget 400] [--log profiles/sensors/exp_sensors.log]

One JSON line per measurement, printed and written to the log; float32 and float64 (config.precision follows).  Every case is timed
against the same formulas as torch operations:
- `psi`: degroot_formalism_psi with 5 (SCHWIDER) and 13 (ZYGO_THIRTEEN_FRAME) separately allocated frames at 1024^2 and 4096^2, float
  frames and uint16 frames.  `floor_us` is (K + 1) N^2 s bytes (s: the frame's element for the K reads, the output's for the store)
  at `--hbm-gbs` (default 6290 GB/s, the store rate the README quotes) and `floor_share` = floor_us / us.  `torch_us`: the reference's
  route in torch -- torch.stack of the frames, two tensordot with the weights, atan2 (integer frames are cast to the output dtype
  first, which the reference does not do and is wrong without).
- `shack_hartmann`: 64 x 64 lenslets on 2048^2 and 4096^2 (shape= / dx=), against the reference's double loop over lenslet windows
  written in torch on stored coordinate maps (4096 iterations).
- `pspdi`, `sri`: one forward_model at 1024^2 with the default arm sizes; `pointwise_us` is the time of the unit's pointwise launches
  alone (grating + combination; fibre scale + combination) and `executor_us` the rest; `torch_pointwise_us` the same steps as torch
  operations.
`us` brackets the whole Python call; `torch_over_call` > 1 means the unit's call wins.  A timed batch is as many calls as fill
`--window` seconds (at least 2); batches repeat until two agree within 3 % (at most 5), and the median of three more is reported with
the count as `reps`.  When `--budget` seconds have passed the remaining cases are logged as skipped.  --quick runs each twice only.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prysm_amd import _ops, geometry  # noqa: E402
from prysm_amd.conf import config  # noqa: E402
from prysm_amd.coordinates import make_xy_grid  # noqa: E402
from prysm_amd.x import pdi, psi, shack_hartmann as shmod, sri  # noqa: E402


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


def sh_loop_torch(pitch, n, efl, wavelength, x, y):
    """the reference's loop (shack_hartmann.py:102-117) with torch operations and the rectangle written out"""
    dx = float(x[0, 1] - x[0, 0])
    spl = int(pitch / dx + 1)
    c = torch.arange(-(n // 2), -(n // 2) + n, dtype=torch.float64) * pitch
    cx, cy = math.ceil(x.shape[1] / 2), math.ceil(x.shape[0] / 2)
    total = torch.zeros_like(x)
    for yy in c.tolist():
        for xx in c.tolist():
            ox, oy = cx + int(xx / dx) - spl, cy + int(yy / dx) - spl
            win = (slice(max(oy, 0), max(min(oy + 2 * spl, x.shape[0]), 0)), slice(max(ox, 0), max(min(ox + 2 * spl, x.shape[1]), 0)))
            lx, ly = x[win] - xx, y[win] - yy
            rsq = lx * lx + ly * ly
            total[win] += rsq / (2 * efl) * ((lx[0:1, :].abs() - pitch / 2 <= 0) & (ly[:, 0:1].abs() - pitch / 2 <= 0))
    return torch.exp((-1j * 2 * np.pi / (wavelength / 1e3)) * total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--budget', type=float, default=400)
    ap.add_argument('--hbm-gbs', type=float, default=6290.0)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'sensors', 'exp_sensors.log'))
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

    emit({'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hbm_gbs': a.hbm_gbs})
    rng = np.random.default_rng(1)
    for prec, rdt in ((32, torch.float32), (64, torch.float64)):
        config.precision = prec
        for side in (1024, 4096):
            for sch, name in ((psi.SCHWIDER, 'schwider5'), (psi.ZYGO_THIRTEEN_FRAME, 'zygo13')):
                for fdt in (rdt, torch.uint16):
                    K = len(sch.s)
                    if over():
                        emit({'case': 'psi', 'side': side, 'frames': K, 'skipped': 'budget'})
                        continue
                    if fdt == torch.uint16:
                        fr = [torch.from_numpy(rng.integers(0, 4000, (side, side)).astype(np.uint16)).cuda() for _ in range(K)]
                    else:
                        fr = [torch.rand((side, side), dtype=rdt, device='cuda') * 4000 for _ in range(K)]
                    us, reps = timed(lambda: psi.degroot_formalism_psi(fr, sch), a.quick, a.window)
                    ws, wc = (torch.as_tensor(np.asarray(v, dtype=np.float64), device='cuda').to(rdt) for v in (sch.s, sch.c))

                    def ref():
                        g = torch.stack(fr)
                        g = g.to(rdt) if g.dtype != rdt else g
                        return torch.atan2(torch.tensordot(ws, g, dims=1), torch.tensordot(wc, g, dims=1))
                    tus, _ = timed(ref, a.quick, a.window)
                    nbytes = side * side * (K * fr[0].element_size() + torch.empty(0, dtype=rdt).element_size())
                    floor = nbytes / (a.hbm_gbs * 1e9) * 1e6
                    emit({'case': 'psi', 'scheme': name, 'frames': K, 'side': side, 'frame_dtype': str(fdt), 'out_dtype': str(rdt), 'us': round(us, 2),
                          'floor_us': round(floor, 2), 'floor_share': round(floor / us, 3), 'torch_us': round(tus, 2),
                          'torch_over_call': round(tus / us, 2), 'reps': reps})
                    del fr
        for side in (2048, 4096):
            if over():
                emit({'case': 'shack_hartmann', 'side': side, 'skipped': 'budget'})
                continue
            pitch, dx = 1.0, 64.0 / side
            us, reps = timed(lambda: shmod.shack_hartmann(pitch, 64, 50.0, 0.5, shape=(side, side), dx=dx), a.quick, a.window)
            x, y = make_xy_grid(side, dx=dx)
            tus = batch_ms(lambda: sh_loop_torch(pitch, 64, 50.0, 0.5, x, y), 1) * 1e3
            tus = min(tus, batch_ms(lambda: sh_loop_torch(pitch, 64, 50.0, 0.5, x, y), 1) * 1e3)
            emit({'case': 'shack_hartmann', 'lenslets': '64x64', 'side': side, 'dtype': str(rdt), 'us': round(us, 2),
                  'store_gbs': round(side * side * 2 * x.element_size() / us / 1e3, 1), 'torch_us': round(tus, 1),
                  'torch_over_call': round(tus / us, 1), 'reps': reps})
            del x, y
        if over():
            emit({'case': 'interferometers', 'skipped': 'budget'})
            continue
        side, epd = 1024, 10.0
        x, y = make_xy_grid(side, diameter=epd)
        r = torch.sqrt(x * x + y * y)
        cdt = torch.complex64 if prec == 32 else torch.complex128
        field = (geometry.circle(epd / 2, r).to(rdt) * torch.exp(1j * 0.3 * (x / epd) ** 3)).to(cdt)
        for gt in ('sin_amp', 'ronchi'):
            p = pdi.PSPDI(x, y, 100.0, epd, 0.6328, grating_type=gt)
            us, reps = timed(lambda: p.forward_model(field, phase_shift=1.3), a.quick, a.window)
            p.forward_model(field, phase_shift=1.3)
            ra, ta = p.ref_beam.data, p.test_beam.data
            sh = 1.3 / (2 * np.pi) * p.grating_period

            def point():
                pdi._grating(*p._grating, p.x, shift=sh, field=field)
                _ops.beam_combine(ra, 1.0, ta, 1.0)

            def point_torch():
                xs = p.x + sh
                if gt == 'ronchi':
                    xw = torch.remainder(xs, p.grating_period)
                    g = torch.where(xw < 0.5 * p.grating_period, 1.0, 0.0)
                    g = torch.where(xw.abs() < torch.finfo(rdt).eps, 0.5, g)
                else:
                    g = 1 - (torch.sin(16 * np.pi / (epd / 2) * xs) + 1) / 2 * 0.1
                i = field * g
                tot = ra + ta
                return i, tot.real ** 2 + tot.imag ** 2
            pus, _ = timed(point, a.quick, a.window)
            tpus, _ = timed(point_torch, a.quick, a.window)
            emit({'case': 'pspdi', 'grating': gt, 'side': side, 'dtype': str(rdt), 'us': round(us, 2), 'pointwise_us': round(pus, 2),
                  'executor_us': round(us - pus, 2), 'torch_pointwise_us': round(tpus, 2), 'torch_over_call': round(tpus / pus, 2), 'reps': reps})
        s = sri.SelfReferencedInterferometer(x, y, 100.0, epd, 0.6328)
        us, reps = timed(lambda: s.forward_model(field, phase_shift=0.3), a.quick, a.window)
        ref = sri.to_photonic_fiber_and_back(sri.WF(field, 0.6328, s.dx), s.efl, s.Efib, s.dxfib, s.Ifibsum, executor=s._executor((side, side)))
        pw, eta = torch.ones(1, dtype=rdt, device='cuda'), torch.full((1,), 0.2, dtype=rdt, device='cuda')
        efib = s.Efib.to(rdt)

        def point():
            _ops.fiber_scale(efib, pw, eta, 0.3)
            _ops.beam_combine(ref.data, s.ref_r, field, s.test_t)

        def point_torch():
            e = efib * (pw * eta) ** 0.5 * complex(math.cos(0.3), math.sin(0.3))
            tot = ref.data * s.ref_r + field * s.test_t
            return e, tot.real ** 2 + tot.imag ** 2
        pus, _ = timed(point, a.quick, a.window)
        tpus, _ = timed(point_torch, a.quick, a.window)
        emit({'case': 'sri', 'side': side, 'dtype': str(rdt), 'us': round(us, 2), 'pointwise_us': round(pus, 2), 'executor_us': round(us - pus, 2),
              'torch_pointwise_us': round(tpus, 2), 'torch_over_call': round(tpus / pus, 2), 'reps': reps})
        del x, y, r, field
    config.precision = 64
    log.close()


if __name__ == '__main__':
    main()
