"""Time the masked modal fits (csrc/modalfit.hip) on the device with HIP events.

    python tools/exp_modalfit.py [--window 0.15] [--quick] [--budget 400] [--log profiles/modalfit/exp_modalfit.log]

One JSON line per measurement, printed and written to the log; float32 and float64, 1024^2 and 4096^2, K = 4, 37 and 128 stored planes
of unit normal noise (the passes do the same work whatever the planes hold) and a measurement that is NaN outside a disc and on 5 % of
the pixels.  `torch_us` is the same formula as torch operations on the device; `torch_over_call` > 1 means the unit's call wins.
- `gram`: pm_modes_gram alone (G, b for one vector and the count; two launches), no host read.  `floor_us` is ONE read of the
  (K + 1) N^2 s bytes at the store rate this run measures (the first line of the log: `store_gbs`, a zero fill of 1 GiB),
  `floor_share` = floor_us / us.  `tflops` counts the useful products and sums, 2 (K (K + 1) / 2 + K) per point; the kernel
  multiplies whole 16-blocks, `tflops_issued` counts those.
- `lstsq`: polynomials.lstsq against torch.linalg.lstsq on the gathered columns (K up to 37: the gathered copy of 128 planes and its
  factorisation do not fit the budget of a run and are logged as skipped when they do not).
- `orthogonalize`: polynomials.orthogonalize_modes against torch.linalg.qr of the gathered columns scattered back.
- `fit1`, `fit8`: a prepared ModalFit.fit of 1 and 8 frames against torch.linalg.lstsq with as many right-hand sides.
- `pvr`: Interferogram.pvr against the same steps as torch operations (K is 37 by definition; logged once per size and precision).
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

from prysm_amd import _lib as L  # noqa: E402
from prysm_amd.conf import config  # noqa: E402
from prysm_amd.interferogram import Interferogram  # noqa: E402
from prysm_amd.polynomials import fitting, fringe_to_nm, lstsq, orthogonalize_modes, prepare_lstsq, zernike_nm_seq  # noqa: E402


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


def measurement(side, dtype, frames=1):
    v = (torch.arange(side, dtype=torch.float64, device='cuda') - side // 2) * (2.0 / side)
    r = torch.hypot(v[None, :], v[:, None])
    g = torch.Generator(device='cuda').manual_seed(3)
    z = torch.randn((frames, side, side), dtype=torch.float64, device='cuda', generator=g)
    bad = (r > 1) | (torch.rand((side, side), device='cuda', generator=g) < 0.05)
    z[:, bad] = math.nan
    return z.to(dtype), ~bad


# ---------------------------------------------------------------- the same formulas as torch operations
def t_lstsq(modes, data):
    fin = torch.isfinite(data[0])
    A = modes[:, fin].T
    return torch.linalg.lstsq(A, data[:, fin].T).solution


def t_orthogonalize(modes, mask):
    Q, R = torch.linalg.qr(modes[:, mask].T)
    out = torch.zeros_like(modes)
    out[:, mask] = (Q * torch.sign(torch.diagonal(R))).T
    return out


def t_pvr(z, r, t, nms):
    rmax = r[r.shape[0] - 1, r.shape[1] // 2]
    rn = r / rmax
    data = torch.where(rn > 1, torch.full_like(z, math.nan), z)
    basis = zernike_nm_seq(nms, rn, t, norm=False)
    c = t_lstsq(basis, data[None])[:, 0]
    proj = torch.where(rn > 1, torch.full_like(z, math.nan), torch.tensordot(c, basis, dims=1))
    res = data - proj
    pf, rf = proj[torch.isfinite(proj)], res[torch.isfinite(res)]
    return (pf.max() - pf.min()).item() + 3 * torch.sqrt((rf * rf).mean()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.15)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--budget', type=float, default=400)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'modalfit', 'exp_modalfit.log'))
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
    nms = [fringe_to_nm(j) for j in range(1, 38)]
    for prec, rdt in ((32, torch.float32), (64, torch.float64)):
        config.precision = prec
        for side in (1024, 4096):
            z8, mask = measurement(side, rdt, 8)
            z = z8[:1]
            es = z.element_size()
            n2 = side * side

            def case(name, K, fn, ref, **more):
                if over():
                    emit({'case': name, 'K': K, 'side': side, 'dtype': str(rdt), 'skipped': 'budget'})
                    return
                us, reps = timed(fn, a.quick, a.window)
                rec = {'case': name, 'K': K, 'side': side, 'dtype': str(rdt), 'us': round(us, 2), 'reps': reps}
                if ref is not None and not over():
                    tus, _ = timed(ref, True, a.window)      # the torch formulation runs for milliseconds to seconds: two calls
                    rec.update(torch_us=round(tus, 2), torch_over_call=round(tus / us, 2))
                rec.update({k: (v(us) if callable(v) else v) for k, v in more.items()})
                emit(rec)

            for K in (4, 37, 128):
                g = torch.Generator(device='cuda').manual_seed(K)
                modes = torch.randn((K, side, side), dtype=rdt, device='cuda', generator=g)
                rec = fitting._new_record(K, 1, modes.device)
                floor = (K + 1) * n2 * es / (store_gbs * 1e9) * 1e6
                useful = 2.0 * (K * (K + 1) / 2 + K) * n2
                KB = (K + 15) // 16
                issued = 2.0 * 256 * (KB * (KB + 1) / 2 + KB) * n2
                case('gram', K, lambda: fitting._gram(modes, L.PM_MODES_GRAM | L.PM_MODES_RHS, rec, z.reshape(1, -1), None, True), None,
                     floor_us=round(floor, 2), floor_share=lambda us: round(floor / us, 3), tflops=lambda us: round(useful / us / 1e6, 2),
                     tflops_issued=lambda us: round(issued / us / 1e6, 2))
                heavy = K > 37 and side > 1024       # the gathered (pixels x 128) copy and its factorisation: seconds per call
                case('lstsq', K, lambda: lstsq(modes, z[0]), None if heavy else (lambda: t_lstsq(modes, z)))
                case('orthogonalize', K, lambda: orthogonalize_modes(modes, mask), None if heavy else (lambda: t_orthogonalize(modes, mask)))
                fit = prepare_lstsq(modes, mask)
                zf = torch.nan_to_num(z8, nan=0.0)
                case('fit1', K, lambda: fit.fit(zf[0]), None if heavy else (lambda: torch.linalg.lstsq(modes[:, mask].T, zf[:1][:, mask].T)))
                case('fit8', K, lambda: fit.fit(zf), None if heavy else (lambda: torch.linalg.lstsq(modes[:, mask].T, zf[:, mask].T)))
                del modes, fit, zf, rec
                torch.cuda.empty_cache()
            I = Interferogram(z[0].clone(), dx=2.0 / side)
            r, t = I.r, I.t
            case('pvr', 37, lambda: I.pvr(), lambda: t_pvr(z[0], r, t, nms))
            del z8, z, mask, I
            torch.cuda.empty_cache()
    config.precision = 64
    log.close()


if __name__ == '__main__':
    main()
