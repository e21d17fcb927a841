"""Time the image-chain unit (csrc/imagechain.hip) on the device with HIP events.

    python tools/exp_imagechain.py [--window 0.25] [--quick] [--sides 1024 4096] [--budget 900] [--log profiles/imagechain/exp_imagechain.log]

One JSON line per measurement, printed and written to the log.  Square grids of side^2 samples at dx = 0.5, float32 and float64
(config.precision follows, so both paths of a comparison run in the same precision).  Every case is timed against the same formulas
as torch operations:
- `tf_product`: H from smear + jitter + pinhole + pixel + Airy transfer functions.  `us`: convolution.transfer_function on their
  `.spec(...)` records, one launch; `store_gbs` is the rate of its stores (side^2 complex samples) and `store_share` that rate over
  `--hbm-gbs` (default 6290 GB/s, the store rate the README quotes).  `torch_us`: what apply_transfer_functions does with callables in
  front of the chain -- forward_ft_unit for both axes, hypot and atan2 over the grid, each callable as torch operations on the
  maps, the running product, the cast to complex and the roll (the callables are torch formulas: torch.sinc, torch.exp, the
  arccos form of the Airy transform, and J1 from torch.special.bessel_j1).
- `apply`: the whole convolution.apply_transfer_functions call on a real object, records against those torch callables.
- `siemensstar`, `slantededge_crossed`: objects.siemensstar(shape=, dx=) / objects.slantededge(crossed=True, shape=, dx=) against
  the reference's array expressions in torch on stored (r, t) / (x, y) maps; `store_gbs` as above (side^2 real samples).
- `centroid`: psf.centroid_device against (sum d, sum rows d, sum cols d) by torch reductions.
- `fwhm`: psf.fwhm on a displaced Gaussian; the torch side is the resample by torch.nn.functional.grid_sample (bilinear, zero padding)
  and the reference's loop over the rows of the polar map replaced by its vectorised form (argmax over the change mask), ending in
  one host read like the call.
`us` brackets the whole Python call; `torch_over_call` > 1 means the unit's call wins.  A timed batch is as many calls as fill
`--window` seconds (at least 2); batches repeat until two agree within 3 % (at most 5), and the median of three more is reported with
the count as `reps`.  Sizes are visited smallest first; when `--budget` seconds have passed the rest are logged as skipped.  --quick
runs each measurement twice only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prysm_amd import convolution, degradations, detector, objects, psf  # noqa: E402
from prysm_amd.conf import config  # noqa: E402

DX = 0.5
SMEAR, JITTER, PINHOLE, PIXEL, FNO, WVL = (1.3, 0.7), 0.9, 1.1, (0.9, 1.1), 4.0, 0.55


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


def torch_callables():
    """the five transfer functions as torch operations on the frequency maps apply_transfer_functions hands to a callable"""
    ext = 1 / (WVL * FNO)

    def jinc(x):
        return torch.where(x.abs() < 1e-8, torch.full_like(x, 0.5), torch.special.bessel_j1(x) / x)

    def airy_ft(fr):
        s = torch.clamp(fr.abs() / ext, max=1)
        return (2 / np.pi) * (torch.arccos(s) - s * torch.sqrt(1 - s * s))

    return [lambda fx, fy: torch.sinc(fx * SMEAR[0]) * torch.sinc(fy * SMEAR[1]),
            lambda fr: torch.exp(-2 * (np.pi * JITTER * fr) ** 2),
            lambda fr: jinc(fr * (PINHOLE * 2 * np.pi)),
            lambda fx, fy: torch.sinc(fx * PIXEL[0]) * torch.sinc(fy * PIXEL[1]),
            airy_ft]


def records():
    return [degradations.smear_ft.spec(*SMEAR), degradations.jitter_ft.spec(JITTER), objects.pinhole_ft.spec(PINHOLE),
            detector.pixel_ft.spec(*PIXEL), psf.airydisk_ft.spec(FNO, WVL)]


def torch_fwhm(d, dx):
    """estimate_size(metric='fwhm') as torch operations: grid_sample for the resample, the row loop vectorised"""
    ny, nx = d.shape
    dt = d.dtype
    x = (torch.arange(nx, device=d.device, dtype=dt) - nx // 2) * dx
    y = (torch.arange(ny, device=d.device, dtype=dt) - ny // 2) * dx
    _max = max(abs(float(x[0])), abs(float(x[-1])), abs(float(y[0])), abs(float(y[-1])))
    rho = torch.linspace(0, _max, nx, device=d.device, dtype=dt)
    phi = torch.linspace(0, 2 * np.pi, ny, device=d.device, dtype=dt)
    xq, yq = rho[None, :] * torch.cos(phi[:, None]), rho[None, :] * torch.sin(phi[:, None])
    gx = 2 * (xq - x[0]) / (x[-1] - x[0]) - 1
    gy = 2 * (yq - y[0]) / (y[-1] - y[0]) - 1
    polar = torch.nn.functional.grid_sample(d[None, None], torch.stack([gx, gy], dim=-1)[None], mode='bilinear', padding_mode='zeros',
                                            align_corners=True)[0, 0]
    hm = polar.max() / 2
    above = polar > hm
    change = above[:, :-1] != above[:, 1:]
    has = change.any(dim=1)
    i = change.shape[1] - 1 - torch.argmax(change.flip(1).to(torch.uint8), dim=1)
    rows = torch.arange(ny, device=d.device)
    y0, y1 = polar[rows, i], polar[rows, i + 1]
    frac = torch.where(y1 == y0, torch.zeros_like(y0), (hm - y0) / (y1 - y0))
    rc = rho[i] + frac * (rho[i + 1] - rho[i])
    return float((rc * has).sum() / has.sum()) * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sides', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--budget', type=float, default=900.0)
    ap.add_argument('--hbm-gbs', type=float, default=6290.0)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'imagechain', 'exp_imagechain.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    log = open(a.log, 'w')
    t0 = time.time()

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    assert torch.cuda.is_available(), 'exp_imagechain.py needs an MI355X'
    fns, recs = torch_callables(), records()
    try:
        for side in sorted(a.sides):
            for dt in (torch.float32, torch.float64):
                name = str(dt).split('.')[1]
                config.precision = 32 if dt == torch.float32 else 64
                cdt = torch.complex64 if dt == torch.float32 else torch.complex128
                el = 4 if dt == torch.float32 else 8
                head = dict(side=side, dtype=name)
                if time.time() - t0 > a.budget:
                    emit(**head, skipped='budget')
                    continue
                shape = (side, side)
                n = side * side

                def report(op, mine, theirs, nbytes=None, **extra):
                    (us, reps), (tus, treps) = timed(mine, a.quick, a.window), timed(theirs, a.quick, a.window)
                    row = dict(**head, op=op, us=round(us, 1), reps=reps, torch_us=round(tus, 1), torch_reps=treps,
                               torch_over_call=round(tus / us, 2), **extra)
                    if nbytes:
                        gbs = nbytes / us / 1e3
                        row.update(store_gbs=round(gbs, 1), store_share=round(gbs / a.hbm_gbs, 3))
                    emit(**row)

                # H alone: the torch side is apply_transfer_functions' map-by-map path up to the chain, a unit object keeps the chain out
                def torch_H():
                    uy, ux = [convolution.forward_ft_unit(DX, k, shift=True) for k in shape]
                    fx, fy = ux.reshape(1, -1), uy.reshape(-1, 1)
                    fr, ft = torch.hypot(fx, fy), torch.atan2(fy + 0 * fx, fx + 0 * fy)
                    H = None
                    for f in fns:
                        names = f.__code__.co_varnames[:f.__code__.co_argcount]
                        tf = f(**{k: v for k, v in (('fx', fx), ('fy', fy), ('fr', fr), ('ft', ft)) if k in names})
                        tf = torch.broadcast_to(tf, shape)
                        H = tf if H is None else H * tf
                    return convolution._ifftshift2(H.to(cdt)).contiguous()

                H, Ht = convolution.transfer_function(shape, DX, recs, shift=True, dtype=cdt), torch_H()
                diff = float((H - Ht).abs().max())
                report('tf_product', lambda: convolution.transfer_function(shape, DX, recs, shift=True, dtype=cdt), torch_H, nbytes=2 * n * el,
                       max_diff=diff)
                del H, Ht
                obj = torch.rand(shape, dtype=dt, device='cuda')
                o1, o2 = convolution.apply_transfer_functions(obj, DX, recs, shift=True), convolution.apply_transfer_functions(obj, DX, fns, shift=True)
                diff = float((o1 - o2).abs().max() / o2.abs().max())
                del o1, o2
                report('apply', lambda: convolution.apply_transfer_functions(obj, DX, recs, shift=True),
                       lambda: convolution.apply_transfer_functions(obj, DX, fns, shift=True), rel_diff=diff)
                del obj
                torch.cuda.empty_cache()

                gdx = 2.0 / side
                v = (torch.arange(side, dtype=dt, device='cuda') - side // 2) * gdx
                y, x = torch.meshgrid(v, v, indexing='ij')
                r, t = torch.hypot(x, y), torch.atan2(y, x)

                def torch_star():
                    arr = (0.9 * torch.cos(36 / 2 * t) + 1) / 2
                    arr[(r > 0.8) | (r < 0.1)] = 0
                    arr[arr < 0.5] = (1 - 0.9) / 2
                    arr[arr > 0.5] = 1 - (1 - 0.9) / 2
                    return arr

                def torch_crossed():
                    ang = np.radians(4)
                    m = x * np.cos(ang) - y * np.sin(ang) > 0
                    ur = m & torch.rot90(m)
                    m = ur | torch.rot90(ur, 2)
                    arr = torch.full_like(x, 1 - (1 - 0.9) / 2)
                    arr[m] = (1 - 0.9) / 2
                    return arr

                report('siemensstar', lambda: objects.siemensstar(None, None, 36, oradius=0.8, iradius=0.1, shape=shape, dx=gdx), torch_star,
                       nbytes=n * el, differing=int((objects.siemensstar(None, None, 36, oradius=0.8, iradius=0.1, shape=shape, dx=gdx) != torch_star()).sum()))
                report('slantededge_crossed', lambda: objects.slantededge(shape=shape, dx=gdx, crossed=True), torch_crossed, nbytes=n * el,
                       differing=int((objects.slantededge(shape=shape, dx=gdx, crossed=True) != torch_crossed()).sum()))
                del r, t
                d = torch.exp(-((x - 0.1) ** 2 + (y + 0.05) ** 2) / (2 * 0.2 ** 2))
                rows_, cols_ = torch.arange(side, device='cuda', dtype=torch.float64)[:, None], torch.arange(side, device='cuda', dtype=torch.float64)[None, :]

                def torch_centroid():
                    d64 = d.to(torch.float64)
                    s = d64.sum()
                    return torch.stack([(rows_ * d64).sum() / s, (cols_ * d64).sum() / s])

                report('centroid', lambda: psf.centroid_device(d), torch_centroid, max_diff=float((psf.centroid_device(d) - torch_centroid()).abs().max()))
                del x, y
                report('fwhm', lambda: psf.fwhm(d, dx=gdx), lambda: torch_fwhm(d, gdx), diff=abs(psf.fwhm(d, dx=gdx) - torch_fwhm(d, gdx)))
                del d
                torch.cuda.empty_cache()
    finally:
        config.precision = 64


if __name__ == '__main__':
    main()
