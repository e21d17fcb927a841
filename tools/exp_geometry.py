"""Time prysm_amd.geometry.render on the device with HIP events after warm-up, next to a plain torch fill of the same output (the
store-rate ceiling) and to the same aperture composed from the single-shape functions with torch.minimum / maximum.

    python tools/exp_geometry.py [--reps 20] [--quick] [--sizes 1024 2048 4096]

One JSON line per (size, precision, aperture): (a) `circle`, (b) `four` -- circle & hexagon, minus a central obscuration, minus a
three-vane spider, (c) `hex18` -- a union of 18 hexagons; each as mask and as coverage, in grid mode (coordinates from the pixel
index) and pointwise mode (coordinate arrays read).  us: microseconds per call.  render_over_fill = render time / fill time of the
same output; composed_over_render = time of the composed single-shape calls (coordinates given, distance combined with torch, then
`<= 0` or antialias) / render time in grid mode.  Before the timings, one line per mask case with the measured distance error of the
kernel against the numpy walk of its table (every 37th row) and the share of pixels inside the float band that the mask rule leaves
out.  --quick runs each configuration a few times only (for a rocprofv3 --kernel-trace --stats run).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prysm_amd import geometry as G, geometry_plan as GP, coordinates as K  # noqa: E402

S = G.shape
FOUR = dict(r_outer=3.0137, hex_radius=2.7319, hex_rotation=11.3, r_inner=0.7113, vanes=3, vane_width=0.1371, vane_rotation=13.7)


def hex_centers(pitch=1.0137):
    cs = []
    for q in range(-2, 3):
        for r in range(-2, 3):
            if (q or r) and abs(q + r) <= 2:
                cs.append((pitch * (q + r / 2) + 0.0113, pitch * r * np.sqrt(3) / 2 - 0.0071))
    return cs


def apertures():
    P = FOUR
    four = S.circle(P['r_outer']).intersect(S.regular_polygon(6, P['hex_radius'], rotation=P['hex_rotation'])) \
        .subtract(S.circle(P['r_inner'])).subtract(S.spider(P['vanes'], P['vane_width'], rotation=P['vane_rotation']))
    hex18 = S.union(*[S.regular_polygon(6, 0.5713, center=c, rotation=3.7) for c in hex_centers()])
    return dict(circle=S.circle(P['r_outer']), four=four, hex18=hex18)


def composed(name, x, y, r):
    """the same distance from the single-shape calls, one full-array sweep per combination"""
    P = FOUR
    if name == 'circle':
        return G.circle_sdf(P['r_outer'], r)
    if name == 'four':
        d = G.intersect(G.circle_sdf(P['r_outer'], r), G.regular_polygon_sdf(6, P['hex_radius'], x, y, rotation=P['hex_rotation']))
        d = G.subtract(d, G.circle_sdf(P['r_inner'], r))
        return G.subtract(d, G.spider_sdf(P['vanes'], P['vane_width'], x, y, rotation=P['vane_rotation']))
    return G.union(*[G.regular_polygon_sdf(6, 0.5713, x, y, center=c, rotation=3.7) for c in hex_centers()])


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def accuracy(name, ap, N, dx):
    """distance error of the kernel against the numpy walk (every 37th row) and the share the mask rule leaves out, both precisions"""
    rows = np.arange(0, N, 37)
    xv, yv = GP.grid_axis(N, dx, np.float64), GP.grid_axis(N, dx, np.float64)
    want = GP.evaluate(GP.plan(ap, np.float64)[0], xv[None, :], yv[rows][:, None])
    top = np.max(np.abs(want))
    rec = dict(check='accuracy', N=N, aperture=name)
    for dt, tol in ((torch.float64, 1e-12), (torch.float32, 5e-5)):
        d = G.render(ap, shape=(N, N), dx=dx, output='sdf', dtype=dt).cpu().numpy()[rows]
        m = G.render(ap, shape=(N, N), dx=dx, dtype=dt).cpu().numpy()[rows]
        judged = np.abs(want) > tol * top
        key = str(dt).split('.')[-1]
        rec[key] = dict(distance_error=float(np.max(np.abs(d - want)) / top), left_out_share=float(1 - judged.mean()),
                        mask_mismatches_outside_band=int(np.sum(m[judged] != (want <= 0)[judged])))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    a = ap.parse_args()
    if a.quick:
        a.reps, a.warmup = 2, 1
    torch.cuda.set_device(0)
    aps = apertures()
    for N in a.sizes:
        dx = 6.5137 / N
        for name, node in aps.items():
            accuracy(name, node, N, dx)
    for N in a.sizes:
        dx = 6.5137 / N
        for dt in (torch.float32, torch.float64):
            xv, yv = (torch.arange(N, dtype=dt, device='cuda') - N // 2) * dx, (torch.arange(N, dtype=dt, device='cuda') - N // 2) * dx
            y, x = torch.meshgrid(yv, xv, indexing='ij')
            x, y = x.contiguous(), y.contiguous()
            r = torch.hypot(x, y)
            fm, ff = torch.empty((N, N), dtype=torch.bool, device='cuda'), torch.empty((N, N), dtype=dt, device='cuda')
            for name, node in aps.items():
                fns = dict(
                    fill_mask=lambda: fm.fill_(True),
                    fill_float=lambda: ff.fill_(0.5),
                    grid_mask=lambda: G.render(node, shape=(N, N), dx=dx, dtype=dt, out=fm),
                    grid_coverage=lambda: G.render(node, shape=(N, N), dx=dx, antialias=True, dtype=dt, out=ff),
                    pointwise_mask=lambda: G.render(node, x=x, y=y, out=fm),
                    pointwise_coverage=lambda: G.render(node, x=x, y=y, antialias=dx, out=ff),
                    composed_mask=lambda: composed(name, x, y, r) <= 0,
                    composed_coverage=lambda: G.antialias(composed(name, x, y, r), dx),
                )
                for fn in fns.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                us = {k: timed(fn, max(2, a.reps // 4) if k.startswith('composed') else a.reps) for k, fn in fns.items()}
                rec = dict(N=N, dtype=str(dt).split('.')[-1], aperture=name, steps=int(GP.plan(node, np.float64).shape[1]),
                           us={k: round(v, 1) for k, v in us.items()})
                for mode in ('grid', 'pointwise'):
                    rec[f'{mode}_mask_over_fill'] = round(us[f'{mode}_mask'] / us['fill_mask'], 2)
                    rec[f'{mode}_coverage_over_fill'] = round(us[f'{mode}_coverage'] / us['fill_float'], 2)
                rec['composed_mask_over_render'] = round(us['composed_mask'] / us['grid_mask'], 1)
                rec['composed_coverage_over_render'] = round(us['composed_coverage'] / us['grid_coverage'], 1)
                print(json.dumps(rec), flush=True)
            del x, y, r, fm, ff
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
