"""Time prysm_amd.x.raytracing.raytrace on the device with HIP events, after a run-in until batch times stop drifting (DESIGN.md
section 5).

    python tools/exp_raytrace.py [--reps 20] [--window 0.25] [--quick] [--log profiles/raytrace/exp_raytrace.log]

One JSON line per configuration, printed and written to the log.  2^20 rays on a 1024 x 1024 grid, float32 and float64, with and
without history, through prepared prescriptions (tests/raytrace_common.py CASES):
- `A`: the mixed lens (sphere, conic, even asphere, tilted plane, mirror, evaluation plane), half-width 11 so that nearly every ray
  is valid;
- `D`: the steep aspheres, half-width 22 at 8 degrees: Newton failures and the Lipschitz rescue;
- `A_analytic`: A without its asphere.  This one is also timed as the SAME steps written as torch operations on the same device
  (`torch_us`) -- the only honest torch formulation without a host loop over Newton iterations.  torch_over_call > 1 means the
  kernel's whole call wins.
Two times per configuration: `call_us` brackets the whole `raytrace` call of a prepared prescription (the launch, the five output
allocations, the composition of the complex status), `kernel_us` brackets pm_rt_trace alone on outputs allocated once.  A timed
batch is as many calls as fill `--window` seconds (at least `--reps`; the count is logged as `reps`), batches repeat until two
agree within 3 %, and the median of three more is reported.  The torch formulation has its constants (vertices, rotations) on the
device before it is timed, as the prepared prescription has its table.
`floor_us` is the time the history's stores alone would take at `--hbm-gbs` (default 6290 GB/s, the rate a float4 copy reaches on
an MI355X): (J + 1) x 7 values per ray, or 7 without history; `kernel_over_floor` says how far from it a trace is.
--quick runs each configuration a few times only.
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import raytrace_common as RC  # noqa: E402
from prysm_amd import _lib as L  # noqa: E402
from prysm_amd import _ops  # noqa: E402
from prysm_amd.x import raytrace_plan as plan  # noqa: E402
from prysm_amd.x import raytracing as RT  # noqa: E402
from prysm_amd.x.raytracing import surfaces as SF  # noqa: E402


def batch_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def timed(fn, reps, quick, window=0.25):
    """(us per call, calls per batch): batches long enough to fill `window` seconds (at least `reps` calls) until two successive
    batches agree within 3 % (at most 8), then the median of three more"""
    fn()
    torch.cuda.synchronize()
    if quick:
        return batch_ms(fn, 2) * 1e3, 2
    reps = max(reps, int(window * 1e3 / batch_ms(fn, 5)) + 1)
    prev = batch_ms(fn, reps)
    for _ in range(8):
        cur = batch_ms(fn, reps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return sorted(batch_ms(fn, reps) for _ in range(3))[1] * 1e3, reps


def torch_constants(recs, dt, dev):
    """per surface the vertex and the rotation (or None) as device tensors: uploaded once, outside what is timed"""
    return [(torch.tensor(r['P'], dtype=dt, device=dev), None if r['R'] is None else torch.tensor(r['R'], dtype=dt, device=dev)) for r in recs]


def torch_trace(recs, consts, n_launch, P, S):
    """the kernel's steps for planes and conics as torch operations: histories of P, S, OPL and the status code and surface"""
    dt, dev = P.dtype, P.device
    N = P.shape[0]
    n = n_launch
    code = torch.zeros(N, dtype=torch.int32, device=dev)
    surface = torch.zeros(N, dtype=torch.int32, device=dev)
    Ph, Sh, Oh = [P], [S], [torch.zeros(N, dtype=dt, device=dev)]
    X, D = P, S
    for j, r in enumerate(recs):
        vertex, R = consts[j]
        p0, sl = X - vertex, D
        if R is not None:
            p0, sl = p0 @ R.T, sl @ R.T
        c, k, dx, dy = r['c'], r['k'], r['dx'], r['dy']
        sz = sl[:, 2]
        s0 = -p0[:, 2] / sz
        p1 = p0 + s0[:, None] * sl
        if r['shape'] == plan.PLANE or c == 0.0:
            q, valid = p1, sz != 0
            nh = torch.zeros_like(q)
            nh[:, 2] = 1.0
        else:
            xp, yp = p1[:, 0] + dx, p1[:, 1] + dy
            A, B, C = 1 + k * sz * sz, xp * sl[:, 0] + yp * sl[:, 1] - sz / c, xp * xp + yp * yp
            disc = B * B - A * C
            ok = disc >= 0
            sq = torch.sqrt(torch.where(ok, disc, torch.zeros_like(disc)))
            denom = torch.where(sz < 0, -1.0, 1.0) * (1.0 if c > 0 else -1.0) * sq - B
            tangent = denom == 0
            t = torch.where(tangent, torch.zeros_like(C), C / torch.where(tangent, torch.ones_like(denom), denom))
            q = p1 + t[:, None] * sl
            xq, yq = q[:, 0] + dx, q[:, 1] + dy
            rr = xq * xq + yq * yq
            phi_arg = 1 - (1 + k) * c * c * rr
            phi = torch.sqrt(torch.clamp(phi_arg, min=0))
            mag_sq = 1 - k * c * c * rr
            mag = torch.sqrt(torch.where(mag_sq < 0, torch.ones_like(mag_sq), mag_sq))
            nh = torch.stack([-c * xq / mag, -c * yq / mag, phi / mag], dim=1)
            valid = ok & (phi_arg >= 0)
        step = torch.where(valid, plan.OK, plan.MISS).to(torch.int32)
        kind, x0, y0, rin, rout = r['aperture']
        if kind != plan.AP_NONE:
            ax, ay = q[:, 0] - x0, q[:, 1] - y0
            rsq = ax * ax + ay * ay
            inside = rsq <= rout * rout if kind == plan.AP_CIRCULAR else (rsq >= rin * rin) & (rsq <= rout * rout)
            step = torch.where(valid & ~inside, plan.CLIP, step)
        sp = sl
        if r['interaction'] == plan.REFLECT:
            cos_i = torch.sum(sl * nh, dim=1)
            sp = sl - 2 * cos_i[:, None] * nh
        elif r['interaction'] == plan.REFRACT:
            mu = n / r['n_post']
            cos_i = torch.sum(sl * nh, dim=1)
            cos_t = torch.sqrt(1 - mu * mu * (1 - cos_i * cos_i))
            sp = mu * sl + (torch.sign(cos_i) * cos_t - mu * cos_i)[:, None] * nh
            step = torch.where((step == plan.OK) & torch.isnan(sp).any(dim=1), plan.TIR, step)
        if R is not None:
            q, sp = q @ R, sp @ R
        q = q + vertex
        seg = q - X
        opl = n * torch.sign(torch.sum(seg * D, dim=1)) * torch.sqrt(torch.sum(seg * seg, dim=1))
        failed = (code == plan.OK) & (step != plan.OK)
        code, surface = torch.where(failed, step, code), torch.where(failed, j + 1, surface)
        if r['interaction'] == plan.REFRACT:
            n = r['n_post']
        dead = code != plan.OK
        X, D = torch.where(dead[:, None], torch.nan, q), torch.where(dead[:, None], torch.nan, sp)
        Ph.append(X), Sh.append(D), Oh.append(torch.where(dead, torch.nan, opl))
    surface = torch.where(code == plan.OK, len(recs), surface)
    return torch.stack(Ph), torch.stack(Sh), torch.stack(Oh), surface, code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--window', type=float, default=0.25)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--side', type=int, default=1024)
    ap.add_argument('--hbm-gbs', type=float, default=6290.0)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'raytrace', 'exp_raytrace.log'))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    log = open(a.log, 'w')

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

    warnings.simplefilter('ignore')
    lib = L.load()
    surfs = {'A': RC.build('A', SF), 'D': RC.build('D', SF)}
    surfs['A_analytic'] = [s for s in surfs['A'] if not isinstance(s.shape, SF.EvenAsphere)]
    rays = {'A': dict(nrays=a.side, maxx=11, yangle=2, xangle=-1), 'D': dict(nrays=a.side, maxx=22, yangle=8)}
    rays['A_analytic'] = rays['A']
    for name in ('A', 'A_analytic', 'D'):
        rx = RT.prepare(surfs[name], RC.WVL)
        recs = plan.unpack_table(rx.host_table)
        J = len(rx)
        P64, S64 = RT.generate_collimated_rect_ray_grid(**rays[name])
        S64 = S64.contiguous()
        for dt in (torch.float32, torch.float64):
            P, S = P64.to(dt), S64.to(dt)
            N, el = P.shape[0], P.element_size()
            res = RT.raytrace(rx, P, S, RC.WVL)
            valid = float(torch.mean((res.status.imag == 0).to(torch.float64)))
            code = L.PM_F32 if dt == torch.float32 else L.PM_F64
            tol = plan.resolve_tol_sag(None, 'float32' if dt == torch.float32 else 'float64')
            for history in (True, False):
                call, reps = timed(lambda: RT.raytrace(rx, P, S, RC.WVL, history=history), a.reps, a.quick, a.window)
                Po, So, Oo, sf, cd = _ops.rt_trace(rx.table, rx.n_launch, tol, P, S, history)      # the outputs, allocated once

                def launch():
                    L.check(lib.pm_rt_trace(code, N, J, L.ptr(rx.table), rx.n_launch, tol, int(history), L.ptr(P), L.ptr(S), L.ptr(Po), L.ptr(So),
                                            L.ptr(Oo), L.ptr(sf), L.ptr(cd), L.stream_ptr()))
                us, kreps = timed(launch, a.reps, a.quick, a.window)
                stored = N * ((J + 1) * 7 if history else 7) * el + N * 8
                floor = stored / (a.hbm_gbs * 1e9) * 1e6
                row = dict(case=name, surfaces=J, rays=N, dtype=str(dt).split('.')[1], history=history, valid_share=round(valid, 4),
                           call_us=round(call, 1), kernel_us=round(us, 1), reps=reps, kernel_reps=kreps, mrays_per_s=round(N / us, 1),
                           stored_mb=round(stored / 1e6, 1), floor_us=round(floor, 1), kernel_over_floor=round(us / floor, 2))
                if name == 'A_analytic' and history:
                    consts = torch_constants(recs, dt, P.device)
                    want = torch_trace(recs, consts, rx.n_launch, P, S)
                    same = bool(torch.equal(want[4], res.status_record.code)) and bool(torch.equal(want[3], res.status_record.surface))
                    del want
                    comp, treps = timed(lambda: torch_trace(recs, consts, rx.n_launch, P, S), a.reps, a.quick, a.window)
                    row.update(torch_us=round(comp, 1), torch_reps=treps, torch_over_call=round(comp / call, 2), torch_statuses_equal=same)
                emit(**row)
                del Po, So, Oo, sf, cd
            del res


if __name__ == '__main__':
    main()
