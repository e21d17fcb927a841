"""Time the Jones / Mueller unit (csrc/jones.hip) on the device with HIP events.

    python tools/exp_polarization.py [--window 0.2] [--quick] [--step-timeout 120] [--log profiles/polarization/exp_polarization.log]

The parent process never touches the device: every case -- (what, size, precision) -- runs as a child process of its own under
`timeout`, and the first child that fails or is killed ends the run (nothing more is started on the device after a fault).  One JSON
line per measurement, printed and appended to the log.  At 1024^2 and 4096^2, complex64 and complex128:
- `retarder`: linear_retarder(delta map, theta map) against the reference's route in torch (the diagonal matrix, two rotation
  matrices, two torch.matmul on (M, N, 2, 2));
- `vortex_field`: vector_vortex_retarder(2, t, field=E) against the same in torch followed by the broadcast product with the field;
- `chain3`: jones_product(A, B, C) against torch.matmul(torch.matmul(A, B), C);
- `mueller`: jones_to_mueller against einsum + linalg.inv + two matmul, as the reference writes it;
- `relayout`: to_planes against permute(2, 3, 0, 1).contiguous().
`floor_us` is the bytes the call must read and write at the store rate measured in the same child (`store_gbs`: zero_() of 1 GiB), and
`floor_share` = floor_us / us; `torch_over_call` > 1 means the unit's call wins.  A timed batch is as many calls as fill `--window`
seconds (at least 2); batches repeat until two agree within 3 % (at most 5), and the median of three more is reported.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WHAT = ('retarder', 'vortex_field', 'chain3', 'mueller', 'relayout')
SIZES = (1024, 4096)
PRECISIONS = (32, 64)


def batch_ms(torch, fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def timed(torch, fn, quick, window):
    fn()
    torch.cuda.synchronize()
    if quick:
        return batch_ms(torch, fn, 2) * 1e3, 2
    reps = max(2, int(window * 1e3 / batch_ms(torch, fn, 2)) + 1)
    prev = batch_ms(torch, fn, reps)
    for _ in range(5):
        cur = batch_ms(torch, fn, reps)
        if abs(cur - prev) <= 0.03 * prev:
            break
        prev = cur
    return sorted(batch_ms(torch, fn, reps) for _ in range(3))[1] * 1e3, reps


def child(what, n, precision, quick, window):
    import math

    import torch

    from prysm_amd.conf import config
    from prysm_amd.x import polarization as pol
    config.precision = precision
    rd, cd = (torch.float32, torch.complex64) if precision == 32 else (torch.float64, torch.complex128)
    es = 8 if precision == 32 else 16
    g = torch.Generator(device='cuda').manual_seed(3)
    rmap = lambda: (torch.rand((n, n), generator=g, device='cuda', dtype=rd) - 0.5) * 6      # noqa: E731
    jones = lambda: torch.randn((n, n, 2, 2), generator=g, device='cuda', dtype=cd)      # noqa: E731
    buf = torch.empty(1 << 30, dtype=torch.uint8, device='cuda')
    store_us, _ = timed(torch, buf.zero_, quick, window)
    store_gbs = (1 << 30) / store_us / 1e3
    del buf

    def rot(t, sign=1.0):
        c, s = torch.cos(t), torch.sin(t) * sign
        return torch.stack([torch.stack([c, s], -1), torch.stack([-s, c], -1)], -2).to(cd)

    px = n * n
    if what == 'retarder':
        d, t = rmap(), rmap()
        ours = lambda: pol.linear_retarder(d, t)      # noqa: E731

        def ref():
            j = torch.zeros((n, n, 2, 2), dtype=cd, device='cuda')
            j[..., 0, 0] = 1
            j[..., 1, 1] = torch.exp(1j * d)
            return torch.matmul(torch.matmul(rot(t, -1.0), j), rot(t))
        nbytes = px * (2 * es // 2 + 4 * es)
    elif what == 'vortex_field':
        t, E = rmap(), torch.randn((n, n), generator=g, device='cuda', dtype=cd)
        ours = lambda: pol.vector_vortex_retarder(2, t, 2.5, 0.3, field=E)      # noqa: E731
        r0, r1 = rot(torch.tensor(-0.3, device='cuda', dtype=rd)), rot(torch.tensor(0.3, device='cuda', dtype=rd))

        def ref():
            th = t * 2
            c, s = torch.cos(th), torch.sin(th)
            lhs = torch.stack([torch.stack([c, s], -1), torch.stack([s, -c], -1)], -2).to(cd) * math.sin(1.25)
            lhs[..., 0, 0] += -1j * math.cos(1.25)
            return torch.matmul(torch.matmul(r0, lhs), r1) * E[..., None, None]
        nbytes = px * (es // 2 + es + 4 * es)
    elif what == 'chain3':
        A, B, C = jones(), jones(), jones()
        ours = lambda: pol.jones_product(A, B, C)      # noqa: E731
        ref = lambda: torch.matmul(torch.matmul(A, B), C)      # noqa: E731
        nbytes = px * 16 * es
    elif what == 'mueller':
        J = jones()
        U = torch.tensor([[1, 0, 0, 1], [1, 0, 0, -1], [0, 1, 1, 0], [0, 1j, -1j, 0]], dtype=cd, device='cuda') / math.sqrt(2)
        ours = lambda: pol.jones_to_mueller(J)      # noqa: E731

        def ref():
            k = torch.einsum('...ik,...jl->...ijkl', torch.conj(J), J).reshape(n, n, 4, 4)
            return torch.real(torch.matmul(torch.matmul(U, k), torch.linalg.inv(U)))
        nbytes = px * (4 * es + 16 * es // 2)
    else:
        J = jones()
        ours = lambda: pol.to_planes(J)      # noqa: E731
        ref = lambda: J.permute(2, 3, 0, 1).contiguous()      # noqa: E731
        nbytes = px * 8 * es
    us, reps = timed(torch, ours, quick, window)
    torch_us, _ = timed(torch, ref, quick, window)
    floor_us = nbytes / (store_gbs * 1e3)
    return dict(case=what, n=n, precision=precision, us=round(us, 2), reps=reps, torch_us=round(torch_us, 2),
                torch_over_call=round(torch_us / us, 3), bytes=nbytes, store_gbs=round(store_gbs, 1), floor_us=round(floor_us, 2),
                floor_share=round(floor_us / us, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'polarization', 'exp_polarization.log'))
    ap.add_argument('--case', nargs=3, metavar=('WHAT', 'N', 'PRECISION'), help='run one case in this process (what the parent starts)')
    a = ap.parse_args()
    if a.case:
        print(json.dumps(child(a.case[0], int(a.case[1]), int(a.case[2]), a.quick, a.window)))
        return 0
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, 'w') as log:
        for what in WHAT:
            for n in SIZES:
                for precision in PRECISIONS:
                    cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--window', str(a.window),
                           '--case', what, str(n), str(precision)] + (['--quick'] if a.quick else [])
                    r = subprocess.run(cmd, capture_output=True, text=True)
                    line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''
                    if r.returncode != 0 or not line.startswith('{'):
                        line = json.dumps(dict(case=what, n=n, precision=precision, failed=r.returncode, stderr=r.stderr[-400:]))
                    print(line, flush=True)
                    log.write(line + '\n')
                    log.flush()
                    if r.returncode != 0:
                        return r.returncode      # nothing more is started on the device after a failure
    return 0


if __name__ == '__main__':
    sys.exit(main())
