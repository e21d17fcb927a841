"""Planner A/B of two builds of the library, on the CPU: every pm_plan_explain line and workspace query of a corpus of shapes must
be the same text.  python tools/exp_plan_corpus.py <libA> <libB>   (child processes, one library each through PRYSM_AMD_LIB)
The corpus: ROUTES and ROUTES_KW of tests/test_capi_symbols.py in both precisions, whole / padded / cropped, with the spectral and
chain variants, under the default knobs and one knob at a time."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [{}, dict(fold=0), dict(fold=1), dict(log_k=0), dict(r2c=2), dict(herm_t=0), dict(herm_t=1), dict(mix=0), dict(col_log_g=2)]

if len(sys.argv) == 3:
    outs = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, PRYSM_AMD_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, __file__, '--child'], env=env, capture_output=True, text=True)
        if r.returncode:
            sys.exit('child failed for %s:\n%s' % (lib, r.stderr[-2000:]))
        outs.append(r.stdout.splitlines())
    a, b = outs
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i, x, y in diff[:40]:
        print('line %d\n  A %s\n  B %s' % (i, x, y))
    import hashlib
    print('A: %d lines sha256 %s' % (len(a), hashlib.sha256('\n'.join(a).encode()).hexdigest()))
    print('B: %d lines sha256 %s' % (len(b), hashlib.sha256('\n'.join(b).encode()).hexdigest()))
    print('identical' if a == b else 'DIFFERENT: %d lines differ, lengths %d / %d' % (len(diff), len(a), len(b)))
    sys.exit(0 if a == b else 1)

sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_capi_symbols as t       # noqa: E402
from prysm_amd import _lib as L     # noqa: E402
lib = L.load()


def variants():
    shapes = []
    for args, _ in t.ROUTES:
        shapes.append(dict(m=args[0], n=args[1]))
    for kw, _ in t.ROUTES_KW:
        kw = dict(kw)
        kw.pop('dt', None)
        shapes.append(kw)
    for kw in shapes:
        for dt in ('c64', 'c128'):
            op = kw.get('op', 0)
            base = {k: v for k, v in kw.items() if k != 'op'}
            yield dict(base, dt=dt), op, 'whole'
            if 'Q' not in base:
                yield dict(base, dt=dt, Q=2), op, 'padded'
            yield dict(base, dt=dt), op, 'cropped'
    # the forms the two tables do not hold: packed synthesis with the accumulating epilogue (the grouped wavelength loop), the real chain
    for m, n in ((32, 32), (1024, 1024), (2048, 2048), (2048, 4096), (4096, 4096), (1000, 1000)):
        for dt in ('c64', 'c128'):
            yield dict(m=m, n=n, dt=dt, synth=True, epi=2), 0, 'packed'
            yield dict(m=m, n=n, dt=dt, real=True), 1, 'real-chain'
            yield dict(m=m, n=n, dt=dt, mul=True, batch=40), 1, 'stack'


def describe(kw, op, form):
    d = t._desc(**kw)
    m, n = kw['m'], kw['n']
    if form == 'cropped':
        d.out_y, d.out_x, d.out_ld = L.pm_axis(m, m // 2, m // 4, m // 2), L.pm_axis(n, n // 2 // 2 * 2, n // 4, n // 2), n // 2 // 2 * 2
        if kw.get('batch'):
            d.out_bstride = m * n
    if form == 'packed':
        d.flags |= L.PM_FLAG_SYNTH_PACKED
    if form == 'real-chain':
        d.flags |= L.PM_FLAG_REAL_OUTPUT
        d.mul_kind, d.mul = L.PM_MUL_FULL, 16
    buf = ctypes.create_string_buffer(512)
    out = []
    for o in (0, 1):
        rc = lib.pm_plan_explain(ctypes.byref(d), o, buf, 512)
        out.append(buf.value.decode() if rc == 0 else 'rc=%d %s' % (rc, lib.pm_last_error().decode()))
    dt = L.PM_C64 if kw['dt'] == 'c64' else L.PM_C128
    ws = (lib.pm_fft2_workspace(ctypes.byref(d)), lib.pm_fft2_mul_ifft2_workspace(ctypes.byref(d)),
          lib.pm_fft2_spectral_workspace(ctypes.byref(d), 3), lib.pm_fft2_spectral_workspace(ctypes.byref(d), 8),
          lib.pm_fft1_workspace(dt, 1, 4, n), lib.pm_fft1_workspace(dt, 0, 4, m))
    return '%s %s | %s | %s | ws %s' % (form, sorted(kw.items()), out[0], out[1], ' '.join(map(str, ws)))


for knobs in KNOBS:
    print('#', knobs)
    with L.tuning_local(**knobs):
        for kw, op, form in variants():
            print(describe(kw, op, form))
