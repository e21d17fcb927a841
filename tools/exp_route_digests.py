"""Results A/B of two builds of the library on the GPU: SHA-256 of the outputs of one case per route and of the benchmark's shapes, from
seeded inputs, in one child process per library (PRYSM_AMD_LIB).  python tools/exp_route_digests.py <libA> <libB>
The two builds are meant to launch the same kernels with the same arguments: any differing digest is a defect."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) == 3:
    outs = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, PRYSM_AMD_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, __file__, '--child'], env=env, capture_output=True, text=True)
        if r.returncode:
            sys.exit('child failed for %s (exit %d):\n%s' % (lib, r.returncode, r.stderr[-2000:]))
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith('DIGEST')])
    a, b = outs
    for x, y in zip(a, b):
        print(('same  ' if x == y else 'DIFFER') + ' ' + x[7:] + ('' if x == y else '   B: ' + y[7:]))
    ok = a == b and len(a) > 0
    print('%d cases, %s' % (len(a), 'all digests equal' if ok else 'DIGESTS DIFFER'))
    sys.exit(0 if ok else 1)

sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402
from prysm_amd import _lib as L, _ops, propagation as P, otf    # noqa: E402
from prysm_amd import convolution as CV                         # noqa: E402

g = torch.Generator(device='cuda').manual_seed(2026)


def c(*shape, dt=torch.complex64):
    return torch.randn(*shape, dtype=dt, device='cuda', generator=g)


def r(*shape, dt=torch.float32):
    return torch.randn(*shape, dtype=dt, device='cuda', generator=g)


def digest(name, t):
    t = t.data if hasattr(t, 'data') and not isinstance(t, torch.Tensor) else t
    torch.cuda.synchronize()
    print('DIGEST %-44s %s' % (name, hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()), flush=True)


def f2(x, **kw):
    return _ops.fft2(x, direction=-1, scale=1.0, **kw)


def chain(x, mul, **kw):
    return _ops.fft2_mul_ifft2(x, scale=1.0, mul=mul, **kw)


ABS = L.PM_EPI_ABS
# one case per route (the shapes of tests/test_gpu_engine.py's workspace guard test)
digest('engine 16x32', f2(c(16, 32)))
digest('engine 16x32 padded', f2(c(8, 16), shape=(16, 32), in_off=(4, 8)))
with L.tuning_local(fold=1):
    digest('engine-fold 8x2048 c64', f2(c(8, 2048)))
    digest('engine-fold 8x2048 c128', f2(c(8, 2048, dt=torch.complex128)))
digest('engine stack 3x32x32', f2(c(3, 32, 32)))
with L.tuning_local(herm_t=0, r2c=2):
    digest('hermitian 32x64', f2(r(32, 64), epilogue=ABS))
    with L.tuning_local(fold=1):
        digest('hermitian-fold 32x64', f2(r(32, 64), epilogue=ABS))
digest('hermitian-transposed 32x32', f2(r(32, 32), epilogue=ABS))
with L.tuning_local(herm_t_fold=1):
    digest('hermitian-transposed fold 2048x32', f2(r(2048, 32), epilogue=ABS))
digest('fused 16x32', chain(c(16, 32), c(16, 32)))
digest('fused 16x32 padded', chain(c(8, 16), c(16, 32), shape=(16, 32), in_off=(4, 8)))
with L.tuning_local(fold=1):
    digest('fused fold 8x2048', chain(c(8, 2048), c(8, 2048)))
with L.tuning_local(r2c=2):
    digest('hermitian-chain 2x64', chain(r(2, 64), c(2, 64), real_out=True))
    with L.tuning_local(fold=1):
        digest('hermitian-chain fold 4x4096', chain(r(4, 4096), c(4, 4096), real_out=True))
digest('fused-composite 96x100', chain(c(96, 100), c(96, 100)))
digest('natural-mixed 36x36', f2(c(36, 36)))
digest('rows=bluestein 2x97', f2(c(2, 97)))
digest('bluestein-2d 97x97', f2(c(97, 97)))
digest('radix-step 2x16384', f2(c(2, 16384)))
digest('radix-step 16384x2', f2(c(16384, 2)))
digest('fft1 16384 rows', _ops.fft1(c(2, 16384), axis=1))
digest('fft1 16384 columns', _ops.fft1(c(16384, 2), axis=0))
digest('fft1 97 rows', _ops.fft1(c(2, 97), axis=1))
digest('fft1 97 columns', _ops.fft1(c(97, 2), axis=0))
packed = _ops.pack_amp_opd((r(32, 32) > 0).float(), r(32, 32))
digest('spectral 32x32 x3', _ops.fft2(packed, direction=-1, scale=1.0, epilogue=L.PM_EPI_ABS2_ACCUM, synth=('packed', 0.011),
                                      spectral=([0.011, 0.012, 0.013], [1.0, 0.5, 0.25]), out=torch.zeros(32, 32, device='cuda')))
# the benchmark's shapes
digest('focus c64 4096', P.focus(c(4096, 4096), 1))
digest('focus c64 2048', P.focus(c(2048, 2048), 1))
digest('focus c128 4096', P.focus(c(4096, 4096, dt=torch.complex128), 1))
digest('focus c64 3000', P.focus(c(3000, 3000), 1))
digest('focus c64 1024 Q=2', P.focus(c(1024, 1024), 2))
digest('mtf_from_psf 4096', otf.mtf_from_psf(torch.rand(4096, 4096, device='cuda', generator=g) + 0.01, 1.0))
digest('conv real 4096', CV.conv(torch.rand(4096, 4096, device='cuda', generator=g), torch.rand(4096, 4096, device='cuda', generator=g)))
digest('angular spectrum c128 4096', P.angular_spectrum(c(4096, 4096, dt=torch.complex128), 0.6328, 0.01, 10.0, Q=1))
