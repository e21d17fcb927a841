"""GPU parity tests, by component: the polychromatic driver -- BASELINE config 5 at full size, the wavelength loop as launch pairs (pm_fft2_spectral), the
reduce forms on a process group, two-rank launches (prysm_amd/polychromatic.py, csrc/fft_spectral.h).

All through the C ABI (ctypes -> libprysm_amd.so), against the fp64 oracle / numpy first and a second HIP route only afterwards.
Tolerances (max error / max magnitude against fp64): 1e-10 complex128, 5e-6 complex64 transforms, 3e-5 the MFMA matrix DFT.
(Regrouped in round 6 from the per-round files of rounds 2 - 5; the tests themselves are unchanged.)
"""
import ctypes
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_max
from oracle import prysm_oracle as O
from gpu_common import (  # noqa: F401
    TOL64, TOL32, TOL32_MDFT, tonp, _real_vdot, crandn_, _np_transform_psf, _two_rank_backend, _env, _spectral_case,
    crandn, _op_np, _poly_numpy, _seven_planes, CE_LENGTHS, _ce_ref)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('batched', [False, True])
def test_config5_variant_f_full_size(pa, config5, batched):
    """64 wavelengths x 4096^2 fp32, FFT focus Q = 1, |.|^2 and the weighted sum on the device: field by field with the
    accumulate epilogue (pupil synthesised inside the row pass), and as stacks + sum_of_2d_modes."""
    from prysm_amd.polychromatic import polychromatic_psf
    c = config5
    got = tonp(polychromatic_psf(c['amp'], c['opd'], c['wvls'], c['wts'], c['dx'], 100.0, Q=1, batched=batched))
    assert got.dtype == np.float32 and got.shape == (4096, 4096)
    assert rel_max(got, c['want_f']) < 2e-5     # 64 fp32 intensities accumulated in fp32 against the fp64 oracle sum
    assert abs(got.sum(dtype=np.float64) / c['want_f'].sum() - 1) < 1e-5     # energy (unitary transform: 64 x sum amp^2)


def test_config5_variant_m_full_size(pa, config5):
    """the how-to's variant: per wavelength prepare_executor + matrix-DFT focus 4096^2 -> 512^2 (MFMA) + |.|^2 accumulate"""
    from prysm_amd.conf import config
    from prysm_amd.polychromatic import polychromatic_psf
    c = config5
    prec = config.precision
    try:
        config.precision = 32
        got = tonp(polychromatic_psf(c['amp'], c['opd'], c['wvls'], c['wts'], c['dx'], 100.0, focal_dx=0.55 * 10 / 4,
                                     samples=512, kind='mdft'))
    finally:
        config.precision = prec
    assert got.dtype == np.float32 and got.shape == (512, 512)
    assert rel_max(got, c['want_m']) < 1e-4     # K = 4096 complex64 contractions, squared and summed 64 times


def test_config5_variant_m_by_chirp_z(pa, config5):
    """the same 512^2 focal grid per wavelength through the chirp-Z executor (kind='czt': fused convolution kernels, K = 8192) gives
    the image of the matrix-DFT variant"""
    from prysm_amd.conf import config
    from prysm_amd.polychromatic import polychromatic_psf
    c = config5
    prec = config.precision
    try:
        config.precision = 32
        got = tonp(polychromatic_psf(c['amp'], c['opd'], c['wvls'], c['wts'], c['dx'], 100.0, focal_dx=0.55 * 10 / 4,
                                     samples=512, kind='czt'))
    finally:
        config.precision = prec
    assert got.dtype == np.float32 and got.shape == (512, 512)
    assert rel_max(got, c['want_m']) < 1e-4


def test_bench_two_ranks_selflaunch(pa):
    """`python bench.py --gpus 2` with no launcher: bench.py re-executes itself under torch.distributed.run, one rank per GPU
    over RCCL when two GPUs are visible (both ranks on GPU 0 over gloo otherwise) and prints ONE line with n_gpus = 2 and a
    timed config-5 run."""
    be = _two_rank_backend()
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '5', '--warmup', '2', '--edge', '1024',
           '--full', '--no-cpu-baseline', '--backend', be]
    env = _env()
    env.pop('WORLD_SIZE', None)
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['value'] > 0 and line['scaling'] == 'weak'
    poly = line['polychromatic']
    assert poly['wavelengths_per_gpu'] == 32
    assert poly['variant_F_fft_focus']['psf_ms'] > 0 and poly['variant_M_mdft_512']['psf_ms'] > 0
    assert line['n2048']['value'] > 0 and line['reduce_ms'] > 0


def test_bench_plain_run_is_the_headline_only(pa, tmp_path):
    """`python bench.py` without --full: ONE line with the headline keys and the dumped focal field of the last timed step, and none
    of the side measurements --full adds"""
    import bench
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '5', '--warmup', '2', '--edge', '1024', '--dump-outputs', str(tmp_path)]
    res = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['unit'] == 'propagations/s' and line['higher_is_better'] is True and line['dtype'] == 'c64' and line['steps'] == 5
    assert line['value'] > 0 and abs(line['value'] * line['ms_per_step'] / 1e3 - 1) < 1e-5
    for key in ('roofline', 'repeat_ms', 'n2048', 'polychromatic', 'polychromatic_2048', 'psf_variant', 'other_configs', 'cpu_baseline'):
        assert key not in line, key
    assert line['dumped_outputs']['arrays'] == {'focus': {'shape': [1024, 1024, 2], 'dtype': 'float32'}}
    got = np.load(tmp_path / 'focus.npy')
    x = bench.make_field(1024, np.complex64, 4096)
    want = tonp(pa.propagation.focus(x, 1))
    assert rel_max(got[..., 0] + 1j * got[..., 1], want) < TOL32


def test_polychromatic_two_ranks_vs_oracle(pa):
    """tests/multi_rank_poly.py: stacks, field-by-field and matrix-DFT variants sharded over two ranks, reduce and the
    all-to-all reduce, against the oracle's single-process sum"""
    be = _two_rank_backend()
    env = _env()
    env['PM_TEST_BACKEND'] = be
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29541', os.path.join(ROOT, 'tests', 'multi_rank_poly.py')]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert res.stdout.count('OK') >= 2


def test_polychromatic_one_rank_rccl_group(pa):
    """the same script as ONE rank under an `nccl` process group -- RCCL initialises and reduce,
    all_to_all_single, gather and all_reduce execute on the device for real (a group of one rank still runs its collective,
    polychromatic._group_info), plus the pipelined form with its side stream"""
    env = _env()
    env['PM_TEST_BACKEND'] = 'nccl'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', '29543', os.path.join(ROOT, 'tests', 'multi_rank_poly.py')]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-3000:])
    assert res.stdout.count('OK') >= 1


@pytest.mark.parametrize('m,n,Q,count', [(64, 64, 1, 3), (256, 256, 1, 11), (256, 512, 1, 8), (256, 256, 2, 5), (1024, 1024, 1, 9),
                                         (2048, 2048, 1, 4), (32, 2048, 1, 2), (64, 2048, 1, 3), (4096, 2048, 1, 3)])
def test_spectral_call_equals_the_wavelength_loop(pa, m, n, Q, count):
    """pm_fft2_spectral (groups of wavelengths per launch pair: packed map read once, w |.|^2 summed in registers) against the
    loop it replaces -- one accumulate-epilogue transform pair per wavelength -- and against the fp64 oracle sum; every group size
    and both register / memory forms of its two kernels (tuning keys spectral, spectral_mode)."""
    from prysm_amd import _lib, _ops
    P = pa.propagation
    lib = _lib.load()
    rng = np.random.default_rng(m * 7 + n + count)
    amp, opd = _spectral_case(rng, m, n)
    packed = _ops.pack_amp_opd(amp, opd)
    wvls = np.linspace(0.5, 0.7, count)
    ks = [2 * np.pi / w / 1e3 for w in wvls]
    wts = list(np.linspace(0.5, 1.5, count))
    M, N = int(m * Q), int(n * Q)
    loop = torch.zeros((M, N), device='cuda')
    for k, w in zip(ks, wts):
        P.focus_intensity(packed, Q, out=loop, weight=w, synth=('packed', k))
    a64, o64 = amp.cpu().numpy().astype(np.float64), opd.cpu().numpy().astype(np.float64)
    want = sum(w * O.intensity(O.focus(O.from_amp_and_phase(a64, o64, float(wl)), Q)) for wl, w in zip(wvls, wts))
    assert rel_max(tonp(loop), want) < 2e-5
    try:
        if n == 2048 and m <= 64:
            lib.pm_set_tuning(b'fold', 1)      # the folded kernels (automatic from 4096 rows) on short columns too
        for group in (1, 2, 3, 8):
            for mode in (0, 1, 2, 3):
                assert lib.pm_set_tuning(b'spectral', group) == 0
                if lib.pm_set_tuning(b'spectral_mode', mode) != 0:     # forms 0 - 2 lost their measurements and left the library (experiments/README.md)
                    assert mode != 3
                    continue
                got = torch.full((M, N), 0.0, device='cuda')
                P.focus_intensity(packed, Q, out=got, synth=('packed', ks[0]), spectral=(ks, wts))
                # same terms in the same order; only the association of the fp32 sum differs (per group: acc + (w0 i0 + w1 i1 ...))
                assert rel_max(tonp(got), tonp(loop)) < 2e-6, (group, mode)
                assert rel_max(tonp(got), want) < 2e-5, (group, mode)
    finally:
        lib.pm_set_tuning(b'spectral', 8)
        lib.pm_set_tuning(b'spectral_mode', 3)
        lib.pm_set_tuning(b'fold', -1)


def test_spectral_call_accumulates_and_falls_back(pa):
    """the call ADDS to its accumulator; descriptors outside the fused form (two-array synthesis; 4096^2 bins, where the loop is as
    fast) run the plain loop and give the same image"""
    from prysm_amd import _lib, _ops
    P = pa.propagation
    lib = _lib.load()
    rng = np.random.default_rng(5)
    amp, opd = _spectral_case(rng, 256, 256)
    packed = _ops.pack_amp_opd(amp, opd)
    ks = [2 * np.pi / w / 1e3 for w in (0.5, 0.6, 0.7)]
    wts = [1.0, 2.0, 0.5]
    base = torch.rand((256, 256), device='cuda')
    once = torch.zeros((256, 256), device='cuda')
    P.focus_intensity(packed, 1, out=once, synth=('packed', ks[0]), spectral=(ks, wts))
    got = base.clone()
    P.focus_intensity(packed, 1, out=got, synth=('packed', ks[0]), spectral=(ks, wts))
    assert rel_max(tonp(got), tonp(base + once)) < 1e-6
    two = torch.zeros((256, 256), device='cuda')
    P.focus_intensity(opd, 1, out=two, synth=(amp, ks[0]), spectral=(ks, wts))     # amplitude and OPD as two arrays: the loop
    assert rel_max(tonp(two), tonp(once)) < 2e-6
    try:
        assert lib.pm_set_tuning(b'spectral_area_log', 10) == 0     # 256^2 = 2^16 bins >= 2^10: the loop
        loop = torch.zeros((256, 256), device='cuda')
        P.focus_intensity(packed, 1, out=loop, synth=('packed', ks[0]), spectral=(ks, wts))
    finally:
        lib.pm_set_tuning(b'spectral_area_log', 24)
    assert rel_max(tonp(loop), tonp(once)) < 2e-6
    with pytest.raises(ValueError):
        P.focus_intensity(packed, 1, out=once, synth=('packed', ks[0]), spectral=(ks, wts[:2]))


@pytest.mark.parametrize('n,Q', [(512, 2), (1024, 1)])
def test_polychromatic_psf_spectral_equals_loop_and_oracle(pa, n, Q):
    """the driver's default below 4096^2 transforms (one pm_fft2_spectral call per rank) against its per-wavelength loop
    (spectral=False), the stacked form (batched=True) and the oracle sum"""
    from prysm_amd.polychromatic import polychromatic_psf
    x, y = O.make_xy_grid(n, diameter=10)
    r, _ = O.cart_to_polar(x, y)
    amp = O.circle(5, r).astype(np.float32)
    opd = O.hopkins_w040(r / 5, 400.0).astype(np.float32)
    dx = float(x[0, 1] - x[0, 0])
    wvls = np.linspace(0.5, 0.7, 13)
    wts = np.linspace(1.0, 2.0, 13)
    want = sum(w * O.intensity(O.focus(O.from_amp_and_phase(amp.astype(np.float64), opd.astype(np.float64), float(wl)), Q))
               for wl, w in zip(wvls, wts))
    fused = tonp(polychromatic_psf(amp, opd, wvls, wts, dx, 100.0, Q=Q))
    loop = tonp(polychromatic_psf(amp, opd, wvls, wts, dx, 100.0, Q=Q, spectral=False, batched=False))
    stacks = tonp(polychromatic_psf(amp, opd, wvls, wts, dx, 100.0, Q=Q, batched=True))
    assert fused.dtype == np.float32 and fused.shape == want.shape
    assert rel_max(fused, want) < 2e-5
    assert rel_max(fused, loop) < 2e-6
    assert rel_max(fused, stacks) < 2e-6


@pytest.mark.parametrize('m,n,Q,count', [(64, 64, 1, 3), (256, 256, 1, 9), (256, 512, 1, 8), (128, 128, 2, 5), (1024, 1024, 1, 4),
                                         (2048, 2048, 1, 3), (64, 4096, 1, 2)])
def test_spectral_call_complex128(pa, m, n, Q, count):
    """the grouped wavelength kernels for float64 maps (complex128 transforms; rows of up to 2048 samples -- longer rows keep the loop):
    against the loop they replace and the fp64 oracle sum, every group size and kernel form"""
    from prysm_amd import _lib, _ops
    P = pa.propagation
    lib = _lib.load()
    rng = np.random.default_rng(m + 3 * n + count)
    amp = (rng.random((m, n)) > 0.25).astype(np.float64)
    opd = 200 * rng.standard_normal((m, n))
    packed = _ops.pack_amp_opd(torch.from_numpy(amp).cuda(), torch.from_numpy(opd).cuda())
    assert packed.dtype == torch.complex128
    wvls = np.linspace(0.5, 0.7, count)
    ks = [2 * np.pi / w / 1e3 for w in wvls]
    wts = list(np.linspace(0.5, 1.5, count))
    M, N = int(m * Q), int(n * Q)
    loop = torch.zeros((M, N), device='cuda', dtype=torch.float64)
    for k, w in zip(ks, wts):
        P.focus_intensity(packed, Q, out=loop, weight=w, synth=('packed', k))
    want = sum(w * O.intensity(O.focus(O.from_amp_and_phase(amp, opd, float(wl)), Q)) for wl, w in zip(wvls, wts))
    assert rel_max(tonp(loop), want) < 4 * TOL64
    try:
        for group in (1, 3, 8):
            for mode in (0, 1, 2, 3):
                assert lib.pm_set_tuning(b'spectral', group) == 0
                if lib.pm_set_tuning(b'spectral_mode', mode) != 0:
                    assert mode != 3
                    continue
                got = torch.zeros((M, N), device='cuda', dtype=torch.float64)
                P.focus_intensity(packed, Q, out=got, synth=('packed', ks[0]), spectral=(ks, wts))
                assert rel_max(tonp(got), tonp(loop)) < 1e-13, (group, mode)
                assert rel_max(tonp(got), want) < 4 * TOL64, (group, mode)
    finally:
        lib.pm_set_tuning(b'spectral', 8)
        lib.pm_set_tuning(b'spectral_mode', 3)


def test_spectral_call_config5_shape_vs_numpy(pa):
    """pm_fft2_spectral at BASELINE config 5's shape (4096^2 fp32 maps, Q = 1) on the default route: 5 wavelengths against numpy fp64
    and against the loop; the knob of the removed grouped kernels is refused"""
    from prysm_amd import _lib, _ops
    from prysm_amd.propagation import focus_intensity
    lib = _lib.load()
    assert lib.pm_set_tuning_local(b'spectral2', 4) == _lib.PM_ERR_UNSUPPORTED
    lib.pm_reset_tuning_local()
    n = 4096
    rng = np.random.default_rng(5)
    ax = (np.arange(n) - n // 2) * (10.0 / n)
    r = np.hypot(ax[None, :], ax[:, None])
    amp = (r <= 5).astype(np.float32)
    opd = (500.0 * (r / 5) ** 4 + 5 * rng.standard_normal((n, n))).astype(np.float32)
    wl = np.linspace(0.5, 0.7, 5)
    ks = [2 * math.pi / w / 1e3 for w in wl]
    wts = [1.0, 0.5, 2.0, 1.5, 0.75]
    packed = _ops.pack_amp_opd(torch.from_numpy(amp).cuda(), torch.from_numpy(opd).cuda())

    def run(**knobs):
        acc = torch.zeros((n, n), device='cuda', dtype=torch.float32)
        with _lib.tuning_local(**knobs):
            focus_intensity(packed, 1, out=acc, synth=('packed', ks[0]), spectral=(ks, wts))
        return acc.cpu().numpy().astype(np.float64)

    ref = _poly_numpy(amp, opd, ks, wts, 1)
    loop = run(spectral=1)
    assert rel_max(loop, ref) < 2 * TOL32
    assert rel_max(run(), loop) < 1e-6


def test_packed_pupil_cache_is_per_stream(pa):
    from prysm_amd import polychromatic as pc
    amp = torch.ones((64, 64), device='cuda')
    opd = torch.randn((64, 64), device='cuda')
    pc.clear_packed_pupil_cache()
    a = pc.packed_pupil(amp, opd, amp, opd, cache=True)
    assert pc.packed_pupil(amp, opd, amp, opd, cache=True) is a
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = pc.packed_pupil(amp, opd, amp, opd, cache=True)
        assert b is not a and pc.packed_pupil(amp, opd, amp, opd, cache=True) is b
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(a, b)
    pc.clear_packed_pupil_cache()


def test_root_only_reduce_forms_on_a_one_rank_group(pa):
    """'reduce', 'a2a' and 'rs' on RCCL with a process group of one rank: every collective of the 8-GPU path executes here
    (all_to_all_single, reduce_scatter_tensor, gather into views of the image), twice (the receive buffers are kept)"""
    import os
    import socket
    import torch.distributed as dist
    from prysm_amd.polychromatic import _reduce_image
    if dist.is_initialized():
        pytest.skip('a process group is already up in this process')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        img = torch.rand((512, 512), device='cuda')
        for method in ('reduce', 'a2a', 'rs'):
            for _ in range(2):
                acc = img.clone()
                out = _reduce_image(acc, 1, None, False, method=method, use_dist=True)
                torch.cuda.synchronize()
                assert out is acc and torch.equal(out, img)
    finally:
        dist.destroy_process_group()
