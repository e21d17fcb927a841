"""The references of tests/test_gpu_pointwise.py checked on the host: if these are wrong, the GPU tests prove nothing."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import pointwise_common as PC
from oracle import prysm_oracle as O

# 20 hand-picked turns: zero, the quadrant points, just either side of them, negative values, fractions that no binary float holds,
# fp32 / fp64 values with many turns, and integers and half-integers far beyond 2^53 where a float reduction has no fraction left
TURNS = [
    Fraction(0), Fraction(1, 4), Fraction(1, 2), Fraction(3, 4), Fraction(1), Fraction(-1, 4), Fraction(1, 3), Fraction(-2, 7),
    Fraction(1, 8) + Fraction(1, 2 ** 60), Fraction(1, 2) - Fraction(1, 2 ** 70), Fraction(float(np.float32(159154.94))), Fraction(-159154.94309189534),
    Fraction(float(np.float32(1e6)) * 0.15915494309189535), Fraction(12345678901234567890, 7), Fraction(10 ** 30) + Fraction(1, 6),
    Fraction(-(10 ** 40)) - Fraction(5, 12), Fraction(2 ** 80 + 1, 2), Fraction(3 * 2 ** 200 + 1, 8), Fraction(1e-30), Fraction(-1e300) / 3,
]


def test_exact_unit_phase_against_mpmath():
    assert len(TURNS) == 20
    with mpmath.workdps(400):       # enough digits to carry 1e300 turns into the fraction without the exact reduction
        for t in TURNS:
            x = 2 * mpmath.pi * mpmath.mpf(t.numerator) / mpmath.mpf(t.denominator)
            want_c, want_s = mpmath.cos(x), mpmath.sin(x)
            c, s = PC.exact_unit_phase(t)
            assert abs(c - want_c) < mpmath.mpf(10) ** -38 and abs(s - want_s) < mpmath.mpf(10) ** -38, t


def test_exact_unit_phase_exact_points():
    assert PC.exact_unit_phase(Fraction(5, 4)) == (0, 1)
    assert PC.exact_unit_phase(Fraction(-7, 2)) == (-1, 0)
    assert PC.exact_unit_phase(Fraction(10 ** 50)) == (1, 0)


def test_phase_errors_and_bound_tell_fp32_phase_from_fp64():
    """a phase formed in fp32 at 1e6 rad misses the bound by orders of magnitude; one formed in fp64 meets it"""
    rng = np.random.default_rng(5)
    opd = (rng.uniform(-1, 1, 64) * 1e6).astype(np.float32)
    k2 = 1.0 / (2 * math.pi)
    turns = [Fraction(float(o)) * Fraction(k2) for o in opd]
    good = np.exp(2j * np.pi * np.array([float(t - round(t)) for t in turns])).astype(np.complex64)
    bad = np.exp(2j * np.pi * (opd * np.float32(k2)).astype(np.float64)).astype(np.complex64)
    bound = PC.phase_bound(np.float32, turns)
    assert bound.max() < 7e-8
    assert (PC.phase_errors(good, turns) <= bound).all()
    assert PC.phase_errors(bad, turns).max() > 1e3 * bound.max()


@pytest.mark.parametrize('mode', [1, 2, 3, 4])
@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (4, 1), (3, 5)])
def test_pad_reference_against_numpy(mode, shape):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape)
    m, n = shape
    for before, after in (((0, 0), (0, 0)), ((1, 0), (0, 1)), ((m - 1, n), (m, n - 1)), ((3 * m + 2, 3 * n + 2), (3 * m + 2, 1)),
                          ((2 * m, 5 * n + 1), (7, 4 * n))):
        want = np.pad(x, ((before[0], after[0]), (before[1], after[1])), mode=PC.PAD_MODES[mode])
        assert np.array_equal(PC.ref_pad_index(x, before, after, mode), want), (before, after)


def test_embed_reference():
    x = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(PC.ref_embed(x, (5, 6), (1, 1), -1.0), np.pad(x, ((1, 1), (1, 1)), constant_values=-1.0))
    assert np.array_equal(PC.ref_embed(x, (2, 2), (-1, -2), 9.0), x[1:3, 2:4])
    assert np.array_equal(PC.ref_embed(x, (2, 7), (-1, 2), 9.0), np.pad(x[1:3], ((0, 0), (2, 1)), constant_values=9.0))
    assert np.array_equal(PC.ref_embed(x, (2, 2), (5, 0), 9.0), np.full((2, 2), 9.0))
    assert np.array_equal(PC.ref_embed(x, (2, 2), (0, -4), 9.0), np.full((2, 2), 9.0))


def test_ee_reference_against_oracle():
    rng = np.random.default_rng(3)
    psf = rng.random((8, 8)) + 0.05
    dx = 2.5
    radii_um = np.array([0.0, 1.5, 7.0, 40.0])
    mtf = O.mtf_from_psf(psf)
    df = 1000 / (psf.shape[0] * dx)
    got = PC.ref_encircled_energy(mtf, df, radii_um / 1e3)
    want = O.encircled_energy(psf, dx, radii_um)
    assert got[0] == 0.0
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    # the adjoint reference is the gradient of the forward one: <EE(m), w> = <m, adj(w)>
    w = rng.standard_normal(4)
    adj = PC.ref_encircled_energy_adjoint(mtf.shape, df, radii_um / 1e3, w)
    assert abs(np.dot(got, w) - np.sum(mtf * adj)) <= 1e-13 * np.sum(np.abs(mtf * adj))


def test_window_guards_notice_a_stray_store():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.complex128, np.uint8):
        w = PC.window((3, 5), dtype, ld_pad=2, base_off=1, rng=rng, device='cpu')
        assert w.ld == 7 and w.start - 1 >= w.ld + 64 and (w.start - 1) % 16 == 0
        w.check_guards()
        w.set(PC.random_values(rng, (3, 5), dtype))      # the window itself may change
        w.check_guards()
        for at in (w.start - 1, w.start + 5, w.start + 3 * w.ld, w.total - 1, 0):
            flat = w.host().copy()
            flat[at] = 0
            keep = w.buf.clone()
            w.buf.copy_(torch.from_numpy(flat.view(np.uint8)))
            with pytest.raises(AssertionError):
                w.check_guards()
            w.buf.copy_(keep)
    with pytest.raises(ValueError):
        PC.window((3, 5), np.float32, ld_pad=-1, device='cpu')
