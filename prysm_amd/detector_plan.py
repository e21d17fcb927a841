"""The detector kernels restated in numpy, in the kernels' own operation order (csrc/detector.hip).

Host only: numpy, no torch, no device.  It is what the CPU tests check against the reference and against theory, and what the GPU
tests check the kernels against, bit for bit:

- philox4x32(counter, key): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).
- The stream of one sample.  key = the 64-bit seed (low word, high word); counter = (pixel low word, pixel high word, global frame
  index mod 2^32, draw block).  The global frame index is the exposure index (frames exposed before this call) plus the frame
  within the call, so F frames in one call are the next F single-frame calls.  Block 0 of a sample belongs to the read noise, block
  1 + j to the j-th attempt of the shot-noise sampler; a block is four 32-bit words = two 53-bit uniforms
  uniform53(w0, w1), uniform53(w2, w3), each in [0, 1).
- normal_walk: Box-Muller, sqrt(-2 log(1 - ua)) cos(2 pi ub), from block 0.
- poisson_walk: exact at every mean.  mean < PTRS_MIN: inversion by sequential search from the first uniform of block 1 (p = exp(-mean),
  then p = p * mean / k, cumulated in fp64).  mean >= PTRS_MIN: Hoermann's transformed rejection PTRS ("The transformed rejection method
  for generating Poisson random variables", Insurance: Mathematics and Economics 12, 1993), attempt j from block 1 + j; log k! comes
  from a table below LOGFACT_N and from four terms of Stirling's series above (truncation below 2e-16 relative), so the only library
  functions on the path are exp, log, sqrt, cos and floor.
- digitize: the deterministic tail of prysm's Detector.expose (prysm/detector.py:123-146), in fp64.
- expose_walk: mean, shot, read, digitize, as pm_detector_expose does it.
- bindown / tile: the two resampling kernels with their fixed summation order (row-major within a bin, one running sum).
"""
import numpy as np

PTRS_MIN = 10.0              # means below: inversion; from here on: PTRS (valid for mean >= 10)
INVERSION_MAX_K = 200        # the search stops here: P(k > 200 | mean < 10) < 1e-180, it only bounds the loop when u rounds above the cumulated sum
PTRS_MAX_ATTEMPTS = 256      # an attempt accepts with probability > 0.7: unreachable, it only bounds the loop; the floor of the mean is returned
TWO_PI = 6.283185307179586
HALF_LOG_2PI = 0.9189385332046727
ST1, ST2, ST3 = 0.08333333333333333, 0.002777777777777778, 0.0007936507936507937
LOGFACT_N = 32
# log k! for k < 32, the doubles csrc/detector.hip holds as well
LOGFACT = np.array([
    0.0, 0.0, 0.693147180559945, 1.7917594692280554, 3.178053830347945, 4.787491742782047, 6.579251212010102, 8.525161361065415,
    10.604602902745249, 12.801827480081467, 15.104412573075514, 17.502307845873887, 19.987214495661885, 22.55216385312342,
    25.191221182738683, 27.89927138384089, 30.671860106080672, 33.50507345013689, 36.39544520803305, 39.339884187199495,
    42.335616460753485, 45.38013889847691, 48.47118135183522, 51.60667556776438, 54.78472939811232, 58.00360522298052,
    61.26170176100201, 64.55753862700634, 67.88974313718153, 71.257038967168, 74.65823634883017, 78.0922235533153])

_M32 = np.uint64(0xFFFFFFFF)
_PM0, _PM1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PW0, _PW1 = 0x9E3779B9, 0xBB67AE85
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """Philox4x32: counter = four 32-bit words (arrays broadcast against each other), key = two.  Returns four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _M32 for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0, p1 = _PM0 * c0, _PM1 * c2            # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + _PW0) & 0xFFFFFFFF, (k1 + _PW1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform53(hi, lo):
    """two words -> a double in [0, 1) with 53 random bits: ((hi >> 5) 2^26 + (lo >> 6)) 2^-53, every step exact"""
    hi, lo = np.asarray(hi, dtype=np.uint32), np.asarray(lo, dtype=np.uint32)
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def seed_key(seed):
    """the 64-bit seed as Philox's key (low word, high word)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def sample_words(seed, exposure, frame, pixel, block):
    """the four words of one draw block of the samples (pixel, exposure + frame)"""
    pixel = np.asarray(pixel, dtype=np.int64).astype(np.uint64)
    gframe = (np.asarray(exposure, dtype=np.int64) + np.asarray(frame, dtype=np.int64)).astype(np.uint64)
    return philox4x32((pixel & _M32, pixel >> _S32, gframe & _M32, np.asarray(block, dtype=np.uint64)), seed_key(seed))


def sample_uniforms(seed, exposure, frame, pixel, block):
    w = sample_words(seed, exposure, frame, pixel, block)
    return uniform53(w[0], w[1]), uniform53(w[2], w[3])


def normal_walk(seed, exposure, frame, pixel):
    """standard normal of each sample (block 0)"""
    ua, ub = sample_uniforms(seed, exposure, frame, pixel, 0)
    return np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(TWO_PI * ub)


def log_factorial(k):
    """log k! for integer-valued doubles k >= 0: the table, or Stirling's series of x = k + 1"""
    k = np.asarray(k, dtype=np.float64)
    small = k < LOGFACT_N
    x = np.where(small, 40.0, k + 1.0)
    x2 = x * x
    corr = (ST1 - (ST2 - ST3 / x2) / x2) / x
    big = (x - 0.5) * np.log(x) - x + HALF_LOG_2PI + corr
    return np.where(small, LOGFACT[np.where(small, k, 0).astype(np.int64)], big)


def _inversion(mean, u):
    p = np.exp(-mean)
    s = p.copy()
    k = np.zeros(mean.shape)
    live = u > s
    while live.any():
        kk = k[live] + 1.0
        pp = p[live] * mean[live] / kk
        ss = s[live] + pp
        k[live], p[live], s[live] = kk, pp, ss
        live[live] = (u[live] > ss) & (kk < INVERSION_MAX_K)
    return k


def _ptrs(mean, seed, exposure, frame, pixel):
    slam, loglam = np.sqrt(mean), np.log(mean)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    log_invalpha = np.log(1.1239 + 1.1328 / (b - 3.4))
    vr = 0.9277 - 3.6224 / (b - 2.0)
    out = np.floor(mean)
    live = np.ones(mean.shape, dtype=bool)
    for j in range(PTRS_MAX_ATTEMPTS):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        U, V = sample_uniforms(seed, exposure[idx], frame[idx], pixel[idx], 1 + j)
        U = U - 0.5
        us = 0.5 - np.abs(U)
        m_, a_, b_ = mean[idx], a[idx], b[idx]
        with np.errstate(divide='ignore', invalid='ignore'):
            k = np.floor((2.0 * a_ / us + b_) * U + m_ + 0.43)
            quick = (us >= 0.07) & (V <= vr[idx])
            again = ~quick & ((k < 0) | ((us < 0.013) & (V > us)) | ~np.isfinite(k))
            kk = np.where(again | quick, 0.0, k)
            lhs = np.log(V) + log_invalpha[idx] - np.log(a_ / (us * us) + b_)
            rhs = -m_ + kk * loglam[idx] - log_factorial(kk)
            accept = quick | (~again & (lhs <= rhs))
        out[idx[accept]] = k[accept]
        live[idx[accept]] = False
    return out


def poisson_walk(mean, seed, exposure, frame, pixel, invalid='raise'):
    """Poisson counts (float64, integer-valued) of the samples (pixel, exposure + frame) with the given means; the arguments broadcast.
    A negative, NaN or infinite mean raises ValueError (numpy's rule), or gives 0 with invalid='zero' (the kernel's)."""
    mean, exposure, frame, pixel = np.broadcast_arrays(np.asarray(mean, dtype=np.float64), np.asarray(exposure, dtype=np.int64),
                                                       np.asarray(frame, dtype=np.int64), np.asarray(pixel, dtype=np.int64))
    shape = mean.shape
    mean, exposure, frame, pixel = mean.ravel(), exposure.ravel(), frame.ravel(), pixel.ravel()
    bad = ~((mean >= 0) & (mean < np.inf))
    if bad.any() and invalid == 'raise':
        raise ValueError('the mean of a Poisson draw is negative, NaN or infinite')
    out = np.zeros(mean.shape)
    lo = ~bad & (mean < PTRS_MIN)
    hi = ~bad & ~lo
    if lo.any():
        u, _ = sample_uniforms(seed, exposure[lo], frame[lo], pixel[lo], 1)
        out[lo] = _inversion(mean[lo], u)
    if hi.any():
        out[hi] = _ptrs(mean[hi], seed, exposure[hi], frame[hi], pixel[hi])
    return out.reshape(shape)


def container(bits, lut=None):
    """dtype of an exposure: the LUT's when there is one, else uint8 / uint16 / uint32 by bits; ValueError above 32 bits"""
    if bits > 32:
        raise ValueError("more than 32 unsigned bits are not supported (the reference: numpy's random functionality is inadequate)")
    if lut is not None:
        return np.asarray(lut).dtype
    return np.dtype(np.uint8 if bits <= 8 else np.uint16 if bits <= 16 else np.uint32)


def digitize(electrons, bias, fwc, conversion_gain, bits, lut=None):
    """electrons (any real dtype, widened to fp64) -> DN: + bias, clip at fwc, * (1 / conversion_gain), clip to [0, 2^bits - 1],
    truncating cast, LUT."""
    container(bits, lut)
    x = np.asarray(electrons).astype(np.float64) + float(bias)
    x = np.where(x > fwc, float(fwc), x)
    y = x * (1 / conversion_gain)
    cap = float(2 ** bits - 1)
    y = np.where(y < 0, 0.0, y)
    y = np.where(y > cap, cap, y)
    dn = y.astype(np.uint32)
    if lut is not None:
        return np.take(np.asarray(lut), dn)
    return dn.astype(container(bits))


def mean_electrons(img, exposure_time, dark_current, prnu=None, dcnu=None):
    """the Poisson mean per pixel, img * t * prnu + dark * t * dcnu in fp64; maps broadcast over a leading stack dimension"""
    e = np.asarray(img).astype(np.float64) * float(exposure_time)
    if prnu is not None:
        e = e * np.asarray(prnu, dtype=np.float64)
    d = float(dark_current) * float(exposure_time)
    if dcnu is not None:
        d = d * np.asarray(dcnu, dtype=np.float64)
    return e + d


def expose_walk(img, *, dark_current, read_noise, bias, fwc, conversion_gain, bits, exposure_time, prnu=None, dcnu=None, lut=None,
                seed=0, exposure=0, frames=1, pixel_offset=0, invalid='raise', parts=False):
    """pm_detector_expose in numpy: (frames, *img.shape) DN (frames == 1 is NOT squeezed here).  pixel index = pixel_offset + the
    row-major index into img (a stack counts on through its members).  parts=True returns (dn, shot, read, mean)."""
    mean = mean_electrons(img, exposure_time, dark_current, prnu, dcnu)
    pix = pixel_offset + np.arange(mean.size, dtype=np.int64).reshape(mean.shape)
    fr = np.arange(frames, dtype=np.int64).reshape((frames,) + (1,) * mean.ndim)
    shot = poisson_walk(mean[None], seed, exposure, fr, pix[None], invalid=invalid)
    if read_noise != 0:
        read = normal_walk(seed, exposure, fr, pix[None]) * float(read_noise)
        el = shot + read
    else:
        read = np.zeros(shot.shape)
        el = shot
    dn = digitize(el, bias, fwc, conversion_gain, bits, lut)
    return (dn, shot, read, mean) if parts else dn


# ---------------------------------------------------------------- bindown / tile
def factors_of(shape, factor):
    """the reference's factor rule (a number broadcasts to every axis) reduced to (stack shape, (fy, fx)): leading factors of an
    N-D array must be 1.  ValueError for a shape that is not a multiple (the reference fails inside reshape with the same type)."""
    ndim = len(shape)
    if ndim < 2:
        raise ValueError('bindown / tile take 2-D arrays or stacks of them')
    if isinstance(factor, (int, np.integer)):
        factor = (int(factor),) * ndim
    factor = tuple(int(f) for f in factor)
    if len(factor) != ndim:
        raise ValueError(f'{len(factor)} factors for an array of {ndim} dimensions')
    if any(f < 1 for f in factor):
        raise ValueError('binning factors must be positive integers')
    if any(f != 1 for f in factor[:-2]):
        raise NotImplementedError('only the last two axes are binned: the leading factors of a stack must be 1')
    return factor[-2], factor[-1]


def bin_mode(mode):
    m = str(mode).lower()
    if m in ('avg', 'average', 'mean'):
        return 'avg'
    if m == 'sum':
        return 'sum'
    raise ValueError('mode must be average or sum.')


def bindown(array, factor, mode='avg'):
    """pm_bindown in numpy: each bin is ONE running sum in the array's dtype, rows of the bin in order and left to right within a row;
    'avg' divides that sum by the count"""
    a = np.asarray(array)
    fy, fx = factors_of(a.shape, factor)
    mode = bin_mode(mode)
    m, n = a.shape[-2:]
    if m % fy or n % fx:
        raise ValueError(f'shape {a.shape} is not a multiple of the factors {(fy, fx)}')
    v = a.reshape(a.shape[:-2] + (m // fy, fy, n // fx, fx))
    acc = np.zeros(a.shape[:-2] + (m // fy, n // fx), dtype=a.dtype)
    for j in range(fy):
        for i in range(fx):
            acc = acc + v[..., :, j, :, i]
    if mode == 'avg':
        acc = acc / a.dtype.type(fy * fx)
    return acc


def tile(array, factor, scaling='sum'):
    """pm_tile in numpy: every element repeated fy x fx times, times 1 / (fy fx) for 'sum' (the adjoint of bindown 'avg'), times 1
    for 'avg' (the adjoint of bindown 'sum')"""
    a = np.asarray(array)
    fy, fx = factors_of(a.shape, factor)
    if scaling == 'sum':
        sf = 1 / (fy * fx)
    elif scaling in ('avg', 'average', 'mean'):
        sf = 1
    else:
        raise ValueError('scaling must be average or sum')
    out = np.repeat(np.repeat(a, fy, axis=-2), fx, axis=-1)
    return out * a.dtype.type(sf) if sf != 1 else out
