// The detector (prysm/detector.py) (gfx950):
//
//  - pm_detector_expose: Detector.expose fused -- per pixel the Poisson mean (img * t * prnu + dark * t * dcnu) and the constants of
//    its sampler ONCE, then a loop over frames: shot electrons (exact Poisson), read noise (Box-Muller), + bias, full well, gain,
//    ADC clip, truncating cast, look-up table, and ONE store of the sample in its final width (1, 2, 4 or 8 bytes).  A lane owns a
//    pixel, so every frame's store of a wave is one contiguous run; small images spread chunks of frames over grid.y.
//  - pm_detector_digitize: the deterministic tail alone, on electrons the caller brings.
//  - pm_detector_words: the raw Philox words of a range of pixels (what the tests pin the generator with).
//  - pm_bindown / pm_tile: bindown and its adjoint, one launch each, no atomics, a fixed summation order.
//
// Random numbers are Philox4x32-10 (Salmon et al., SC'11), integer arithmetic only: key = seed, counter = (pixel low, pixel high,
// exposure index + frame, draw block).  Block 0 of a sample is its read noise, block 1 + j attempt j of its shot noise.  The shot
// noise is exact at every mean: inversion by sequential search below 10, Hoermann's PTRS transformed rejection from 10 on; log k! is
// a table below 32 and four terms of Stirling's series above.  The rejection loop diverges within a wave (accepted: DESIGN.md).
// The exposure index is read from a device state word and advanced by a one-thread kernel after the launch, so a captured graph
// draws fresh frames on every replay.  A negative, NaN or infinite mean sets a status word (a plain store of 1) and draws 0.
//
// prysm_amd/detector_plan.py is this file in numpy, operation by operation.  The unit is compiled with -ffp-contract=off
// (csrc/Makefile) so that every product and sum is rounded by itself, as numpy does; all thresholds and sums are fp64.
#include <cmath>

#include "pm_entry.h"
#include "pm_philox.h"      // Words, philox4x32, uniform53

namespace pm {
namespace {

constexpr int kThreads = 256;
constexpr double kPtrsMin = 10.0;        // detector_plan.PTRS_MIN
constexpr int kInversionMaxK = 200;      // detector_plan.INVERSION_MAX_K
constexpr int kPtrsMaxAttempts = 256;    // detector_plan.PTRS_MAX_ATTEMPTS
constexpr double kTwoPi = 6.283185307179586, kHalfLog2Pi = 0.9189385332046727;
constexpr double kSt1 = 0.08333333333333333, kSt2 = 0.002777777777777778, kSt3 = 0.0007936507936507937;
constexpr int kLogFactN = 32;
__constant__ double kLogFact[kLogFactN] = {
    0.0, 0.0, 0.693147180559945, 1.7917594692280554, 3.178053830347945, 4.787491742782047, 6.579251212010102, 8.525161361065415,
    10.604602902745249, 12.801827480081467, 15.104412573075514, 17.502307845873887, 19.987214495661885, 22.55216385312342,
    25.191221182738683, 27.89927138384089, 30.671860106080672, 33.50507345013689, 36.39544520803305, 39.339884187199495,
    42.335616460753485, 45.38013889847691, 48.47118135183522, 51.60667556776438, 54.78472939811232, 58.00360522298052,
    61.26170176100201, 64.55753862700634, 67.88974313718153, 71.257038967168, 74.65823634883017, 78.0922235533153};

// the stream of one sample: key = seed, counter = (pixel, global frame, block)
struct Stream {
    uint32_t k0, k1, p0, p1, frame;
    __device__ __forceinline__ Words block(uint32_t b) const { return philox4x32(p0, p1, frame, b, k0, k1); }
};

__device__ __forceinline__ double log_factorial(double k) {
    if (k < double(kLogFactN)) return kLogFact[int(k)];
    const double x = k + 1.0, x2 = x * x;
    const double corr = (kSt1 - (kSt2 - kSt3 / x2) / x2) / x;
    return (x - 0.5) * log(x) - x + kHalfLog2Pi + corr;
}

// what depends on the pixel alone
struct Sampler {
    int regime;              // 0: no draw (mean 0 electrons by rule: an invalid mean), 1: inversion, 2: PTRS
    double mean, p0;         // inversion: p0 = exp(-mean)
    double loglam, a, b, log_invalpha, vr;
};

__device__ __forceinline__ Sampler make_sampler(double mean, bool ok) {
    Sampler s;
    s.mean = mean;
    s.regime = !ok ? 0 : mean < kPtrsMin ? 1 : 2;
    s.p0 = s.loglam = s.a = s.b = s.log_invalpha = s.vr = 0.0;
    if (s.regime == 1) s.p0 = exp(-mean);
    if (s.regime == 2) {
        const double slam = sqrt(mean);
        s.loglam = log(mean);
        s.b = 0.931 + 2.53 * slam;
        s.a = -0.059 + 0.02483 * s.b;
        s.log_invalpha = log(1.1239 + 1.1328 / (s.b - 3.4));
        s.vr = 0.9277 - 3.6224 / (s.b - 2.0);
    }
    return s;
}

__device__ __forceinline__ double poisson_draw(const Sampler& s, const Stream& st) {
    if (s.regime == 0) return 0.0;
    if (s.regime == 1) {
        const Words w = st.block(1);
        const double u = uniform53(w.w[0], w.w[1]);
        double p = s.p0, sum = p, k = 0.0;
        while (u > sum && k < double(kInversionMaxK)) {
            k += 1.0;
            p = p * s.mean / k;
            sum += p;
        }
        return k;
    }
    for (int j = 0; j < kPtrsMaxAttempts; ++j) {
        const Words w = st.block(1 + j);
        const double U = uniform53(w.w[0], w.w[1]) - 0.5, V = uniform53(w.w[2], w.w[3]);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * s.a / us + s.b) * U + s.mean + 0.43);
        if (us >= 0.07 && V <= s.vr) return k;
        if (!(k >= 0.0) || (us < 0.013 && V > us)) continue;
        const double lhs = log(V) + s.log_invalpha - log(s.a / (us * us) + s.b);
        const double rhs = -s.mean + k * s.loglam - log_factorial(k);
        if (lhs <= rhs) return k;
    }
    return floor(s.mean);
}

__device__ __forceinline__ double normal_draw(const Stream& st) {
    const Words w = st.block(0);
    const double ua = uniform53(w.w[0], w.w[1]), ub = uniform53(w.w[2], w.w[3]);
    return sqrt(-2.0 * log(1.0 - ua)) * cos(kTwoPi * ub);
}

struct Tail {
    double bias, fwc, inv_gain, cap;
    const void* lut;
};

// + bias, full well, gain as a multiply, ADC clip, truncation toward zero; then the LUT (elements of sizeof(O) bytes)
template <typename O>
__device__ __forceinline__ O digitize(double electrons, const Tail& t) {
    double x = electrons + t.bias;
    if (x > t.fwc) x = t.fwc;
    double y = x * t.inv_gain;
    if (!(y > 0.0)) y = 0.0;
    if (y > t.cap) y = t.cap;
    const uint32_t dn = uint32_t(y);
    return t.lut ? static_cast<const O*>(t.lut)[dn] : O(dn);
}

struct ExposeArgs {
    int64_t npix, plane, nx;         // pixels of the whole stack, of one image, of one row
    const void* img;
    int64_t ld, bstride;
    const double* prnu;
    const double* dcnu;
    double t, dark_t, read_noise;
    Tail tail;
    int64_t frames, fchunk;
    uint64_t seed;
    int64_t pixel_offset;
    int64_t* state;                  // [0] exposure index (frames exposed so far), [1] status: 1 after an invalid mean
    void* out;
};

template <typename T, typename O>
__global__ __launch_bounds__(kThreads) void expose_kernel(ExposeArgs a) {
    const int64_t p = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p >= a.npix) return;
    const int64_t b = p / a.plane, rem = p - b * a.plane, r = rem / a.nx, c = rem - r * a.nx;
    double e = double(static_cast<const T*>(a.img)[b * a.bstride + r * a.ld + c]) * a.t;
    if (a.prnu) e = e * a.prnu[rem];
    double d = a.dark_t;
    if (a.dcnu) d = d * a.dcnu[rem];
    const double mean = e + d;
    const bool ok = mean >= 0.0 && mean < INFINITY;
    if (!ok) a.state[1] = 1;
    const Sampler s = make_sampler(mean, ok);
    const int64_t exposure = a.state[0];
    const uint64_t pid = uint64_t(a.pixel_offset + p);
    Stream st;
    st.k0 = uint32_t(a.seed), st.k1 = uint32_t(a.seed >> 32), st.p0 = uint32_t(pid), st.p1 = uint32_t(pid >> 32);
    const int64_t f0 = int64_t(blockIdx.y) * a.fchunk, f1 = f0 + a.fchunk < a.frames ? f0 + a.fchunk : a.frames;
    O* __restrict__ out = static_cast<O*>(a.out) + p;
    for (int64_t f = f0; f < f1; ++f) {
        st.frame = uint32_t(uint64_t(exposure + f));
        double el = poisson_draw(s, st);
        if (a.read_noise != 0.0) el = el + normal_draw(st) * a.read_noise;
        out[f * a.npix] = digitize<O>(el, a.tail);
    }
}

// after the exposure, on the same stream: the next call (or the next replay of a graph) continues the sequence
__global__ void advance_kernel(int64_t* state, int64_t frames) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] = state[0] + frames;
}

template <typename T, typename O>
__global__ __launch_bounds__(kThreads) void digitize_kernel(int64_t n, int64_t plane, int64_t nx, const T* __restrict__ in, int64_t ld,
                                                            int64_t bstride, Tail tail, O* __restrict__ out) {
    const int64_t p = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p >= n) return;
    const int64_t b = p / plane, rem = p - b * plane, r = rem / nx, c = rem - r * nx;
    out[p] = digitize<O>(double(in[b * bstride + r * ld + c]), tail);
}

__global__ __launch_bounds__(kThreads) void words_kernel(uint64_t seed, int64_t pixel0, int64_t npix, uint32_t frame, uint32_t block,
                                                         uint32_t* __restrict__ out) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= npix) return;
    const uint64_t pid = uint64_t(pixel0 + i);
    const Words w = philox4x32(uint32_t(pid), uint32_t(pid >> 32), frame, block, uint32_t(seed), uint32_t(seed >> 32));
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * i + j] = w.w[j];
}

// ---------------------------------------------------------------- bindown / tile
// One output element per lane: its bin is fy rows of fx consecutive inputs, read in pieces of C elements (16 bytes when the factor and
// the alignment allow: a wave instruction then covers 1 KiB of one input row), summed into ONE running sum, rows in order, left to
// right.  grid.y: the member of a stack.
template <typename T, int C>
__global__ __launch_bounds__(kThreads) void bindown_kernel(int64_t my, int64_t nx, int64_t fy, int64_t fx, int avg, const T* __restrict__ in,
                                                           int64_t in_ld, int64_t in_bstride, T* __restrict__ out, int64_t out_ld,
                                                           int64_t out_bstride) {
    using cv = T __attribute__((ext_vector_type(C)));
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= my * nx) return;
    const int64_t r = i / nx, c = i - r * nx;
    const T* __restrict__ src = in + int64_t(blockIdx.y) * in_bstride + r * fy * in_ld + c * fx;
    T acc = T(0);
    for (int64_t j = 0; j < fy; ++j) {
        const T* __restrict__ row = src + j * in_ld;
        for (int64_t k = 0; k < fx; k += C) {
            if (C == 1) {
                acc = acc + row[k];
            } else {
                const cv v = *reinterpret_cast<const cv*>(row + k);
#pragma unroll
                for (int q = 0; q < C; ++q) acc = acc + v[q];
            }
        }
    }
    if (avg) acc = acc / T(fy * fx);
    out[int64_t(blockIdx.y) * out_bstride + r * out_ld + c] = acc;
}

// out (my fy x nx fx) from in (my x nx): one output element per lane, the input through the cache
template <typename T>
__global__ __launch_bounds__(kThreads) void tile_kernel(int64_t oy, int64_t ox, int64_t fy, int64_t fx, T scale, int scaled,
                                                        const T* __restrict__ in, int64_t in_ld, int64_t in_bstride, T* __restrict__ out,
                                                        int64_t out_ld, int64_t out_bstride) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= oy * ox) return;
    const int64_t r = i / ox, c = i - r * ox;
    T v = in[int64_t(blockIdx.y) * in_bstride + (r / fy) * in_ld + c / fx];
    if (scaled) v = v * scale;
    out[int64_t(blockIdx.y) * out_bstride + r * out_ld + c] = v;
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }
bool width_ok(int32_t out_bytes) { return out_bytes == 1 || out_bytes == 2 || out_bytes == 4 || out_bytes == 8; }

// the checks pm_detector_expose and pm_detector_digitize share; returns 0 or the failure
int check_tail(const char* who, int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* in, int64_t ld, int64_t bstride,
               double conversion_gain, int32_t bits, const void* lut, int64_t lut_len, int32_t out_bytes, const void* out) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (bits < 1 || bits > 32) return fail(PM_ERR_ARG, "%s: bits must be in 1 .. 32, got %d", who, int(bits));
    if (batch < 0 || ny < 0 || nx < 0 || !in || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (ld < nx) return fail(PM_ERR_ARG, "%s: ld %lld is smaller than the row of %lld", who, (long long)ld, (long long)nx);
    if (!stack_ok(batch, ny, ld, bstride)) return fail(PM_ERR_ARG, "%s: bstride: the members of a stack would overlap", who);
    if (!(conversion_gain != 0.0) || !std::isfinite(conversion_gain)) return fail(PM_ERR_ARG, "%s: conversion_gain must be finite and not 0", who);
    if (!width_ok(out_bytes)) return fail(PM_ERR_ARG, "%s: out_bytes must be 1, 2, 4 or 8", who);
    if (lut && lut_len < (int64_t(1) << bits))
        return fail(PM_ERR_ARG, "%s: the look-up table has %lld entries, %d bits need %lld", who, (long long)lut_len, int(bits),
                    (long long)(int64_t(1) << bits));
    if (!lut && out_bytes * 8 < bits) return fail(PM_ERR_ARG, "%s: %d bits do not fit into %d output bytes", who, int(bits), int(out_bytes));
    if (ny > INT32_MAX || nx > INT32_MAX || batch > INT32_MAX || blocks_of(batch * ny * nx) > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: %lld x %lld x %lld is too large", who, (long long)batch, (long long)ny, (long long)nx);
    return 0;
}

Tail make_tail(double bias, double fwc, double conversion_gain, int32_t bits, const void* lut) {
    Tail t;
    t.bias = bias, t.fwc = fwc, t.inv_gain = 1 / conversion_gain, t.cap = double((int64_t(1) << bits) - 1), t.lut = lut;
    return t;
}

// shared by pm_bindown and pm_tile: (my, nx) is the SMALL array, the large one is (my fy, nx fx)
int check_bin(const char* who, int32_t dtype, int64_t batch, int64_t my, int64_t nx, int64_t fy, int64_t fx, const void* in, int64_t big_ld,
              int64_t big_bstride, int64_t small_ld, int64_t small_bstride, const void* out) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (fy < 1 || fx < 1) return fail(PM_ERR_ARG, "%s: the factors must be at least 1, got %lld and %lld", who, (long long)fy, (long long)fx);
    if (batch < 0 || my < 0 || nx < 0 || !in || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (my > INT32_MAX || nx > INT32_MAX || fy > INT32_MAX || fx > INT32_MAX || my * fy > INT32_MAX || nx * fx > INT32_MAX || batch > 65535 ||
        blocks_of(my * fy * nx * fx) > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: %lld x %lld by %lld x %lld (stack of %lld) is too large", who, (long long)my, (long long)nx, (long long)fy,
                    (long long)fx, (long long)batch);
    if (big_ld < nx * fx || small_ld < nx) return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than its row", who);
    if (!stack_ok(batch, my * fy, big_ld, big_bstride) || !stack_ok(batch, my, small_ld, small_bstride))
        return fail(PM_ERR_ARG, "%s: bstride: the members of a stack would overlap", who);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_bindown(int32_t dtype, int64_t batch, int64_t my, int64_t nx, int64_t fy, int64_t fx, int32_t mode, const void* in, int64_t in_ld,
               int64_t in_bstride, void* out, int64_t out_ld, int64_t out_bstride, void* stream) {
    if (mode != PM_BIN_AVG && mode != PM_BIN_SUM) return fail(PM_ERR_ARG, "pm_bindown: mode must be PM_BIN_AVG or PM_BIN_SUM");
    if (int rc = check_bin("pm_bindown", dtype, batch, my, nx, fy, fx, in, in_ld, in_bstride, out_ld, out_bstride, out)) return rc;
    if (batch == 0 || my == 0 || nx == 0) return 0;
    return by_rdtype(dtype, "pm_bindown", [&](auto real) {
        using T = decltype(real);
        const size_t es = sizeof(T);
        // pieces of C elements: the factor is a multiple of C and every bin row starts on a multiple of C * es bytes
        auto fits = [&](int C) { return fx % C == 0 && aligned(in, C * es) && (in_ld * es) % (C * es) == 0 && (in_bstride * es) % (C * es) == 0; };
        auto launch = [&](auto pieces) {
            hipLaunchKernelGGL((bindown_kernel<T, decltype(pieces)::value>), dim3(unsigned(blocks_of(my * nx)), unsigned(batch)), dim3(kThreads), 0,
                               PM_STREAM(stream), my, nx, fy, fx, mode == PM_BIN_AVG, static_cast<const T*>(in), in_ld, in_bstride,
                               static_cast<T*>(out), out_ld, out_bstride);
        };
        if (16 / es >= 4 && fits(4))
            launch(std::integral_constant<int, 4>{});
        else if (fits(2))
            launch(std::integral_constant<int, 2>{});
        else
            launch(std::integral_constant<int, 1>{});
        return int(hipGetLastError());
    });
}

int pm_tile(int32_t dtype, int64_t batch, int64_t my, int64_t nx, int64_t fy, int64_t fx, double scale, const void* in, int64_t in_ld,
            int64_t in_bstride, void* out, int64_t out_ld, int64_t out_bstride, void* stream) {
    if (!std::isfinite(scale)) return fail(PM_ERR_ARG, "pm_tile: scale must be finite");
    if (int rc = check_bin("pm_tile", dtype, batch, my, nx, fy, fx, in, out_ld, out_bstride, in_ld, in_bstride, out)) return rc;
    if (batch == 0 || my == 0 || nx == 0) return 0;
    return by_rdtype(dtype, "pm_tile", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(tile_kernel<T>, dim3(unsigned(blocks_of(my * fy * nx * fx)), unsigned(batch)), dim3(kThreads), 0, PM_STREAM(stream),
                           my * fy, nx * fx, fy, fx, T(scale), scale != 1.0, static_cast<const T*>(in), in_ld, in_bstride, static_cast<T*>(out),
                           out_ld, out_bstride);
        return int(hipGetLastError());
    });
}

int pm_detector_digitize(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* electrons, int64_t ld, int64_t bstride, double bias,
                         double fwc, double conversion_gain, int32_t bits, const void* lut, int64_t lut_len, int32_t out_bytes, void* out,
                         void* stream) {
    if (int rc = check_tail("pm_detector_digitize", dtype, batch, ny, nx, electrons, ld, bstride, conversion_gain, bits, lut, lut_len, out_bytes, out))
        return rc;
    const int64_t n = batch * ny * nx;
    if (n == 0) return 0;
    const Tail t = make_tail(bias, fwc, conversion_gain, bits, lut);
    return by_rdtype(dtype, "pm_detector_digitize", [&](auto real) {
        return by_uint_bytes(out_bytes, "pm_detector_digitize", [&](auto sample) {
            using T = decltype(real);
            using O = decltype(sample);
            hipLaunchKernelGGL((digitize_kernel<T, O>), dim3(unsigned(blocks_of(n))), dim3(kThreads), 0, PM_STREAM(stream), n, ny * nx, nx,
                               static_cast<const T*>(electrons), ld, bstride, t, static_cast<O*>(out));
            return int(hipGetLastError());
        });
    });
}

int pm_detector_expose(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* img, int64_t ld, int64_t bstride, const void* prnu,
                       const void* dcnu, double exposure_time, double dark_current, double read_noise, double bias, double fwc,
                       double conversion_gain, int32_t bits, const void* lut, int64_t lut_len, int32_t out_bytes, int64_t frames, int64_t seed,
                       int64_t pixel_offset, void* state, void* out, void* stream) {
    if (int rc = check_tail("pm_detector_expose", dtype, batch, ny, nx, img, ld, bstride, conversion_gain, bits, lut, lut_len, out_bytes, out))
        return rc;
    if (!state) return fail(PM_ERR_ARG, "pm_detector_expose: the state tensor is missing (null pointer)");
    if (frames < 0 || frames > INT32_MAX) return fail(PM_ERR_ARG, "pm_detector_expose: frames must be in 0 .. 2^31 - 1");
    if (pixel_offset < 0) return fail(PM_ERR_ARG, "pm_detector_expose: pixel_offset must not be negative");
    if (!std::isfinite(exposure_time) || !std::isfinite(dark_current) || !std::isfinite(read_noise))
        return fail(PM_ERR_ARG, "pm_detector_expose: exposure_time, dark_current and read_noise must be finite");
    const int64_t npix = batch * ny * nx;
    if (npix == 0 || frames == 0) return 0;
    ExposeArgs a;
    a.npix = npix, a.plane = ny * nx, a.nx = nx, a.img = img, a.ld = ld, a.bstride = bstride;
    a.prnu = static_cast<const double*>(prnu), a.dcnu = static_cast<const double*>(dcnu);
    a.t = exposure_time, a.dark_t = dark_current * exposure_time, a.read_noise = read_noise;
    a.tail = make_tail(bias, fwc, conversion_gain, bits, lut);
    a.frames = frames, a.seed = uint64_t(seed), a.pixel_offset = pixel_offset, a.state = static_cast<int64_t*>(state), a.out = out;
    // frames of a small image are spread over grid.y until about 2048 workgroups (8 per CU) are in flight
    const int64_t blocks = blocks_of(npix);
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(frames, 2048 / blocks));
    a.fchunk = (frames + chunks - 1) / chunks;
    const dim3 grid{unsigned(blocks), unsigned((frames + a.fchunk - 1) / a.fchunk)};
    hipStream_t st = PM_STREAM(stream);
    const int rc = by_rdtype(dtype, "pm_detector_expose", [&](auto real) {
        return by_uint_bytes(out_bytes, "pm_detector_expose", [&](auto sample) {
            hipLaunchKernelGGL((expose_kernel<decltype(real), decltype(sample)>), grid, dim3(kThreads), 0, st, a);
            return int(hipGetLastError());
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(advance_kernel, dim3{1}, dim3{64}, 0, st, a.state, frames);
    return int(hipGetLastError());
}

int pm_detector_words(int64_t seed, int64_t pixel0, int64_t npix, int64_t frame, int32_t block, void* out, void* stream) {
    if (npix < 0 || pixel0 < 0 || frame < 0 || block < 0 || !out)
        return fail(PM_ERR_ARG, "pm_detector_words: bad argument (null pointer or negative value)");
    if (blocks_of(npix) > INT32_MAX) return fail(PM_ERR_ARG, "pm_detector_words: %lld pixels are too many", (long long)npix);
    if (npix == 0) return 0;
    hipLaunchKernelGGL(words_kernel, dim3{unsigned(blocks_of(npix))}, dim3{kThreads}, 0, PM_STREAM(stream), uint64_t(seed), pixel0, npix,
                       uint32_t(uint64_t(frame)), uint32_t(block), static_cast<uint32_t*>(out));
    return int(hipGetLastError());
}

}  // extern "C"
