// Surfaces synthesised from a PSD (prysm/interferogram.py:333-432) (gfx950): the pointwise passes between the two transforms of
//     z = real(ifftshift(ifft2(fftshift(exp(i angle(fft2(rand))) sqrt(A psd))))) / (dx dy),  NaN outside a mask,  z *= rms / rms(z)
// on a stack of `batch` surfaces of rows x cols samples, rows `ld` and members `bstride` elements apart.
//
//  - pm_psd_uniform: uniform numbers in [0, 1) from Philox4x32-10 (pm_philox.h), key = seed, counter = (pixel low, pixel high,
//    surface index, 0) with pixel = row * cols + col: the layout of csrc/detector.hip with the surface where it has the frame.
//    float32: word 0 >> 8 times 2^-24 (24 bits); float64: ((word 0 >> 5) 2^26 + (word 1 >> 6)) 2^-53 (53 bits).  Every step exact.
//  - pm_psd_signal: in place on the spectrum X of the random numbers, X -> (X / |X|, or 1 where X == 0) sqrt(A psd).  The unit phasor
//    is exp(i angle(X)) without atan2 and sincos.  psd is read from an array shared by the stack, or evaluated from a model record:
//    the frequencies of forward_ft_unit(dxg, n) with the centre sample replaced by a tenth of the next one (interferogram.py:404-408),
//    their root sum of squares and abc_psd / ab_psd in double, rounded once to T.  |X|, the divide, A psd and the root are in T; a
//    negative psd gives NaN as in the reference.  complex64 rows are walked in 16-byte pairs with a scalar head and tail where the
//    row does not start on a 16-byte boundary; a complex128 element is 16 bytes by itself.
//  - pm_psd_finish: z = real(field), NaN where the mask predicate fails (none; an array of bytes; a circle hypot(x, y) <= radius on
//    make_xy_grid's coordinates T(c - cols / 2) T(step)), and per surface the count and the sum of squares of the finite pixels:
//    one launch that leaves a partial per workgroup, one launch of a workgroup per surface that folds them (pm_reduce.h: no atomics,
//    the same bits every run).  Sums are accumulated in double.
//  - pm_psd_scale: z *= rms / sqrt(sum z^2 / count), the sums read on the device; a surface with count 0 or sum 0 is left as it is.
//
// prysm_amd/psdsynth_plan.py restates every kernel in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile).
#include <cmath>
#include <limits>

#include "pm_entry.h"
#include "pm_math.h"
#include "pm_philox.h"
#include "pm_reduce.h"
#include "pm_sweep.h"

namespace pm {
namespace {

constexpr int kThreads = 256;
constexpr int kWgs = 1024;      // most workgroups per surface of the first stage of pm_psd_finish: as many partials per value
constexpr int kSums = 2;        // finite count, sum of squares

int groups(int64_t n) { return reduce_groups(n, kThreads, kWgs); }

bool too_large(int64_t m, int64_t n) { return m > INT32_MAX || n > INT32_MAX; }

template <typename T>
__device__ __forceinline__ bool finite_(T z) {
    return abs_(z) <= std::numeric_limits<T>::max();
}

// ---------------------------------------------------------------- uniform numbers
template <typename T>
struct UniformOp {
    T* out;
    int64_t ld, bstride, cols;
    uint32_t k0, k1;
    int64_t surface0;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t b, int64_t r, int64_t c, NoColumn) const {
        const uint64_t pixel = uint64_t(r * cols + c);
        const Words w = philox4x32(uint32_t(pixel), uint32_t(pixel >> 32), uint32_t(uint64_t(surface0 + b)), 0u, k0, k1);
        T u;
        if constexpr (sizeof(T) == 4)
            u = uniform24(w.w[0]);
        else
            u = uniform53(w.w[0], w.w[1]);
        out[b * bstride + r * ld + c] = u;
    }
};

// ---------------------------------------------------------------- signal
// element j of forward_ft_unit(dxg, n), unit = 1 / (n dxg), with render_synthetic_surface's replacement of the centre sample
__device__ __forceinline__ double freq_(int64_t j, int64_t n, double unit) { return j == n / 2 ? unit / 10.0 : double(j - n / 2) * unit; }

struct Model {
    int on, kind;
    double a, b, c, ux, uy;      // ux, uy: 1 / (cols dxg), 1 / (rows dxg)
};

template <typename T>
struct SignalOp {
    cx<T>* spec;
    int64_t ld, bstride, rows, cols;
    const T* psd;
    int64_t pld;
    Model m;
    T area;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ T density(int64_t r, int64_t c) const {
        if (!m.on) return psd[r * pld + c];
        const double fx = freq_(c, cols, m.ux), fy = freq_(r, rows, m.uy);
        const double nu = sqrt(fx * fx + fy * fy);
        return m.kind == PM_IFG_PSD_ABC ? T(m.a / (1.0 + pow(nu / m.b, m.c))) : T(m.a * pow(nu, -m.b));
    }

    __device__ __forceinline__ cx<T> shape(cx<T> X, int64_t r, int64_t c) const {
        const T amp = sqrt_(area * density(r, c));
        const T mag = hypot_(X.x, X.y);
        if (mag == T(0)) return cx<T>{amp, T(0) * amp};
        return cx<T>{X.x / mag * amp, X.y / mag * amp};
    }

    // `s` is a slot of the row: one element (complex128), or the pair of elements 2 s - head, 2 s - head + 1 (complex64) where head
    // is 1 for a row that starts 8 bytes past a 16-byte boundary; a pair inside the row is one 16-byte load and store
    __device__ __forceinline__ void point(int64_t b, int64_t r, int64_t s, NoColumn) const {
        cx<T>* row = spec + b * bstride + r * ld;
        if constexpr (sizeof(T) == 8) {
            row[s] = shape(row[s], r, s);
        } else {
            const int64_t head = (reinterpret_cast<uintptr_t>(row) >> 3) & 1;
            const int64_t c0 = 2 * s - head;
            if (c0 >= 0 && c0 + 1 < cols) {
                float4* p = reinterpret_cast<float4*>(row + c0);
                const float4 v = *p;
                const cx<T> u0 = shape(cx<T>{v.x, v.y}, r, c0), u1 = shape(cx<T>{v.z, v.w}, r, c0 + 1);
                *p = make_float4(u0.x, u0.y, u1.x, u1.y);
            } else {
                const int64_t c = c0 < 0 ? 0 : c0;      // the head (column 0) or the tail (column cols - 1)
                if (c < cols) row[c] = shape(row[c], r, c);
            }
        }
    }
};

// ---------------------------------------------------------------- finish
// (row, column) of flat index i of a rows x n window, advanced by the grid's stride without a division per element
struct Walk {
    int64_t r, c, sr, sc, n;
    __device__ __forceinline__ Walk(int64_t i, int64_t stride, int64_t n_) : n(n_) {
        r = i / n, c = i - r * n;
        sr = stride / n, sc = stride - sr * n;
    }
    __device__ __forceinline__ void step() {
        r += sr, c += sc;
        if (c >= n) c -= n, ++r;
    }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void finish_kernel(int64_t rows, int64_t cols, const cx<T>* __restrict__ field, int64_t ld, int64_t bstride,
                                                          int mask_kind, const unsigned char* __restrict__ mask, int64_t mld, T radius, T step,
                                                          T* __restrict__ out, int64_t old, int64_t obstride, double* __restrict__ part) {
    double s[kSums] = {0.0, 0.0};
    const int64_t b = blockIdx.y;
    const cx<T>* f = field + b * bstride;
    T* z = out + b * obstride;
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kThreads;
    int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        bool keep = true;
        if (mask_kind == PM_PSD_MASK_ARRAY)
            keep = mask[w.r * mld + w.c] != 0;
        else if (mask_kind == PM_PSD_MASK_CIRCLE)
            keep = hypot_(T(w.c - cols / 2) * step, T(w.r - rows / 2) * step) <= radius;
        const T v = keep ? f[w.r * ld + w.c].x : std::numeric_limits<T>::quiet_NaN();
        z[w.r * old + w.c] = v;
        if (finite_(v)) {
            const double d = double(v);
            s[0] = s[0] + 1.0;
            s[1] = s[1] + d * d;
        }
    }
    wg_fold<kThreads, FoldSum>(threadIdx.x, s, part + (b * gridDim.x + blockIdx.x) * kSums);
}

// one workgroup per surface: sums[b] = (count, sum of squares)
__global__ __launch_bounds__(kThreads) void finish_fold_kernel(int nparts, const double* __restrict__ part, double* __restrict__ sums) {
    const int64_t b = blockIdx.x;
    double s[kSums];
    fold_partials<kThreads, FoldSum>(threadIdx.x, nparts, part + b * nparts * kSums, 0.0, s);
    if (threadIdx.x < kSums) sums[b * kSums + threadIdx.x] = s[threadIdx.x];
}

// ---------------------------------------------------------------- scale
template <typename T>
struct ScaleOp {
    T* z;
    int64_t ld, bstride;
    const double* sums;
    double rms;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t b, int64_t r, int64_t c, NoColumn) const {
        const double n = sums[b * kSums], ss = sums[b * kSums + 1];
        if (!(n > 0.0) || !(ss > 0.0)) return;
        const double k = rms / sqrt(ss / n);
        T* p = z + b * bstride + r * ld + c;
        *p = T(double(*p) * k);
    }
};

// the shape of a stack; 0, or the refusal
int check_stack(const char* who, int64_t batch, int64_t rows, int64_t cols, int64_t ld, int64_t bstride) {
    if (batch <= 0 || rows <= 0 || cols <= 0) return fail(PM_ERR_ARG, "%s: bad argument (empty array)", who);
    if (too_large(rows, cols) || batch > 65535) return fail(PM_ERR_ARG, "%s: %lld x %lld x %lld is too large", who, (long long)batch, (long long)rows, (long long)cols);
    if (!ld_ok(rows, cols, ld)) return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than the number of columns", who);
    if (!stack_ok(batch, rows, ld, bstride)) return fail(PM_ERR_ARG, "%s: the members of the stack overlap (bstride < rows * ld)", who);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_psd_uniform(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, int64_t seed, int64_t surface0, void* out, int64_t ld, int64_t bstride,
                   void* stream) {
    const char* who = "pm_psd_uniform";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (const int rc = check_stack(who, batch, rows, cols, ld, bstride)) return rc;
    if (surface0 < 0) return fail(PM_ERR_ARG, "%s: the index of the first surface must not be negative", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        UniformOp<T> op{static_cast<T*>(out), ld, bstride, cols, uint32_t(uint64_t(seed)), uint32_t(uint64_t(seed) >> 32), surface0};
        return sweep(batch, rows, cols, PM_STREAM(stream), op);
    });
}

int pm_psd_signal(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, void* spectrum, int64_t ld, int64_t bstride, const void* psd, int64_t psd_ld,
                  const pm_psd_model* model, double area, void* stream) {
    const char* who = "pm_psd_signal";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!spectrum) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (const int rc = check_stack(who, batch, rows, cols, ld, bstride)) return rc;
    if (!psd == !model) return fail(PM_ERR_ARG, "%s: exactly one of the psd array and the model record is given", who);
    if (psd && !ld_ok(rows, cols, psd_ld)) return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than the number of columns", who);
    Model m{0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (model) {
        if (model->kind != PM_IFG_PSD_ABC && model->kind != PM_IFG_PSD_AB) return fail(PM_ERR_ARG, "%s: the model's kind must be PM_IFG_PSD_ABC or PM_IFG_PSD_AB", who);
        if (!(std::isfinite(model->dxg) && model->dxg != 0)) return fail(PM_ERR_ARG, "%s: the model's sample spacing must be finite and nonzero", who);
        m = Model{1, model->kind, model->a, model->b, model->c, 1.0 / (double(cols) * model->dxg), 1.0 / (double(rows) * model->dxg)};
    }
    if (!aligned(spectrum, 2 * elem_of(dtype))) return fail(PM_ERR_ARG, "%s: the spectrum is not aligned like a complex element", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        SignalOp<T> op{static_cast<cx<T>*>(spectrum), ld, bstride, rows, cols, static_cast<const T*>(psd), psd_ld, m, T(area)};
        const int64_t slots = sizeof(T) == 8 ? cols : cols / 2 + 1;
        return sweep(batch, rows, slots, PM_STREAM(stream), op);
    });
}

size_t pm_psd_finish_workspace(int64_t batch, int64_t rows, int64_t cols) {
    if (batch <= 0 || rows <= 0 || cols <= 0 || too_large(rows, cols) || batch > 65535) return 0;
    return size_t(batch) * groups(rows * cols) * kSums * sizeof(double);
}

int pm_psd_finish(int32_t dtype, int32_t mask_kind, int64_t batch, int64_t rows, int64_t cols, const void* field, int64_t ld, int64_t bstride,
                  const void* mask, int64_t mask_ld, double radius, double step, void* out, int64_t out_ld, int64_t out_bstride, void* sums,
                  void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_psd_finish";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (mask_kind != PM_PSD_MASK_NONE && mask_kind != PM_PSD_MASK_ARRAY && mask_kind != PM_PSD_MASK_CIRCLE)
        return fail(PM_ERR_ARG, "%s: mask_kind must be PM_PSD_MASK_NONE, PM_PSD_MASK_ARRAY or PM_PSD_MASK_CIRCLE", who);
    if (!field || !out || !sums || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (const int rc = check_stack(who, batch, rows, cols, ld, bstride)) return rc;
    if (const int rc = check_stack(who, batch, rows, cols, out_ld, out_bstride)) return rc;
    if (mask_kind == PM_PSD_MASK_ARRAY && !mask) return fail(PM_ERR_ARG, "%s: the mask is missing (null pointer)", who);
    if (mask_kind == PM_PSD_MASK_ARRAY && !ld_ok(rows, cols, mask_ld)) return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than the number of columns", who);
    if (mask_kind == PM_PSD_MASK_CIRCLE && !(std::isfinite(radius) && std::isfinite(step))) return fail(PM_ERR_ARG, "%s: the circle's radius and step must be finite", who);
    if (workspace_bytes < pm_psd_finish_workspace(batch, rows, cols)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_psd_finish_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(sums, 8)) return fail(PM_ERR_ARG, "%s: the sums and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = groups(rows * cols);
        double* part = static_cast<double*>(workspace);
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((finish_kernel<T>), dim3(wgs, unsigned(batch)), dim3(kThreads), 0, st, rows, cols, static_cast<const cx<T>*>(field), ld, bstride,
                           int(mask_kind), static_cast<const unsigned char*>(mask), mask_ld, T(radius), T(step), static_cast<T*>(out), out_ld, out_bstride, part);
        hipLaunchKernelGGL(finish_fold_kernel, dim3(unsigned(batch)), dim3(kThreads), 0, st, wgs, part, static_cast<double*>(sums));
        return int(hipGetLastError());
    });
}

int pm_psd_scale(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, void* z, int64_t ld, int64_t bstride, const void* sums, double rms, void* stream) {
    const char* who = "pm_psd_scale";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!z || !sums) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (const int rc = check_stack(who, batch, rows, cols, ld, bstride)) return rc;
    if (!aligned(sums, 8)) return fail(PM_ERR_ARG, "%s: the sums are doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        ScaleOp<T> op{static_cast<T*>(z), ld, bstride, static_cast<const double*>(sums), rms};
        return sweep(batch, rows, cols, PM_STREAM(stream), op);
    });
}

}  // extern "C"
