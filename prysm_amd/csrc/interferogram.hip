// Measured surface maps with invalid pixels (prysm/interferogram.py, prysm/util.py) (gfx950).  A map is a rows x cols window of a real
// array with leading dimension ld (Interferogram.crop hands views around), NaN marks an invalid pixel, +-inf is left out of every sum.
//
//  - pm_ifg_stats: the masked statistics record (PM_IFG_* in prysm_amd.h) in two passes of two launches each.  Pass A: counts, sum,
//    sum of squares, extrema and the bounding box of the finite values; its one-workgroup second stage leaves the mean.  Pass B reads
//    that mean from the device and adds sum|z - mean| and sum (z - mean)^2; its second stage leaves std, rms and Sa.  The variance is
//    two-pass on purpose: a piston of 1000 on a sigma of 35 in float32 loses a one-pass variance.
//  - pm_ifg_fit: the normal equations of a subset of {1, x, y, x^2 + y^2} over the finite pixels (10 Gram sums, 4 right-hand sides);
//    the second stage solves the subsystem by elimination with diagonal pivoting and leaves four coefficients on the device.  A pivot
//    below eps (largest pivot) drops its term: coefficient 0, never a NaN the input did not hold.
//  - pm_ifg_remove (subtract chosen fitted terms from the finite pixels), pm_ifg_edit (fill NaN, NaN outside a mask, NaN above
//    nsigma std with std read from the record) and pm_ifg_slope (np.gradient and its hypot): pointwise, in place where they edit.
//  - pm_ifg_window: height x window (Welch from the generated radius, Hann as an outer product, or the caller's array) and
//    S2 = sum window^2 in the same pass; pm_ifg_psd_scale divides the |.|^2 of the transform by S2 fs^2, S2 read on the device.
//  - pm_ifg_band: sum w_r w_c psd over flow <= nu <= fhigh with the trapezoid rule's weights, nu generated or read, times the
//    square of the spacing, which its second stage takes from two samples of nu.
//  - pm_ifg_iir: hann2d x ideal_lpf_iir2d for one or two corner frequencies (the jinc of csrc/fibers_coefs.h, in double);
//    pm_ifg_combine: the 1 - H combinations of the four filter types; pm_ifg_psd_model: abc_psd and ab_psd.
//
// Every sum is accumulated in double.  First stages run a flat grid-stride loop of kIfgThreads x at most kIfgWgs threads and end in the
// tree of pm_reduce.h; second stages are one workgroup over the partials: no atomics, the same bits every run.  Minima ride the
// maximum tree negated, so one FoldMax tree serves the extrema and the bounding box.  The pointwise kernels ride on pm_sweep.h.  The
// unit is compiled with -ffp-contract=off (csrc/Makefile), as prysm_amd/interferogram_plan.py restates it in numpy.
#include <cmath>
#include <limits>

#include "fibers_coefs.h"
#include "pm_entry.h"
#include "pm_math.h"
#include "pm_reduce.h"
#include "pm_sweep.h"

namespace pm {
namespace {

constexpr int kIfgThreads = 256;
constexpr int kIfgWgs = 1024;      // most workgroups of a first stage: as many partials per value

int ifg_groups(int64_t n) { return reduce_groups(n, kIfgThreads, kIfgWgs); }

template <typename T>
__device__ __forceinline__ bool finite_(T z) {
    return abs_(z) <= std::numeric_limits<T>::max();      // false for NaN and for +-inf
}

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

// ---------------------------------------------------------------- statistics
constexpr int kSumA = 4;      // finite count, NaN count, sum, sum of squares
constexpr int kMaxA = 6;      // -min, max, -first row, last row, -first column, last column
constexpr int kSumB = 2;      // sum |z - mean|, sum (z - mean)^2

template <typename T>
__global__ __launch_bounds__(kIfgThreads) void stats_a_kernel(int64_t rows, int64_t cols, const T* __restrict__ d, int64_t ld,
                                                              double* __restrict__ psum, double* __restrict__ pmax) {
    double s[kSumA] = {0.0, 0.0, 0.0, 0.0};
    double m[kMaxA];
#pragma unroll
    for (int k = 0; k < kMaxA; ++k) m[k] = -INFINITY;
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kIfgThreads;
    int64_t i = int64_t(blockIdx.x) * kIfgThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        const T z = d[w.r * ld + w.c];
        if (z != z) {
            s[1] = s[1] + 1.0;
        } else if (finite_(z)) {
            const double v = double(z), fr = double(w.r), fc = double(w.c);
            s[0] = s[0] + 1.0;
            s[2] = s[2] + v;
            s[3] = s[3] + v * v;
            m[0] = FoldMax::of(m[0], -v);
            m[1] = FoldMax::of(m[1], v);
            m[2] = FoldMax::of(m[2], -fr);
            m[3] = FoldMax::of(m[3], fr);
            m[4] = FoldMax::of(m[4], -fc);
            m[5] = FoldMax::of(m[5], fc);
        }
    }
    wg_fold<kIfgThreads, FoldSum>(threadIdx.x, s, psum + int64_t(blockIdx.x) * kSumA);
    wg_fold<kIfgThreads, FoldMax>(threadIdx.x, m, pmax + int64_t(blockIdx.x) * kMaxA);
}

__global__ __launch_bounds__(kIfgThreads) void stats_a_fold_kernel(int nparts, const double* __restrict__ psum, const double* __restrict__ pmax,
                                                                   double* __restrict__ rec) {
    double s[kSumA], m[kMaxA];
    fold_partials<kIfgThreads, FoldSum>(threadIdx.x, nparts, psum, 0.0, s);
    fold_partials<kIfgThreads, FoldMax>(threadIdx.x, nparts, pmax, -INFINITY, m);
    if (threadIdx.x == 0) {
        const bool any = s[0] > 0.0;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        rec[PM_IFG_N] = s[0];
        rec[PM_IFG_NNAN] = s[1];
        rec[PM_IFG_SUM] = s[2];
        rec[PM_IFG_SUMSQ] = s[3];
        rec[PM_IFG_MIN] = any ? -m[0] : nan;
        rec[PM_IFG_MAX] = any ? m[1] : nan;
        rec[PM_IFG_ROW0] = any ? -m[2] : -1.0;
        rec[PM_IFG_ROW1] = any ? m[3] : -1.0;
        rec[PM_IFG_COL0] = any ? -m[4] : -1.0;
        rec[PM_IFG_COL1] = any ? m[5] : -1.0;
        rec[PM_IFG_MEAN] = s[2] / s[0];      // 0 / 0: NaN for a map without a finite value
    }
}

template <typename T>
__global__ __launch_bounds__(kIfgThreads) void stats_b_kernel(int64_t rows, int64_t cols, const T* __restrict__ d, int64_t ld,
                                                              const double* __restrict__ rec, double* __restrict__ part) {
    const double mean = rec[PM_IFG_MEAN];
    double s[kSumB] = {0.0, 0.0};
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kIfgThreads;
    int64_t i = int64_t(blockIdx.x) * kIfgThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        const T z = d[w.r * ld + w.c];
        if (finite_(z)) {
            const double e = double(z) - mean;
            s[0] = s[0] + fabs(e);
            s[1] = s[1] + e * e;
        }
    }
    wg_fold<kIfgThreads, FoldSum>(threadIdx.x, s, part + int64_t(blockIdx.x) * kSumB);
}

__global__ __launch_bounds__(kIfgThreads) void stats_b_fold_kernel(int nparts, const double* __restrict__ part, double* __restrict__ rec) {
    double s[kSumB];
    fold_partials<kIfgThreads, FoldSum>(threadIdx.x, nparts, part, 0.0, s);
    if (threadIdx.x == 0) {
        const double n = rec[PM_IFG_N];
        const bool any = n > 0.0;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        rec[PM_IFG_SAD] = s[0];
        rec[PM_IFG_M2] = s[1];
        rec[PM_IFG_STD] = any ? sqrt(s[1] / n) : nan;
        rec[PM_IFG_RMS] = any ? sqrt(rec[PM_IFG_SUMSQ] / n) : nan;
        rec[PM_IFG_SA] = any ? s[0] / n : nan;
    }
}

// ---------------------------------------------------------------- coordinates
// where x and y of pixel (r, c) come from, as doubles.  GRID: make_xy_grid's elements T(c - ox) * T(dx), or (linspace) x0 + c dx in
// double; SEPARABLE: x[c], y[r * ldy]; POINTWISE: x[r * ldx + c], y[r * ldy + c]
template <typename T>
struct Co {
    int mode, lin;
    const T* x;
    const T* y;
    int64_t ldx, ldy, ox, oy;
    double dx, dy, x0, y0;
    __device__ __forceinline__ double X(int64_t r, int64_t c) const {
        if (mode == PM_COORDS_GRID) return lin ? x0 + double(c) * dx : double(T(c - ox) * T(dx));
        return mode == PM_COORDS_SEPARABLE ? double(x[c]) : double(x[r * ldx + c]);
    }
    __device__ __forceinline__ double Y(int64_t r, int64_t c) const {
        if (mode == PM_COORDS_GRID) return lin ? y0 + double(r) * dy : double(T(r - oy) * T(dy));
        return mode == PM_COORDS_SEPARABLE ? double(y[r * ldy]) : double(y[r * ldy + c]);
    }
};

template <typename T>
Co<T> make_co(const pm_ifg_coords* co) {
    return Co<T>{co->mode, co->linspace, static_cast<const T*>(co->x), static_cast<const T*>(co->y), co->ldx, co->ldy, co->ox, co->oy,
                 co->dx, co->dy, co->x0, co->y0};
}

// ---------------------------------------------------------------- fit
constexpr int kFitSums = 14;      // Gram, upper triangle by rows over (1, x, y, q): 11 1x 1y 1q xx xy xq yy yq qq; then z, xz, yz, qz

template <typename T>
__global__ __launch_bounds__(kIfgThreads) void fit_kernel(int64_t rows, int64_t cols, const T* __restrict__ d, int64_t ld, const Co<T> co,
                                                          double* __restrict__ part) {
    double s[kFitSums];
#pragma unroll
    for (int k = 0; k < kFitSums; ++k) s[k] = 0.0;
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kIfgThreads;
    int64_t i = int64_t(blockIdx.x) * kIfgThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        const T zt = d[w.r * ld + w.c];
        if (!finite_(zt)) continue;
        const double z = double(zt), x = co.X(w.r, w.c), y = co.Y(w.r, w.c);
        const double q = x * x + y * y;
        s[0] = s[0] + 1.0;
        s[1] = s[1] + x;
        s[2] = s[2] + y;
        s[3] = s[3] + q;
        s[4] = s[4] + x * x;
        s[5] = s[5] + x * y;
        s[6] = s[6] + x * q;
        s[7] = s[7] + y * y;
        s[8] = s[8] + y * q;
        s[9] = s[9] + q * q;
        s[10] = s[10] + z;
        s[11] = s[11] + x * z;
        s[12] = s[12] + y * z;
        s[13] = s[13] + q * z;
    }
    wg_fold<kIfgThreads, FoldSum>(threadIdx.x, s, part + int64_t(blockIdx.x) * kFitSums);
}

// one workgroup: the sums, then thread 0 solves the chosen subsystem.  Elimination with diagonal pivoting on the symmetric Gram
// matrix: the largest remaining diagonal is the pivot, so pivots do not grow; one below eps (first pivot) ends the elimination and
// the terms not yet eliminated get coefficient 0
__global__ __launch_bounds__(kIfgThreads) void fit_solve_kernel(int nparts, const double* __restrict__ part, int terms, double* __restrict__ coef) {
    double s[kFitSums];
    fold_partials<kIfgThreads, FoldSum>(threadIdx.x, nparts, part, 0.0, s);
    if (threadIdx.x != 0) return;
    double A[4][4], b[4], x[4] = {0.0, 0.0, 0.0, 0.0};
    A[0][0] = s[0], A[0][1] = s[1], A[0][2] = s[2], A[0][3] = s[3];
    A[1][1] = s[4], A[1][2] = s[5], A[1][3] = s[6];
    A[2][2] = s[7], A[2][3] = s[8];
    A[3][3] = s[9];
    for (int i = 0; i < 4; ++i) {
        b[i] = s[10 + i];
        for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
    }
    bool left[4];
    int m = 0;
    for (int i = 0; i < 4; ++i) {
        left[i] = (terms >> i) & 1;
        m += left[i];
    }
    int perm[4], done = 0;
    double first = 0.0;
    for (int step = 0; step < m; ++step) {
        int p = -1;
        for (int i = 0; i < 4; ++i)
            if (left[i] && (p < 0 || A[i][i] > A[p][p])) p = i;
        if (step == 0) first = A[p][p];
        if (!(A[p][p] > 2.220446049250313e-16 * first) || !(A[p][p] > 0.0)) break;
        left[p] = false;
        perm[done++] = p;
        for (int i = 0; i < 4; ++i) {
            if (!left[i]) continue;
            const double f = A[i][p] / A[p][p];
            for (int j = 0; j < 4; ++j)
                if (left[j]) A[i][j] = A[i][j] - f * A[p][j];
            b[i] = b[i] - f * b[p];
        }
    }
    for (int k = done - 1; k >= 0; --k) {
        const int p = perm[k];
        double acc = b[p];
        for (int t = k + 1; t < done; ++t) acc = acc - A[p][perm[t]] * x[perm[t]];
        x[p] = acc / A[p][p];
    }
    for (int i = 0; i < 4; ++i) coef[i] = x[i];
}

struct Coefs {
    double k[4];
};

template <typename T>
struct RemoveOp {
    T* d;
    int64_t ld;
    Co<T> co;
    int terms;
    const double* coef;

    __device__ __forceinline__ Coefs column(int64_t) const { return Coefs{{coef[0], coef[1], coef[2], coef[3]}}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, const Coefs& k) const {
        const T z = d[r * ld + c];
        if (!finite_(z)) return;
        double p = 0.0;
        if (terms & (PM_IFG_TERM_X | PM_IFG_TERM_Y | PM_IFG_TERM_R2)) {
            const double x = co.X(r, c), y = co.Y(r, c);
            if (terms & PM_IFG_TERM_X) p = p + k.k[1] * x;
            if (terms & PM_IFG_TERM_Y) p = p + k.k[2] * y;
            if (terms & PM_IFG_TERM_R2) p = p + k.k[3] * (x * x + y * y);
        }
        if (terms & PM_IFG_TERM_PISTON) p = p + k.k[0];
        d[r * ld + c] = T(double(z) - p);
    }
};

// ---------------------------------------------------------------- edits
template <typename T>
struct EditOp {
    T* d;
    int64_t ld;
    int op;
    double value;
    const unsigned char* mask;
    int64_t mld;
    const double* rec;

    // CLIP: the threshold nsigma std, read once per thread
    __device__ __forceinline__ double column(int64_t) const { return op == PM_IFG_CLIP ? value * rec[PM_IFG_STD] : 0.0; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, double thr) const {
        const T nan = std::numeric_limits<T>::quiet_NaN();
        if (op == PM_IFG_MASK) {
            if (!mask[r * mld + c]) d[r * ld + c] = nan;
            return;
        }
        const T z = d[r * ld + c];
        if (op == PM_IFG_FILL) {
            if (z != z) d[r * ld + c] = T(value);
        } else if (double(abs_(z)) > thr) {      // false for a NaN pixel and for a NaN threshold
            d[r * ld + c] = nan;
        }
    }
};

// np.gradient(data, dx), edge_order 1: central differences over 2 dx inside, one-sided ones over dx on the border, every operation in T
template <typename T>
struct SlopeOp {
    const T* d;
    int64_t ld, rows, cols;
    T dx, two_dx;
    T* gx;
    T* gy;
    T* gr;
    int64_t old;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        const T* row = d + r * ld;
        T sx, sy;
        if (c == 0) sx = (row[1] - row[0]) / dx;
        else if (c == cols - 1) sx = (row[c] - row[c - 1]) / dx;
        else sx = (row[c + 1] - row[c - 1]) / two_dx;
        if (r == 0) sy = (row[ld + c] - row[c]) / dx;
        else if (r == rows - 1) sy = (row[c] - row[c - ld]) / dx;
        else sy = (row[c + ld] - row[c - ld]) / two_dx;
        if (gx) gx[r * old + c] = sx;
        if (gy) gy[r * old + c] = sy;
        if (gr) gr[r * old + c] = hypot_(sx, sy);
    }
};

// ---------------------------------------------------------------- window and PSD
constexpr double kPi = 3.141592653589793;

// np.hanning(n)[j] = 0.5 + 0.5 cos(pi (1 - n + 2 j) / (n - 1)), [1] for n = 1
__device__ __forceinline__ double hanning_(int64_t j, int64_t n) {
    if (n == 1) return 1.0;
    return 0.5 + 0.5 * cos(kPi * double(1 - n + 2 * j) / double(n - 1));
}

// out = height x window (the window itself without a height) and one partial of sum window^2 per workgroup.  WELCH: 1 - |r / rmax|^alpha
// on make_xy_grid's radius, rmax its sample at (rows - 1, cols / 2); HANN: hanning(rows) (x) hanning(cols); ARRAY: the caller's window
template <typename T>
__global__ __launch_bounds__(kIfgThreads) void window_kernel(int kind, int64_t rows, int64_t cols, const T* __restrict__ h, int64_t ld, T dx,
                                                             double alpha, const T* __restrict__ win, int64_t wld, T* __restrict__ out, int64_t old,
                                                             double* __restrict__ part) {
    double s[1] = {0.0};
    const double rmax = double(hypot_(T(0) * dx, T(rows - 1 - rows / 2) * dx));
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kIfgThreads;
    int64_t i = int64_t(blockIdx.x) * kIfgThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        double v;
        if (kind == PM_IFG_WIN_WELCH) {
            const double rad = double(hypot_(T(w.c - cols / 2) * dx, T(w.r - rows / 2) * dx));
            v = 1.0 - pow(fabs(rad / rmax), alpha);
        } else if (kind == PM_IFG_WIN_HANN) {
            v = hanning_(w.r, rows) * hanning_(w.c, cols);
        } else {
            v = double(win[w.r * wld + w.c]);
        }
        s[0] = s[0] + v * v;
        out[w.r * old + w.c] = h ? T(double(h[w.r * ld + w.c]) * v) : T(v);
    }
    wg_fold<kIfgThreads, FoldSum>(threadIdx.x, s, part + blockIdx.x);
}

__global__ __launch_bounds__(kIfgThreads) void window_fold_kernel(int nparts, const double* __restrict__ part, double* __restrict__ s2) {
    double s[1];
    fold_partials<kIfgThreads, FoldSum>(threadIdx.x, nparts, part, 0.0, s);
    if (threadIdx.x == 0) s2[0] = s[0];
}

// psd /= S2 fs fs, S2 read on the device
template <typename T>
struct PsdScaleOp {
    T* d;
    int64_t ld;
    const double* s2;
    double fs;

    __device__ __forceinline__ double column(int64_t) const { return s2[0] * fs * fs; }
    __device__ __forceinline__ void point(int64_t r, int64_t c, double coef) const { d[r * ld + c] = T(double(d[r * ld + c]) / coef); }
};

// ---------------------------------------------------------------- band-limited integral
// sum w_r w_c psd[r, c] over flow <= nu <= fhigh with the trapezoid rule's weights, 0.5 ((i > 0) + (i < n - 1)) per axis (columns
// unweighted for a 1-D spectrum).  nu: generated, hypot((c - cols / 2) / (cols dx), (r - rows / 2) / (rows dx)) in double, or read
template <typename T>
__global__ __launch_bounds__(kIfgThreads) void band_kernel(int64_t rows, int64_t cols, const T* __restrict__ p, int64_t ld, int gen,
                                                           const T* __restrict__ nu, int64_t nld, double ux, double uy, double flow, double fhigh,
                                                           int one_d, double* __restrict__ part) {
    double s[1] = {0.0};
    const int64_t total = rows * cols, stride = int64_t(gridDim.x) * kIfgThreads;
    int64_t i = int64_t(blockIdx.x) * kIfgThreads + threadIdx.x;
    for (Walk w(i, stride, cols); i < total; i += stride, w.step()) {
        const double f = gen ? hypot(double(w.c - cols / 2) * ux, double(w.r - rows / 2) * uy) : double(nu[w.r * nld + w.c]);
        if (f < flow || f > fhigh) continue;      // a NaN frequency stays in, as in the reference's two assignments
        const double wr = 0.5 * (double(w.r > 0) + double(w.r < rows - 1));
        const double wc = one_d ? 1.0 : 0.5 * (double(w.c > 0) + double(w.c < cols - 1));
        s[0] = s[0] + (wr * wc) * double(p[w.r * ld + w.c]);
    }
    wg_fold<kIfgThreads, FoldSum>(threadIdx.x, s, part + blockIdx.x);
}

// out[0] = the sum times spacing^2 (spacing for a 1-D spectrum), out[1] = the spacing: given, or |nu[i2] - nu[i1]| read here
template <typename T>
__global__ __launch_bounds__(kIfgThreads) void band_fold_kernel(int nparts, const double* __restrict__ part, const T* __restrict__ nu, int64_t i1,
                                                                int64_t i2, double spacing, int one_d, double* __restrict__ out) {
    double s[1];
    fold_partials<kIfgThreads, FoldSum>(threadIdx.x, nparts, part, 0.0, s);
    if (threadIdx.x == 0) {
        const double d = nu ? fabs(double(nu[i2]) - double(nu[i1])) : spacing;
        out[0] = one_d ? s[0] * d : s[0] * d * d;
        out[1] = d;
    }
}

// ---------------------------------------------------------------- filter design
// sum_k c_k T_k(t) by Clenshaw over the tables of csrc/fibers_coefs.h, as csrc/imagechain.hip walks them
#define PM_IFG_SERIES(NAME)                                                                                            \
    __device__ __forceinline__ double cheb_##NAME(double t) {                                                          \
        constexpr int n = fibers_coefs::NAME##_N64;                                                                    \
        const double t2 = t + t;                                                                                       \
        double b1 = 0.0, b2 = 0.0;                                                                                     \
        _Pragma("unroll") for (int k = n - 1; k > 0; --k) {                                                            \
            const double b = t2 * b1 - b2 + fibers_coefs::NAME[k];                                                     \
            b2 = b1;                                                                                                   \
            b1 = b;                                                                                                    \
        }                                                                                                              \
        return t * b1 - b2 + fibers_coefs::NAME[0];                                                                    \
    }
PM_IFG_SERIES(J1S)
PM_IFG_SERIES(P1)
PM_IFG_SERIES(Q1)
#undef PM_IFG_SERIES

// J1(x) / x in double, 0.5 below 1e-8 as the reference sets it
__device__ __forceinline__ double jinc_(double x) {
    const double ax = fabs(x);
    if (ax < 1e-8) return 0.5;
    if (ax <= 8.0) return cheb_J1S(ax * ax * 0.03125 - 1.0);
    const double z = 8.0 / ax;
    const double t = 2.0 * (z * z) - 1.0;
    double s, c;
    sincos(ax, &s, &c);
    const double amp = sqrt(0.6366197723675814 / ax);
    const double c0 = (c + s) * 0.7071067811865476, s0 = (s - c) * 0.7071067811865476;
    return amp * (cheb_P1(t) * s0 + z * cheb_Q1(t) * c0) / ax;
}

// hann2d(rows, cols), ideal_lpf_iir2d(r, dx, fcn) or their product for one or two corner frequencies, in double, rounded once to T
template <typename T>
struct IirOp {
    int parts, gen;
    const T* rad;
    int64_t rld, oy, ox, rows, cols;
    T rdx;
    double dx, fcn[2];
    T* out[2];
    int64_t old;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        double w = 1.0;
        if (parts & PM_IFG_IIR_HANN) {
            const int64_t nmin = cols < rows ? cols : rows;
            const double nn = hypot(double(c - cols / 2), double(r - rows / 2));
            const double cw = cos(kPi / double(nmin) * nn);
            w = nn > double(nmin / 2) ? 0.0 : cw * cw;
        }
        if (!(parts & PM_IFG_IIR_LPF)) {
            out[0][r * old + c] = T(w);
            return;
        }
        const double rho = gen ? double(hypot_(T(c - ox) * rdx, T(r - oy) * rdx)) : double(rad[r * rld + c]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!out[k]) continue;
            const double cc = kPi * fcn[k] / dx;
            const double h = jinc_(rho * cc) * (fcn[k] * fcn[k] * kPi / 2.0);
            out[k][r * old + c] = T(w * h);
        }
    }
};

// the reference's combinations of |fft2(h')|: LP Hl; HP 1 - Hl; BP 1 - ((1 - Hh) + Hl); BR (1 - Hh) + Hl, in T; real, or complex (v, 0)
template <typename T>
struct CombineOp {
    int typ, cplx;
    const T* hl;
    const T* hh;
    int64_t ldl, ldh;
    void* out;
    int64_t old;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        const T a = hl[r * ldl + c];
        T v;
        if (typ == PM_IFG_LP) {
            v = a;
        } else if (typ == PM_IFG_HP) {
            v = T(1) - a;
        } else {
            const T b = (T(1) - hh[r * ldh + c]) + a;
            v = typ == PM_IFG_BP ? T(1) - b : b;
        }
        if (cplx)
            static_cast<cx<T>*>(out)[r * old + c] = cx<T>{v, T(0)};
        else
            static_cast<T*>(out)[r * old + c] = v;
    }
};

// abc_psd a / (1 + (nu / b)^c) and ab_psd a nu^(-b), in T
template <typename T>
struct PsdModelOp {
    int kind;
    const T* nu;
    T a, b, c;
    T* out;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t, int64_t i, NoColumn) const {
        const T f = nu[i];
        if (kind == PM_IFG_PSD_ABC)
            out[i] = a / (T(1) + T(pow(double(f / b), double(c))));
        else
            out[i] = a * T(pow(double(f), double(-b)));
    }
};

bool too_large(int64_t m, int64_t n) { return m > INT32_MAX || n > INT32_MAX; }

bool terms_ok(int32_t terms) { return terms > 0 && terms < 16; }

// the coordinates of a fit or a removal; 0, or the refusal
int check_coords(const char* who, const pm_ifg_coords* co, int32_t terms, int64_t rows, int64_t cols) {
    if (!co) return fail(PM_ERR_ARG, "%s: the coordinates are missing (null pointer)", who);
    if (co->mode != PM_COORDS_GRID && co->mode != PM_COORDS_SEPARABLE && co->mode != PM_COORDS_POINTWISE)
        return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID, PM_COORDS_SEPARABLE or PM_COORDS_POINTWISE", who);
    if (co->mode == PM_COORDS_GRID) {
        if (!(std::isfinite(co->dx) && std::isfinite(co->dy) && std::isfinite(co->x0) && std::isfinite(co->y0)))
            return fail(PM_ERR_ARG, "%s: the grid's origin and spacing must be finite", who);
        return 0;
    }
    if ((terms & ~PM_IFG_TERM_PISTON) && (!co->x || !co->y)) return fail(PM_ERR_ARG, "%s: coordinate arrays are missing (null pointer)", who);
    if (co->mode == PM_COORDS_SEPARABLE && (terms & ~PM_IFG_TERM_PISTON) && co->ldy < 1)
        return fail(PM_ERR_ARG, "%s: the values of y must lie at least one element apart", who);
    if (co->mode == PM_COORDS_POINTWISE && !(ld_ok(rows, cols, co->ldx) && ld_ok(rows, cols, co->ldy)))
        return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than the number of columns", who);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

size_t pm_ifg_stats_workspace(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || too_large(rows, cols)) return 0;
    return size_t(ifg_groups(rows * cols)) * (kSumA + kMaxA + kSumB) * sizeof(double);
}

int pm_ifg_stats(int32_t dtype, int64_t rows, int64_t cols, const void* data, int64_t ld, void* record, void* workspace, size_t workspace_bytes,
                 void* stream) {
    const char* who = "pm_ifg_stats";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (rows <= 0 || cols <= 0 || !data || !record || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    PM_CHECK_LD("pm_ifg_stats", ld_ok(rows, cols, ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (workspace_bytes < pm_ifg_stats_workspace(rows, cols))
        return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_ifg_stats_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(record, 8)) return fail(PM_ERR_ARG, "%s: the record and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = ifg_groups(rows * cols);
        double* psum = static_cast<double*>(workspace);
        double* pmax = psum + size_t(wgs) * kSumA;
        double* pb = pmax + size_t(wgs) * kMaxA;
        double* rec = static_cast<double*>(record);
        const T* d = static_cast<const T*>(data);
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((stats_a_kernel<T>), dim3(wgs), dim3(kIfgThreads), 0, st, rows, cols, d, ld, psum, pmax);
        hipLaunchKernelGGL(stats_a_fold_kernel, dim3(1), dim3(kIfgThreads), 0, st, wgs, psum, pmax, rec);
        hipLaunchKernelGGL((stats_b_kernel<T>), dim3(wgs), dim3(kIfgThreads), 0, st, rows, cols, d, ld, rec, pb);
        hipLaunchKernelGGL(stats_b_fold_kernel, dim3(1), dim3(kIfgThreads), 0, st, wgs, pb, rec);
        return int(hipGetLastError());
    });
}

size_t pm_ifg_fit_workspace(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || too_large(rows, cols)) return 0;
    return size_t(ifg_groups(rows * cols)) * kFitSums * sizeof(double);
}

int pm_ifg_fit(int32_t dtype, int32_t terms, int64_t rows, int64_t cols, const void* data, int64_t ld, const pm_ifg_coords* coords, void* coef,
               void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_ifg_fit";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!terms_ok(terms)) return fail(PM_ERR_ARG, "%s: terms must be a non-empty set of PM_IFG_TERM_* bits", who);
    if (rows <= 0 || cols <= 0 || !data || !coef || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    PM_CHECK_LD("pm_ifg_fit", ld_ok(rows, cols, ld));
    if (const int rc = check_coords(who, coords, terms, rows, cols)) return rc;
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (workspace_bytes < pm_ifg_fit_workspace(rows, cols)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_ifg_fit_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(coef, 8)) return fail(PM_ERR_ARG, "%s: the coefficients and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = ifg_groups(rows * cols);
        double* part = static_cast<double*>(workspace);
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((fit_kernel<T>), dim3(wgs), dim3(kIfgThreads), 0, st, rows, cols, static_cast<const T*>(data), ld, make_co<T>(coords), part);
        hipLaunchKernelGGL(fit_solve_kernel, dim3(1), dim3(kIfgThreads), 0, st, wgs, part, int(terms), static_cast<double*>(coef));
        return int(hipGetLastError());
    });
}

int pm_ifg_remove(int32_t dtype, int32_t terms, int64_t rows, int64_t cols, void* data, int64_t ld, const pm_ifg_coords* coords, const void* coef,
                  void* stream) {
    const char* who = "pm_ifg_remove";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!terms_ok(terms)) return fail(PM_ERR_ARG, "%s: terms must be a non-empty set of PM_IFG_TERM_* bits", who);
    if (rows < 0 || cols < 0 || !data || !coef) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    PM_CHECK_LD("pm_ifg_remove", ld_ok(rows, cols, ld));
    if (const int rc = check_coords(who, coords, terms, rows, cols)) return rc;
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (!aligned(coef, 8)) return fail(PM_ERR_ARG, "%s: the coefficients are doubles (8-byte alignment)", who);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        RemoveOp<T> op{static_cast<T*>(data), ld, make_co<T>(coords), int(terms), static_cast<const double*>(coef)};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

int pm_ifg_edit(int32_t dtype, int32_t op, int64_t rows, int64_t cols, void* data, int64_t ld, double value, const void* mask, int64_t mask_ld,
                const void* record, void* stream) {
    const char* who = "pm_ifg_edit";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (op != PM_IFG_FILL && op != PM_IFG_MASK && op != PM_IFG_CLIP) return fail(PM_ERR_ARG, "%s: op must be PM_IFG_FILL, PM_IFG_MASK or PM_IFG_CLIP", who);
    if (rows < 0 || cols < 0 || !data) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (op == PM_IFG_MASK && !mask) return fail(PM_ERR_ARG, "%s: the mask is missing (null pointer)", who);
    if (op == PM_IFG_CLIP && !record) return fail(PM_ERR_ARG, "%s: the statistics record is missing (null pointer)", who);
    PM_CHECK_LD("pm_ifg_edit", ld_ok(rows, cols, ld) && (op != PM_IFG_MASK || ld_ok(rows, cols, mask_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (op == PM_IFG_CLIP && !aligned(record, 8)) return fail(PM_ERR_ARG, "%s: the record holds doubles (8-byte alignment)", who);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        EditOp<T> e{static_cast<T*>(data), ld, int(op), value, static_cast<const unsigned char*>(mask), mask_ld, static_cast<const double*>(record)};
        return sweep(rows, cols, PM_STREAM(stream), e);
    });
}

int pm_ifg_slope(int32_t dtype, int64_t rows, int64_t cols, const void* data, int64_t ld, double dx, void* gx, void* gy, void* gr, int64_t out_ld,
                 void* stream) {
    const char* who = "pm_ifg_slope";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!data) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (rows < 2 || cols < 2) return fail(PM_ERR_ARG, "%s: a gradient needs at least 2 samples along each axis", who);
    if (!gx && !gy && !gr) return fail(PM_ERR_ARG, "%s: no output (gx, gy and gr are all null)", who);
    PM_CHECK_LD("pm_ifg_slope", ld_ok(rows, cols, ld) && ld_ok(rows, cols, out_ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        SlopeOp<T> op{static_cast<const T*>(data), ld, rows, cols, T(dx), T(2.0 * dx), static_cast<T*>(gx), static_cast<T*>(gy), static_cast<T*>(gr), out_ld};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

size_t pm_ifg_window_workspace(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || too_large(rows, cols)) return 0;
    return size_t(ifg_groups(rows * cols)) * sizeof(double);
}

int pm_ifg_window(int32_t dtype, int32_t kind, int64_t rows, int64_t cols, const void* height, int64_t ld, double dx, double alpha, const void* window,
                  int64_t window_ld, void* out, int64_t out_ld, void* s2, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_ifg_window";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (kind != PM_IFG_WIN_WELCH && kind != PM_IFG_WIN_HANN && kind != PM_IFG_WIN_ARRAY)
        return fail(PM_ERR_ARG, "%s: kind must be PM_IFG_WIN_WELCH, PM_IFG_WIN_HANN or PM_IFG_WIN_ARRAY", who);
    if (rows <= 0 || cols <= 0 || !out || !s2 || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    if (kind == PM_IFG_WIN_ARRAY && !window) return fail(PM_ERR_ARG, "%s: the window array is missing (null pointer)", who);
    PM_CHECK_LD("pm_ifg_window", (!height || ld_ok(rows, cols, ld)) && ld_ok(rows, cols, out_ld) && (kind != PM_IFG_WIN_ARRAY || ld_ok(rows, cols, window_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (workspace_bytes < pm_ifg_window_workspace(rows, cols))
        return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_ifg_window_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(s2, 8)) return fail(PM_ERR_ARG, "%s: S2 and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = ifg_groups(rows * cols);
        double* part = static_cast<double*>(workspace);
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((window_kernel<T>), dim3(wgs), dim3(kIfgThreads), 0, st, int(kind), rows, cols, static_cast<const T*>(height), ld, T(dx), alpha,
                           static_cast<const T*>(window), window_ld, static_cast<T*>(out), out_ld, part);
        hipLaunchKernelGGL(window_fold_kernel, dim3(1), dim3(kIfgThreads), 0, st, wgs, part, static_cast<double*>(s2));
        return int(hipGetLastError());
    });
}

int pm_ifg_psd_scale(int32_t dtype, int64_t rows, int64_t cols, void* data, int64_t ld, const void* s2, double fs, void* stream) {
    const char* who = "pm_ifg_psd_scale";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (rows < 0 || cols < 0 || !data || !s2) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    PM_CHECK_LD("pm_ifg_psd_scale", ld_ok(rows, cols, ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (!aligned(s2, 8)) return fail(PM_ERR_ARG, "%s: S2 is a double (8-byte alignment)", who);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        PsdScaleOp<T> op{static_cast<T*>(data), ld, static_cast<const double*>(s2), fs};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

size_t pm_ifg_band_workspace(int64_t rows, int64_t cols) { return pm_ifg_window_workspace(rows, cols); }

int pm_ifg_band(int32_t dtype, int32_t coords, int32_t ndim, int64_t rows, int64_t cols, const void* psd, int64_t ld, const void* nu, int64_t nu_ld, double dx,
                double flow, double fhigh, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_ifg_band";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (coords != PM_COORDS_GRID && coords != PM_COORDS_POINTWISE) return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID or PM_COORDS_POINTWISE", who);
    if (ndim != 1 && ndim != 2) return fail(PM_ERR_ARG, "%s: ndim must be 1 or 2", who);
    if (rows <= 0 || cols <= 0 || !psd || !out || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    if (ndim == 1 && cols != 1) return fail(PM_ERR_ARG, "%s: a 1-D spectrum is passed as rows x 1", who);
    if (coords == PM_COORDS_POINTWISE && !nu) return fail(PM_ERR_ARG, "%s: the frequencies are missing (null pointer)", who);
    if (coords == PM_COORDS_GRID && !(std::isfinite(dx) && dx != 0)) return fail(PM_ERR_ARG, "%s: the sample spacing must be finite and nonzero", who);
    if (std::isnan(flow) || std::isnan(fhigh)) return fail(PM_ERR_ARG, "%s: the band limits must not be NaN", who);
    PM_CHECK_LD("pm_ifg_band", ld_ok(rows, cols, ld) && (coords != PM_COORDS_POINTWISE || ld_ok(rows, cols, nu_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (workspace_bytes < pm_ifg_band_workspace(rows, cols)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_ifg_band_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(out, 8)) return fail(PM_ERR_ARG, "%s: out and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = ifg_groups(rows * cols);
        const int gen = coords == PM_COORDS_GRID, one_d = ndim == 1;
        double* part = static_cast<double*>(workspace);
        const T* f = gen ? nullptr : static_cast<const T*>(nu);
        // fftfreq's step 1 / (n dx) per axis; the spacing of the reference: two samples along axis 0 through the centre
        const double ux = 1.0 / (double(cols) * dx), uy = 1.0 / (double(rows) * dx);
        const int64_t rc = rows / 2, rp = (rc - 1 + rows) % rows, cc = one_d ? 0 : cols / 2;
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((band_kernel<T>), dim3(wgs), dim3(kIfgThreads), 0, st, rows, cols, static_cast<const T*>(psd), ld, gen, f, nu_ld, ux, uy, flow, fhigh,
                           one_d, part);
        hipLaunchKernelGGL((band_fold_kernel<T>), dim3(1), dim3(kIfgThreads), 0, st, wgs, part, f, rc * nu_ld + cc, rp * nu_ld + cc,
                           std::fabs(double(rp - rc) * uy), one_d, static_cast<double*>(out));
        return int(hipGetLastError());
    });
}

int pm_ifg_iir(int32_t dtype, int32_t parts, int32_t coords, int64_t rows, int64_t cols, const void* r, int64_t r_ld, int64_t oy, int64_t ox, double r_dx,
               double dx, double fcn_low, double fcn_high, void* h_low, void* h_high, int64_t out_ld, void* stream) {
    const char* who = "pm_ifg_iir";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (parts < 1 || parts > (PM_IFG_IIR_HANN | PM_IFG_IIR_LPF)) return fail(PM_ERR_ARG, "%s: parts must be PM_IFG_IIR_HANN, PM_IFG_IIR_LPF or both", who);
    const bool lpf = parts & PM_IFG_IIR_LPF;
    if (coords != PM_COORDS_GRID && coords != PM_COORDS_POINTWISE) return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID or PM_COORDS_POINTWISE", who);
    if (rows < 0 || cols < 0 || !h_low) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (lpf && coords == PM_COORDS_POINTWISE && !r) return fail(PM_ERR_ARG, "%s: the radial coordinate is missing (null pointer)", who);
    if (lpf && !(std::isfinite(dx) && dx != 0)) return fail(PM_ERR_ARG, "%s: the sample spacing must be finite and nonzero", who);
    if (lpf && coords == PM_COORDS_GRID && !std::isfinite(r_dx)) return fail(PM_ERR_ARG, "%s: the grid spacing must be finite", who);
    PM_CHECK_LD("pm_ifg_iir", ld_ok(rows, cols, out_ld) && (!lpf || coords != PM_COORDS_POINTWISE || ld_ok(rows, cols, r_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        IirOp<T> op{int(parts), coords == PM_COORDS_GRID, static_cast<const T*>(r), r_ld, oy, ox, rows, cols, T(r_dx), dx, {fcn_low, fcn_high},
                    {static_cast<T*>(h_low), static_cast<T*>(h_high)}, out_ld};
        return sweep_heavy(rows, cols, PM_STREAM(stream), op);
    });
}

int pm_ifg_combine(int32_t dtype, int32_t typ, int32_t complex_out, int64_t rows, int64_t cols, const void* h_low, int64_t low_ld, const void* h_high,
                   int64_t high_ld, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_ifg_combine";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (typ != PM_IFG_LP && typ != PM_IFG_HP && typ != PM_IFG_BP && typ != PM_IFG_BR)
        return fail(PM_ERR_ARG, "%s: typ must be PM_IFG_LP, PM_IFG_HP, PM_IFG_BP or PM_IFG_BR", who);
    const bool two = typ == PM_IFG_BP || typ == PM_IFG_BR;
    if (rows < 0 || cols < 0 || !h_low || !out || (two && !h_high)) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    PM_CHECK_LD("pm_ifg_combine", ld_ok(rows, cols, low_ld) && ld_ok(rows, cols, out_ld) && (!two || ld_ok(rows, cols, high_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        CombineOp<T> op{int(typ), complex_out != 0, static_cast<const T*>(h_low), static_cast<const T*>(h_high), low_ld, high_ld, out, out_ld};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

int pm_ifg_psd_model(int32_t dtype, int32_t kind, int64_t n, const void* nu, double a, double b, double c, void* out, void* stream) {
    const char* who = "pm_ifg_psd_model";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (kind != PM_IFG_PSD_ABC && kind != PM_IFG_PSD_AB) return fail(PM_ERR_ARG, "%s: kind must be PM_IFG_PSD_ABC or PM_IFG_PSD_AB", who);
    if (n < 0 || !nu || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (n > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld values are too many", who, (long long)n);
    if (n == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        PsdModelOp<T> op{int(kind), static_cast<const T*>(nu), T(a), T(b), T(c), static_cast<T*>(out)};
        return sweep(1, n, PM_STREAM(stream), op);
    });
}

}  // extern "C"
