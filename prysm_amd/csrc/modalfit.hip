// Masked fitting of a stored basis (prysm/polynomials/fitting.py lstsq, normalize_modes, orthogonalize_modes) (gfx950).  K real planes
// modes[k * mode_stride + p] of npts points, float or double; a point is VALID when (mask == NULL || mask[p] != 0) and, with
// finite_from_data, data[0][p] is finite.  Validity is a select: a NaN at an invalid point leaves no trace in any sum.
//
//  - pm_modes_gram: count, G = sum_valid m_i m_j and b = sum_valid m_i d for nrhs data vectors, into the record (PM_MODES_REC_* in
//    prysm_amd.h).  A SYRK whose inner index is the point, on v_mfma_f64_16x16x4_f64: the modes are padded to 16-blocks, a workgroup
//    stages a step of points of every plane in LDS as doubles -- each stored plane is read once -- and its waves share out the block
//    pairs (I <= J of G, then (I, data) of b); lane l holds mode 16 I + (l & 15) at point 4 ks + (l >> 4), which is both the A operand
//    of block I and the B operand of block I.  Every product and sum is in double (float x float is exact there).  The next step's
//    loads are in flight while the current one is multiplied.  Each wave leaves its raw accumulators per (workgroup, split, pair); the
//    second stage adds them in slot order, mirrors the upper triangle and adds the counts: no atomics, the same bits every run.
//  - pm_modes_small: one workgroup on the record.  FACTOR: unpivoted Cholesky G = L L^T in mode order, a mode whose pivot is not above
//    K eps (largest pivot so far) is dropped (row and column zero, flagged, rank counted); SOLVE: coef = G^-1 b by the two
//    substitutions, dropped modes 0; INVERT: T = L^-1; NORMS: T = diag(1 / norm) from the pm_modes_stats record.
//  - pm_modes_transform: out[k][p] = sum_{j <= k} T[k][j] modes[j][p] (LOWER) or T[k][k] modes[k][p] (DIAGONAL), T DEVICE doubles; all
//    K values of a point are in LDS before any is stored, so out may be modes.
//  - pm_modes_stats: per mode over the valid points count, sum, min, max, mean, then sum (m - mean)^2 with the mean read on the device
//    (two-pass, as pm_ifg_stats) and numpy's population std.
//
// Compiled with -ffp-contract=off (csrc/Makefile), as prysm_amd/polynomials/fit_plan.py restates the kernels in numpy.
#include <cmath>
#include <limits>

#include "modal_tile.h"
#include "pm_reduce.h"

namespace pm {
namespace {

constexpr int kFitMax = PM_MODES_FIT_MAX;
constexpr int kGramGroups = 1024;       // most workgroups of the Gram pass: as many partial slots (times the split) per pair
constexpr int kStepWide = 128;          // points per LDS step while the planes fit 32 rows (K <= 16), kStepNarrow beyond
constexpr int kStepNarrow = 32;
constexpr int kMaxPass = 5;             // (128 + 16) rows / 32 rows per pass of the narrow step; the wide step has 32 rows / 8 = 4
constexpr int kRhsBlock = 16;           // data vectors per launch: one 16-block beside the modes

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ bool finite_(T z) {
    return abs_(z) <= std::numeric_limits<T>::max();      // false for NaN and for +-inf
}

__host__ __device__ inline int blocks_of(int64_t K) { return int((K + 15) / 16); }

// pairs of a launch: the upper triangle of the KB x KB blocks of G (with GRAM), then (I, data block) for every I (with data rows)
inline int pairs_of(int KB, bool gram, bool rhs) { return (gram ? KB * (KB + 1) / 2 : 0) + (rhs ? KB : 0); }
// with one or two pairs the four waves split the points of a step instead: 4 or 2 splits
inline int splits_of(int npairs) { return npairs <= 2 ? 4 / npairs : 1; }

template <typename T>
struct GramArgs {
    int K, KB, nrhs, npairs, ngram, splits, vec;
    int64_t npts, mode_stride, data_stride;
    const T* modes;
    const T* data;           // the launch's first data row (read with RHS)
    const T* data0;          // data[0] of the call: the finite half of the predicate, or NULL
    const unsigned char* mask;
};

// 4 consecutive points of a plane at p; 0 past n.  vec: p is a multiple of 4, n too, and the plane starts on a 16-byte boundary
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ src, int64_t p, int64_t n, bool vec, T out[4]) {
    using RT = Runs<T>;
    if (vec) {
        if (p < n) {
#pragma unroll
            for (int r = 0; r < 4 / RT::W; ++r) {
                const typename RT::vec q = *reinterpret_cast<const typename RT::vec*>(src + p + r * RT::W);
#pragma unroll
                for (int e = 0; e < RT::W; ++e) out[r * RT::W + e] = q[e];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] = T(0);
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = p + q < n ? src[p + q] : T(0);
    }
}

// block offsets (LDS rows) of pair t: (16 I, 16 J) of G's upper triangle by rows, then (16 I, the data block at 16 KB)
__host__ __device__ inline void pair_blocks(int t, int ngram, int KB, int& I, int& J) {
    if (t < ngram) {
        I = 0;
        while (t >= KB - I) t -= KB - I, ++I;
        J = I + t;
    } else {
        I = t - ngram;
        J = KB;
    }
}

// STEP points per LDS step; a thread loads 4 consecutive points of a row, STEP / 4 threads per row, kThreads * 4 / STEP rows per pass
template <typename T, int NPW, int STEP>
__global__ __launch_bounds__(kThreads) void gram_kernel(const GramArgs<T> a, double* __restrict__ part, double* __restrict__ pcount) {
    constexpr int LD = STEP + 4;                       // doubles per LDS row: 8 words past a multiple of 64 banks, rows stay 16-byte aligned
    constexpr int PER_ROW = STEP / 4, ROWS_PASS = kThreads / PER_ROW;
    constexpr int NPASS = STEP == kStepWide ? 4 : kMaxPass;
    constexpr int KSTEPS = STEP / 4;
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rows_lds = 16 * a.KB + (a.nrhs ? 16 : 0), nrows = a.K + a.nrhs;
    int* flag = reinterpret_cast<int*>(smem + rows_lds * LD);
    for (int e = tid; e < rows_lds * LD; e += kThreads) smem[e] = 0.0;      // the padding rows stay 0

    // this wave's pairs and its share of a step's points
    int offA[NPW], offB[NPW];
    bool live[NPW];
    const int t0 = a.splits > 1 ? wave % a.npairs : wave * NPW;
    const int split = a.splits > 1 ? wave / a.npairs : 0;
    const int ks0 = split * (KSTEPS / a.splits), ks1 = ks0 + KSTEPS / a.splits;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
        const int t = t0 + i;
        live[i] = t < a.npairs;
        int I = 0, J = 0;
        if (live[i]) pair_blocks(t, a.ngram, a.KB, I, J);
        offA[i] = 16 * I, offB[i] = 16 * J;
    }
    f64x4 acc[NPW];
#pragma unroll
    for (int i = 0; i < NPW; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};

    const int c4 = (tid % PER_ROW) * 4, r0 = tid / PER_ROW;
    T v[NPASS][4];
    int okv = 0;
    double cnt = 0.0;
    const int64_t tile = int64_t(kThreads) * kVec;
    const int64_t ntiles = (a.npts + tile - 1) / tile;

    auto fetch = [&](int64_t p0) {
#pragma unroll
        for (int j = 0; j < NPASS; ++j) {
            const int row = r0 + j * ROWS_PASS;
            if (row < nrows) {
                const T* src = row < a.K ? a.modes + int64_t(row) * a.mode_stride : a.data + int64_t(row - a.K) * a.data_stride;
                load4(src, p0 + c4, a.npts, a.vec != 0, v[j]);
            }
        }
        if (tid < STEP) {
            const int64_t p = p0 + tid;
            bool ok = p < a.npts;
            if (ok && a.mask) ok = a.mask[p] != 0;
            if (ok && a.data0) ok = finite_(a.data0[p]);
            okv = ok;
        }
    };

    // the steps of this workgroup: tiles blockIdx.x, + gridDim.x, ..., each tile / STEP steps
    constexpr int STEPS_TILE = kThreads * kVec / STEP;
    int64_t ti = blockIdx.x;
    int st = 0;
    if (ti < ntiles) fetch(ti * tile);
    __syncthreads();                                    // the zeroes above
    while (ti < ntiles) {
#pragma unroll
        for (int j = 0; j < NPASS; ++j) {
            const int row = r0 + j * ROWS_PASS;
            if (row < nrows) {
                double* dst = smem + (row < a.K ? row : 16 * a.KB + (row - a.K)) * LD + c4;
                reinterpret_cast<double2*>(dst)[0] = double2{double(v[j][0]), double(v[j][1])};
                reinterpret_cast<double2*>(dst)[1] = double2{double(v[j][2]), double(v[j][3])};
            }
        }
        if (tid < STEP) {
            flag[tid] = okv;
            cnt = cnt + double(okv);
        }
        __syncthreads();
        // the next step's loads fly while this one is multiplied
        int64_t tn = ti;
        int sn = st + 1;
        if (sn == STEPS_TILE) sn = 0, tn += gridDim.x;
        if (tn < ntiles) fetch(tn * tile + int64_t(sn) * STEP);
        for (int ks = ks0; ks < ks1; ++ks) {
            const int col = ks * 4 + (lane >> 4);
            const bool ok = flag[col] != 0;
            double av = 0.0;
#pragma unroll
            for (int i = 0; i < NPW; ++i) {
                if (!live[i]) continue;
                if (i == 0 || offA[i] != offA[i - 1]) {
                    const double x = smem[(offA[i] + (lane & 15)) * LD + col];
                    av = ok ? x : 0.0;
                }
                const double y = smem[(offB[i] + (lane & 15)) * LD + col];
                const double bv = ok ? y : 0.0;
                acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
        ti = tn, st = sn;
    }

    const int64_t slot = int64_t(blockIdx.x) * a.splits + split;
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
        if (!live[i]) continue;
        double* dst = part + (slot * a.npairs + (t0 + i)) * 256;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[r * 64 + lane] = acc[i][r];
    }
    // the flags were counted by the first STEP threads: their waves' sums, added in wave order (the loop ended on a barrier)
    const double c = wave_sum(cnt);
    if (lane == 0) smem[wave] = c;
    __syncthreads();
    if (tid == 0) pcount[blockIdx.x] = ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// block t < npairs: element e of pair t added over the slots in order and placed (accumulator register e / 64 of lane e % 64 is row
// (lane >> 4) + 4 reg, column lane & 15 of the 16 x 16 block), G's lower triangle mirrored; block npairs: the count
__global__ __launch_bounds__(256) void gram_fold_kernel(int64_t nslots, int64_t ngroups, int npairs, int ngram, int KB, int K, int nrhs,
                                                        const double* __restrict__ part, const double* __restrict__ pcount, double* __restrict__ G,
                                                        double* __restrict__ b, double* __restrict__ count) {
    const int t = blockIdx.x, e = threadIdx.x;
    if (t == npairs) {
        if (e == 0 && count) {
            double c = 0.0;
            for (int64_t g = 0; g < ngroups; ++g) c = c + pcount[g];
            count[0] = c;
        }
        return;
    }
    double s = 0.0;
    for (int64_t sl = 0; sl < nslots; ++sl) s = s + part[(sl * npairs + t) * 256 + e];
    const int lane = e & 63, reg = e >> 6;
    const int row = (lane >> 4) + 4 * reg, col = lane & 15;
    int I, J;
    pair_blocks(t, ngram, KB, I, J);
    const int gi = 16 * I + row;
    if (gi >= K) return;
    if (t < ngram) {
        const int gj = 16 * J + col;
        if (gj >= K) return;
        G[int64_t(gi) * K + gj] = s;
        if (I != J) G[int64_t(gj) * K + gi] = s;
    } else if (col < nrhs) {
        b[int64_t(col) * K + gi] = s;
    }
}

// ---------------------------------------------------------------- the small algebra, one workgroup on the record
constexpr int kSmallThreads = 256;
constexpr double kEps64 = 2.220446049250313e-16;

__device__ __forceinline__ double* rec_G(double* rec) { return rec + PM_MODES_REC_G; }
__device__ __forceinline__ double* rec_L(double* rec, int K) { return rec + PM_MODES_REC_G + int64_t(K) * K; }
__device__ __forceinline__ double* rec_drop(double* rec, int K) { return rec + PM_MODES_REC_G + 2 * int64_t(K) * K; }
__device__ __forceinline__ double* rec_T(double* rec, int K) { return rec + PM_MODES_REC_G + 2 * int64_t(K) * K + K; }
__device__ __forceinline__ double* rec_b(double* rec, int K) { return rec + PM_MODES_REC_G + 3 * int64_t(K) * K + K; }

template <typename T>
__global__ __launch_bounds__(kSmallThreads) void small_kernel(int op, int K, int nrhs, double* __restrict__ rec, const double* __restrict__ stats,
                                                              T* __restrict__ coef) {
    const int tid = threadIdx.x;
    double* G = rec_G(rec);
    double* Lm = rec_L(rec, K);
    double* drop = rec_drop(rec, K);
    double* Tm = rec_T(rec, K);
    double* b = rec_b(rec, K);
    double* x = b + int64_t(nrhs) * K;       // the coefficients in double; the substitutions run in place here

    if (op == PM_MODES_FACTOR) {
        // left-looking by columns: every thread forms the pivot of column j itself, in the same order, then the rows below are shared out
        double largest = 0.0;
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            double d = G[int64_t(j) * K + j];
            for (int t = 0; t < j; ++t) d = d - Lm[int64_t(j) * K + t] * Lm[int64_t(j) * K + t];
            const bool keep = d > 0.0 && d > double(K) * kEps64 * largest;
            if (keep) {
                const double ljj = sqrt(d);
                if (d > largest) largest = d;
                ++rank;
                for (int i = j + 1 + tid; i < K; i += kSmallThreads) {
                    double s = G[int64_t(i) * K + j];
                    for (int t = 0; t < j; ++t) s = s - Lm[int64_t(i) * K + t] * Lm[int64_t(j) * K + t];
                    Lm[int64_t(i) * K + j] = s / ljj;
                }
                __syncthreads();       // every thread has read row j's old diagonal slot
                if (tid == 0) Lm[int64_t(j) * K + j] = ljj, drop[j] = 0.0;
            } else {
                __syncthreads();
                for (int i = tid; i < K; i += kSmallThreads) {
                    Lm[int64_t(i) * K + j] = 0.0;      // the column
                    Lm[int64_t(j) * K + i] = 0.0;      // the row (and what lies right of the diagonal)
                }
                if (tid == 0) drop[j] = 1.0;
            }
            for (int i = tid; i < j; i += kSmallThreads) Lm[int64_t(i) * K + j] = 0.0;      // above the diagonal
            __syncthreads();
        }
        if (tid == 0) rec[PM_MODES_REC_RANK] = double(rank);
        return;
    }
    if (op == PM_MODES_SOLVE) {
        const int n = K * nrhs;
        for (int e = tid; e < n; e += kSmallThreads) x[e] = b[e];
        __syncthreads();
        // L y = b by columns: y_j = w_j / L_jj, then w_i -= L_ij y_j below
        for (int j = 0; j < K; ++j) {
            if (drop[j] != 0.0) continue;
            const double ljj = Lm[int64_t(j) * K + j];
            for (int r = tid; r < nrhs; r += kSmallThreads) x[int64_t(r) * K + j] = x[int64_t(r) * K + j] / ljj;
            __syncthreads();
            const int below = K - 1 - j;
            for (int e = tid; e < below * nrhs; e += kSmallThreads) {
                const int r = e / below, i = j + 1 + e % below;
                x[int64_t(r) * K + i] = x[int64_t(r) * K + i] - Lm[int64_t(i) * K + j] * x[int64_t(r) * K + j];
            }
            __syncthreads();
        }
        // L^T x = y by rows of L from the last: x_j = w_j / L_jj, then w_i -= L_ji x_j above
        for (int j = K - 1; j >= 0; --j) {
            if (drop[j] != 0.0) {
                for (int r = tid; r < nrhs; r += kSmallThreads) x[int64_t(r) * K + j] = 0.0;
                __syncthreads();
                continue;
            }
            const double ljj = Lm[int64_t(j) * K + j];
            for (int r = tid; r < nrhs; r += kSmallThreads) x[int64_t(r) * K + j] = x[int64_t(r) * K + j] / ljj;
            __syncthreads();
            for (int e = tid; e < j * nrhs; e += kSmallThreads) {
                const int r = e / j, i = e % j;
                x[int64_t(r) * K + i] = x[int64_t(r) * K + i] - Lm[int64_t(j) * K + i] * x[int64_t(r) * K + j];
            }
            __syncthreads();
        }
        for (int e = tid; e < n; e += kSmallThreads) coef[e] = T(x[e]);
        return;
    }
    if (op == PM_MODES_INVERT) {
        // column c of T = L^-1 by forward substitution, one thread per column; dropped rows and columns are 0
        for (int c = tid; c < K; c += kSmallThreads) {
            const bool cdrop = drop[c] != 0.0;
            for (int i = 0; i < K; ++i) {
                double val = 0.0;
                if (i >= c && !cdrop && drop[i] == 0.0) {
                    double s = i == c ? 1.0 : 0.0;
                    for (int t = c; t < i; ++t) s = s - Lm[int64_t(i) * K + t] * Tm[int64_t(t) * K + c];
                    val = s / Lm[int64_t(i) * K + i];
                }
                Tm[int64_t(i) * K + c] = val;
            }
        }
        return;
    }
    // NORMS: T = diag(1 / norm), norm the std or the peak-to-valley of the mode over the mask, 1 where it is below 1e-9
    for (int e = tid; e < K * K; e += kSmallThreads) {
        const int i = e / K, j = e % K;
        double val = 0.0;
        if (i == j) {
            const double* s = stats + int64_t(i) * PM_MODES_STAT_RECORD;
            double norm = op == PM_MODES_NORMS_STD ? s[PM_MODES_STAT_STD] : s[PM_MODES_STAT_MAX] - s[PM_MODES_STAT_MIN];
            if (norm < 1e-9) norm = 1.0;
            val = 1.0 / norm;
        }
        Tm[e] = val;
    }
}

// ---------------------------------------------------------------- transform
constexpr int kXfPts = 64;      // points per workgroup: thread (point = tid & 63, quarter = tid >> 6) forms the modes k = quarter mod 4

template <typename T>
__global__ __launch_bounds__(kThreads) void transform_kernel(int diag, int zero_outside, int K, int64_t npts, const T* __restrict__ modes,
                                                             int64_t mode_stride, const double* __restrict__ Tm,
                                                             const unsigned char* __restrict__ mask, T* __restrict__ out, int64_t out_stride) {
    extern __shared__ double smem[];
    T* v = reinterpret_cast<T*>(smem);
    const int tid = threadIdx.x, pt = tid & 63, kq = tid >> 6;
    const int64_t p = int64_t(blockIdx.x) * kXfPts + pt;
    const bool in = p < npts;
    for (int j = kq; j < K; j += 4) v[j * kXfPts + pt] = in ? modes[int64_t(j) * mode_stride + p] : T(0);
    const bool keep = in && !(zero_outside && mask && mask[in ? p : 0] == 0);
    __syncthreads();
    for (int k = kq; k < K; k += 4) {
        double s = 0.0;
        if (diag) {
            s = Tm[int64_t(k) * K + k] * double(v[k * kXfPts + pt]);
        } else {
            for (int j = 0; j <= k; ++j) s = s + Tm[int64_t(k) * K + j] * double(v[j * kXfPts + pt]);
        }
        if (in) out[int64_t(k) * out_stride + p] = keep ? T(s) : T(0);
    }
}

// ---------------------------------------------------------------- statistics per mode
constexpr int kStatWgs = 256;      // most workgroups per mode of a first stage

int stat_groups(int64_t n) { return reduce_groups(n, kThreads, kStatWgs); }

template <typename T>
__global__ __launch_bounds__(kThreads) void mstats_a_kernel(int64_t npts, const T* __restrict__ modes, int64_t mode_stride,
                                                            const unsigned char* __restrict__ mask, double* __restrict__ psum, double* __restrict__ pmax) {
    const T* m = modes + int64_t(blockIdx.y) * mode_stride;
    double s[2] = {0.0, 0.0};
    double x[2] = {-INFINITY, -INFINITY};
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < npts; i += stride) {
        if (mask && !mask[i]) continue;
        const double z = double(m[i]);
        s[0] = s[0] + 1.0;
        s[1] = s[1] + z;
        x[0] = FoldNanMax::of(x[0], -z);
        x[1] = FoldNanMax::of(x[1], z);
    }
    const int64_t o = (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 2;
    wg_fold<kThreads, FoldSum>(threadIdx.x, s, psum + o);
    wg_fold<kThreads, FoldNanMax>(threadIdx.x, x, pmax + o);
}

__global__ __launch_bounds__(kThreads) void mstats_a_fold_kernel(int nparts, const double* __restrict__ psum, const double* __restrict__ pmax,
                                                                 double* __restrict__ stats) {
    double s[2], x[2];
    const int64_t o = int64_t(blockIdx.x) * nparts * 2;
    fold_partials<kThreads, FoldSum>(threadIdx.x, nparts, psum + o, 0.0, s);
    fold_partials<kThreads, FoldNanMax>(threadIdx.x, nparts, pmax + o, -INFINITY, x);
    if (threadIdx.x == 0) {
        double* r = stats + int64_t(blockIdx.x) * PM_MODES_STAT_RECORD;
        const bool any = s[0] > 0.0;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        r[PM_MODES_STAT_N] = s[0];
        r[PM_MODES_STAT_SUM] = s[1];
        r[PM_MODES_STAT_MIN] = any ? -x[0] : nan;
        r[PM_MODES_STAT_MAX] = any ? x[1] : nan;
        r[PM_MODES_STAT_MEAN] = s[1] / s[0];
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mstats_b_kernel(int64_t npts, const T* __restrict__ modes, int64_t mode_stride,
                                                            const unsigned char* __restrict__ mask, const double* __restrict__ stats,
                                                            double* __restrict__ part) {
    const T* m = modes + int64_t(blockIdx.y) * mode_stride;
    const double mean = stats[int64_t(blockIdx.y) * PM_MODES_STAT_RECORD + PM_MODES_STAT_MEAN];
    double s[1] = {0.0};
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < npts; i += stride) {
        if (mask && !mask[i]) continue;
        const double e = double(m[i]) - mean;
        s[0] = s[0] + e * e;
    }
    wg_fold<kThreads, FoldSum>(threadIdx.x, s, part + int64_t(blockIdx.y) * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void mstats_b_fold_kernel(int nparts, const double* __restrict__ part, double* __restrict__ stats) {
    double s[1];
    fold_partials<kThreads, FoldSum>(threadIdx.x, nparts, part + int64_t(blockIdx.x) * nparts, 0.0, s);
    if (threadIdx.x == 0) {
        double* r = stats + int64_t(blockIdx.x) * PM_MODES_STAT_RECORD;
        r[PM_MODES_STAT_M2] = s[0];
        r[PM_MODES_STAT_STD] = r[PM_MODES_STAT_N] > 0.0 ? sqrt(s[0] / r[PM_MODES_STAT_N]) : std::numeric_limits<double>::quiet_NaN();
    }
}

// ---------------------------------------------------------------- host
bool k_ok(int64_t K) { return K >= 1 && K <= kFitMax; }

int64_t gram_groups(int64_t npts) { return project_groups(npts, kGramGroups); }

// doubles of workspace per workgroup of the largest launch of a call: the raw accumulators of every (split, pair), and the count
size_t gram_group_doubles(int64_t K, int64_t nrhs) {
    const int KB = blocks_of(K);
    size_t most = 0;
    for (int np : {pairs_of(KB, true, nrhs > 0), pairs_of(KB, true, false), pairs_of(KB, false, true)})
        most = std::max(most, size_t(splits_of(np)) * np * 256);
    return most + 1;
}

template <int STEP>
size_t gram_lds(int KB, bool rhs) { return size_t(16 * KB + (rhs ? 16 : 0)) * (STEP + 4) * sizeof(double) + STEP * sizeof(int); }

template <typename T, int NPW, int STEP>
void gram_launch(const GramArgs<T>& a, int64_t groups, double* part, double* pcount, hipStream_t st) {
    const size_t lds = gram_lds<STEP>(a.KB, a.nrhs > 0);
    hipLaunchKernelGGL((gram_kernel<T, NPW, STEP>), dim3(unsigned(groups)), dim3(kThreads), lds, st, a, part, pcount);
}

template <typename T>
void gram_dispatch(const GramArgs<T>& a, int64_t groups, double* part, double* pcount, hipStream_t st) {
    if (a.KB == 1) return gram_launch<T, 1, kStepWide>(a, groups, part, pcount, st);
    const int npw = a.splits > 1 ? 1 : (a.npairs + kWaves - 1) / kWaves;
    if (npw <= 1) return gram_launch<T, 1, kStepNarrow>(a, groups, part, pcount, st);
    if (npw <= 2) return gram_launch<T, 2, kStepNarrow>(a, groups, part, pcount, st);
    if (npw <= 3) return gram_launch<T, 3, kStepNarrow>(a, groups, part, pcount, st);
    if (npw <= 4) return gram_launch<T, 4, kStepNarrow>(a, groups, part, pcount, st);
    if (npw <= 6) return gram_launch<T, 6, kStepNarrow>(a, groups, part, pcount, st);
    if (npw <= 8) return gram_launch<T, 8, kStepNarrow>(a, groups, part, pcount, st);
    return gram_launch<T, 11, kStepNarrow>(a, groups, part, pcount, st);
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

size_t pm_modes_record_doubles(int64_t K, int64_t nrhs) {
    if (!k_ok(K) || nrhs < 0 || nrhs > INT32_MAX / kFitMax) return 0;
    return size_t(PM_MODES_REC_G) + 3 * size_t(K) * K + K + 2 * size_t(nrhs) * K;
}

size_t pm_modes_gram_workspace(int32_t dtype, int64_t K, int64_t npts, int64_t nrhs) {
    if (!real_dtype(dtype) || !k_ok(K) || npts <= 0 || nrhs < 0) return 0;
    return size_t(gram_groups(npts)) * gram_group_doubles(K, nrhs) * sizeof(double);
}

int pm_modes_gram(int32_t dtype, int32_t parts, int64_t K, int64_t npts, const void* modes, int64_t mode_stride, int64_t nrhs, const void* data,
                  int64_t data_stride, const void* mask, int32_t finite_from_data, void* record, void* workspace, size_t workspace_bytes,
                  void* stream) {
    const char* who = "pm_modes_gram";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (parts < 1 || parts > (PM_MODES_GRAM | PM_MODES_RHS)) return fail(PM_ERR_ARG, "%s: parts must be PM_MODES_GRAM, PM_MODES_RHS or both", who);
    if (K < 1) return fail(PM_ERR_ARG, "%s: the number of modes must be at least 1", who);
    if (K > kFitMax) return fail(PM_ERR_UNSUPPORTED, "%s: %lld modes are more than PM_MODES_FIT_MAX = %d", who, (long long)K, kFitMax);
    if (npts <= 0 || nrhs < 0 || !modes || !record || !workspace || (nrhs > 0 && !data))
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer, no point or a negative count)", who);
    if (finite_from_data && nrhs == 0) return fail(PM_ERR_ARG, "%s: finite_from_data needs a data vector", who);
    if (npts > INT32_MAX || nrhs > INT32_MAX / kFitMax) return fail(PM_ERR_ARG, "%s: %lld points or %lld vectors are too many", who, (long long)npts, (long long)nrhs);
    if (mode_stride < npts || (nrhs > 0 && data_stride < npts)) return fail(PM_ERR_ARG, "%s: a stride is smaller than the number of points", who);
    if (workspace_bytes < pm_modes_gram_workspace(dtype, K, npts, nrhs))
        return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_modes_gram_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(record, 8)) return fail(PM_ERR_ARG, "%s: the record and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        const T* d = static_cast<const T*>(data);
        const bool want_g = parts & PM_MODES_GRAM, want_b = (parts & PM_MODES_RHS) && nrhs > 0;
        if (!want_g && !want_b) return 0;
        const int KB = blocks_of(K);
        const int64_t groups = gram_groups(npts);
        double* rec = static_cast<double*>(record);
        double* part = static_cast<double*>(workspace);
        const int vec = vec_ok(npts, {modes, want_b ? data : nullptr, finite_from_data ? data : nullptr}) && (mode_stride * sizeof(T)) % 16 == 0 &&
                        (!want_b || (data_stride * sizeof(T)) % 16 == 0);
        double* G = rec + PM_MODES_REC_G;
        double* b = G + 3 * K * K + K;
        // the first launch forms G (if asked) and the count beside the first 16 vectors; further vectors take launches of their own
        for (int64_t r0 = 0; r0 == 0 || (want_b && r0 < nrhs); r0 += kRhsBlock) {
            GramArgs<T> a;
            a.K = int(K), a.KB = KB;
            a.nrhs = want_b ? int(std::min<int64_t>(kRhsBlock, nrhs - r0)) : 0;
            a.ngram = want_g && r0 == 0 ? KB * (KB + 1) / 2 : 0;
            a.npairs = a.ngram + (a.nrhs ? KB : 0);
            a.splits = splits_of(a.npairs);
            a.vec = vec;
            a.npts = npts, a.mode_stride = mode_stride, a.data_stride = data_stride;
            a.modes = static_cast<const T*>(modes);
            a.data = want_b ? d + r0 * data_stride : nullptr;
            a.data0 = finite_from_data ? d : nullptr;
            a.mask = static_cast<const unsigned char*>(mask);
            double* pcount = part + size_t(groups) * a.splits * a.npairs * 256;
            gram_dispatch<T>(a, groups, part, pcount, st);
            hipLaunchKernelGGL(gram_fold_kernel, dim3(a.npairs + 1), dim3(256), 0, st, groups * a.splits, groups, a.npairs, a.ngram, KB, int(K), a.nrhs,
                               part, pcount, G, b + r0 * K, want_g && r0 == 0 ? rec + PM_MODES_REC_COUNT : nullptr);
        }
        return int(hipGetLastError());
    });
}

int pm_modes_small(int32_t dtype, int32_t op, int64_t K, int64_t nrhs, void* record, const void* stats, void* coef, void* stream) {
    const char* who = "pm_modes_small";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (op < PM_MODES_FACTOR || op > PM_MODES_NORMS_PTP) return fail(PM_ERR_ARG, "%s: op must be one of PM_MODES_FACTOR .. PM_MODES_NORMS_PTP", who);
    if (K < 1) return fail(PM_ERR_ARG, "%s: the number of modes must be at least 1", who);
    if (K > kFitMax) return fail(PM_ERR_UNSUPPORTED, "%s: %lld modes are more than PM_MODES_FIT_MAX = %d", who, (long long)K, kFitMax);
    if (nrhs < 0 || nrhs > INT32_MAX / kFitMax) return fail(PM_ERR_ARG, "%s: bad argument (the number of vectors)", who);
    if (!record) return fail(PM_ERR_ARG, "%s: the record is missing (null pointer)", who);
    if (op == PM_MODES_SOLVE && nrhs > 0 && !coef) return fail(PM_ERR_ARG, "%s: the coefficients are missing (null pointer)", who);
    if ((op == PM_MODES_NORMS_STD || op == PM_MODES_NORMS_PTP) && !stats) return fail(PM_ERR_ARG, "%s: the statistics are missing (null pointer)", who);
    if (!aligned(record, 8) || !aligned(stats, 8)) return fail(PM_ERR_ARG, "%s: the record and the statistics hold doubles (8-byte alignment)", who);
    if (op == PM_MODES_SOLVE && nrhs == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL((small_kernel<T>), dim3(1), dim3(kSmallThreads), 0, PM_STREAM(stream), int(op), int(K), int(nrhs), static_cast<double*>(record),
                           static_cast<const double*>(stats), static_cast<T*>(coef));
        return int(hipGetLastError());
    });
}

int pm_modes_transform(int32_t dtype, int32_t form, int32_t zero_outside, int64_t K, int64_t npts, const void* modes, int64_t mode_stride,
                       const void* record, const void* mask, void* out, int64_t out_stride, void* stream) {
    const char* who = "pm_modes_transform";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (form != PM_MODES_LOWER && form != PM_MODES_DIAGONAL) return fail(PM_ERR_ARG, "%s: form must be PM_MODES_LOWER or PM_MODES_DIAGONAL", who);
    if (K < 1) return fail(PM_ERR_ARG, "%s: the number of modes must be at least 1", who);
    if (K > kFitMax) return fail(PM_ERR_UNSUPPORTED, "%s: %lld modes are more than PM_MODES_FIT_MAX = %d", who, (long long)K, kFitMax);
    if (npts < 0 || !modes || !record || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (zero_outside && !mask) return fail(PM_ERR_ARG, "%s: zero_outside needs the mask (null pointer)", who);
    if (npts > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld points are too many", who, (long long)npts);
    if (mode_stride < npts || out_stride < npts) return fail(PM_ERR_ARG, "%s: a stride is smaller than the number of points", who);
    if (!aligned(record, 8)) return fail(PM_ERR_ARG, "%s: the record holds doubles (8-byte alignment)", who);
    if (npts == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const double* Tm = static_cast<const double*>(record) + PM_MODES_REC_G + 2 * K * K + K;
        const int64_t groups = (npts + kXfPts - 1) / kXfPts;
        const size_t lds = (size_t(K) * kXfPts * sizeof(T) + 7) / 8 * 8;
        hipLaunchKernelGGL((transform_kernel<T>), dim3(unsigned(groups)), dim3(kThreads), lds, PM_STREAM(stream), int(form == PM_MODES_DIAGONAL),
                           int(zero_outside != 0), int(K), npts, static_cast<const T*>(modes), mode_stride, Tm, static_cast<const unsigned char*>(mask),
                           static_cast<T*>(out), out_stride);
        return int(hipGetLastError());
    });
}

size_t pm_modes_stats_workspace(int64_t K, int64_t npts) {
    if (!k_ok(K) || npts <= 0 || npts > INT32_MAX) return 0;
    return size_t(K) * stat_groups(npts) * 5 * sizeof(double);
}

int pm_modes_stats(int32_t dtype, int64_t K, int64_t npts, const void* modes, int64_t mode_stride, const void* mask, void* stats, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const char* who = "pm_modes_stats";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (K < 1) return fail(PM_ERR_ARG, "%s: the number of modes must be at least 1", who);
    if (K > kFitMax) return fail(PM_ERR_UNSUPPORTED, "%s: %lld modes are more than PM_MODES_FIT_MAX = %d", who, (long long)K, kFitMax);
    if (npts <= 0 || !modes || !stats || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or no point)", who);
    if (npts > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld points are too many", who, (long long)npts);
    if (mode_stride < npts) return fail(PM_ERR_ARG, "%s: a stride is smaller than the number of points", who);
    if (workspace_bytes < pm_modes_stats_workspace(K, npts)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_modes_stats_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(stats, 8)) return fail(PM_ERR_ARG, "%s: the statistics and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = stat_groups(npts);
        double* psum = static_cast<double*>(workspace);
        double* pmax = psum + size_t(K) * wgs * 2;
        double* pb = pmax + size_t(K) * wgs * 2;
        double* rec = static_cast<double*>(stats);
        const T* m = static_cast<const T*>(modes);
        const unsigned char* mk = static_cast<const unsigned char*>(mask);
        hipStream_t st = PM_STREAM(stream);
        hipLaunchKernelGGL((mstats_a_kernel<T>), dim3(wgs, unsigned(K)), dim3(kThreads), 0, st, npts, m, mode_stride, mk, psum, pmax);
        hipLaunchKernelGGL(mstats_a_fold_kernel, dim3(unsigned(K)), dim3(kThreads), 0, st, wgs, psum, pmax, rec);
        hipLaunchKernelGGL((mstats_b_kernel<T>), dim3(wgs, unsigned(K)), dim3(kThreads), 0, st, npts, m, mode_stride, mk, rec, pb);
        hipLaunchKernelGGL(mstats_b_fold_kernel, dim3(unsigned(K)), dim3(kThreads), 0, st, wgs, pb, rec);
        return int(hipGetLastError());
    });
}

}  // extern "C"
