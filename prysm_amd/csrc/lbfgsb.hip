// L-BFGS-B (prysm/x/optym/_prysm_lbfgsb.py) (gfx950): the passes over the n variables of one step of PrysmLBFGSB.
//
// The history is S and Y, (ring, n) row-major `ld` apart, a ring in PHYSICAL order: logical pair j (oldest first) of the k live ones is
// physical row (start + j) % ring, and nothing is rolled or gathered.  The compact form's W = [Y, theta S] has 2k rows q: q < k is
// Y's logical row q, q >= k is S's logical row q - k; every result below is in that LOGICAL order, and theta is applied by the caller
// to the small products.  Sums are in double.
//
//  - dots_kernel: for one tile of kTile history rows (grid.y) the products row . v of one or two vectors, and a few sums of the
//    vectors themselves.  The vector comes from a source: a stored vector under a byte mask (W^T g, W_F^T r, phi' = g . p), the
//    projected steepest-descent ray of the breakpoint pass (which also stores t and d0), or the new pair s, y of the history update
//    (which also stores them into the ring's free row).  Every history row is read once; the source is read (and, for the
//    breakpoints, t and d0 recomputed) once per tile, up to 8 times at 2k = 64.
//  - gram_kernel: the masked products of two row tiles, W_F^T W_F in 8 x 8 blocks over grid.y.  A row is read once per tile pair
//    it belongs to (ntile + 1 times), not once.
//  - combine_kernel: out = a v + b (u1 - u2) + sum_q coef[q] row_q in double, rounded at the store, with the tails of -H g, of the
//    reduced gradient r, and of the subspace step (dx on the free set, x_hat, x_bar, both directions and their sums).
//  - cauchy_kernel, trial_kernel: elementwise stores.
//  - small_kernel: everything of size 2k x 2k, one workgroup per use: it adds the partials of the pass before it, assembles M and N from
//    the three Gram matrices kept on the device, solves with partial pivoting, takes the curvature decision and theta, updates the
//    Gram matrices, and leaves the next combination's coefficients on the device and a small record for the host.
//  - fold_kernel (for a caller that wants a pass's sums themselves, e.g. phi' = g . p): one workgroup per tile adds (or takes the max / min of) the first-stage partials in a fixed order (pm_reduce.h)
//    into a record of doubles.  No atomics: a launch shape gives the same bits run after run.
//
// prysm_amd/x/lbfgsb_plan.py is this file in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile).
#include <algorithm>
#include <cmath>

#include "pm_entry.h"
#include "pm_reduce.h"

namespace pm {
namespace {

constexpr int kThreads = PM_LBFGSB_THREADS;
constexpr int kWgs = PM_LBFGSB_WGS;              // most first-stage workgroups of a dots or combine pass
constexpr int kGramWgs = PM_LBFGSB_GRAM_WGS;     // ... of the Gram pass, per tile pair
constexpr int kMaxMemory = PM_LBFGSB_MAX_MEMORY;
constexpr int kTile = PM_LBFGSB_TILE;            // history rows of a tile: kTile * NV + NX double accumulators per thread
constexpr int kMaxTiles = 2 * kMaxMemory / kTile;
constexpr int kMaxPairs = kMaxTiles * (kMaxTiles + 1) / 2;
constexpr int kMaxSlots = kTile * 2 + 3;         // most sums of a dots pass per tile (the history update)
constexpr int kCombineSlots = 5;                 // g.p, nnz(p), g.p_hat, nnz(p_hat) | min alpha
constexpr int kElemBlocks = 1 << 18;             // most workgroups of an elementwise pass (grid-stride beyond)

constexpr size_t kWsDoubles = std::max({size_t(kMaxTiles) * kWgs * kMaxSlots, size_t(kMaxPairs) * kGramWgs * kTile * kTile, size_t(kWgs) * kCombineSlots});

struct FoldMin {
    template <typename V> static __device__ __forceinline__ V of(V u, V w) { return w < u ? w : u; }
};

template <typename T>
struct Hist {
    const T* S; const T* Y; int64_t ld; int ring, start, k;
    // row q of W's 2k, logical order
    __host__ __device__ const T* row(int q) const {
        const T* base = q < k ? Y : S;
        const int j = q < k ? q : q - k;
        return base + int64_t((start + j) % ring) * ld;
    }
};

// ---------------------------------------------------------------------------------------------------------------- vector sources

// a stored vector v under an optional mask; the extra sum is v . w (v . v without w)
template <typename T>
struct SrcVec {
    static constexpr int NV = 1, NX = 1;
    const T* v; const T* w; const uint8_t* mask;
    __device__ bool load(int64_t i, bool, double (&val)[NV], double (&ex)[NX]) const {
        if (mask && !mask[i]) return false;
        val[0] = double(v[i]);
        ex[0] = val[0] * (w ? double(w[i]) : val[0]);
        return true;
    }
};

// _compute_breakpoints (lines 477-507) and the start of _cauchy (lines 565-609): t_i, and d0 = -g where t_i > 0, 0 elsewhere (the
// variables with t_i = 0 leave the path at once).  Extra sums: d0 . d0, the count of t_i <= 0, the count of finite t_i > 0
template <typename T>
struct SrcBreak {
    static constexpr int NV = 1, NX = 3;
    const T* x; const T* g; const T* lo; const T* hi; T* t; T* d0;
    __device__ bool load(int64_t i, bool first, double (&val)[NV], double (&ex)[NX]) const {
        const T xi = x[i], gi = g[i], l = lo[i], u = hi[i];
        T ti = T(INFINITY);
        if (gi > T(0) && isfinite(l)) ti = (xi - l) / gi;
        if (gi < T(0) && isfinite(u)) ti = (xi - u) / gi;
        const T d = ti > T(0) ? -gi : T(0);
        if (first) t[i] = ti, d0[i] = d;
        val[0] = double(d);
        ex[0] = val[0] * val[0];
        ex[1] = ti <= T(0) ? 1.0 : 0.0;
        ex[2] = (ti > T(0) && isfinite(ti)) ? 1.0 : 0.0;
        return true;
    }
};

// step(), lines 1086-1096: s = alpha p (unbounded) or s = x_trial - x (bounded: the trial point was clipped), y = g_new - g, stored
// into the ring's free row.  Extra sums: s . s, s . y, y . y
template <typename T>
struct SrcPair {
    static constexpr int NV = 2, NX = 3;
    const T* xt; const T* x; const T* p; T alpha; int bounded; const T* gn; const T* g; T* srow; T* yrow;
    __device__ bool load(int64_t i, bool first, double (&val)[NV], double (&ex)[NX]) const {
        const T s = bounded ? xt[i] - x[i] : p[i] * alpha;
        const T y = gn[i] - g[i];
        if (first) srow[i] = s, yrow[i] = y;
        val[0] = double(s), val[1] = double(y);
        ex[0] = val[0] * val[0];
        ex[1] = val[0] * val[1];
        ex[2] = val[1] * val[1];
        return true;
    }
};

// partial[(tile * gridDim.x + wg) * NS + j]: j = r * NV + vi the product of the tile's row r with vector vi, then the NX extra sums
template <typename T, typename Src>
__global__ __launch_bounds__(kThreads) void dots_kernel(int64_t n, Hist<T> h, Src src, double* __restrict__ partial) {
    constexpr int NV = Src::NV, NX = Src::NX, NS = kTile * NV + NX;
    const int tile = blockIdx.y, q0 = tile * kTile;
    const int nq = min(kTile, 2 * h.k - q0);
    const T* rows[kTile];
#pragma unroll
    for (int r = 0; r < kTile; ++r) rows[r] = r < nq ? h.row(q0 + r) : nullptr;
    double a[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = 0.0;
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        double val[NV], ex[NX];
        if (!src.load(i, tile == 0, val, ex)) continue;
#pragma unroll
        for (int r = 0; r < kTile; ++r)
            if (r < nq) {
                const double w = double(rows[r][i]);
#pragma unroll
                for (int vi = 0; vi < NV; ++vi) a[r * NV + vi] = a[r * NV + vi] + w * val[vi];
            }
#pragma unroll
        for (int e = 0; e < NX; ++e) a[kTile * NV + e] = a[kTile * NV + e] + ex[e];
    }
    wg_fold<kThreads, FoldSum>(threadIdx.x, a, partial + (int64_t(tile) * gridDim.x + blockIdx.x) * NS);
}

// record[grp * ns + j] from partial[(grp * nparts + i) * ns + j], i < nparts: a sum for j < first_min, a minimum from there on.  One
// workgroup per group (blockIdx.x), one value after the other
__global__ __launch_bounds__(kThreads) void fold_kernel(int nparts, int ns, int first_min, const double* __restrict__ partial,
                                                         double* __restrict__ record) {
    const int grp = blockIdx.x, tid = threadIdx.x;
    const double* p = partial + int64_t(grp) * nparts * ns;
    for (int j = 0; j < ns; ++j) {
        const bool is_min = j >= first_min;
        double a[1] = {is_min ? double(INFINITY) : 0.0}, total[1];
        for (int i = tid; i < nparts; i += kThreads) {
            const double v = p[int64_t(i) * ns + j];
            a[0] = is_min ? FoldMin::of(a[0], v) : a[0] + v;
        }
        if (is_min)
            wg_total<kThreads, FoldMin>(tid, a, total);
        else
            wg_total<kThreads, FoldSum>(tid, a, total);
        if (tid == 0) record[int64_t(grp) * ns + j] = total[0];
        __syncthreads();      // the next turn may run the same instantiation of wg_tree: its LDS array is reused
    }
}

// partial[(pair * gridDim.x + wg) * 64 + r * 8 + c] = sum over the free i of row (ti * 8 + r) x row (tj * 8 + c), pair = blockIdx.y
// counting the tile pairs ti <= tj row by row (_subspace_solve, line 883)
template <typename T>
__global__ __launch_bounds__(kThreads) void gram_kernel(int64_t n, Hist<T> h, const uint8_t* __restrict__ mask, double* __restrict__ partial) {
    const int ntile = (2 * h.k + kTile - 1) / kTile;
    int ti = 0, rem = blockIdx.y;
    while (rem >= ntile - ti) rem -= ntile - ti, ++ti;
    const int tj = ti + rem;
    const int na = min(kTile, 2 * h.k - ti * kTile), nb = min(kTile, 2 * h.k - tj * kTile);
    const T* A[kTile];
    const T* B[kTile];
#pragma unroll
    for (int r = 0; r < kTile; ++r) {
        A[r] = r < na ? h.row(ti * kTile + r) : nullptr;
        B[r] = r < nb ? h.row(tj * kTile + r) : nullptr;
    }
    double acc[kTile * kTile];
#pragma unroll
    for (int j = 0; j < kTile * kTile; ++j) acc[j] = 0.0;
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        double a[kTile], b[kTile];
#pragma unroll
        for (int r = 0; r < kTile; ++r) {
            a[r] = r < na ? double(A[r][i]) : 0.0;
            b[r] = r < nb ? double(B[r][i]) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < kTile; ++r)
#pragma unroll
            for (int c = 0; c < kTile; ++c) acc[r * kTile + c] = acc[r * kTile + c] + a[r] * b[c];
    }
    double* dst = partial + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * (kTile * kTile);
    // 64 sums through a tree of 16 at a time: the tree's LDS is 16 x 256 doubles, 32 KiB
#pragma unroll
    for (int grp = 0; grp < kTile * kTile / 16; ++grp) {
        double part[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) part[j] = acc[grp * 16 + j];
        wg_fold<kThreads, FoldSum>(threadIdx.x, part, dst + grp * 16);
        __syncthreads();
    }
}

// out = a v + b (u1 - u2) + sum_q coef[q] row_q, in double, rounded once.
//   PM_LBFGSB_DIRECTION: out = p (-H g of _Hg, lines 430-437, with v = g); sums g . p and the count of p != 0.
//   PM_LBFGSB_RESIDUAL:  out = r = g + theta (xc - x) - W M^-1 c (lines 856-863); no sums.
//   PM_LBFGSB_SUBSPACE:  dx = out's value on the free set, 0 elsewhere (lines 893-903); x_hat = xc + dx, x_bar = clip(x_hat),
//     out = p = x_bar - x, out2 = p_hat = x_hat - x (lines 1045-1061); sums g . p, count p != 0, g . p_hat, count p_hat != 0 and the
//     minimum of _max_alpha_inside_box's bound_alpha for p_hat (lines 906-926)
template <typename T>
__global__ __launch_bounds__(kThreads) void combine_kernel(int mode, int64_t n, Hist<T> h, double a, const T* __restrict__ v, double b,
                                                            const T* __restrict__ u1, const T* __restrict__ u2, const double* __restrict__ coef,
                                                            const uint8_t* __restrict__ mask, const T* __restrict__ xc, const T* __restrict__ x,
                                                            const T* __restrict__ lo, const T* __restrict__ hi, const T* __restrict__ g,
                                                            T* __restrict__ out, T* __restrict__ out2, double* __restrict__ partial) {
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    double amin[1] = {double(INFINITY)};
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        double acc = a * double(v[i]);
        if (u1) acc = acc + b * (double(u1[i]) - double(u2[i]));
        for (int j = 0, ph = h.start; j < h.k; ++j, ph = ph + 1 == h.ring ? 0 : ph + 1) acc = acc + coef[j] * double(h.Y[int64_t(ph) * h.ld + i]);
        for (int j = 0, ph = h.start; j < h.k; ++j, ph = ph + 1 == h.ring ? 0 : ph + 1) acc = acc + coef[h.k + j] * double(h.S[int64_t(ph) * h.ld + i]);
        if (mode == PM_LBFGSB_RESIDUAL) {
            out[i] = T(acc);
            continue;
        }
        T p;
        if (mode == PM_LBFGSB_DIRECTION) {
            p = T(acc);
        } else {
            const T dx = (!mask || mask[i]) ? T(acc) : T(0);
            const T xi = x[i], l = lo[i], u = hi[i];
            const T xhat = xc[i] + dx;
            T xbar = xhat;
            if (xbar == xbar) xbar = fmin(fmax(xbar, l), u);      // numpy's maximum / minimum hand a NaN through
            p = xbar - xi;
            const T ph = xhat - xi;
            out2[i] = ph;
            sums[2] = sums[2] + double(g[i]) * double(ph);
            sums[3] = sums[3] + (ph != T(0) ? 1.0 : 0.0);
            T ba = T(INFINITY);
            if (ph > T(0)) ba = (u - xi) / ph;
            if (ph < T(0)) ba = (l - xi) / ph;
            amin[0] = FoldMin::of(amin[0], double(ba));
        }
        out[i] = p;
        sums[0] = sums[0] + double(g[i]) * double(p);
        sums[1] = sums[1] + (p != T(0) ? 1.0 : 0.0);
    }
    if (mode == PM_LBFGSB_RESIDUAL) return;
    double* dst = partial + int64_t(blockIdx.x) * kCombineSlots;
    // no barrier between the two folds: wg_tree's static LDS array is one per template instantiation, and <FoldSum, 4> and <FoldMin, 1>
    // are two.  gram_kernel below calls ONE instantiation four times and needs the barrier
    wg_fold<kThreads, FoldSum>(threadIdx.x, sums, dst);
    wg_fold<kThreads, FoldMin>(threadIdx.x, amin, dst + 4);
}

// the Cauchy point write, lines 746-775: a variable is visited when t_i <= t_last (the sweep never stops inside a tie), then
// xc = x - t g; the others move along -g by t_stop = t_old + dt_min and stay free
template <typename T>
__global__ __launch_bounds__(kThreads) void cauchy_kernel(int64_t n, const T* __restrict__ x, const T* __restrict__ g, const T* __restrict__ t,
                                                           T t_last, T t_stop, T* __restrict__ xc, uint8_t* __restrict__ free_mask) {
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        const T ti = t[i], gi = g[i], xi = x[i];
        const bool visited = ti <= t_last;
        xc[i] = visited ? xi - ti * gi : (-gi) * t_stop + xi;
        free_mask[i] = uint8_t(!visited);
    }
}

// the trial point x + alpha p of _wolfe_eval (line 25).  Under bounds EVERY trial point is clipped into the box, where the reference
// clips only the accepted one (lines 1088-1093): the accepted trial point is x_new itself
template <typename T>
__global__ __launch_bounds__(kThreads) void trial_kernel(int64_t n, const T* __restrict__ x, const T* __restrict__ p, T alpha,
                                                          const T* __restrict__ lo, const T* __restrict__ hi, T* __restrict__ xt) {
    const int64_t stride = int64_t(gridDim.x) * kThreads;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
        T v = x[i] + alpha * p[i];
        if (lo && v == v) v = fmin(fmax(v, lo[i]), hi[i]);
        xt[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- small algebra

constexpr int kN = 2 * kMaxMemory;      // most rows of W
constexpr int kLd = kN + 2;             // a row of the augmented matrix in LDS: kN columns, the right-hand side, one of padding

struct Small {
    int op, m, k, nparts, gparts, f32;
    double eps;
};

// Everything of size 2k x 2k, in double, ONE workgroup per use (the compact form, lines 316-345; _WM, lines 362-407; _Hg, lines
// 424-437; _subspace_solve, lines 856-899; _update_history, lines 979-1007).  `st` is the optimizer's small state on the device:
// S S^T, S Y^T ([i][j] = s_i . y_j) and Y Y^T, m x m each, in LOGICAL order (oldest pair first), then theta.  The kernel first adds
// the first-stage partials of the pass before it in a fixed order (the same bits run after run), then
//   PM_LBFGSB_SMALL_DIRECTION: N = -M + W^T W / theta from the maintained Gram, N z = W^T g, coef = the raw rows' weights in
//     (1 / theta^2) W z; record[0] = g . g.
//   PM_LBFGSB_SMALL_BREAK: record = [raw W^T d0 (2k) | d0 . d0, count t <= 0, count finite t > 0 | theta | M (2k x 2k, row-major)]:
//     what the host's sweep over the breakpoints needs, in one read.
//   PM_LBFGSB_SMALL_RESIDUAL: coef = -W-scaled M^-1 c, c = `c_in` (2k doubles).
//   PM_LBFGSB_SMALL_SUBSPACE: N from the masked Gram's partials (gparts > 0) or the maintained Gram, N z = W_F^T r, coef as above.
//   PM_LBFGSB_SMALL_UPDATE: the curvature test s . y > eps max(y . y, 1); an accepted pair becomes the newest row and column of the
//     three Gram matrices (a full history drops its oldest: the matrices move up and left by one) and theta = y . y / s . y rounded to
//     the data's type; record = [accepted, s . s, s . y, y . y, theta].
// The solves are Gaussian elimination with partial pivoting on the matrix in LDS, the row updates spread over the threads.
__global__ __launch_bounds__(kThreads) void small_kernel(Small a, double* __restrict__ st, const double* __restrict__ c_in, double* __restrict__ coef,
                                                          double* __restrict__ rec, const double* __restrict__ part, const double* __restrict__ gpart) {
    __shared__ double A[kN][kLd];
    __shared__ double f[kMaxTiles * kMaxSlots];
    __shared__ double z[kN];
    __shared__ int piv;
    const int tid = threadIdx.x, k = a.k, n2 = 2 * a.k, m = a.m, op = a.op;
    double* SS = st;
    double* SY = st + m * m;
    double* YY = st + 2 * m * m;
    const int NV = op == PM_LBFGSB_SMALL_UPDATE ? 2 : 1;
    const int NS = op == PM_LBFGSB_SMALL_RESIDUAL ? 0 : op == PM_LBFGSB_SMALL_BREAK ? kTile + 3 : op == PM_LBFGSB_SMALL_UPDATE ? 2 * kTile + 3 : kTile + 1;
    const int tiles = n2 > 0 ? (n2 + kTile - 1) / kTile : 1;
    // the partials: the workgroup's threads split into C chunks of Sp >= S lanes; lane s of chunk ch adds every C-th partial of sum s,
    // then lane s of chunk 0 adds the C chunk sums in order.  The split depends on the launch shape alone: the same bits run after run
    __shared__ double fc[kThreads];
    const int S = tiles * NS;
    int Sp = 1;
    while (Sp < S) Sp <<= 1;
    const int C = kThreads / Sp;
    {
        const int s = tid % Sp, ch = tid / Sp;
        double acc = 0.0;
        if (s < S) {
            const double* p = part + int64_t(s / NS) * a.nparts * NS + s % NS;
            for (int i = ch; i < a.nparts; i += C) acc = acc + p[int64_t(i) * NS];
        }
        fc[tid] = acc;
    }
    __syncthreads();
    if (tid < S) {
        double acc = fc[tid];
        for (int ch = 1; ch < C; ++ch) acc = acc + fc[ch * Sp + tid];
        f[tid] = acc;
    }
    __syncthreads();
    const double theta = st[3 * m * m];
    auto prod = [&](int q, int vi) { return f[(q / kTile) * NS + (q % kTile) * NV + vi]; };
    auto extra = [&](int e) { return f[kTile * NV + e]; };
    auto scale = [&](int q) { return q < k ? 1.0 : theta; };
    auto Mat = [&](int r, int c) -> double {      // M = [[-D, L^T], [L, theta S S^T]]
        if (r < k && c < k) return r == c ? -SY[r * m + r] : 0.0;
        if (r >= k && c < k) return r - k > c ? SY[(r - k) * m + c] : 0.0;
        if (r < k) return c - k > r ? SY[(c - k) * m + r] : 0.0;
        return theta * SS[(r - k) * m + (c - k)];
    };
    auto Gram = [&](int r, int c) -> double {     // the raw products of W's rows over all variables
        if (r < k && c < k) return YY[r * m + c];
        if (r < k) return SY[(c - k) * m + r];
        if (c < k) return SY[(r - k) * m + c];
        return SS[(r - k) * m + (c - k)];
    };

    if (op == PM_LBFGSB_SMALL_UPDATE) {
        const double ss = extra(0), sy = extra(1), yy = extra(2);
        const bool accept = !(sy <= a.eps * fmax(yy, 1.0));
        int kk = k, drop = 0;
        if (accept) {
            if (k == m) {      // every thread takes its elements into registers, then all store: in place
                constexpr int kPer = (kMaxMemory * kMaxMemory + kThreads - 1) / kThreads;
                double v[kPer][3];
                const int cnt = (m - 1) * (m - 1);
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int idx = tid + u * kThreads;
                    if (idx < cnt) {
                        const int src = (idx / (m - 1) + 1) * m + idx % (m - 1) + 1;
                        v[u][0] = SS[src], v[u][1] = SY[src], v[u][2] = YY[src];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < kPer; ++u) {
                    const int idx = tid + u * kThreads;
                    if (idx < cnt) {
                        const int dst = (idx / (m - 1)) * m + idx % (m - 1);
                        SS[dst] = v[u][0], SY[dst] = v[u][1], YY[dst] = v[u][2];
                    }
                }
                __syncthreads();
                kk = m - 1, drop = 1;
            }
            const int j = kk;
            if (tid < kk) {
                const int i = tid, q = tid + drop;
                const double Ys = prod(q, 0), Ss = prod(k + q, 0), Yy = prod(q, 1), Sy = prod(k + q, 1);
                SS[j * m + i] = Ss, SS[i * m + j] = Ss;
                SY[j * m + i] = Ys, SY[i * m + j] = Sy;
                YY[j * m + i] = Yy, YY[i * m + j] = Yy;
            }
            if (tid == 0) SS[j * m + j] = ss, SY[j * m + j] = sy, YY[j * m + j] = yy;
        }
        if (tid == 0) {
            double th = theta;
            if (accept) {
                th = yy / sy;
                if (a.f32) th = double(float(th));
                st[3 * m * m] = th;
            }
            rec[0] = accept ? 1.0 : 0.0, rec[1] = ss, rec[2] = sy, rec[3] = yy, rec[4] = th;
        }
        return;
    }
    if (op == PM_LBFGSB_SMALL_BREAK) {
        for (int q = tid; q < n2; q += kThreads) rec[q] = prod(q, 0);
        if (tid < 3) rec[n2 + tid] = extra(tid);
        if (tid == 3) rec[n2 + 3] = theta;
        for (int e = tid; e < n2 * n2; e += kThreads) rec[n2 + 4 + e] = Mat(e / n2, e % n2);
        return;
    }
    if (op == PM_LBFGSB_SMALL_DIRECTION && tid == 0) rec[0] = extra(0);
    if (n2 == 0) return;
    // the matrix and the right-hand side
    const int ntile = (n2 + kTile - 1) / kTile;
    for (int e = tid; e < n2 * n2; e += kThreads) {
        const int r = e / n2, c = e % n2;
        double v;
        if (op == PM_LBFGSB_SMALL_RESIDUAL) {
            v = Mat(r, c);
        } else {
            double g;
            if (op == PM_LBFGSB_SMALL_SUBSPACE && a.gparts > 0) {
                int ti = r / kTile, tj = c / kTile, rr = r % kTile, cc = c % kTile;
                if (ti > tj) { int t = ti; ti = tj; tj = t; t = rr; rr = cc; cc = t; }
                const int pair = ti * ntile - ti * (ti - 1) / 2 + (tj - ti);
                const double* p = gpart + int64_t(pair) * a.gparts * (kTile * kTile) + rr * kTile + cc;
                g = 0.0;
                for (int i = 0; i < a.gparts; ++i) g = g + p[int64_t(i) * (kTile * kTile)];
            } else {
                g = Gram(r, c);
            }
            v = ((scale(r) * g) * scale(c)) / theta - Mat(r, c);
        }
        A[r][c] = v;
    }
    for (int r = tid; r < n2; r += kThreads) A[r][kN] = op == PM_LBFGSB_SMALL_RESIDUAL ? c_in[r] : scale(r) * prod(r, 0);
    __syncthreads();
    for (int c = 0; c < n2; ++c) {
        if (tid == 0) {
            int best = c;
            double big = fabs(A[c][c]);
            for (int r = c + 1; r < n2; ++r)
                if (fabs(A[r][c]) > big) big = fabs(A[r][c]), best = r;
            piv = best;
        }
        __syncthreads();
        const int p = piv;
        if (p != c && tid <= n2) {
            const int j = tid < n2 ? tid : kN;
            const double t = A[c][j];
            A[c][j] = A[p][j], A[p][j] = t;
        }
        __syncthreads();
        const int w = n2 - c;      // the columns c + 1 .. n2 - 1 and the right-hand side
        const double d = A[c][c];
        for (int e = tid; e < (n2 - c - 1) * w; e += kThreads) {
            const int r = c + 1 + e / w, jj = e % w;
            const int j = jj == w - 1 ? kN : c + 1 + jj;
            A[r][j] = A[r][j] - (A[r][c] / d) * A[c][j];
        }
        __syncthreads();
    }
    if (tid == 0)
        for (int i = n2 - 1; i >= 0; --i) {
            double s = A[i][kN];
            for (int j = i + 1; j < n2; ++j) s = s - A[i][j] * z[j];
            z[i] = s / A[i][i];
        }
    __syncthreads();
    for (int q = tid; q < n2; q += kThreads)
        coef[q] = op == PM_LBFGSB_SMALL_RESIDUAL ? -(scale(q) * z[q]) : (scale(q) * z[q]) / (theta * theta);
}

int elem_blocks(int64_t n) { return int(std::min<int64_t>(kElemBlocks, (n + kThreads - 1) / kThreads)); }

// the checks every entry point with a history shares; 0 when they pass
int check_hist(const char* who, int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (k < 0) return fail(PM_ERR_ARG, "%s: k must not be negative, got %d", who, int(k));
    if (k > kMaxMemory) return fail(PM_ERR_UNSUPPORTED, "%s: %d history pairs are above PM_LBFGSB_MAX_MEMORY = %d", who, int(k), kMaxMemory);
    if (k > 0) {
        if (!S || !Y) return fail(PM_ERR_ARG, "%s: null pointer: the history", who);
        if (ring < k || start < 0 || start >= ring) return fail(PM_ERR_ARG, "%s: the ring of %d rows does not hold k = %d from row %d", who, int(ring), int(k), int(start));
        if (ld < n) return fail(PM_ERR_ARG, "%s: the row stride %lld is smaller than n = %lld", who, (long long)ld, (long long)n);
    }
    return 0;
}

// a NULL record leaves the first-stage partials in the workspace for pm_lbfgsb_small and launches no fold
int check_ws(const char* who, const void* record, const void* workspace, size_t bytes) {
    if (!workspace) return fail(PM_ERR_ARG, "%s: null pointer: the workspace", who);
    if (bytes < kWsDoubles * sizeof(double)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_lbfgsb_workspace()", who);
    if ((record && !aligned(record, 8)) || !aligned(workspace, 8)) return fail(PM_ERR_ARG, "%s: the record and the workspace must be aligned to 8 bytes", who);
    return 0;
}

template <typename T>
Hist<T> hist_of(const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k) {
    return Hist<T>{static_cast<const T*>(S), static_cast<const T*>(Y), ld, k > 0 ? int(ring) : 1, k > 0 ? int(start) : 0, int(k)};
}

// a dots pass and its fold: record[tile * NS + j]
template <typename T, typename Src>
int dots_run(int64_t n, const Hist<T>& h, const Src& src, double* record, double* ws, hipStream_t st) {
    constexpr int NS = kTile * Src::NV + Src::NX;
    const int wgs = reduce_groups(n, kThreads, kWgs);
    const int tiles = std::max(1, (2 * h.k + kTile - 1) / kTile);
    hipLaunchKernelGGL((dots_kernel<T, Src>), dim3(wgs, tiles), dim3(kThreads), 0, st, n, h, src, ws);
    if (record) hipLaunchKernelGGL(fold_kernel, dim3(tiles), dim3(kThreads), 0, st, wgs, NS, NS, ws, record);
    return int(hipGetLastError());
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

size_t pm_lbfgsb_workspace(void) { return kWsDoubles * sizeof(double); }

int pm_lbfgsb_dots(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* v,
                   const void* w, const void* mask, void* record, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_lbfgsb_dots";
    if (int rc = check_hist(who, dtype, n, S, Y, ld, ring, start, k)) return rc;
    if (!v) return fail(PM_ERR_ARG, "%s: null pointer: v", who);
    if (int rc = check_ws(who, record, workspace, workspace_bytes)) return rc;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return dots_run(n, hist_of<T>(S, Y, ld, ring, start, k),
                        SrcVec<T>{static_cast<const T*>(v), static_cast<const T*>(w), static_cast<const uint8_t*>(mask)},
                        static_cast<double*>(record), static_cast<double*>(workspace), PM_STREAM(stream));
    });
}

int pm_lbfgsb_breakpoints(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* x,
                          const void* g, const void* lower, const void* upper, void* t, void* d0, void* record, void* workspace,
                          size_t workspace_bytes, void* stream) {
    const char* who = "pm_lbfgsb_breakpoints";
    if (int rc = check_hist(who, dtype, n, S, Y, ld, ring, start, k)) return rc;
    if (!x || !g || !lower || !upper || !t || !d0) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_ws(who, record, workspace, workspace_bytes)) return rc;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return dots_run(n, hist_of<T>(S, Y, ld, ring, start, k),
                        SrcBreak<T>{static_cast<const T*>(x), static_cast<const T*>(g), static_cast<const T*>(lower), static_cast<const T*>(upper),
                                    static_cast<T*>(t), static_cast<T*>(d0)},
                        static_cast<double*>(record), static_cast<double*>(workspace), PM_STREAM(stream));
    });
}

int pm_lbfgsb_update(int32_t dtype, int64_t n, void* S, void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, int32_t slot, const void* xt,
                     const void* x, const void* p, double alpha, const void* g_new, const void* g, void* record, void* workspace,
                     size_t workspace_bytes, void* stream) {
    const char* who = "pm_lbfgsb_update";
    if (int rc = check_hist(who, dtype, n, S, Y, ld, ring, start, k)) return rc;
    if (!S || !Y) return fail(PM_ERR_ARG, "%s: null pointer: the history", who);
    if (ld < n) return fail(PM_ERR_ARG, "%s: the row stride %lld is smaller than n = %lld", who, (long long)ld, (long long)n);
    if (slot < 0 || slot >= ring) return fail(PM_ERR_ARG, "%s: the slot %d is outside the ring of %d rows", who, int(slot), int(ring));
    for (int j = 0; j < k; ++j)
        if ((start + j) % ring == slot) return fail(PM_ERR_ARG, "%s: the slot %d is a live row", who, int(slot));
    if (!g_new || !g || (!p && !(xt && x))) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_ws(who, record, workspace, workspace_bytes)) return rc;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        T* srow = static_cast<T*>(S) + int64_t(slot) * ld;
        T* yrow = static_cast<T*>(Y) + int64_t(slot) * ld;
        const int bounded = xt != nullptr && x != nullptr;
        return dots_run(n, hist_of<T>(S, Y, ld, ring, start, k),
                        SrcPair<T>{static_cast<const T*>(xt), static_cast<const T*>(x), static_cast<const T*>(p), T(alpha), bounded,
                                   static_cast<const T*>(g_new), static_cast<const T*>(g), srow, yrow},
                        static_cast<double*>(record), static_cast<double*>(workspace), PM_STREAM(stream));
    });
}

int pm_lbfgsb_gram(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* mask,
                   void* record, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_lbfgsb_gram";
    if (int rc = check_hist(who, dtype, n, S, Y, ld, ring, start, k)) return rc;
    if (k < 1) return fail(PM_ERR_ARG, "%s: k must be at least 1", who);
    if (int rc = check_ws(who, record, workspace, workspace_bytes)) return rc;
    const int wgs = reduce_groups(n, kThreads, kGramWgs);
    const int ntile = (2 * k + kTile - 1) / kTile, pairs = ntile * (ntile + 1) / 2;
    hipStream_t st = PM_STREAM(stream);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        double* ws = static_cast<double*>(workspace);
        hipLaunchKernelGGL(gram_kernel<T>, dim3(wgs, pairs), dim3(kThreads), 0, st, n, hist_of<T>(S, Y, ld, ring, start, k),
                           static_cast<const uint8_t*>(mask), ws);
        if (record) hipLaunchKernelGGL(fold_kernel, dim3(pairs), dim3(kThreads), 0, st, wgs, kTile * kTile, kTile * kTile, ws, static_cast<double*>(record));
        return int(hipGetLastError());
    });
}

int pm_lbfgsb_combine(int32_t dtype, int32_t mode, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k,
                      double a, const void* v, double b, const void* u1, const void* u2, const void* coef, const void* mask, const void* xc,
                      const void* x, const void* lower, const void* upper, const void* g, void* out, void* out2, void* record, void* workspace,
                      size_t workspace_bytes, void* stream) {
    const char* who = "pm_lbfgsb_combine";
    if (int rc = check_hist(who, dtype, n, S, Y, ld, ring, start, k)) return rc;
    if (mode < PM_LBFGSB_DIRECTION || mode > PM_LBFGSB_SUBSPACE) return fail(PM_ERR_ARG, "%s: mode must be one of PM_LBFGSB_*, got %d", who, int(mode));
    if (!v || !out || (k > 0 && !coef)) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if ((u1 == nullptr) != (u2 == nullptr)) return fail(PM_ERR_ARG, "%s: u1 and u2 come together", who);
    if (mode != PM_LBFGSB_RESIDUAL && !g) return fail(PM_ERR_ARG, "%s: null pointer: g", who);
    if (mode == PM_LBFGSB_SUBSPACE && (!xc || !x || !lower || !upper || !out2)) return fail(PM_ERR_ARG, "%s: null pointer: the subspace tail", who);
    if (coef && !aligned(coef, 8)) return fail(PM_ERR_ARG, "%s: coef must be aligned to 8 bytes", who);
    if (mode != PM_LBFGSB_RESIDUAL)
        if (int rc = check_ws(who, record, workspace, workspace_bytes)) return rc;
    const int wgs = reduce_groups(n, kThreads, kWgs);
    hipStream_t st = PM_STREAM(stream);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        double* ws = static_cast<double*>(workspace);
        hipLaunchKernelGGL(combine_kernel<T>, dim3(wgs), dim3(kThreads), 0, st, int(mode), n, hist_of<T>(S, Y, ld, ring, start, k), a,
                           static_cast<const T*>(v), b, static_cast<const T*>(u1), static_cast<const T*>(u2), static_cast<const double*>(coef),
                           static_cast<const uint8_t*>(mask), static_cast<const T*>(xc), static_cast<const T*>(x), static_cast<const T*>(lower),
                           static_cast<const T*>(upper), static_cast<const T*>(g), static_cast<T*>(out), static_cast<T*>(out2), ws);
        if (mode != PM_LBFGSB_RESIDUAL)
            hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(kThreads), 0, st, wgs, kCombineSlots, 4, ws, static_cast<double*>(record));
        return int(hipGetLastError());
    });
}

int pm_lbfgsb_cauchy_point(int32_t dtype, int64_t n, const void* x, const void* g, const void* t, double t_last, double t_stop, void* xc,
                           void* free_mask, void* stream) {
    const char* who = "pm_lbfgsb_cauchy_point";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (!x || !g || !t || !xc || !free_mask) return fail(PM_ERR_ARG, "%s: null pointer", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(cauchy_kernel<T>, dim3(elem_blocks(n)), dim3(kThreads), 0, PM_STREAM(stream), n, static_cast<const T*>(x),
                           static_cast<const T*>(g), static_cast<const T*>(t), T(t_last), T(t_stop), static_cast<T*>(xc),
                           static_cast<uint8_t*>(free_mask));
        return int(hipGetLastError());
    });
}

int pm_lbfgsb_trial(int32_t dtype, int64_t n, const void* x, const void* p, double alpha, const void* lower, const void* upper, void* xt,
                    void* stream) {
    const char* who = "pm_lbfgsb_trial";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (!x || !p || !xt) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if ((lower == nullptr) != (upper == nullptr)) return fail(PM_ERR_ARG, "%s: lower and upper bounds come together (infinite where there is none)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(trial_kernel<T>, dim3(elem_blocks(n)), dim3(kThreads), 0, PM_STREAM(stream), n, static_cast<const T*>(x),
                           static_cast<const T*>(p), T(alpha), static_cast<const T*>(lower), static_cast<const T*>(upper), static_cast<T*>(xt));
        return int(hipGetLastError());
    });
}

size_t pm_lbfgsb_state_doubles(int32_t memory) { return memory < 1 || memory > kMaxMemory ? 0 : size_t(3) * memory * memory + 8; }

int pm_lbfgsb_small(int32_t dtype, int32_t op, int32_t memory, int32_t k, int32_t nparts, int32_t gram_parts, void* state, const void* c_in,
                    void* coef, void* record, const void* partials, const void* gram_partials, void* stream) {
    const char* who = "pm_lbfgsb_small";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (op < PM_LBFGSB_SMALL_DIRECTION || op > PM_LBFGSB_SMALL_UPDATE) return fail(PM_ERR_ARG, "%s: op must be one of PM_LBFGSB_SMALL_*, got %d", who, int(op));
    if (memory > kMaxMemory) return fail(PM_ERR_UNSUPPORTED, "%s: a memory of %d is above PM_LBFGSB_MAX_MEMORY = %d", who, int(memory), kMaxMemory);
    if (memory < 1 || k < 0 || k > memory) return fail(PM_ERR_ARG, "%s: memory must be at least 1 and k in [0, memory], got %d, %d", who, int(memory), int(k));
    if (!state || !record) return fail(PM_ERR_ARG, "%s: null pointer: the state and the record", who);
    if (op != PM_LBFGSB_SMALL_RESIDUAL && (!partials || nparts < 1 || nparts > kWgs)) return fail(PM_ERR_ARG, "%s: the partials of the pass before it: null pointer or a count outside [1, %d]", who, kWgs);
    if (gram_parts < 0 || gram_parts > kGramWgs || (gram_parts > 0 && !gram_partials)) return fail(PM_ERR_ARG, "%s: the Gram pass's partials: null pointer or a count outside [0, %d]", who, kGramWgs);
    if (op == PM_LBFGSB_SMALL_RESIDUAL && k > 0 && !c_in) return fail(PM_ERR_ARG, "%s: null pointer: c", who);
    if (op != PM_LBFGSB_SMALL_BREAK && op != PM_LBFGSB_SMALL_UPDATE && k > 0 && !coef) return fail(PM_ERR_ARG, "%s: null pointer: coef", who);
    if (!aligned(state, 8) || !aligned(record, 8)) return fail(PM_ERR_ARG, "%s: the state and the record must be aligned to 8 bytes", who);
    const Small a{int(op), int(memory), int(k), int(nparts), int(gram_parts), dtype == PM_F32 ? 1 : 0, dtype == PM_F32 ? 1.1920928955078125e-07 : 2.220446049250313e-16};
    hipLaunchKernelGGL(small_kernel, dim3(1), dim3(kThreads), 0, PM_STREAM(stream), a, static_cast<double*>(state), static_cast<const double*>(c_in),
                       static_cast<double*>(coef), static_cast<double*>(record), static_cast<const double*>(partials),
                       static_cast<const double*>(gram_partials));
    return int(hipGetLastError());
}

}  // extern "C"
