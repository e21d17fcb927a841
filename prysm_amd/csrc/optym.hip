// Gradient-based optimisation (prysm/x/optym) (gfx950): costs, first-order optimizer steps, activations and the spatial gradient.
//
//  - pm_optym_cost: mean_square_error, bias_and_gain_invariant_error and negative_loglikelihood with their gradients.  A mask is a
//    per-element predicate (bytes), never a compaction: the selected count is one of the sums, so nothing is read on the host.
//      pass A: one read of M, D and the mask; every thread keeps the sums the cost needs in DOUBLE (the element arithmetic is double
//        too: the kernels are memory-bound), a workgroup of 256 folds them in LDS in a fixed order (pm_reduce.h wg_fold) and leaves
//        one partial per sum in the workspace.  At most kCostWgs workgroups, grid-stride.
//      fold: ONE workgroup adds the partials in a fixed order (pm_reduce.h fold_partials) and forms the scalars (1/N, alpha, beta, R)
//        in double on the device.
//      centred pass (bias and gain invariant only): the covariance and the variance are sums of CENTRED data, as the reference
//        writes them (Ihat = I - I.mean()).  Pass A keeps N, sum I, sum D and sum D^2, its fold leaves the two means on the device,
//        this pass reads M, D and the mask again for sum (I - Imean)(D - Dmean) and sum (I - Imean)^2, and its fold forms alpha and
//        beta.  The one-pass form sum(I D) - sum(I) Dmean loses (mean / spread)^2 eps of alpha to a pedestal, which is what the cost
//        is meant not to see (csrc/interferogram.hip and csrc/modalfit.hip take their variances in two passes for the same reason).
//      pass B: the gradient store (zero where the mask is false).  For the bias-and-gain-invariant cost it also carries the partials
//        of sum(raw_err^2) and a last fold forms R * that sum, so the cost is the reference's sum of squared residuals.
//    No float atomics, no tickets, no host read: the same launch shape adds the same numbers in the same order, run after run.
//  - pm_optym_advance / pm_optym_step: one step of GradientDescent, AdaGrad, RMSProp, Adam, RAdam, AdaMomentum or Yogi as one
//    one-thread kernel (the step counter, a device int64, and what depends on it: 1 - beta1^k, 1 - beta2^k, RAdam's rho, r and its
//    branch, in double) and ONE kernel over the variables: projected gradient, moments, step, clamp; x and the state in place, the
//    pre-step iterate to x_prev and, under bounds, g_step and the active-bound bytes.  Arithmetic in the data's type, expression by
//    expression as the reference writes it (scalars are formed in double and rounded once, as numpy rounds a Python float).
//  - pm_optym_activation: Tanh, Arctan, Softplus, Sigmoid, forward or backprop, one sweep.
//  - pm_optym_softmax / pm_optym_softmax_backprop: rows of K logits, K last.  A row is spread over the smallest power-of-two group
//    of lanes that holds K (at most 64) and reduced with cross-lane shuffles; longer rows loop.  Adjacent groups hold adjacent rows,
//    so a wavefront's loads are contiguous.  With `u` the Gumbel noise -log(-log(u + eps) + eps), the add and / tau are formed in the load
//    (once per element: rows longer than 64 stage their logits and exponentials in the output).  The backprop keeps its two row sums
//    (sum g y and sum y) and its bracket in double.
//  - pm_optym_spatial_gradient: forward_x / adjoint_x / forward_y / adjoint_y of SpatialGradient2D, the adjoints as gathers.
//
// prysm_amd/x/optym_plan.py is this file in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile) so that every product
// and sum is rounded by itself, as numpy does.
#include <algorithm>
#include <cmath>

#include "pm_entry.h"
#include "pm_reduce.h"
#include "pm_sweep.h"

namespace pm {
namespace {

constexpr int kCostThreads = 256;
constexpr int kCostWgs = 1024;       // most workgroups of a cost pass: as many partials per sum
constexpr int kCostSums = 4;         // most sums of pass A (bias and gain invariant: N, sum I, sum D, sum D^2)
constexpr int kCentredSums = 2;      // sums of the centred pass: sum (I - Imean)(D - Dmean), sum (I - Imean)^2
constexpr int kScalars = 8;          // doubles at the head of the workspace: 0 N, 1 1/N or R, 2 alpha, 3 beta, 4 Imean, 5 Dmean
constexpr int kFlatW = 256;          // a flat array is swept as rows of this many elements (pm_sweep.h)
constexpr int kSoftThreads = 256;

// workspace: [scalars | partials of pass A (kCostWgs x kCostSums) | of the centred pass (kCostWgs x kCentredSums) | of pass B (kCostWgs)]
constexpr size_t kWsDoubles = size_t(kScalars) + size_t(kCostWgs) * kCostSums + size_t(kCostWgs) * kCentredSums + size_t(kCostWgs);

__host__ __device__ constexpr int sums_of(int kind) { return kind == PM_COST_BGI ? kCostSums : 2; }

template <typename T, int KIND>
__global__ __launch_bounds__(kCostThreads) void cost_sums_kernel(int64_t n, const T* __restrict__ M, const T* __restrict__ D, double dscalar,
                                                                  const uint8_t* __restrict__ mask, double* __restrict__ partial) {
    constexpr int NS = sums_of(KIND);
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    const int64_t stride = int64_t(gridDim.x) * kCostThreads;
    for (int64_t i = int64_t(blockIdx.x) * kCostThreads + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        const double m = double(M[i]), d = D ? double(D[i]) : dscalar;
        a[0] = a[0] + 1.0;
        if constexpr (KIND == PM_COST_MSE) {
            const double diff = m - d;
            a[1] = a[1] + diff * diff;
        } else if constexpr (KIND == PM_COST_NLL) {
            a[1] = a[1] + (d * log(m) + (1.0 - d) * log(1.0 - m));
        } else {
            a[1] = a[1] + m;
            a[2] = a[2] + d;
            a[3] = a[3] + d * d;
        }
    }
    wg_fold<kCostThreads, FoldSum>(threadIdx.x, a, partial + int64_t(blockIdx.x) * NS);
}

template <typename T, int KIND>
__global__ __launch_bounds__(kCostThreads) void cost_fold_kernel(int nparts, const double* __restrict__ partial, double* __restrict__ sc,
                                                                  T* __restrict__ cost) {
    constexpr int NS = sums_of(KIND);
    double s[NS];
    fold_partials<kCostThreads, FoldSum>(threadIdx.x, nparts, partial, 0.0, s);
    if (threadIdx.x != 0) return;
    const double N = s[0];
    sc[0] = N;
    if constexpr (KIND == PM_COST_MSE) {
        const double inv = 1.0 / N;
        sc[1] = inv;
        *cost = T(s[1] * inv);
    } else if constexpr (KIND == PM_COST_NLL) {
        const double inv = 1.0 / N;
        sc[1] = inv;
        *cost = T(-inv * s[1]);
    } else {
        sc[1] = 1.0 / s[3];
        sc[4] = s[1] / N;
        sc[5] = s[2] / N;
    }
}

// the centred pass of the bias-and-gain-invariant cost: the means are pass A's, read from the device
template <typename T>
__global__ __launch_bounds__(kCostThreads) void cost_centred_kernel(int64_t n, const T* __restrict__ M, const T* __restrict__ D,
                                                                     const uint8_t* __restrict__ mask, const double* __restrict__ sc,
                                                                     double* __restrict__ partial) {
    const double Imean = sc[4], Dmean = sc[5];
    double a[kCentredSums] = {0.0, 0.0};
    const int64_t stride = int64_t(gridDim.x) * kCostThreads;
    for (int64_t i = int64_t(blockIdx.x) * kCostThreads + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) continue;
        const double ci = double(M[i]) - Imean, cd = double(D[i]) - Dmean;
        a[0] = a[0] + ci * cd;
        a[1] = a[1] + ci * ci;
    }
    wg_fold<kCostThreads, FoldSum>(threadIdx.x, a, partial + int64_t(blockIdx.x) * kCentredSums);
}

__global__ __launch_bounds__(kCostThreads) void cost_centred_fold_kernel(int nparts, const double* __restrict__ partial, double* __restrict__ sc) {
    double s[kCentredSums];
    fold_partials<kCostThreads, FoldSum>(threadIdx.x, nparts, partial, 0.0, s);
    if (threadIdx.x != 0) return;
    const double alpha = s[0] / s[1];
    sc[2] = alpha;
    sc[3] = sc[5] - alpha * sc[4];
}

template <typename T, int KIND>
__global__ __launch_bounds__(kCostThreads) void cost_grad_kernel(int64_t n, const T* __restrict__ M, const T* __restrict__ D, double dscalar,
                                                                  const uint8_t* __restrict__ mask, const double* __restrict__ sc,
                                                                  T* __restrict__ grad, double* __restrict__ partial) {
    const double c1 = sc[1], alpha = sc[2], beta = sc[3];
    double a[1] = {0.0};
    const int64_t stride = int64_t(gridDim.x) * kCostThreads;
    for (int64_t i = int64_t(blockIdx.x) * kCostThreads + threadIdx.x; i < n; i += stride) {
        if (mask && !mask[i]) {
            grad[i] = T(0);
            continue;
        }
        const double m = double(M[i]), d = D ? double(D[i]) : dscalar;
        if constexpr (KIND == PM_COST_MSE) {
            grad[i] = T(2.0 * c1 * (m - d));
        } else if constexpr (KIND == PM_COST_NLL) {
            grad[i] = T(((-d / m) + ((1.0 - d) / (1.0 - m))) * c1);
        } else {
            const double raw = (alpha * m + beta) - d;
            a[0] = a[0] + raw * raw;
            grad[i] = T(2.0 * c1 * alpha * raw);
        }
    }
    if constexpr (KIND == PM_COST_BGI) wg_fold<kCostThreads, FoldSum>(threadIdx.x, a, partial + blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(kCostThreads) void cost_fold2_kernel(int nparts, const double* __restrict__ partial, const double* __restrict__ sc,
                                                                   T* __restrict__ cost) {
    double s[1];
    fold_partials<kCostThreads, FoldSum>(threadIdx.x, nparts, partial, 0.0, s);
    if (threadIdx.x == 0) *cost = T(sc[1] * s[0]);
}

template <typename T, int KIND>
int cost_run(int64_t n, const void* M, const void* D, double dscalar, const void* mask, void* cost, void* grad, double* ws, hipStream_t st) {
    const int wgs = reduce_groups(n, kCostThreads, kCostWgs);
    double* sc = ws;
    double* pa = ws + kScalars;
    double* pc = pa + size_t(kCostWgs) * kCostSums;
    double* pb = pc + size_t(kCostWgs) * kCentredSums;
    const T* m = static_cast<const T*>(M);
    const T* d = static_cast<const T*>(D);
    const uint8_t* mk = static_cast<const uint8_t*>(mask);
    hipLaunchKernelGGL((cost_sums_kernel<T, KIND>), dim3(wgs), dim3(kCostThreads), 0, st, n, m, d, dscalar, mk, pa);
    hipLaunchKernelGGL((cost_fold_kernel<T, KIND>), dim3(1), dim3(kCostThreads), 0, st, wgs, pa, sc, static_cast<T*>(cost));
    if (KIND == PM_COST_BGI) {
        hipLaunchKernelGGL(cost_centred_kernel<T>, dim3(wgs), dim3(kCostThreads), 0, st, n, m, d, mk, sc, pc);
        hipLaunchKernelGGL(cost_centred_fold_kernel, dim3(1), dim3(kCostThreads), 0, st, wgs, pc, sc);
    }
    hipLaunchKernelGGL((cost_grad_kernel<T, KIND>), dim3(wgs), dim3(kCostThreads), 0, st, n, m, d, dscalar, mk, sc, static_cast<T*>(grad), pb);
    if (KIND == PM_COST_BGI) hipLaunchKernelGGL(cost_fold2_kernel<T>, dim3(1), dim3(kCostThreads), 0, st, wgs, pb, sc, static_cast<T*>(cost));
    return int(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------- optimizers

// coefficients of a step, eight doubles: 0 1 - beta1^k, 1 1 - beta2^k, 2 rho, 3 r, 4 RAdam's branch (1: rho >= 5), 5 sqrt(1 - beta2^k)

__global__ void advance_kernel(int kind, double beta1, double beta2, int64_t* __restrict__ counter, double* __restrict__ coef) {
    const int64_t k = *counter + 1;
    *counter = k;
    const double b1k = pow(beta1, double(k)), b2k = pow(beta2, double(k));
    coef[0] = 1.0 - b1k;
    coef[1] = 1.0 - b2k;
    double rho = 0.0, r = 0.0, flag = 0.0;
    if (kind == PM_OPT_RADAM) {
        const double rhoinf = 2.0 / (1.0 - beta2) - 1.0;
        rho = rhoinf - (2.0 * double(k) * b2k) / (1.0 - b2k);
        if (rho >= 5.0) {
            const double num = (rho - 4.0) * (rho - 2.0) * rhoinf;
            const double den = (rhoinf - 4.0) * (rhoinf - 2.0) * rho;
            r = sqrt(num / den);
            flag = 1.0;
        }
    }
    coef[2] = rho;
    coef[3] = r;
    coef[4] = flag;
    coef[5] = sqrt(1.0 - b2k);
    coef[6] = 0.0;
    coef[7] = 0.0;
}

template <typename T>
__device__ __forceinline__ T sign_of(T v) { return v > T(0) ? T(1) : v < T(0) ? T(-1) : v; }      // numpy's sign: 0 stays 0, NaN stays NaN

template <typename T>
struct Step {
    int kind;
    int64_t n;
    T* x; const T* g; T* s1; T* s2; const T* lo; const T* hi;
    T alpha, beta1, omb1, beta2, omb2, eps;
    double alpha_d;
    const double* coef;
    T* x_prev; T* g_step; uint8_t* active;
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t r, int64_t c, NoColumn) const {
        const int64_t i = r * kFlatW + c;
        if (i >= n) return;
        const T xi = x[i];
        T gs = g[i];
        const bool bounded = lo != nullptr;
        T l = T(0), u = T(0);
        if (bounded) {
            l = lo[i], u = hi[i];
            const bool at_lower = isfinite(l) && xi <= l && gs > T(0);
            const bool at_upper = isfinite(u) && xi >= u && gs < T(0);
            if (at_lower || at_upper) gs = T(0);
        }
        T xn;
        switch (kind) {
        case PM_OPT_GD:
            xn = xi - alpha * gs;
            break;
        case PM_OPT_ADAGRAD: {
            const T acc = s1[i] + gs * gs;
            s1[i] = acc;
            xn = xi - alpha * gs / (sqrt(acc) + eps);
            break;
        }
        case PM_OPT_RMSPROP: {
            const T acc = beta1 * s1[i] + omb1 * (gs * gs);
            s1[i] = acc;
            xn = xi - alpha * gs / (sqrt(acc) + eps);
            break;
        }
        case PM_OPT_ADAM: {
            const T m = beta1 * s1[i] + omb1 * gs;
            const T v = beta2 * s2[i] + omb2 * (gs * gs);
            s1[i] = m, s2[i] = v;
            const T mhat = m / T(coef[0]), vhat = v / T(coef[1]);
            xn = xi - alpha * mhat / (sqrt(vhat) + eps);
            break;
        }
        case PM_OPT_RADAM: {
            const T m = beta1 * s1[i] + omb1 * gs;
            const T v = beta2 * s2[i] + omb2 * (gs * gs);
            s1[i] = m, s2[i] = v;
            if (coef[4] != 0.0) {
                const T mhat = m / T(coef[0]);
                const T lk = T(coef[5]) / (sqrt(v) + eps);
                xn = xi - T(alpha_d * coef[3]) * mhat * lk;
            } else {
                xn = xi - alpha * gs;
            }
            break;
        }
        case PM_OPT_ADAMOMENTUM: {
            const T m = beta1 * s1[i] + omb1 * gs;
            const T v = beta2 * s2[i] + omb2 * (m * m) + eps;
            s1[i] = m, s2[i] = v;
            const T mhat = m / T(coef[0]), vhat = v / T(coef[1]);
            xn = xi - alpha * mhat / sqrt(vhat);
            break;
        }
        default: {      // PM_OPT_YOGI
            const T gsq = gs * gs;
            const T m = beta1 * s1[i] + omb1 * gs;
            const T v0 = s2[i];
            const T v = v0 - omb2 * sign_of(v0 - gsq) * gsq;
            s1[i] = m, s2[i] = v;
            const T vhat = sqrt(v + eps);
            xn = xi - alpha * m / (sqrt(vhat) + eps);
            break;
        }
        }
        if (bounded) {
            if (xn == xn) xn = fmin(fmax(xn, l), u);      // numpy's maximum / minimum hand a NaN through
            g_step[i] = gs;
            active[i] = uint8_t((isfinite(l) && xn <= l) || (isfinite(u) && xn >= u));
        }
        x_prev[i] = xi;
        x[i] = xn;
    }
};

// a flat array of n elements as rows of kFlatW for the row sweep
template <typename F>
int flat_sweep(int64_t n, hipStream_t st, const F& f) { return sweep((n + kFlatW - 1) / kFlatW, int64_t(kFlatW), st, f); }

// ---------------------------------------------------------------------------------------------------------------- activations

template <typename T>
struct Activation {
    int kind, back;
    int64_t n;
    const T* x; T a, m2a, ma, x0, y0; T* out;
    __device__ T forward(T xs) const {
        switch (kind) {
        case PM_ACT_TANH: return T(2) / (T(1) + exp(m2a * xs)) - T(1) + y0;
        case PM_ACT_ARCTAN: return atan(a * xs) + y0;
        case PM_ACT_SOFTPLUS: return log(T(1) + exp(a * xs)) + y0;
        default: return (T(1) / (T(1) + exp(ma * xs))) + y0;
        }
    }
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t r, int64_t c, NoColumn) const {
        const int64_t i = r * kFlatW + c;
        if (i >= n) return;
        const T xs = x[i] - x0;
        if (!back) {
            out[i] = forward(xs);
            return;
        }
        T v;
        switch (kind) {
        case PM_ACT_TANH: {
            const T fx = forward(xs) - y0;
            v = a * (T(1) - fx * fx);
            break;
        }
        case PM_ACT_ARCTAN: {
            const T u = a * xs;
            v = a / (u * u + T(1));
            break;
        }
        case PM_ACT_SOFTPLUS:
            v = a / (T(1) + exp(ma * xs));
            break;
        default: {
            const T sig = forward(xs) - y0;
            v = a * sig * (T(1) - sig);
            break;
        }
        }
        out[i] = v;
    }
};

// ---------------------------------------------------------------------------------------------------------------- softmax

template <typename T>
__device__ __forceinline__ T group_max(T v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ T group_sum(T v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T logit(const T* __restrict__ x, const T* __restrict__ u, int64_t i, T tau, T eps) {
    T v = x[i];
    if (u) v = (v + (-log(-log(u[i] + eps) + eps))) / tau;
    return v;
}

// G lanes per row (a power of two, 1 .. 64), 256 / G rows per workgroup; lanes of rows past the end stay in the shuffles and skip memory
template <typename T>
__global__ __launch_bounds__(kSoftThreads) void softmax_kernel(int64_t rows, int64_t K, int G, const T* __restrict__ x, const T* __restrict__ u,
                                                                T tau, T eps, T* __restrict__ out) {
    const int64_t t = int64_t(blockIdx.x) * kSoftThreads + threadIdx.x;
    const int64_t row = t / G;
    const int j = int(t % G);
    const bool live = row < rows;
    const int64_t base = row * K;
    if (K <= G) {
        const bool has = live && j < K;
        const T v = has ? logit(x, u, base + j, tau, eps) : T(-INFINITY);
        const T mx = group_max(v, G);
        const T e = has ? exp(v - mx) : T(0);
        const T s = group_sum(e, G);
        if (has) out[base + j] = e / s;
        return;
    }
    // longer rows loop, staged through `out`: a lane reads back only what it stored itself, so the logits (two logs each under
    // Gumbel noise) and the exponentials are formed once
    T mx = T(-INFINITY);
    if (live)
        for (int64_t k = j; k < K; k += G) {
            const T v = logit(x, u, base + k, tau, eps);
            out[base + k] = v;
            mx = fmax(mx, v);
        }
    mx = group_max(mx, G);
    T s = T(0);
    if (live)
        for (int64_t k = j; k < K; k += G) {
            const T e = exp(out[base + k] - mx);
            out[base + k] = e;
            s = s + e;
        }
    s = group_sum(s, G);
    if (live)
        for (int64_t k = j; k < K; k += G) out[base + k] = out[base + k] / s;
}

// gin_k = y_k (g_k S - sum_j g_j y_j) / tau with S = sum_j y_j, the sums and the bracket in DOUBLE, one rounding at the store.  S is 1
// up to the rounding of the stored y; written as the reference's y_k (g_k - sum_j g_j y_j) the bracket of a saturated row (y_k -> 1)
// cancels down to that rounding, g_k S - sum_j g_j y_j = sum_j y_j (g_k - g_j) does not
template <typename T>
__global__ __launch_bounds__(kSoftThreads) void softmax_back_kernel(int64_t rows, int64_t K, int G, const T* __restrict__ y, const T* __restrict__ grad,
                                                                     double tau, T* __restrict__ gin) {
    const int64_t t = int64_t(blockIdx.x) * kSoftThreads + threadIdx.x;
    const int64_t row = t / G;
    const int j = int(t % G);
    const bool live = row < rows;
    const int64_t base = row * K;
    double dot = 0.0, sum = 0.0;
    if (live)
        for (int64_t k = j; k < K; k += G) {
            const double yk = double(y[base + k]);
            dot = dot + double(grad[base + k]) * yk;
            sum = sum + yk;
        }
    dot = group_sum(dot, G);
    sum = group_sum(sum, G);
    if (live)
        for (int64_t k = j; k < K; k += G) gin[base + k] = T(double(y[base + k]) * (double(grad[base + k]) * sum - dot) / tau);
}

int group_of(int64_t K) {
    int G = 1;
    while (G < K && G < 64) G <<= 1;
    return G;
}

// ---------------------------------------------------------------------------------------------------------------- spatial gradient

// m x n, contiguous.  compute = [1, end - 2], lookahead = compute + 1 along the axis of the operator
template <typename T, int OP>
struct SpatialGradient {
    int64_t m, n; const T* in; T* out;
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t r, int64_t c, NoColumn) const {
        constexpr bool alongx = OP == PM_GRAD_FORWARD_X || OP == PM_GRAD_ADJOINT_X;
        const int64_t p = alongx ? c : r, end = alongx ? n : m, step = alongx ? 1 : n;
        const int64_t i = r * n + c;
        const bool compute = p >= 1 && p <= end - 2;
        T v = T(0);
        if constexpr (OP == PM_GRAD_FORWARD_X || OP == PM_GRAD_FORWARD_Y) {
            if (compute) v = in[i + step] - in[i];
        } else {
            if (compute) v = v - in[i];
            if (p >= 2 && p <= end - 1) v = v + in[i - step];
        }
        out[i] = v;
    }
};

bool cost_kind(int32_t k) { return k == PM_COST_MSE || k == PM_COST_BGI || k == PM_COST_NLL; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

size_t pm_optym_cost_workspace(void) { return kWsDoubles * sizeof(double); }

int pm_optym_cost(int32_t dtype, int32_t kind, int64_t n, const void* M, const void* D, double d_scalar, const void* mask, void* cost, void* grad,
                  void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_optym_cost";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!cost_kind(kind)) return fail(PM_ERR_ARG, "%s: kind must be PM_COST_MSE, PM_COST_BGI or PM_COST_NLL, got %d", who, int(kind));
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (!M || !cost || !grad || !workspace) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (!D && kind != PM_COST_NLL) return fail(PM_ERR_ARG, "%s: null pointer: only PM_COST_NLL takes a scalar D", who);
    if (workspace_bytes < pm_optym_cost_workspace()) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_optym_cost_workspace()", who);
    if (!aligned(workspace, sizeof(double))) return fail(PM_ERR_ARG, "%s: the workspace must be aligned to 8 bytes", who);
    hipStream_t st = PM_STREAM(stream);
    double* ws = static_cast<double*>(workspace);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        switch (kind) {
        case PM_COST_MSE: return cost_run<T, PM_COST_MSE>(n, M, D, d_scalar, mask, cost, grad, ws, st);
        case PM_COST_BGI: return cost_run<T, PM_COST_BGI>(n, M, D, d_scalar, mask, cost, grad, ws, st);
        default: return cost_run<T, PM_COST_NLL>(n, M, D, d_scalar, mask, cost, grad, ws, st);
        }
    });
}

int pm_optym_advance(int32_t kind, double beta1, double beta2, void* counter, void* coef, void* stream) {
    const char* who = "pm_optym_advance";
    if (kind < PM_OPT_GD || kind > PM_OPT_YOGI) return fail(PM_ERR_ARG, "%s: kind must be one of PM_OPT_*, got %d", who, int(kind));
    if (!counter || !coef) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (!aligned(counter, 8) || !aligned(coef, 8)) return fail(PM_ERR_ARG, "%s: counter and coef must be aligned to 8 bytes", who);
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, PM_STREAM(stream), int(kind), beta1, beta2, static_cast<int64_t*>(counter),
                       static_cast<double*>(coef));
    return int(hipGetLastError());
}

int pm_optym_step(int32_t dtype, int32_t kind, int64_t n, void* x, const void* g, void* s1, void* s2, const void* lower, const void* upper,
                  double alpha, double beta1, double beta2, double eps, const void* coef, void* x_prev, void* g_step, void* active, void* stream) {
    const char* who = "pm_optym_step";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (kind < PM_OPT_GD || kind > PM_OPT_YOGI) return fail(PM_ERR_ARG, "%s: kind must be one of PM_OPT_*, got %d", who, int(kind));
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (!x || !g || !x_prev) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (kind != PM_OPT_GD && !s1) return fail(PM_ERR_ARG, "%s: null pointer: the optimizer's state", who);
    if (kind >= PM_OPT_ADAM && (!s2 || !coef)) return fail(PM_ERR_ARG, "%s: null pointer: the second moment and the coefficients", who);
    if ((lower == nullptr) != (upper == nullptr)) return fail(PM_ERR_ARG, "%s: lower and upper bounds come together (infinite where there is none)", who);
    if (lower && (!g_step || !active)) return fail(PM_ERR_ARG, "%s: null pointer: bounds need g_step and active", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        Step<T> s;
        s.kind = kind, s.n = n;
        s.x = static_cast<T*>(x), s.g = static_cast<const T*>(g), s.s1 = static_cast<T*>(s1), s.s2 = static_cast<T*>(s2);
        s.lo = static_cast<const T*>(lower), s.hi = static_cast<const T*>(upper);
        s.alpha = T(alpha), s.beta1 = T(beta1), s.omb1 = T(1.0 - beta1), s.beta2 = T(beta2), s.omb2 = T(1.0 - beta2), s.eps = T(eps);
        s.alpha_d = alpha;
        s.coef = static_cast<const double*>(coef);
        s.x_prev = static_cast<T*>(x_prev), s.g_step = static_cast<T*>(g_step), s.active = static_cast<uint8_t*>(active);
        return flat_sweep(n, PM_STREAM(stream), s);
    });
}

int pm_optym_activation(int32_t dtype, int32_t kind, int32_t backprop, int64_t n, const void* x, double a, double x0, double y0, void* out,
                        void* stream) {
    const char* who = "pm_optym_activation";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (kind < PM_ACT_TANH || kind > PM_ACT_SIGMOID) return fail(PM_ERR_ARG, "%s: kind must be one of PM_ACT_*, got %d", who, int(kind));
    if (n < 1) return fail(PM_ERR_ARG, "%s: n must be at least 1, got %lld", who, (long long)n);
    if (!x || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return flat_sweep(n, PM_STREAM(stream),
                          Activation<T>{kind, backprop != 0, n, static_cast<const T*>(x), T(a), T(-2.0 * a), T(-a), T(x0), T(y0), static_cast<T*>(out)});
    });
}

static int check_rows(const char* who, int64_t rows, int64_t K) {
    if (rows < 1 || K < 1) return fail(PM_ERR_ARG, "%s: rows and K must be at least 1, got %lld, %lld", who, (long long)rows, (long long)K);
    if (K > INT32_MAX || rows > (int64_t(1) << 40)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)K);
    const int64_t per = kSoftThreads / group_of(K);
    if ((rows + per - 1) / per > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld rows are too many", who, (long long)rows);
    return 0;
}

int pm_optym_softmax(int32_t dtype, int64_t rows, int64_t K, const void* x, const void* u, double tau, double eps, void* out, void* stream) {
    const char* who = "pm_optym_softmax";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (int rc = check_rows(who, rows, K)) return rc;
    if (!x || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (u && !(tau > 0.0)) return fail(PM_ERR_ARG, "%s: tau must be positive", who);
    const int G = group_of(K);
    const int64_t per = kSoftThreads / G;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(softmax_kernel<T>, dim3(unsigned((rows + per - 1) / per)), dim3(kSoftThreads), 0, PM_STREAM(stream), rows, K, G,
                           static_cast<const T*>(x), static_cast<const T*>(u), T(tau), T(eps), static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

int pm_optym_softmax_backprop(int32_t dtype, int64_t rows, int64_t K, const void* y, const void* grad, double tau, void* gin, void* stream) {
    const char* who = "pm_optym_softmax_backprop";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (int rc = check_rows(who, rows, K)) return rc;
    if (!y || !grad || !gin) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (!(tau > 0.0)) return fail(PM_ERR_ARG, "%s: tau must be positive", who);
    const int G = group_of(K);
    const int64_t per = kSoftThreads / G;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(softmax_back_kernel<T>, dim3(unsigned((rows + per - 1) / per)), dim3(kSoftThreads), 0, PM_STREAM(stream), rows, K, G,
                           static_cast<const T*>(y), static_cast<const T*>(grad), tau, static_cast<T*>(gin));
        return int(hipGetLastError());
    });
}

int pm_optym_spatial_gradient(int32_t dtype, int32_t op, int64_t m, int64_t n, const void* in, void* out, void* stream) {
    const char* who = "pm_optym_spatial_gradient";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (op < PM_GRAD_FORWARD_X || op > PM_GRAD_ADJOINT_Y) return fail(PM_ERR_ARG, "%s: op must be one of PM_GRAD_*, got %d", who, int(op));
    if (m < 1 || n < 1) return fail(PM_ERR_ARG, "%s: m and n must be at least 1, got %lld, %lld", who, (long long)m, (long long)n);
    if (n > INT32_MAX) return fail(PM_ERR_ARG, "%s: rows of %lld values are too long", who, (long long)n);
    if (!in || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (in == out) return fail(PM_ERR_ARG, "%s: in and out must differ (every output reads a neighbour)", who);
    hipStream_t st = PM_STREAM(stream);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const T* i = static_cast<const T*>(in);
        T* o = static_cast<T*>(out);
        switch (op) {
        case PM_GRAD_FORWARD_X: return sweep(m, n, st, SpatialGradient<T, PM_GRAD_FORWARD_X>{m, n, i, o});
        case PM_GRAD_ADJOINT_X: return sweep(m, n, st, SpatialGradient<T, PM_GRAD_ADJOINT_X>{m, n, i, o});
        case PM_GRAD_FORWARD_Y: return sweep(m, n, st, SpatialGradient<T, PM_GRAD_FORWARD_Y>{m, n, i, o});
        default: return sweep(m, n, st, SpatialGradient<T, PM_GRAD_ADJOINT_Y>{m, n, i, o});
        }
    });
}

}  // extern "C"
