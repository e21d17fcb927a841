// Thin-film multilayers (prysm/thinfilm.py, prysm/x/coatings/stack.py and diff.py) (gfx950): the characteristic-matrix calculation of a
// coating's r, t, R, T, boundary fields and per-layer absorptance, and the gradient of an R / T merit with respect to every thickness.
//
// One thread per sample (a wavelength, an angle, a pixel of an angle-of-incidence map).  A sample's operands -- wavelength, ambient
// angle, ambient and substrate index, and per layer an index and a thickness -- each come with a sample stride of 0 (shared by all
// samples: the address is the same in every lane) or 1; the layer tables also have a layer stride.
//
//  - pm_tf_stack: v = [1, eta_sub]; for j = L - 1 .. 0: v <- M_j v, with cos(theta_j) by Snell's law (the sign flipped where a real
//    sin(theta) exceeds 1, thinfilm.py:75-80), beta_j = 2 pi n_j d_j cos(theta_j) / lambda and eta = n cos(theta) for s, n / cos(theta)
//    for p.  [B, C] = v at boundary 0 gives r = (eta0 B - C) / (eta0 B + C), t = 2 eta0 / (eta0 B + C).  Nothing is kept per layer in
//    registers: with fields or absorptance wanted the sweep stores the UNNORMALISED boundary vectors (and flux differences) into the
//    outputs themselves, [boundary][sample] so that a wavefront's stores are contiguous, and a second loop of the same kernel scales
//    what the thread stored by t (by |t|^2 / Re eta0) once t is known.  With both polarisations one sweep carries two vectors and
//    shares cos(theta_j), sin(beta_j), cos(beta_j).
//  - pm_tf_thickness_grad: grad[j] = sum_k dF/dd_j from seeds dR[k], dT[k].  The assembly cotangent is the outer product
//    [Bbar, Cbar]^T [1, conj eta_sub], so the cotangent of M_j is a_j b_{j+1}^H: b_{j+1} the unnormalised boundary vector of the sweep
//    above (kept in the workspace, [boundary][sample]) and a_0 = [Bbar, Cbar]^T, a_{j+1} = M_j^H a_j a scan from the ambient side.  No
//    matrix is stored or inverted.  A thread's contribution to layer j is summed over its wavefront in DOUBLE with cross-lane shuffles
//    (a fixed butterfly), one partial per wavefront and layer goes to the workspace, and a second launch adds the partials of a layer
//    in a fixed order (pm_reduce.h fold_partials): no atomics, the same bits run after run.
//
// prysm_amd/thinfilm_plan.py is this file in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile) so that every product
// and sum is rounded by itself, as numpy does; sincos, sqrt, hypot and expm1 are the accurate library functions.
#include <cmath>

#include "pm_entry.h"
#include "pm_reduce.h"

namespace pm {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;

template <typename T>
struct Cx {
    T re, im;
};

__device__ __forceinline__ void sin_cos(float x, float& s, float& c) { sincosf(x, &s, &c); }
__device__ __forceinline__ void sin_cos(double x, double& s, double& c) { sincos(x, &s, &c); }

template <typename T> __device__ __forceinline__ Cx<T> operator+(Cx<T> a, Cx<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> __device__ __forceinline__ Cx<T> operator-(Cx<T> a, Cx<T> b) { return {a.re - b.re, a.im - b.im}; }
template <typename T> __device__ __forceinline__ Cx<T> operator-(Cx<T> a) { return {-a.re, -a.im}; }
template <typename T> __device__ __forceinline__ Cx<T> operator*(Cx<T> a, Cx<T> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename T> __device__ __forceinline__ Cx<T> operator*(Cx<T> a, T s) { return {a.re * s, a.im * s}; }
template <typename T> __device__ __forceinline__ Cx<T> operator/(Cx<T> a, T s) { return {a.re / s, a.im / s}; }
template <typename T> __device__ __forceinline__ Cx<T> conj(Cx<T> a) { return {a.re, -a.im}; }
template <typename T> __device__ __forceinline__ Cx<T> minus_i(Cx<T> a) { return {a.im, -a.re}; }      // -i a
template <typename T> __device__ __forceinline__ T abs2(Cx<T> a) { return a.re * a.re + a.im * a.im; }
// a / b by Smith's algorithm (what numpy does)
template <typename T>
__device__ __forceinline__ Cx<T> operator/(Cx<T> a, Cx<T> b) {
    if (fabs(b.re) >= fabs(b.im)) {
        const T rat = b.im / b.re, scl = T(1) / (b.re + b.im * rat);
        return {(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const T rat = b.re / b.im, scl = T(1) / (b.re * rat + b.im);
    return {(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}
// the principal square root; an imaginary part of zero of EITHER sign counts as +0 (a negative real gives +i sqrt(-x))
template <typename T>
__device__ __forceinline__ Cx<T> csqrt(Cx<T> w) {
    const T x = w.re, y = w.im;
    if (y == T(0)) {
        if (x >= T(0)) return {sqrt(x), T(0)};
        return {T(0), sqrt(-x)};
    }
    const T m = hypot(x, y);
    if (x >= T(0)) {
        const T re = sqrt((m + x) / T(2));
        return {re, y / (T(2) * re)};
    }
    const T im = sqrt((m - x) / T(2));
    return {fabs(y) / (T(2) * im), y < T(0) ? -im : im};
}
// sin and cos of a complex argument: sin(a + ib) = sin a cosh b + i cos a sinh b, cos(a + ib) = cos a cosh b - i sin a sinh b, the
// hyperbolic pair from expm1 so that a weakly absorbing layer (small b) keeps its sinh
template <typename T>
__device__ __forceinline__ void csincos(Cx<T> z, Cx<T>& s, Cx<T>& c) {
    T sa, ca;
    sin_cos(z.re, sa, ca);
    const T em = expm1(z.im), e = em + T(1);
    const T sh = T(0.5) * (em + em / e), ch = T(0.5) * (e + T(1) / e);
    s = {sa * ch, ca * sh};
    c = {ca * ch, -(sa * sh)};
}

template <typename T>
struct Operands {
    const T* wvl; int64_t wvl_ss;
    const T* theta; int64_t theta_ss;
    const Cx<T>* n; int64_t n_ls, n_ss;
    const T* d; int64_t d_ls, d_ss;
    const Cx<T>* nsub; int64_t nsub_ss;
    const Cx<T>* n0; int64_t n0_ss;
};

template <typename T>
struct Sample {
    T wvl, sin0, cos0;
    Cx<T> n0, nsub;
};

// a stride of 0 is read at an address without the thread's index: the same in every lane
template <typename T>
__device__ __forceinline__ Sample<T> load_sample(const Operands<T>& op, int64_t k) {
    Sample<T> s;
    s.wvl = op.wvl_ss ? op.wvl[k] : op.wvl[0];
    const T th = op.theta_ss ? op.theta[k] : op.theta[0];
    sin_cos(th, s.sin0, s.cos0);
    s.n0 = op.n0_ss ? op.n0[k] : op.n0[0];
    s.nsub = op.nsub_ss ? op.nsub[k] : op.nsub[0];
    return s;
}

// cos(theta_1) from n0 sin(theta_0) = n1 sin(theta_1), thinfilm.py:75-80
template <typename T>
__device__ __forceinline__ Cx<T> cos_snell(Cx<T> n0, Cx<T> n1, T sin0) {
    const Cx<T> sint = (n0 / n1) * sin0;
    const Cx<T> one = {T(1), T(0)};
    Cx<T> cost = csqrt(one - sint * sint);
    if (sint.im == T(0) && sint.re > T(1)) cost = -cost;
    return cost;
}

template <typename T>
struct Layer {
    Cx<T> n, cost, sinb, cosb, dbdd;      // dbdd = d beta / d thickness = 2 pi n cos(theta) / lambda
};

template <typename T>
__device__ __forceinline__ Layer<T> load_layer(const Operands<T>& op, const Sample<T>& s, int64_t j, int64_t k) {
    Layer<T> ly;
    ly.n = op.n_ss ? op.n[j * op.n_ls + k] : op.n[j * op.n_ls];
    const T d = op.d_ss ? op.d[j * op.d_ls + k] : op.d[j * op.d_ls];
    ly.cost = cos_snell(s.n0, ly.n, s.sin0);
    const Cx<T> tpn = ly.n * T(6.283185307179586476925286766559);
    const Cx<T> beta = ((tpn * d) * ly.cost) / s.wvl;
    ly.dbdd = (tpn * ly.cost) / s.wvl;
    csincos(beta, ly.sinb, ly.cosb);
    return ly;
}

template <int POLS>
__device__ __forceinline__ constexpr bool is_p(int q) { return POLS == PM_TF_P || (POLS == PM_TF_BOTH && q == 1); }

// the tilted admittance of a medium
template <typename T>
__device__ __forceinline__ Cx<T> admittance(Cx<T> n, Cx<T> cost, bool p) { return p ? n / cost : n * cost; }

template <typename T, int POLS>
__global__ __launch_bounds__(kThreads) void stack_kernel(Operands<T> op, int64_t K, int64_t L, int tconv, Cx<T>* __restrict__ r, Cx<T>* __restrict__ t,
                                                          T* __restrict__ R, T* __restrict__ Tr, Cx<T>* __restrict__ E, Cx<T>* __restrict__ H,
                                                          T* __restrict__ A) {
    constexpr int NP = POLS == PM_TF_BOTH ? 2 : 1;
    const int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (k >= K) return;
    const Sample<T> s = load_sample(op, k);
    const Cx<T> cost_sub = cos_snell(s.n0, s.nsub, s.sin0);
    Cx<T> eta0[NP], etas[NP], B[NP], C[NP];
    T flux[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const bool p = is_p<POLS>(q);
        eta0[q] = p ? s.n0 / s.cos0 : s.n0 * s.cos0;
        etas[q] = admittance(s.nsub, cost_sub, p);
        B[q] = {T(1), T(0)};
        C[q] = etas[q];
        flux[q] = B[q].re * C[q].re + B[q].im * C[q].im;      // Re(B conj C)
        if (E) E[(q * (L + 1) + L) * K + k] = B[q];
        if (H) H[(q * (L + 1) + L) * K + k] = C[q];
    }
    for (int64_t j = L - 1; j >= 0; --j) {
        const Layer<T> ly = load_layer(op, s, j, k);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const Cx<T> eta = admittance(ly.n, ly.cost, is_p<POLS>(q));
            const Cx<T> m01 = minus_i(ly.sinb) / eta, m10 = minus_i(eta * ly.sinb);
            const Cx<T> nb = ly.cosb * B[q] + m01 * C[q];
            const Cx<T> nc = m10 * B[q] + ly.cosb * C[q];
            B[q] = nb, C[q] = nc;
            if (E) E[(q * (L + 1) + j) * K + k] = nb;
            if (H) H[(q * (L + 1) + j) * K + k] = nc;
            if (A) {
                const T f = nb.re * nc.re + nb.im * nc.im;
                A[(q * L + j) * K + k] = f - flux[q];
                flux[q] = f;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const bool p = is_p<POLS>(q);
        const Cx<T> den = eta0[q] * B[q] + C[q];
        const Cx<T> rr = (eta0[q] * B[q] - C[q]) / den;
        const Cx<T> tt = (eta0[q] * T(2)) / den;
        r[q * K + k] = rr;
        if (tconv == PM_TF_T_THINFILM && p) {
            const Cx<T> c0 = {s.cos0, T(0)};
            t[q * K + k] = tt * (c0 / cost_sub);
        } else {
            t[q * K + k] = tt;
        }
        const T t2 = abs2(tt);
        if (R) R[q * K + k] = abs2(rr);
        if (Tr) Tr[q * K + k] = etas[q].re / eta0[q].re * t2;
        // what this thread stored above, now that t is known
        if (E)
            for (int64_t b = 0; b <= L; ++b) E[(q * (L + 1) + b) * K + k] = tt * E[(q * (L + 1) + b) * K + k];
        if (H)
            for (int64_t b = 0; b <= L; ++b) H[(q * (L + 1) + b) * K + k] = tt * H[(q * (L + 1) + b) * K + k];
        if (A) {
            const T scale = t2 / eta0[q].re;
            for (int64_t j = 0; j < L; ++j) A[(q * L + j) * K + k] = A[(q * L + j) * K + k] * scale;
        }
    }
}

// workspace of the gradient: [partials: L x nparts doubles | bB: NP x L x K complex | bC: the same]
__host__ __device__ inline int64_t parts_of(int64_t K) { return (K + kWave - 1) / kWave; }

template <typename T, int POLS>
__global__ __launch_bounds__(kThreads) void grad_kernel(Operands<T> op, int64_t K, int64_t L, const T* __restrict__ dR, const T* __restrict__ dT,
                                                         int64_t seed_ps, Cx<T>* __restrict__ bB, Cx<T>* __restrict__ bC, double* __restrict__ partial) {
    constexpr int NP = POLS == PM_TF_BOTH ? 2 : 1;
    const int64_t kk = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if ((kk & ~int64_t(kWave - 1)) >= K) return;      // a wavefront with no sample (the same answer in all its lanes)
    const bool live = kk < K;
    const int64_t k = live ? kk : K - 1;               // the tail's idle lanes walk the last sample, store nothing and add zero
    const int64_t nparts = parts_of(K), part = kk / kWave;
    const Sample<T> s = load_sample(op, k);
    const Cx<T> cost_sub = cos_snell(s.n0, s.nsub, s.sin0);
    Cx<T> eta0[NP], B[NP], C[NP], a0[NP], a1[NP];
    T fac[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const bool p = is_p<POLS>(q);
        eta0[q] = p ? s.n0 / s.cos0 : s.n0 * s.cos0;
        const Cx<T> etas = admittance(s.nsub, cost_sub, p);
        fac[q] = etas.re / eta0[q].re;
        B[q] = {T(1), T(0)};
        C[q] = etas;
    }
    // from the substrate: b_{j+1} to slot j, then v <- M_j v
    for (int64_t j = L - 1; j >= 0; --j) {
        const Layer<T> ly = load_layer(op, s, j, k);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (live) {
                bB[(q * L + j) * K + k] = B[q];
                bC[(q * L + j) * K + k] = C[q];
            }
            const Cx<T> eta = admittance(ly.n, ly.cost, is_p<POLS>(q));
            const Cx<T> m01 = minus_i(ly.sinb) / eta, m10 = minus_i(eta * ly.sinb);
            const Cx<T> nb = ly.cosb * B[q] + m01 * C[q];
            const Cx<T> nc = m10 * B[q] + ly.cosb * C[q];
            B[q] = nb, C[q] = nc;
        }
    }
    // the seeds through r, t to [Bbar, Cbar] (diff.py:162-201)
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const Cx<T> den = eta0[q] * B[q] + C[q];
        const Cx<T> rr = (eta0[q] * B[q] - C[q]) / den;
        const Cx<T> tt = (eta0[q] * T(2)) / den;
        const Cx<T> one = {T(1), T(0)}, zero = {T(0), T(0)};
        const Cx<T> rbar = dR ? rr * (T(2) * dR[q * seed_ps + k]) : zero;
        const Cx<T> tbar = dT ? tt * (T(2) * fac[q] * dT[q * seed_ps + k]) : zero;
        const Cx<T> dr_dB = (eta0[q] * (one - rr)) / den, dr_dC = -((one + rr) / den);
        const Cx<T> dt_dB = -((tt * eta0[q]) / den), dt_dC = -(tt / den);
        a0[q] = conj(dr_dB) * rbar + conj(dt_dB) * tbar;
        a1[q] = conj(dr_dC) * rbar + conj(dt_dC) * tbar;
    }
    // from the ambient: the cotangent of M_j is a_j b_{j+1}^H; a_{j+1} = M_j^H a_j
    for (int64_t j = 0; j < L; ++j) {
        const Layer<T> ly = load_layer(op, s, j, k);
        T g = T(0);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            // the idle lanes of a tail read the slot of the last sample, which its own lane wrote
            const Cx<T> b0 = conj(live ? bB[(q * L + j) * K + k] : Cx<T>{T(1), T(0)});
            const Cx<T> b1 = conj(live ? bC[(q * L + j) * K + k] : Cx<T>{T(1), T(0)});
            const Cx<T> eta = admittance(ly.n, ly.cost, is_p<POLS>(q));
            const Cx<T> d00 = -ly.sinb, d01 = minus_i(ly.cosb) / eta, d10 = minus_i(eta * ly.cosb);
            const Cx<T> cb = conj(d00) * (a0[q] * b0) + conj(d01) * (a0[q] * b1) + conj(d10) * (a1[q] * b0) + conj(d00) * (a1[q] * b1);
            g = g + (cb.re * ly.dbdd.re + cb.im * ly.dbdd.im);      // Re(conj(c_beta) d beta / d d)
            const Cx<T> m01 = minus_i(ly.sinb) / eta, m10 = minus_i(eta * ly.sinb);
            const Cx<T> na0 = conj(ly.cosb) * a0[q] + conj(m10) * a1[q];
            const Cx<T> na1 = conj(m01) * a0[q] + conj(ly.cosb) * a1[q];
            a0[q] = na0, a1[q] = na1;
        }
        double gd = live ? double(g) : 0.0;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) gd = gd + __shfl_xor(gd, o, kWave);
        if ((threadIdx.x & (kWave - 1)) == 0) partial[j * nparts + part] = gd;
    }
}

// one workgroup per layer: its partials in a fixed order
template <typename T>
__global__ __launch_bounds__(kThreads) void grad_fold_kernel(int64_t nparts, const double* __restrict__ partial, int accumulate, T* __restrict__ grad) {
    double sum[1];
    fold_partials<kThreads, FoldSum>(threadIdx.x, nparts, partial + int64_t(blockIdx.x) * nparts, 0.0, sum);
    if (threadIdx.x == 0) grad[blockIdx.x] = accumulate ? grad[blockIdx.x] + T(sum[0]) : T(sum[0]);
}

bool pol_ok(int32_t pol) { return pol == PM_TF_S || pol == PM_TF_P || pol == PM_TF_BOTH; }
bool stride01(int64_t s) { return s == 0 || s == 1; }

// the checks both entry points share; 0 when the operands are well formed
int check_operands(const char* who, int32_t dtype, int32_t pol, int64_t K, int64_t L, const void* wvl, int64_t wvl_ss, const void* theta, int64_t theta_ss,
                   const void* n, int64_t n_ls, int64_t n_ss, const void* d, int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss,
                   const void* n0, int64_t n0_ss) {
    if (dtype != PM_C64 && dtype != PM_C128) return fail(PM_ERR_ARG, "%s: dtype must be PM_C64 or PM_C128", who);
    if (!pol_ok(pol)) return fail(PM_ERR_ARG, "%s: pol must be PM_TF_S, PM_TF_P or PM_TF_BOTH, got %d", who, int(pol));
    if (K < 0 || L < 0) return fail(PM_ERR_ARG, "%s: K and L must not be negative, got %lld, %lld", who, (long long)K, (long long)L);
    if (K > (int64_t(1) << 36) || L > (int64_t(1) << 20)) return fail(PM_ERR_ARG, "%s: %lld samples of %lld layers are too many", who, (long long)K, (long long)L);
    if (!stride01(wvl_ss) || !stride01(theta_ss) || !stride01(n_ss) || !stride01(d_ss) || !stride01(nsub_ss) || !stride01(n0_ss))
        return fail(PM_ERR_ARG, "%s: a sample stride must be 0 (shared) or 1 (per sample)", who);
    if (K == 0) return 0;
    if (!wvl || !theta || !nsub || !n0) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (L > 0) {
        if (!n || !d) return fail(PM_ERR_ARG, "%s: null pointer: the layer tables", who);
        if (n_ls < 0 || d_ls < 0 || (L > 1 && n_ss && n_ls < K) || (L > 1 && d_ss && d_ls < K))
            return fail(PM_ERR_ARG, "%s: a layer stride is smaller than the number of samples", who);
    }
    return 0;
}

template <typename T>
Operands<T> operands(const void* wvl, int64_t wvl_ss, const void* theta, int64_t theta_ss, const void* n, int64_t n_ls, int64_t n_ss, const void* d,
                     int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss, const void* n0, int64_t n0_ss) {
    return {static_cast<const T*>(wvl), wvl_ss, static_cast<const T*>(theta), theta_ss, static_cast<const Cx<T>*>(n), n_ls, n_ss,
            static_cast<const T*>(d), d_ls, d_ss, static_cast<const Cx<T>*>(nsub), nsub_ss, static_cast<const Cx<T>*>(n0), n0_ss};
}

size_t align16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_tf_stack(int32_t dtype, int32_t pol, int32_t t_convention, int64_t K, int64_t L, const void* wvl, int64_t wvl_ss, const void* theta,
                int64_t theta_ss, const void* n, int64_t n_ls, int64_t n_ss, const void* d, int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss,
                const void* n0, int64_t n0_ss, void* r, void* t, void* R, void* T_, void* E, void* H, void* A, void* stream) {
    const char* who = "pm_tf_stack";
    if (int rc = check_operands(who, dtype, pol, K, L, wvl, wvl_ss, theta, theta_ss, n, n_ls, n_ss, d, d_ls, d_ss, nsub, nsub_ss, n0, n0_ss)) return rc;
    if (t_convention != PM_TF_T_STACK && t_convention != PM_TF_T_THINFILM)
        return fail(PM_ERR_ARG, "%s: t_convention must be PM_TF_T_STACK or PM_TF_T_THINFILM, got %d", who, int(t_convention));
    if (K == 0) return 0;
    if (!r || !t) return fail(PM_ERR_ARG, "%s: null pointer: r and t", who);
    if ((E == nullptr) != (H == nullptr)) return fail(PM_ERR_ARG, "%s: E and H come together", who);
    hipStream_t st = PM_STREAM(stream);
    const dim3 grid(unsigned((K + kThreads - 1) / kThreads)), block(kThreads);
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const Operands<T> op = operands<T>(wvl, wvl_ss, theta, theta_ss, n, n_ls, n_ss, d, d_ls, d_ss, nsub, nsub_ss, n0, n0_ss);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, op, K, L, int(t_convention), static_cast<Cx<T>*>(r), static_cast<Cx<T>*>(t), static_cast<T*>(R),
                               static_cast<T*>(T_), static_cast<Cx<T>*>(E), static_cast<Cx<T>*>(H), static_cast<T*>(A));
            return int(hipGetLastError());
        };
        switch (pol) {
        case PM_TF_S: return go(stack_kernel<T, PM_TF_S>);
        case PM_TF_P: return go(stack_kernel<T, PM_TF_P>);
        default: return go(stack_kernel<T, PM_TF_BOTH>);
        }
    });
}

size_t pm_tf_thickness_grad_workspace(int32_t dtype, int32_t pol, int64_t K, int64_t L) {
    if ((dtype != PM_C64 && dtype != PM_C128) || !pol_ok(pol) || K < 1 || L < 1) return 0;
    const size_t np = pol == PM_TF_BOTH ? 2 : 1, cx = dtype == PM_C64 ? 8 : 16;
    return align16(size_t(L) * size_t(parts_of(K)) * sizeof(double)) + 2 * np * size_t(L) * size_t(K) * cx;
}

int pm_tf_thickness_grad(int32_t dtype, int32_t pol, int64_t K, int64_t L, const void* wvl, int64_t wvl_ss, const void* theta, int64_t theta_ss,
                         const void* n, int64_t n_ls, int64_t n_ss, const void* d, int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss,
                         const void* n0, int64_t n0_ss, const void* dR, const void* dT, int64_t seed_pstride, int32_t accumulate, void* grad,
                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_tf_thickness_grad";
    if (int rc = check_operands(who, dtype, pol, K, L, wvl, wvl_ss, theta, theta_ss, n, n_ls, n_ss, d, d_ls, d_ss, nsub, nsub_ss, n0, n0_ss)) return rc;
    if (seed_pstride != 0 && seed_pstride < K) return fail(PM_ERR_ARG, "%s: seed_pstride must be 0 (one seed for both polarisations) or at least K", who);
    if (K == 0 || L == 0) return 0;
    if (!grad || !workspace) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (workspace_bytes < pm_tf_thickness_grad_workspace(dtype, pol, K, L))
        return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_tf_thickness_grad_workspace()", who);
    if (!aligned(workspace, 16)) return fail(PM_ERR_ARG, "%s: the workspace must be aligned to 16 bytes", who);
    hipStream_t st = PM_STREAM(stream);
    const int64_t nparts = parts_of(K);
    const dim3 grid(unsigned((K + kThreads - 1) / kThreads)), block(kThreads);
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const Operands<T> op = operands<T>(wvl, wvl_ss, theta, theta_ss, n, n_ls, n_ss, d, d_ls, d_ss, nsub, nsub_ss, n0, n0_ss);
        const int64_t np = pol == PM_TF_BOTH ? 2 : 1;
        double* partial = static_cast<double*>(workspace);
        Cx<T>* bB = reinterpret_cast<Cx<T>*>(static_cast<char*>(workspace) + align16(size_t(L) * size_t(nparts) * sizeof(double)));
        Cx<T>* bC = bB + np * L * K;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, op, K, L, static_cast<const T*>(dR), static_cast<const T*>(dT), seed_pstride, bB, bC, partial);
        };
        switch (pol) {
        case PM_TF_S: go(grad_kernel<T, PM_TF_S>); break;
        case PM_TF_P: go(grad_kernel<T, PM_TF_P>); break;
        default: go(grad_kernel<T, PM_TF_BOTH>); break;
        }
        hipLaunchKernelGGL(grad_fold_kernel<T>, dim3(unsigned(L)), block, 0, st, nparts, partial, int(accumulate != 0), static_cast<T*>(grad));
        return int(hipGetLastError());
    });
}

}  // extern "C"
