// Step-index fibre LP modes without a stored basis (prysm/x/fibers.py) (gfx950):
//
//  - pm_fiber_modes: every mode of compute_LP_modes, (nmodes, npts), one launch.
//  - pm_fiber_sum: sum_k c[b][k] mode_k for B coefficient vectors, the modes evaluated once per point per group of up to 8 vectors.
//  - pm_fiber_project: sum_p g[b][p] mode_k[p] (what multimode_coupling reads its stored modes for), same walk; g = NULL gives
//    sum_p mode_k[p]^2.
//  - pm_overlap: sum E1 conj(E2), sum |E1|^2, sum |E2|^2 and eta of mode_overlap_integral in one pass, left on the device.
//
// Every point walks one table of records built on the host (prysm_amd/x/fibers_plan.py mode_table), one per radial function (|l|, m),
// sorted by |l|: U, W, the two normalisers 1 / J_l(U) and 1 / (e^W K_l(W)) -- evaluated on the host at the U, W the record holds -- and the
// output slots of the cosine (+l) and sine (-l) mode.  The radial value is J_l(U rn) / J_l(U) in the core (r <= a) and
// e^x K_l(x) / (e^W K_l(W)) exp(-W (rn - 1)), x = W rn, in the cladding; cos(l t), sin(l t) advance by one rotation per order.
//
// The Bessel functions are the unit's own (the coefficients: fibers_coefs.h, from tools/gen_fibers_coefs.py):
//   J0, J1: a Chebyshev series in x^2 for x <= 8, modulus and phase series in (8/x)^2 above;
//   J_l, l >= 2: forward recurrence from J0, J1 where x > l; the leading term (x/2)^l / l! where x^2 <= 4 eps (l + 1); else Miller's
//     backward recurrence from order 2 ((l + sqrt(160 l)) / 2), rescaled above 1e10, normalised by J0 + 2 sum J_2k = 1 -- the trip
//     count depends on l alone, which is the same in every lane;
//   e^x K0, e^x K1: series in x^2 with the logarithm split off for x <= 1, a series in 2/x - 1 above; upward recurrence for l >= 2.
// The unit is compiled with -ffp-contract=off: prysm_amd/x/fibers_plan.py restates the walk in numpy, operation by operation.
//
// The projection's reduction and its launcher are modal_tile.h's, shared with zernike.hip, qpoly.hip, recur.hip and segmented.hip;
// pm_overlap reduces the same way (a partial per workgroup, a fixed-order second launch, no atomics).
#include <cmath>

#include "fibers_coefs.h"
#include "modal_tile.h"
#include "pm_math.h"

namespace pm {
namespace {

enum { FR_STRICT = 1 };          // core is r (1/a) < 1 (smf_mode_field), not r <= a (compute_LP_modes)
constexpr int kMaxL = 255;       // orders above are clamped: the table is the caller's, the trip counts are not

// one record of the table (fibers_plan.record_dtype)
template <typename T>
struct FRec {
    T U, W, invJ, invK;
    int32_t l, slot_cos, slot_sin, flags;
};
static_assert(sizeof(FRec<float>) == 32 && sizeof(FRec<double>) == 48, "FRec layout is shared with fibers_plan.record_dtype");

template <typename T>
__device__ __forceinline__ T eps_() {
    return sizeof(T) == 4 ? T(1.1920928955078125e-07) : T(2.220446049250313e-16);
}

// sum_k c_k T_k(t) by Clenshaw, the first N32 terms in float
#define PM_FIBER_SERIES(NAME)                                                                                          \
    template <typename T>                                                                                              \
    __device__ __forceinline__ T cheb_##NAME(T t) {                                                                    \
        constexpr int n = sizeof(T) == 4 ? fibers_coefs::NAME##_N32 : fibers_coefs::NAME##_N64;                        \
        const T t2 = t + t;                                                                                            \
        T b1 = T(0), b2 = T(0);                                                                                        \
        _Pragma("unroll") for (int k = n - 1; k > 0; --k) {                                                            \
            const T b = t2 * b1 - b2 + T(fibers_coefs::NAME[k]);                                                       \
            b2 = b1;                                                                                                   \
            b1 = b;                                                                                                    \
        }                                                                                                              \
        return t * b1 - b2 + T(fibers_coefs::NAME[0]);                                                                 \
    }
PM_FIBER_SERIES(J0S)
PM_FIBER_SERIES(J1S)
PM_FIBER_SERIES(P0)
PM_FIBER_SERIES(Q0)
PM_FIBER_SERIES(P1)
PM_FIBER_SERIES(Q1)
PM_FIBER_SERIES(I0S)
PM_FIBER_SERIES(I1S)
PM_FIBER_SERIES(K0S)
PM_FIBER_SERIES(K1S)
PM_FIBER_SERIES(K0L)
PM_FIBER_SERIES(K1L)
#undef PM_FIBER_SERIES

// J0(x), J1(x), x >= 0
template <typename T>
__device__ __forceinline__ void j01(T x, T* j0, T* j1) {
    if (x <= T(8)) {
        const T t = x * x * T(0.03125) - T(1);
        *j0 = T(1) - x * x * T(0.25) * cheb_J0S(t);
        *j1 = x * cheb_J1S(t);
    } else {
        const T z = T(8) / x;
        const T t = T(2) * (z * z) - T(1);
        T s, c;
        sincos_(x, &s, &c);
        const T amp = sqrt_(T(0.6366197723675814) / x);
        const T c0 = (c + s) * T(0.7071067811865476), s0 = (s - c) * T(0.7071067811865476);      // cos, sin of x - pi/4
        *j0 = amp * (cheb_P0(t) * c0 - z * cheb_Q0(t) * s0);
        *j1 = amp * (cheb_P1(t) * s0 + z * cheb_Q1(t) * c0);        // cos(x - 3 pi/4) = s0, sin(x - 3 pi/4) = -c0
    }
}

// J_l(x), l >= 0, x >= 0
template <typename T>
__device__ __forceinline__ T bessel_j(int l, T x) {
    if (l <= 1 || x > T(l)) {
        T a, b;
        j01(x, &a, &b);
        if (l == 0) return a;
        const T tox = T(2) / x;
        for (int n = 1; n < l; ++n) {
            const T nb = T(n) * tox * b - a;
            a = b;
            b = nb;
        }
        return b;
    }
    if (x * x <= T(4) * eps_<T>() * T(l + 1)) {
        const T h = x * T(0.5);
        T v = T(1);
        for (int k = 1; k <= l; ++k) v = v * (h / T(k));
        return v;
    }
    const int N = 2 * ((l + int(sqrtf(float(160 * l)))) / 2);
    const T tox = T(2) / x;
    T fp = T(0), f = T(1), sum = T(0), ans = T(0);
    for (int n = N; n > 0; --n) {
        const T fm = T(n) * tox * f - fp;
        fp = f;
        f = fm;
        if (abs_(f) > T(1e10)) {
            f *= T(1e-10);
            fp *= T(1e-10);
            ans *= T(1e-10);
            sum *= T(1e-10);
        }
        if (n & 1) sum += f;
        if (n - 1 == l) ans = f;
    }
    return ans / (T(2) * sum - f);
}

// e^x K0(x), e^x K1(x), x > 0
template <typename T>
__device__ __forceinline__ void k01e(T x, T* k0, T* k1) {
    if (x <= T(1)) {
        const T t = T(2) * (x * x) - T(1);
        const T lg = log_(x * T(0.5)), ex = exp_(x);
        *k0 = (cheb_K0S(t) - lg * cheb_I0S(t)) * ex;
        *k1 = (lg * (x * cheb_I1S(t)) + cheb_K1S(t) / x) * ex;
    } else {
        const T t = T(2) / x - T(1);
        const T rs = T(1) / sqrt_(x);
        *k0 = cheb_K0L(t) * rs;
        *k1 = cheb_K1L(t) * rs;
    }
}

// e^x K_l(x), l >= 0, x > 0
template <typename T>
__device__ __forceinline__ T bessel_ke(int l, T x) {
    T a, b;
    k01e(x, &a, &b);
    if (l == 0) return a;
    const T tox = T(2) / x;
    for (int n = 1; n < l; ++n) {
        const T nb = a + T(n) * tox * b;
        a = b;
        b = nb;
    }
    return b;
}

// the radial value of a record at radius r
template <typename T>
__device__ __forceinline__ T radial(T U, T W, T invJ, T invK, bool strict, int l, T a, T inva, T r) {
    const T rn = strict ? r * inva : r / a;
    const bool core = strict ? rn < T(1) : r <= a;
    if (core) return bessel_j(l, U * rn) * invJ;
    return bessel_ke(l, W * rn) * invK * exp_(-(W * (rn - T(1))));
}

// The walk of the record table over kVec points: per record emit(0, slot, values) for its cosine (or l = 0) mode, emit(1, slot, values)
// for its sine mode, then flush() -- a record costs hundreds of operations per point, so the projection has nothing to gain from
// batching more reductions than these two.  E = 1 (a projection of 8 vectors has one place per group): emit(0, ...) and flush() per
// mode.  The records are visited one at a time and so are the points of a lane within a record -- one copy of the Bessel code per
// kernel; the lane's radii rotate through R[0] and the values come back in their places, so nothing is indexed at run time.
template <int E, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void walk(T a, const T r[kVec], const T t[kVec], const FRec<T>* __restrict__ table, int nrec, int nmodes,
                                     Emit&& emit, Flush&& flush) {
    T c1[kVec], s1[kVec], cl[kVec], sl[kVec];
#pragma unroll
    for (int q = 0; q < kVec; ++q) {
        sincos_(t[q], &s1[q], &c1[q]);
        cl[q] = T(1);
        sl[q] = T(0);
    }
    const T inva = T(1) / a;
    int cur = 0;
#pragma unroll 1
    for (int i = 0; i < nrec; ++i) {
        const T U = table[i].U, W = table[i].W, invJ = table[i].invJ, invK = table[i].invK;
        const int slot_cos = table[i].slot_cos, slot_sin = table[i].slot_sin;
        const bool strict = table[i].flags & FR_STRICT;
        const int l = min(max(table[i].l, 0), kMaxL);
        for (; cur < l; ++cur) {
#pragma unroll
            for (int q = 0; q < kVec; ++q) {
                const T c = cl[q] * c1[q] - sl[q] * s1[q];
                sl[q] = sl[q] * c1[q] + cl[q] * s1[q];
                cl[q] = c;
            }
        }
        T R[kVec];
#pragma unroll
        for (int q = 0; q < kVec; ++q) R[q] = r[q];
#pragma unroll 1
        for (int q = 0; q < kVec; ++q) {
            const T v = radial(U, W, invJ, invK, strict, l, a, inva, R[0]);
#pragma unroll
            for (int e = 0; e + 1 < kVec; ++e) R[e] = R[e + 1];
            R[kVec - 1] = v;
        }
        const bool has_cos = unsigned(slot_cos) < unsigned(nmodes), has_sin = l && unsigned(slot_sin) < unsigned(nmodes);
        if (has_cos) {
            T z[kVec];
#pragma unroll
            for (int q = 0; q < kVec; ++q) z[q] = l ? R[q] * cl[q] : R[q];
            emit(0, slot_cos, z);
            if (E == 1) flush();
        }
        if (has_sin) {
            T z[kVec];
#pragma unroll
            for (int q = 0; q < kVec; ++q) z[q] = R[q] * sl[q];
            emit(E == 1 ? 0 : 1, slot_sin, z);
            if (E == 1) flush();
        }
        if (E > 1 && (has_cos || has_sin)) flush();
    }
}

// ---------------------------------------------------------------- modes: nmodes planes, one launch
template <typename T>
__global__ __launch_bounds__(kThreads) void fiber_modes_kernel(int64_t npts, T a, const T* __restrict__ r, const T* __restrict__ t,
                                                               const FRec<T>* __restrict__ table, int nrec, int nmodes, T* __restrict__ out,
                                                               int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T rr[kVec], tt[kVec];
    load_pts(r, base, lane, npts, full, rr);
    load_pts(t, base, lane, npts, full, tt);
    walk<1>(a, rr, tt, table, nrec, nmodes,
            [&](int, int k, const T z[kVec]) { store_pts<true>(out + int64_t(k) * npts, base, lane, npts, full, z); }, [] {});
}

// ---------------------------------------------------------------- sum: NB coefficient vectors per walk
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void fiber_sum_kernel(int64_t npts, T a, const T* __restrict__ r, const T* __restrict__ t,
                                                             const FRec<T>* __restrict__ table, int nrec, int nmodes,
                                                             const T* __restrict__ coefs, int accumulate, T* __restrict__ out, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T rr[kVec], tt[kVec], acc[NB][kVec];
    load_pts(r, base, lane, npts, full, rr);
    load_pts(t, base, lane, npts, full, tt);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < kVec; ++q) acc[b][q] = T(0);
    walk<1>(a, rr, tt, table, nrec, nmodes,
            [&](int, int k, const T z[kVec]) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const T c = coefs[int64_t(b) * nmodes + k];
#pragma unroll
                    for (int q = 0; q < kVec; ++q) acc[b][q] += c * z[q];
                }
            },
            [] {});
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        T* dst = out + int64_t(b) * npts;
        if (accumulate) {
            T old[kVec];
            load_pts(dst, base, lane, npts, full, old);
#pragma unroll
            for (int q = 0; q < kVec; ++q) acc[b][q] += old[q];
        }
        store_pts<false>(dst, base, lane, npts, full, acc[b]);
    }
}

// ---------------------------------------------------------------- projection: one partial per (workgroup, b, k)
// The reduction of modal_tile.h around walk(): partial[group][b0 + b][k], row length ld = B * nmodes.  g = NULL (NB = 1): the mode
// against itself, sum_p mode_k[p]^2.
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void fiber_project_kernel(int64_t npts, T a, const T* __restrict__ r, const T* __restrict__ t,
                                                                 const FRec<T>* __restrict__ table, int nrec, int nmodes,
                                                                 const T* __restrict__ g, T* __restrict__ partial, int64_t ld, int vec) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nacc = NB * nmodes;
    const bool self = g == nullptr;
    T* sacc = project_begin<T>(smem, nacc, tid);
    T* wacc = sacc + wave * nacc;
    for (int64_t base = wave_tile(wave); base < npts; base += int64_t(gridDim.x) * kThreads * kVec) {
        const bool full = vec && base + 64 * kVec <= npts;
        T rr[kVec], tt[kVec], gg[NB][kVec];
        ProjectStep<T, NB> step;
        load_pts(r, base, lane, npts, full, rr);
        load_pts(t, base, lane, npts, full, tt);
        if (self) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int q = 0; q < kVec; ++q) gg[b][q] = Runs<T>::at(base, lane, q) < npts ? T(1) : T(0);
        } else {
#pragma unroll
            for (int b = 0; b < NB; ++b) load_pts(g + int64_t(b) * npts, base, lane, npts, full, gg[b]);
        }
        step.clear();
        walk<ProjectStep<T, NB>::E>(a, rr, tt, table, nrec, nmodes,
                                    [&](int j, int k, const T z[kVec]) {
                                        const auto value = [&](int q) { return self ? z[q] * z[q] : z[q]; };
                                        if (j == 0)
                                            step.emit_each(0, k, gg, value);
                                        else
                                            step.emit_each(ProjectStep<T, NB>::E > 1 ? 1 : 0, k, gg, value);
                                    },
                                    [&] { step.flush(wacc, nmodes, lane); });
    }
    project_end(sacc, nacc, tid, [&](int o, T s) { partial[int64_t(blockIdx.x) * ld + o] = s; });
}

// ---------------------------------------------------------------- overlap: partial[group][4], then out = Re S, Im S, I1, I2, eta
// C1, C2: the field is complex (interleaved re, im), else real
template <typename T, int C1, int C2>
__global__ __launch_bounds__(kThreads) void overlap_kernel(int64_t npts, const T* __restrict__ e1, const T* __restrict__ e2,
                                                           T* __restrict__ partial) {
    using V2 = T __attribute__((ext_vector_type(2)));
    __shared__ T sw[kWaves][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T sr = T(0), si = T(0), i1 = T(0), i2 = T(0);
#pragma unroll 4
    for (int64_t p = int64_t(blockIdx.x) * kThreads + tid; p < npts; p += int64_t(gridDim.x) * kThreads) {
        T ar, ai = T(0), br, bi = T(0);
        if (C1) {
            const V2 v = reinterpret_cast<const V2*>(e1)[p];
            ar = v[0], ai = v[1];
        } else {
            ar = e1[p];
        }
        if (C2) {
            const V2 v = reinterpret_cast<const V2*>(e2)[p];
            br = v[0], bi = v[1];
        } else {
            br = e2[p];
        }
        sr += ar * br + ai * bi;
        si += ai * br - ar * bi;
        i1 += ar * ar + ai * ai;
        i2 += br * br + bi * bi;
    }
    sr = wave_sum(sr), si = wave_sum(si), i1 = wave_sum(i1), i2 = wave_sum(i2);
    if (lane == 0) sw[wave][0] = sr, sw[wave][1] = si, sw[wave][2] = i1, sw[wave][3] = i2;
    __syncthreads();
    if (tid < 4) {
        T s = sw[0][tid];
        for (int w = 1; w < kWaves; ++w) s += sw[w][tid];
        partial[int64_t(blockIdx.x) * 4 + tid] = s;
    }
}

// one workgroup: wave w sums output w over the groups in a fixed order, thread 0 forms eta
template <typename T>
__global__ __launch_bounds__(kThreads) void overlap_finish_kernel(int64_t ngroups, const T* __restrict__ partial, T* __restrict__ out) {
    __shared__ T tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T s = T(0);
    for (int64_t gi = lane; gi < ngroups; gi += 64) s += partial[gi * 4 + wave];
    s = wave_sum(s);
    if (lane == 0) tot[wave] = s;
    __syncthreads();
    if (tid == 0) {
        out[0] = tot[0], out[1] = tot[1], out[2] = tot[2], out[3] = tot[3];
        out[4] = (tot[0] * tot[0] + tot[1] * tot[1]) / (tot[2] * tot[3]);
    }
}
static_assert(kWaves == 4, "overlap_finish_kernel gives one wave to each of the four sums");

int64_t overlap_groups(int64_t npts) { return project_groups(npts); }

int check_walk(const char* who, int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec,
               int64_t nmodes) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!r || !t || !table || npts < 0 || nrec < 0 || nmodes < 0 || nrec > INT32_MAX || nmodes > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (!(a > 0) || !std::isfinite(a)) return fail(PM_ERR_ARG, "%s: the core radius a must be positive and finite", who);
    if (!aligned(r, elem_of(dtype)) || !aligned(t, elem_of(dtype)) || !aligned(table, 8))
        return fail(PM_ERR_ARG, "%s: unaligned pointer (r, t want the element size, the table 8 bytes)", who);
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld points is too many", who, (long long)npts);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_fiber_modes(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                   void* out, void* stream) {
    if (int rc = check_walk("pm_fiber_modes", dtype, npts, r, t, a, table, nrec, nmodes)) return rc;
    if (!out || !aligned(out, elem_of(dtype))) return fail(PM_ERR_ARG, "pm_fiber_modes: bad argument (null or unaligned pointer out)");
    if (npts == 0 || nmodes == 0) return 0;
    return by_rdtype(dtype, "pm_fiber_modes", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(fiber_modes_kernel<T>, dim3(unsigned(tiles_of(npts))), dim3(kThreads), 0, PM_STREAM(stream), npts, T(a),
                           static_cast<const T*>(r), static_cast<const T*>(t), static_cast<const FRec<T>*>(table), int(nrec), int(nmodes),
                           static_cast<T*>(out), vec_ok(npts, {r, t, out}));
        return int(hipGetLastError());
    });
}

int pm_fiber_sum(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                 int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream) {
    if (int rc = check_walk("pm_fiber_sum", dtype, npts, r, t, a, table, nrec, nmodes)) return rc;
    if (!out || !coefs || batch < 0 || !aligned(out, elem_of(dtype)) || !aligned(coefs, elem_of(dtype)))
        return fail(PM_ERR_ARG, "pm_fiber_sum: bad argument (null or unaligned pointer, or negative batch)");
    if (npts == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_fiber_sum", [&](auto real) {
        using T = decltype(real);
        const T *rp = static_cast<const T*>(r), *tp = static_cast<const T*>(t), *c = static_cast<const T*>(coefs);
        const FRec<T>* recs = static_cast<const FRec<T>*>(table);
        T* o = static_cast<T*>(out);
        const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
        const int vec = vec_ok(npts, {r, t, out});
        for (int64_t b0 = 0; b0 < batch;)
            b0 += by_nb(batch - b0, 8, [&](auto nb) {
                hipLaunchKernelGGL((fiber_sum_kernel<T, decltype(nb)::value>), grid, block, 0, PM_STREAM(stream), npts, T(a), rp, tp, recs,
                                   int(nrec), int(nmodes), c + b0 * nmodes, accumulate != 0, o + b0 * npts, vec);
            });
        return int(hipGetLastError());
    });
}

size_t pm_fiber_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch) {
    if (!real_dtype(dtype) || npts < 0 || nmodes < 0 || batch < 0) return 0;
    return project_workspace_bytes(dtype, npts, size_t(batch) * size_t(nmodes));
}

int pm_fiber_project(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                     int64_t batch, const void* g, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_walk("pm_fiber_project", dtype, npts, r, t, a, table, nrec, nmodes)) return rc;
    if (!out || batch < 0 || !aligned(out, elem_of(dtype)) || !aligned(g, elem_of(dtype)) || !aligned(workspace, elem_of(dtype)))
        return fail(PM_ERR_ARG, "pm_fiber_project: bad argument (null or unaligned pointer, or negative batch)");
    if (!g && batch > 1) return fail(PM_ERR_ARG, "pm_fiber_project: g = NULL (the modes against themselves) takes batch 1");
    const int vec = g ? vec_ok(npts, {r, t, g}) : vec_ok(npts, {r, t});
    return launch_project("pm_fiber_project", "nmodes", "modes", dtype, npts, nmodes, batch, nmodes, 0, out, workspace, workspace_bytes, stream,
                          kMaxProjectGroups, [&](auto real, auto nb, int64_t b0, int64_t groups, size_t lds, hipStream_t st) {
                              using T = decltype(real);
                              hipLaunchKernelGGL((fiber_project_kernel<T, decltype(nb)::value>), dim3(unsigned(groups)), dim3(kThreads), lds, st,
                                                 npts, T(a), static_cast<const T*>(r), static_cast<const T*>(t),
                                                 static_cast<const FRec<T>*>(table), int(nrec), int(nmodes),
                                                 g ? static_cast<const T*>(g) + b0 * npts : nullptr, static_cast<T*>(workspace) + b0 * nmodes,
                                                 batch * nmodes, vec);
                          });
}

size_t pm_overlap_workspace(int32_t dtype, int64_t npts) {
    if (!real_dtype(dtype) || npts < 0) return 0;
    return size_t(overlap_groups(npts)) * 4 * elem_of(dtype);
}

int pm_overlap(int32_t dtype, int64_t npts, const void* e1, int32_t e1_complex, const void* e2, int32_t e2_complex, void* out,
               void* workspace, size_t workspace_bytes, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_overlap: dtype must be PM_F32 or PM_F64");
    if (!e1 || !e2 || !out || npts < 0) return fail(PM_ERR_ARG, "pm_overlap: bad argument (null pointer or negative size)");
    const size_t el = elem_of(dtype);
    if (!aligned(e1, e1_complex ? 2 * el : el) || !aligned(e2, e2_complex ? 2 * el : el) || !aligned(out, el) || !aligned(workspace, el))
        return fail(PM_ERR_ARG, "pm_overlap: unaligned pointer (a complex field wants twice the element size)");
    const size_t need = pm_overlap_workspace(dtype, npts);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "pm_overlap: workspace of %zu bytes is smaller than the %zu pm_overlap_workspace asks for",
                    workspace_bytes, need);
    return by_rdtype(dtype, "pm_overlap", [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        const int64_t groups = overlap_groups(npts);
        const T *p1 = static_cast<const T*>(e1), *p2 = static_cast<const T*>(e2);
        T* partial = static_cast<T*>(workspace);
        const dim3 grid{unsigned(groups)}, block{kThreads};
        if (e1_complex && e2_complex)
            hipLaunchKernelGGL((overlap_kernel<T, 1, 1>), grid, block, 0, st, npts, p1, p2, partial);
        else if (e1_complex)
            hipLaunchKernelGGL((overlap_kernel<T, 1, 0>), grid, block, 0, st, npts, p1, p2, partial);
        else if (e2_complex)
            hipLaunchKernelGGL((overlap_kernel<T, 0, 1>), grid, block, 0, st, npts, p1, p2, partial);
        else
            hipLaunchKernelGGL((overlap_kernel<T, 0, 0>), grid, block, 0, st, npts, p1, p2, partial);
        hipLaunchKernelGGL(overlap_finish_kernel<T>, dim3(1), block, 0, st, groups, partial, static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

}  // extern "C"
