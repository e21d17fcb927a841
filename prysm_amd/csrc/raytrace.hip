// Sequential ray trace (prysm/x/raytracing: spencer_and_murty.raytrace, Surface.interact, intersections.py, sags.py) (gfx950): a bundle of
// N rays through J surfaces in one launch.
//
// One thread per ray.  The thread keeps the ray -- position P, direction S, the index n of the medium it is in and its status -- in
// registers from the first surface to the last; a surface is one record of kRec doubles in a device table that every thread reads at
// an address without its own index (the same in every lane, prysm_amd/x/raytrace_plan.py packs it).  The kernel converts a value to
// its working type as it reads it; the polynomial coefficients of an even asphere are read from the table inside the Horner loop.
//
// Per surface, what Surface.interact does (surfaces.py:1407-1482): to local coordinates, intersect, status code, aperture, bend, back
// to global coordinates, the signed optical path of the segment.  The intersection is one of
//   - the plane (ray_plane_intersect),
//   - the conicoid, on or off axis, in closed form (ray_conic_intersect: Welford's rationalised root, the root by z_dir sign(c), the
//     vertex-tangent case, valid where the discriminant and 1 - (1 + k) c^2 r^2 are not negative),
//   - the even asphere by ConicSeedMixin.intersect: Newton from the seed conic's root (at most 100 iterations), the departure-band
//     policing of that root, the closest-approach band where the seed conic misses, and the Lipschitz march (at most 256 steps) for
//     the rays the policing sends to the rescue; then the rejection of roots behind the origin.
// Every loop is bounded; a lane that has converged waits for the other lanes of its wavefront, which take similar iteration counts.
//
// A ray keeps the FIRST failure: the 1-based surface and the code.  From that surface on its P, S and OPL are stored as NaN.  With
// history the outputs are the reference's (J + 1, N, 3) and (J + 1, N) arrays, row 0 the launch: a wavefront stores 64 x 3 adjacent
// values of a row.  Without it only the last row and the sum of the path lengths, added in surface order, are stored.
//
// prysm_amd/x/raytrace_plan.py is this file in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile): the arithmetic is
// + - * /, sqrt, sign and compares, each rounded by itself, in the order the model writes them.
#include <cmath>
#include <limits>

#include "pm_entry.h"

namespace pm {
namespace {

constexpr int kThreads = 256;

// the surface record, in doubles (prysm_amd/x/raytrace_plan.py REC_*)
enum {
    kInteraction = 0,      // PM_RT_REFLECT, PM_RT_REFRACT, PM_RT_MEASURE
    kShape = 1,            // PM_RT_PLANE, PM_RT_CONIC, PM_RT_ASPHERE
    kC = 2, kK = 3, kDx = 4, kDy = 5,
    kNcoef = 6, kCoef = 7,      // 8 coefficients: r^4, r^6, ...
    kP = 15,               // the vertex, 3
    kR = 18,               // the rotation, 9, row-major
    kHasR = 27,
    kNpost = 28,           // the index after the surface at the traced wavelength
    kApKind = 29,          // 0 none, 1 circular, 2 annular
    kApX0 = 30, kApY0 = 31, kApRin = 32, kApRout = 33,
    kBounded = 34, kMaxDep = 35, kDomainR = 36, kGradBound = 37, kLipschitz = 38,
    kFirst = 39,           // the first surface of the prescription: roots behind the origin are not rejected
    kAnalytic = 40,        // a failed intersection is PM_RT_MISS (closed form) or PM_RT_NEWTON
    kRec = 48,
};

constexpr int kNewtonIters = 100;
constexpr int kMarchSteps = 256;

template <typename T>
struct V3 {
    T x, y, z;
};

template <typename T> __device__ __forceinline__ V3<T> operator+(V3<T> a, V3<T> b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename T> __device__ __forceinline__ V3<T> operator-(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T> __device__ __forceinline__ V3<T> operator*(T s, V3<T> a) { return {s * a.x, s * a.y, s * a.z}; }
template <typename T> __device__ __forceinline__ T dot(V3<T> a, V3<T> b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <typename T> __device__ __forceinline__ bool finite3(V3<T> a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
template <typename T> __device__ __forceinline__ bool nan3(V3<T> a) { return a.x != a.x || a.y != a.y || a.z != a.z; }
template <typename T> __device__ __forceinline__ T qnan() { return std::numeric_limits<T>::quiet_NaN(); }
// numpy's sign: -1, 0, 1, and NaN for NaN
template <typename T> __device__ __forceinline__ T sign(T x) { return x > T(0) ? T(1) : (x < T(0) ? T(-1) : x); }
// numpy's maximum and minimum: a NaN in either operand is the result
template <typename T> __device__ __forceinline__ T np_max(T a, T b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
template <typename T> __device__ __forceinline__ T np_min(T a, T b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

// v M^T (rows of M dotted with v) and v M, M row-major in the record
template <typename T>
__device__ __forceinline__ V3<T> mul_rt(V3<T> v, const double* m) {
    return {(v.x * T(m[0]) + v.y * T(m[1])) + v.z * T(m[2]), (v.x * T(m[3]) + v.y * T(m[4])) + v.z * T(m[5]),
            (v.x * T(m[6]) + v.y * T(m[7])) + v.z * T(m[8])};
}
template <typename T>
__device__ __forceinline__ V3<T> mul_r(V3<T> v, const double* m) {
    return {(v.x * T(m[0]) + v.y * T(m[3])) + v.z * T(m[6]), (v.x * T(m[1]) + v.y * T(m[4])) + v.z * T(m[7]),
            (v.x * T(m[2]) + v.y * T(m[5])) + v.z * T(m[8])};
}

template <typename T>
struct Hit {
    V3<T> q, n;
    bool valid;
};

// ray_plane_intersect (intersections.py:21-47)
template <typename T>
__device__ __forceinline__ Hit<T> hit_plane(V3<T> p, V3<T> s) {
    const T t = (-p.z) / s.z;
    return {p + t * s, {T(0), T(0), T(1)}, s.z != T(0)};
}

// the coefficients of A t^2 + 2 B t + C (intersections.py:50-60)
template <typename T>
__device__ __forceinline__ void conic_abc(T c, T k, V3<T> p1, V3<T> s, T dx, T dy, T& A, T& B, T& C) {
    const T xp = p1.x + dx, yp = p1.y + dy;
    A = T(1) + (k * s.z) * s.z;
    B = (xp * s.x + yp * s.y) - s.z / c;
    C = xp * xp + yp * yp;
}

// ray_conic_intersect (intersections.py:63-134) with conic_sag_and_normal (sags.py:109-121)
template <typename T>
__device__ __forceinline__ Hit<T> hit_conic(V3<T> p, V3<T> s, T c, T k, T dx, T dy) {
    if (c == T(0)) return hit_plane(p, s);
    const T s0 = (-p.z) / s.z;
    const V3<T> p1 = p + s0 * s;
    T A, B, C;
    conic_abc(c, k, p1, s, dx, dy, A, B, C);
    T disc = B * B - A * C;
    const bool disc_nonneg = disc >= T(0);
    disc = disc_nonneg ? disc : T(0);
    const T sq = sqrt(disc);
    const T sign_c = c > T(0) ? T(1) : T(-1), z_dir = s.z < T(0) ? T(-1) : T(1);
    const T denom = (z_dir * sign_c) * sq - B;
    const bool tangent = denom == T(0);
    const T t = tangent ? T(0) : C / denom;
    Hit<T> h;
    h.q = p1 + t * s;
    const T xq = h.q.x + dx, yq = h.q.y + dy, rr = xq * xq + yq * yq;
    const T phi_arg = T(1) - (((T(1) + k) * c) * c) * rr;
    T phi = sqrt(T(1) - ((T(1) + k) * (c * c)) * rr);
    phi = phi != phi ? T(0) : phi;
    const T mag_sq = T(1) - ((k * c) * c) * rr;
    const T mag = sqrt(mag_sq < T(0) ? T(1) : mag_sq);
    h.n = {((-c) * xq) / mag, ((-c) * yq) / mag, phi / mag};
    h.valid = disc_nonneg && phi_arg >= T(0);
    return h;
}

// EvenAsphere.sag_and_normal (surfaces.py:680-688, sags.py:413-483): the coefficients come from the record inside the loop
template <typename T>
__device__ __forceinline__ void asphere(const double* rec, T c, T k, T x, T y, T& z, V3<T>& n) {
    const int nc = int(rec[kNcoef]);
    const T rsq = x * x + y * y;
    const T phi = sqrt(T(1) - ((T(1) + k) * (c * c)) * rsq);
    z = (c * rsq) / (T(1) + phi);
    T fx = (c * x) / phi, fy = (c * y) / phi;
    if (nc > 0) {
        T p = T(0), q = T(0);
        for (int i = nc - 1; i >= 0; --i) {
            const T a = T(rec[kCoef + i]);
            p = p * rsq + a;
            q = q * rsq + T(i + 2) * a;
        }
        z = z + (p * rsq) * rsq;
        const T common = (T(2) * rsq) * q;
        fx = fx + x * common;
        fy = fy + y * common;
    }
    const T inv = T(1) / sqrt((T(1) + fx * fx) + fy * fy);
    n = {(-fx) * inv, (-fy) * inv, inv};
}

// ConicSeedMixin.intersect (intersections.py:337-477) for the even asphere
template <typename T>
__device__ __forceinline__ Hit<T> hit_asphere(const double* rec, V3<T> p, V3<T> s, T c, T k, T tol, T tol100, bool forward_only) {
    const T s0 = (-p.z) / s.z;
    const V3<T> p1 = p + s0 * s;
    const Hit<T> seed = hit_conic(p1, s, c, k, T(0), T(0));
    const T s1 = seed.q.z / s.z;
    // newton_raphson_solve_s (spencer_and_murty.py:207-306): a ray that arrives non-finite does not iterate
    Hit<T> h;
    h.q = h.n = {qnan<T>(), qnan<T>(), qnan<T>()};
    h.valid = false;
    if (finite3(p1) && finite3(s) && isfinite(s1)) {
        T sj = s1;
        for (int it = 0; it < kNewtonIters; ++it) {
            const V3<T> pj = p1 + sj * s;
            T z;
            V3<T> n;
            asphere(rec, c, k, pj.x, pj.y, z, n);
            const T F = pj.z - z;
            if (fabs(F) < tol) {
                h.q = pj, h.n = n, h.valid = true;
                break;
            }
            const T Fp = dot(s, n) / n.z;
            sj = sj - F / Fp;
        }
    }
    const bool bounded = rec[kBounded] != 0.0;
    if (!bounded && !forward_only) return h;
    T s_root = dot(h.q - p1, s);
    if (bounded) {
        const T D = T(rec[kMaxDep]), Rd = T(rec[kDomainR]), G = T(rec[kGradBound]), Lb = T(rec[kLipschitz]);
        T cosi = fabs(dot(s, seed.n));
        const T s_t = sqrt(np_max(T(0), T(1) - s.z * s.z));
        const bool certified = (cosi - G * s_t) > T(1e-3);
        if (!(cosi >= T(1e-3))) cosi = T(1e-3);
        const T band = (D + tol100 * (T(1) + fabs(s1))) / cosi;
        const T rseed_sq = seed.q.x * seed.q.x + seed.q.y * seed.q.y;
        const bool seed_ok = seed.valid && isfinite(s1);
        const bool police = seed_ok && rseed_sq <= Rd * Rd;
        const bool in_band = fabs(s_root - s1) <= band;
        const bool in_domain = (h.q.x * h.q.x + h.q.y * h.q.y) <= Rd * Rd;
        const bool prior_accept = h.valid && (!police || (in_band && in_domain)) && !(!seed_ok && !in_domain);
        const bool certified_accept = h.valid && police && in_band && in_domain && certified;
        bool rescue = police && !certified_accept;
        T lo = s1 - band, hi = s1 + band;
        if (!seed_ok && c != T(0)) {
            // the closest-approach band of a ray whose seed conic misses
            T A, B, C;
            conic_abc(c, k, p1, s, T(0), T(0), A, B, C);
            const T z_max = ((fabs(c) * Rd) * Rd) / T(2) + D;
            const T scale = T(2) / fabs(c) + (T(2) * fabs(T(1) + k)) * z_max;
            const T d_imp = (D + tol100) * scale;
            const T t_star = (-B) / A;
            const T c_min = C - (B * B) / A;
            const T wsq = (d_imp - c_min) / A;
            if (A > T(0) && wsq >= T(0) && isfinite(t_star)) {
                const T w = sqrt(fabs(wsq));
                lo = t_star - w, hi = t_star + w;
                rescue = true;
            }
        }
        bool accept = certified_accept || prior_accept;
        if (rescue) {
            // _domain_corridor and _lipschitz_march_solve_s (intersections.py:169-271)
            const T Rm = T(1.1) * Rd;
            const T a = s.x * s.x + s.y * s.y, b = p1.x * s.x + p1.y * s.y, cc = (p1.x * p1.x + p1.y * p1.y) - Rm * Rm;
            const T disc = b * b - a * cc, sq = sqrt(np_max(disc, T(0)));
            const T s_a = ((-b) - sq) / a, s_b = ((-b) + sq) / a;
            const bool swept = a > T(0), real = swept && disc >= T(0);
            if (real) lo = np_max(lo, s_a), hi = np_min(hi, s_b);
            if ((swept && !real) || (!swept && cc > T(0))) hi = lo - T(1);
            T lip = fabs(s.z) + Lb * s_t;
            lip = lip > T(0) ? lip : T(1);
            bool found = false;
            if (lo <= hi) {
                T sj = lo;
                for (int it = 0; it < kMarchSteps; ++it) {
                    const V3<T> pj = p1 + sj * s;
                    T z;
                    V3<T> n;
                    asphere(rec, c, k, pj.x, pj.y, z, n);
                    const T F = pj.z - z;
                    if (fabs(F) < tol) {
                        h.q = pj, h.n = n, found = true;
                        break;
                    }
                    const T step_lip = fabs(F) / lip;
                    const T Fp = dot(s, n) / n.z;
                    const T step_newton = (-F) / Fp;
                    const bool near = isfinite(step_newton) && fabs(Fp) > T(1e-3) && step_lip < T(1e-2) * (T(1) + fabs(sj));
                    const T s_new = np_min(np_max(near ? sj + step_newton : sj + step_lip, lo), hi);
                    const bool exhausted = !near && (sj + step_lip > hi);
                    sj = s_new;
                    if (exhausted || !isfinite(F)) break;
                }
            }
            // the rescue wins where it converged; where it stalled the earlier acceptance stands
            accept = found || prior_accept;
            s_root = dot(h.q - p1, s);
        }
        h.valid = accept;
    }
    if (forward_only && (s0 + s_root) < (-tol100) * (T(1) + fabs(s0))) h.valid = false;
    return h;
}

template <typename T>
__device__ __forceinline__ void store3(T* __restrict__ dst, int64_t at, V3<T> v) {
    dst[at] = v.x, dst[at + 1] = v.y, dst[at + 2] = v.z;
}

template <typename T, bool HIST>
__global__ __launch_bounds__(kThreads) void trace_kernel(const double* __restrict__ table, int64_t N, int64_t J, T n_launch, T tol, T tol100,
                                                          const T* __restrict__ P, const T* __restrict__ S, T* __restrict__ Po, T* __restrict__ So,
                                                          T* __restrict__ Oo, int32_t* __restrict__ st_surface, int32_t* __restrict__ st_code) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= N) return;
    V3<T> X = {P[3 * i], P[3 * i + 1], P[3 * i + 2]}, D = {S[3 * i], S[3 * i + 1], S[3 * i + 2]};
    T n = n_launch, opl_sum = T(0);
    int32_t surface = 0, code = PM_RT_OK;
    if (HIST) {
        store3(Po, 3 * i, X);
        store3(So, 3 * i, D);
        Oo[i] = T(0);
    }
    const V3<T> nan_v = {qnan<T>(), qnan<T>(), qnan<T>()};
    for (int64_t j = 0; j < J; ++j) {
        const double* rec = table + j * kRec;      // no thread index: the same address in every lane
        const int interaction = int(rec[kInteraction]);
        T opl = qnan<T>();
        if (code == PM_RT_OK) {
            const bool has_r = rec[kHasR] != 0.0;
            const V3<T> vertex = {T(rec[kP]), T(rec[kP + 1]), T(rec[kP + 2])};
            V3<T> p0 = X - vertex, sl = D;
            if (has_r) p0 = mul_rt(p0, rec + kR), sl = mul_rt(sl, rec + kR);
            const int shape = int(rec[kShape]);
            const T c = T(rec[kC]), k = T(rec[kK]);
            Hit<T> h;
            if (shape == PM_RT_PLANE) {
                h = hit_plane(p0, sl);
            } else if (shape == PM_RT_CONIC) {
                h = hit_conic(p0, sl, c, k, T(rec[kDx]), T(rec[kDy]));
            } else {
                h = hit_asphere(rec, p0, sl, c, k, tol, tol100, interaction != PM_RT_MEASURE && rec[kFirst] == 0.0);
            }
            int32_t step = h.valid ? PM_RT_OK : (rec[kAnalytic] != 0.0 ? PM_RT_MISS : PM_RT_NEWTON);
            const int ap = int(rec[kApKind]);
            if (ap != 0 && h.valid) {
                const T ax = h.q.x - T(rec[kApX0]), ay = h.q.y - T(rec[kApY0]), rsq = ax * ax + ay * ay;
                const T rout = T(rec[kApRout]), rin = T(rec[kApRin]);
                const bool inside = ap == 1 ? rsq <= rout * rout : (rsq >= rin * rin && rsq <= rout * rout);
                if (!inside) step = PM_RT_CLIP;
            }
            V3<T> sp = sl;
            if (interaction == PM_RT_REFLECT) {
                const T cos_i = dot(sl, h.n);
                sp = sl - (T(2) * cos_i) * h.n;
            } else if (interaction == PM_RT_REFRACT) {
                const T mu = n / T(rec[kNpost]);
                const T cos_i = dot(h.n, sl);
                const T sin_t_sq = (mu * mu) * (T(1) - cos_i * cos_i);
                const T cos_t = sqrt(T(1) - sin_t_sq);
                const T factor = sign(cos_i) * cos_t - mu * cos_i;
                sp = mu * sl + factor * h.n;
                if (step == PM_RT_OK && nan3(sp)) step = PM_RT_TIR;
            }
            V3<T> q = h.q;
            if (has_r) q = mul_r(q, rec + kR), sp = mul_r(sp, rec + kR);
            q = q + vertex;
            const V3<T> seg = q - X;
            opl = (n * sign(dot(seg, D))) * sqrt(dot(seg, seg));
            X = q, D = sp;
            if (step != PM_RT_OK) code = step, surface = int32_t(j + 1);
        }
        if (interaction == PM_RT_REFRACT) n = T(rec[kNpost]);
        if (code != PM_RT_OK) X = nan_v, D = nan_v, opl = qnan<T>();
        if (HIST) {
            const int64_t row = (j + 1) * N;
            store3(Po, 3 * (row + i), X);
            store3(So, 3 * (row + i), D);
            Oo[row + i] = opl;
        } else {
            opl_sum = opl_sum + opl;
        }
    }
    if (!HIST) {
        store3(Po, 3 * i, X);
        store3(So, 3 * i, D);
        Oo[i] = opl_sum;
    }
    st_surface[i] = code == PM_RT_OK ? int32_t(J) : surface;
    st_code[i] = code;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_rt_trace(int32_t dtype, int64_t N, int64_t J, const void* table, double n_launch, double tol_sag, int32_t history, const void* P,
                const void* S, void* P_out, void* S_out, void* OPL_out, void* status_surface, void* status_code, void* stream) {
    const char* who = "pm_rt_trace";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (N < 0 || J < 0) return fail(PM_ERR_ARG, "%s: N and J must not be negative, got %lld, %lld", who, (long long)N, (long long)J);
    if (J > PM_RT_MAX_SURFACES) return fail(PM_ERR_ARG, "%s: %lld surfaces are more than the table limit of %d", who, (long long)J, PM_RT_MAX_SURFACES);
    if (N > (int64_t(1) << 36)) return fail(PM_ERR_ARG, "%s: %lld rays are too many", who, (long long)N);
    if (history != 0 && history != 1) return fail(PM_ERR_ARG, "%s: history must be 0 or 1, got %d", who, int(history));
    if (!(tol_sag > 0.0)) return fail(PM_ERR_ARG, "%s: tol_sag must be positive", who);
    if (N == 0 || J == 0) return 0;
    if (!table || !P || !S || !P_out || !S_out || !OPL_out || !status_surface || !status_code) return fail(PM_ERR_ARG, "%s: null pointer", who);
    const size_t el = elem_of(dtype);
    if (!aligned(table, 8) || !aligned(P, el) || !aligned(S, el) || !aligned(P_out, el) || !aligned(S_out, el) || !aligned(OPL_out, el) ||
        !aligned(status_surface, 4) || !aligned(status_code, 4))
        return fail(PM_ERR_ARG, "%s: a pointer is not aligned to its element", who);
    hipStream_t st = PM_STREAM(stream);
    const dim3 grid(unsigned((N + kThreads - 1) / kThreads)), block(kThreads);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, st, static_cast<const double*>(table), N, J, T(n_launch), T(tol_sag), T(100.0 * tol_sag),
                               static_cast<const T*>(P), static_cast<const T*>(S), static_cast<T*>(P_out), static_cast<T*>(S_out),
                               static_cast<T*>(OPL_out), static_cast<int32_t*>(status_surface), static_cast<int32_t*>(status_code));
            return int(hipGetLastError());
        };
        return history ? go(trace_kernel<T, true>) : go(trace_kernel<T, false>);
    });
}

}  // extern "C"
