// Jones and Mueller calculus per pixel (prysm/x/polarization.py:45-475, 555-578) (gfx950).  A Jones field over rows x cols pixels has four
// complex components per pixel in the order (0,0), (0,1), (1,0), (1,1), a Jones vector two, (0,0), (1,0), in one of two layouts:
//     PM_JONES_AOS      the reference's (..., 2, 2) / (..., 2, 1): the components of a pixel are consecutive, pixel (r, c) at
//                       (r ld + c) ncomp elements
//     PM_JONES_PLANES   (ncomp, rows, cols): component k of pixel (r, c) at k pstride + r ld + c elements, the stack the FFT routines take
// ld counts pixels, so a 2-D window of a wider array is its base and the wider array's ld.  The layout is a template parameter of every
// kernel.  All of them run on the row sweep of pm_sweep.h: a lane takes one pixel per trip, reads each input once and stores each
// output once; nothing is kept in memory between the steps of a formula.
//
//  - pm_jones_optic: a Jones map from its parameters, each a host double or a real map: ROTATION [[c, s], [-s, c]]; RETARDER
//    rot(-t) diag(1, p) rot(t) = [[c^2 + s^2 p, c s (1 - p)], [c s (1 - p), s^2 + c^2 p]] with p = exp(i delta); DIATTENUATOR the same
//    with p = alpha; VORTEX rot(-rho) (sin(delta / 2) [[ct, st], [st, -ct]] + diag(-i cos(delta / 2), 0 or the same)) rot(rho) with
//    ct, st the cosine and sine of charge theta, the product formed in the map's precision; LINPOL_VECTOR (cos, sin) of charge x angle.  The cosine
//    and sine of a host parameter are taken in double on the host and rounded once; those of a map in the map's type.  An optional
//    complex field multiplies every component (apply_polarization_optic inside the generator).
//  - pm_jones_chain: A_1 @ A_2 @ ... @ A_K from the left, K <= PM_JONES_MAX_CHAIN, each operand a constant or a map, the last one
//    possibly a vector.  A 2-term inner product is the sum of two complex products, each the four real products and two sums of cmul.
//  - pm_jones_scale: field x J for a complex, real or absent field, from one layout to the other or the same: without a field the
//    relayout.  out may be in when the layouts are equal (a lane reads its pixel before it writes it).
//  - pm_jones_to_mueller: the sixteen real elements of M = Re(U (J* (x) J) U^H) (Chipman, Lam and Young eq. 6.99) as sums of products
//    of the four components; no Kronecker array, no inverse.
//  - pm_pauli_coefficients: c0 = (a + d) / 2, c1 = (a - d) / 2, c2 = (b + c) / 2, c3 = i (b - c) / 2 as four complex planes.
//
// Accesses: a complex64 aos pixel is two 16-byte accesses (a vector one) where the base is 16-byte aligned, else one 8-byte access per
// component; a complex128 component is 16 bytes by itself.  A plane access is one component per lane, adjacent lanes adjacent
// elements.  The aos Mueller record (16 reals) is four (float) or eight (double) 16-byte stores where the base is aligned.
//
// prysm_amd/x/polarization_plan.py restates every kernel in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile).
#include <cmath>

#include "pm_entry.h"
#include "pm_math.h"
#include "pm_sweep.h"

namespace pm {
namespace {

// ---------------------------------------------------------------- pixel access
template <typename T>
__device__ __forceinline__ cx<T> ld1(const cx<T>* q) {
    if constexpr (sizeof(T) == 4) {
        const float2 v = *reinterpret_cast<const float2*>(q);
        return cx<T>{v.x, v.y};
    } else {
        const double2 v = *reinterpret_cast<const double2*>(q);
        return cx<T>{v.x, v.y};
    }
}

template <typename T>
__device__ __forceinline__ void st1(cx<T>* q, cx<T> v) {
    if constexpr (sizeof(T) == 4)
        *reinterpret_cast<float2*>(q) = make_float2(v.x, v.y);
    else
        *reinterpret_cast<double2*>(q) = make_double2(v.x, v.y);
}

// NC components per pixel.  wide: an aos complex64 base on a 16-byte boundary (every pixel of it then is)
template <typename T, int NC, bool PLANES>
struct View {
    cx<T>* p;
    int64_t ld, ps;
    int wide;

    __device__ __forceinline__ void load(int64_t r, int64_t c, cx<T> (&e)[NC]) const {
        if constexpr (PLANES) {
            const cx<T>* q = p + r * ld + c;
#pragma unroll
            for (int k = 0; k < NC; ++k) e[k] = ld1(q + k * ps);
        } else {
            const cx<T>* q = p + (r * ld + c) * NC;
            if constexpr (sizeof(T) == 4) {
                if (wide) {
#pragma unroll
                    for (int k = 0; k < NC; k += 2) {
                        const float4 v = *reinterpret_cast<const float4*>(q + k);
                        e[k] = cx<T>{v.x, v.y}, e[k + 1] = cx<T>{v.z, v.w};
                    }
                    return;
                }
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) e[k] = ld1(q + k);
        }
    }

    __device__ __forceinline__ void store(int64_t r, int64_t c, const cx<T> (&e)[NC]) const {
        if constexpr (PLANES) {
            cx<T>* q = p + r * ld + c;
#pragma unroll
            for (int k = 0; k < NC; ++k) st1(q + k * ps, e[k]);
        } else {
            cx<T>* q = p + (r * ld + c) * NC;
            if constexpr (sizeof(T) == 4) {
                if (wide) {
#pragma unroll
                    for (int k = 0; k < NC; k += 2) *reinterpret_cast<float4*>(q + k) = make_float4(e[k].x, e[k].y, e[k + 1].x, e[k + 1].y);
                    return;
                }
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) st1(q + k, e[k]);
        }
    }
};

template <typename T, int NC, bool PLANES>
View<T, NC, PLANES> view_of(const void* p, int64_t ld, int64_t ps) {
    return View<T, NC, PLANES>{static_cast<cx<T>*>(const_cast<void*>(p)), ld, ps, int(aligned(p, 16))};
}

// a b + c d, each product rounded by itself
template <typename T>
__device__ __forceinline__ cx<T> dot2(cx<T> a, cx<T> b, cx<T> c, cx<T> d) {
    return cmul(a, b) + cmul(c, d);
}

// ---------------------------------------------------------------- generators
// a parameter: the map's sample times `mul` where there is a map, else the host's value; co, si: cos and sin of value x mul, from double
template <typename T>
struct Param {
    const T* map;
    int64_t ld;
    T val, co, si;

    __device__ __forceinline__ T at(int64_t r, int64_t c) const { return map ? map[r * ld + c] : val; }
    __device__ __forceinline__ void cs(int64_t r, int64_t c, T mul, T* co_, T* si_) const {
        if (map)
            sincos_(map[r * ld + c] * mul, si_, co_);
        else
            *co_ = co, *si_ = si;
    }
};

template <typename T, int KIND, bool PLANES>
struct OpticOp {
    static constexpr int NC = KIND == PM_JONES_LINPOL_VECTOR ? 2 : 4;
    Param<T> p0, p1, p2;
    T charge;
    int leak;
    const cx<T>* field;
    int64_t fld;
    View<T, NC, PLANES> out;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        cx<T> e[NC];
        const T zero = T(0);
        if constexpr (KIND == PM_JONES_ROTATION) {
            T co, si;
            p0.cs(r, c, T(1), &co, &si);
            e[0] = cx<T>{co, zero}, e[1] = cx<T>{si, zero}, e[2] = cx<T>{-si, zero}, e[3] = cx<T>{co, zero};
        } else if constexpr (KIND == PM_JONES_LINPOL_VECTOR) {
            T co, si;
            p0.cs(r, c, charge, &co, &si);      // the factor on the angle: pi / 180 for degrees
            e[0] = cx<T>{co, zero}, e[1] = cx<T>{si, zero};
        } else if constexpr (KIND == PM_JONES_RETARDER || KIND == PM_JONES_DIATTENUATOR) {
            T pr, pi, co, si;
            if constexpr (KIND == PM_JONES_RETARDER)
                p0.cs(r, c, T(1), &pr, &pi);
            else
                pr = p0.at(r, c), pi = zero;
            p1.cs(r, c, T(1), &co, &si);
            const T c2 = co * co, s2 = si * si, sc = co * si;
            const cx<T> off{sc * (T(1) - pr), -(sc * pi)};
            e[0] = cx<T>{c2 + s2 * pr, s2 * pi}, e[1] = off, e[2] = off, e[3] = cx<T>{s2 + c2 * pr, c2 * pi};
        } else {
            T ct, st, cr, sr, co, si;
            p0.cs(r, c, charge, &ct, &st);
            p1.cs(r, c, T(0.5), &cr, &sr);
            p2.cs(r, c, T(1), &co, &si);
            const cx<T> a{sr * ct, -cr}, b{sr * st, zero}, d{-(sr * ct), leak ? -cr : zero};
            // rot(-rho) @ L, then @ rot(rho), as the reference multiplies
            const cx<T> x00 = cscale(a, co) - cscale(b, si), x01 = cscale(b, co) - cscale(d, si);
            const cx<T> x10 = cscale(a, si) + cscale(b, co), x11 = cscale(b, si) + cscale(d, co);
            e[0] = cscale(x00, co) - cscale(x01, si), e[1] = cscale(x00, si) + cscale(x01, co);
            e[2] = cscale(x10, co) - cscale(x11, si), e[3] = cscale(x10, si) + cscale(x11, co);
        }
        if (field) {
            const cx<T> f = ld1(field + r * fld + c);
#pragma unroll
            for (int k = 0; k < NC; ++k) e[k] = cmul(e[k], f);
        }
        out.store(r, c, e);
    }
};

// ---------------------------------------------------------------- chain
// a value of the kernel's arguments, pinned to scalar registers: without this the compiler merges "load from the map" and "take the
// constant" into one load through a selected pointer and copies the constants to scratch memory for it
__device__ __forceinline__ float uniform_(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ double uniform_(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = __builtin_amdgcn_readfirstlane(int(unsigned(b))), hi = __builtin_amdgcn_readfirstlane(int(unsigned(b >> 32)));
    return __builtin_bit_cast(double, (long long)((unsigned long long)hi << 32 | lo));
}

template <typename T>
struct Operand {
    const cx<T>* map;
    int64_t ld, ps;
    int wide;
    cx<T> k[4];
};

template <typename T, bool PIN, bool POUT, bool VEC>
struct ChainOp {
    static constexpr int NOUT = VEC ? 2 : 4;
    int count;
    Operand<T> op[PM_JONES_MAX_CHAIN];
    View<T, NOUT, POUT> out;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    template <int NC>
    __device__ __forceinline__ void fetch(int i, int64_t r, int64_t c, cx<T> (&e)[NC]) const {
        if (op[i].map) {
            View<T, NC, PIN>{const_cast<cx<T>*>(op[i].map), op[i].ld, op[i].ps, op[i].wide}.load(r, c, e);
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j) e[j] = cx<T>{uniform_(op[i].k[j].x), uniform_(op[i].k[j].y)};
        }
    }

    // every index into op[] is a constant of the unrolled loops: the operands stay in the kernel's arguments
    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        const int nmat = VEC ? count - 1 : count;
        cx<T> a[4];
        if (nmat >= 1) fetch<4>(0, r, c, a);
#pragma unroll
        for (int i = 1; i < PM_JONES_MAX_CHAIN; ++i) {
            if (i < nmat) {
                cx<T> b[4];
                fetch<4>(i, r, c, b);
                const cx<T> n0 = dot2(a[0], b[0], a[1], b[2]), n1 = dot2(a[0], b[1], a[1], b[3]);
                const cx<T> n2 = dot2(a[2], b[0], a[3], b[2]), n3 = dot2(a[2], b[1], a[3], b[3]);
                a[0] = n0, a[1] = n1, a[2] = n2, a[3] = n3;
            }
        }
        if constexpr (VEC) {
            cx<T> v[2];
#pragma unroll
            for (int i = 0; i < PM_JONES_MAX_CHAIN; ++i)
                if (i == nmat) fetch<2>(i, r, c, v);
            if (nmat >= 1) {
                const cx<T> w[2] = {dot2(a[0], v[0], a[1], v[1]), dot2(a[2], v[0], a[3], v[1])};
                out.store(r, c, w);
            } else {
                out.store(r, c, v);
            }
        } else {
            out.store(r, c, a);
        }
    }
};

// ---------------------------------------------------------------- scale and relayout
template <typename T, int NC, bool PIN, bool POUT>
struct ScaleOp {
    View<T, NC, PIN> in;
    int field_kind;
    const void* field;
    int64_t fld;
    View<T, NC, POUT> out;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        cx<T> e[NC];
        in.load(r, c, e);
        if (field_kind == PM_JONES_FIELD_COMPLEX) {
            const cx<T> f = ld1(static_cast<const cx<T>*>(field) + r * fld + c);
#pragma unroll
            for (int k = 0; k < NC; ++k) e[k] = cmul(e[k], f);
        } else if (field_kind == PM_JONES_FIELD_REAL) {
            const T f = static_cast<const T*>(field)[r * fld + c];
#pragma unroll
            for (int k = 0; k < NC; ++k) e[k] = cscale(e[k], f);
        }
        out.store(r, c, e);
    }
};

// ---------------------------------------------------------------- Mueller
// Re(x* y), Im(x* y)
template <typename T> __device__ __forceinline__ T rec(cx<T> x, cx<T> y) { return x.x * y.x + x.y * y.y; }
template <typename T> __device__ __forceinline__ T imc(cx<T> x, cx<T> y) { return x.x * y.y - x.y * y.x; }

template <typename T, bool PIN, bool POUT>
struct MuellerOp {
    View<T, 4, PIN> in;
    T* out;
    int64_t old, ops;
    int wide;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c_, NoColumn) const {
        cx<T> e[4];
        in.load(r, c_, e);
        const cx<T> a = e[0], b = e[1], c = e[2], d = e[3];
        const T h = T(0.5);
        const T na = rec(a, a), nb = rec(b, b), nc = rec(c, c), nd = rec(d, d);
        T m[16];
        m[0] = h * ((na + nb) + (nc + nd));
        m[1] = h * ((na - nb) + (nc - nd));
        m[2] = rec(a, b) + rec(c, d);
        m[3] = imc(a, b) + imc(c, d);
        m[4] = h * ((na + nb) - (nc + nd));
        m[5] = h * ((na - nb) - (nc - nd));
        m[6] = rec(a, b) - rec(c, d);
        m[7] = imc(a, b) - imc(c, d);
        m[8] = rec(a, c) + rec(b, d);
        m[9] = rec(a, c) - rec(b, d);
        m[10] = rec(a, d) + rec(b, c);
        m[11] = imc(a, d) - imc(b, c);
        m[12] = -(imc(a, c) + imc(b, d));
        m[13] = -(imc(a, c) - imc(b, d));
        m[14] = -(imc(a, d) + imc(b, c));
        m[15] = rec(a, d) - rec(b, c);
        if constexpr (POUT) {
            T* q = out + r * old + c_;
#pragma unroll
            for (int k = 0; k < 16; ++k) q[k * ops] = m[k];
        } else {
            T* q = out + (r * old + c_) * 16;
            if (wide) {
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int k = 0; k < 16; k += 4) *reinterpret_cast<float4*>(q + k) = make_float4(m[k], m[k + 1], m[k + 2], m[k + 3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 16; k += 2) *reinterpret_cast<double2*>(q + k) = make_double2(m[k], m[k + 1]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) q[k] = m[k];
            }
        }
    }
};

// ---------------------------------------------------------------- Pauli
template <typename T, bool PIN>
struct PauliOp {
    View<T, 4, PIN> in;
    View<T, 4, true> out;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        cx<T> e[4], o[4];
        in.load(r, c, e);
        const T h = T(0.5), zero = T(0), one = T(1);
        const cx<T> df = e[1] - e[2];
        // 1j * df as numpy's complex product forms it: (0 re - 1 im, 0 im + 1 re)
        const cx<T> j{zero * df.x - one * df.y, zero * df.y + one * df.x};
        o[0] = cscale(e[0] + e[3], h), o[1] = cscale(e[0] - e[3], h), o[2] = cscale(e[1] + e[2], h), o[3] = cscale(j, h);
        out.store(r, c, o);
    }
};

// ---------------------------------------------------------------- the entry points' shared checks
bool layout_ok(int32_t layout) { return layout == PM_JONES_AOS || layout == PM_JONES_PLANES; }

// calls f with std::bool_constant<layout == PM_JONES_PLANES>
template <typename F>
int by_layout(int32_t layout, F&& f) {
    return layout == PM_JONES_PLANES ? f(std::true_type{}) : f(std::false_type{});
}

// a view of `ncomp` components of `elem` bytes each; 0, or the refusal
int check_view(const char* who, const void* p, int32_t layout, int ncomp, int64_t rows, int64_t cols, int64_t ld, int64_t ps, size_t elem) {
    if (!p) return fail(PM_ERR_ARG, "%s: bad argument (null pointer)", who);
    if (!ld_ok(rows, cols, ld)) return fail(PM_ERR_ARG, "%s: a leading dimension is smaller than the number of columns", who);
    if (layout == PM_JONES_PLANES && !stack_ok(ncomp, rows, ld, ps)) return fail(PM_ERR_ARG, "%s: the planes overlap (pstride < rows * ld)", who);
    if (!aligned(p, elem)) return fail(PM_ERR_ARG, "%s: an array is not aligned like its elements", who);
    return 0;
}

// the shape; 1 for an empty one (the entry point returns 0), 0 to go on, or the refusal
int check_shape(const char* who, int64_t rows, int64_t cols) {
    if (rows < 0 || cols < 0) return fail(PM_ERR_ARG, "%s: bad argument (negative shape)", who);
    if (rows > INT32_MAX || cols > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    return rows == 0 || cols == 0 ? 1 : 0;
}

template <typename T>
Param<T> param_of(const pm_jones_param& p, double mul) {
    const double v = p.value * mul;
    return Param<T>{static_cast<const T*>(p.map), p.ld, T(p.value), T(std::cos(v)), T(std::sin(v))};
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_jones_optic(int32_t dtype, const pm_jones_optic_desc* optic, int64_t rows, int64_t cols, const void* field, int64_t field_ld, void* out,
                   int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream) {
    const char* who = "pm_jones_optic";
    if (!optic) return fail(PM_ERR_ARG, "%s: bad argument (null optic)", who);
    const int32_t kind = optic->kind;
    if (kind < PM_JONES_ROTATION || kind > PM_JONES_LINPOL_VECTOR) return fail(PM_ERR_ARG, "%s: unknown kind %d", who, int(kind));
    if (!layout_ok(out_layout)) return fail(PM_ERR_ARG, "%s: the layout must be PM_JONES_AOS or PM_JONES_PLANES", who);
    if (const int rc = check_shape(who, rows, cols)) return rc < 0 ? rc : 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int ncomp = kind == PM_JONES_LINPOL_VECTOR ? 2 : 4;
        if (const int rc = check_view(who, out, out_layout, ncomp, rows, cols, out_ld, out_pstride, 2 * sizeof(T))) return rc;
        const int nparam = kind == PM_JONES_VORTEX ? 3 : (kind == PM_JONES_RETARDER || kind == PM_JONES_DIATTENUATOR) ? 2 : 1;
        for (int i = 0; i < nparam; ++i) {
            const pm_jones_param& p = optic->p[i];
            if (p.map) {
                PM_CHECK_LD("pm_jones_optic", ld_ok(rows, cols, p.ld));
                if (!aligned(p.map, sizeof(T))) return fail(PM_ERR_ARG, "%s: an array is not aligned like its elements", who);
            } else if (!std::isfinite(p.value)) {
                return fail(PM_ERR_ARG, "%s: a scalar parameter must be finite", who);
            }
        }
        if ((kind == PM_JONES_VORTEX || kind == PM_JONES_LINPOL_VECTOR) && !std::isfinite(optic->charge))
            return fail(PM_ERR_ARG, "%s: the charge must be finite", who);
        if (field) {
            PM_CHECK_LD("pm_jones_optic", ld_ok(rows, cols, field_ld));
            if (!aligned(field, 2 * sizeof(T))) return fail(PM_ERR_ARG, "%s: an array is not aligned like its elements", who);
        }
        const bool factor = kind == PM_JONES_VORTEX || kind == PM_JONES_LINPOL_VECTOR;
        const double charge = factor ? optic->charge : 1.0;
        const Param<T> p0 = param_of<T>(optic->p[0], charge);
        const Param<T> p1 = param_of<T>(optic->p[1], kind == PM_JONES_VORTEX ? 0.5 : 1.0);
        const Param<T> p2 = param_of<T>(optic->p[2], 1.0);
        const int leak = (optic->flags & PM_JONES_LEAKAGE_IDENTITY) ? 1 : 0;
        return by_layout(out_layout, [&](auto planes) {
            constexpr bool P = decltype(planes)::value;
            auto run = [&](auto k) {
                constexpr int K = decltype(k)::value;
                using Op = OpticOp<T, K, P>;
                Op op{p0, p1, p2, T(charge), leak, static_cast<const cx<T>*>(field), field_ld, view_of<T, Op::NC, P>(out, out_ld, out_pstride)};
                return sweep_heavy(rows, cols, PM_STREAM(stream), op);
            };
            switch (kind) {
                case PM_JONES_ROTATION: return run(std::integral_constant<int, PM_JONES_ROTATION>{});
                case PM_JONES_RETARDER: return run(std::integral_constant<int, PM_JONES_RETARDER>{});
                case PM_JONES_DIATTENUATOR: return run(std::integral_constant<int, PM_JONES_DIATTENUATOR>{});
                case PM_JONES_VORTEX: return run(std::integral_constant<int, PM_JONES_VORTEX>{});
                default: return run(std::integral_constant<int, PM_JONES_LINPOL_VECTOR>{});
            }
        });
    });
}

int pm_jones_chain(int32_t dtype, int32_t count, const pm_jones_operand* operands, int32_t layout, int32_t vector_tail, int64_t rows, int64_t cols,
                   void* out, int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream) {
    const char* who = "pm_jones_chain";
    if (count < 1 || count > PM_JONES_MAX_CHAIN) return fail(PM_ERR_ARG, "%s: the count of operands must be 1 ... %d", who, PM_JONES_MAX_CHAIN);
    if (!operands) return fail(PM_ERR_ARG, "%s: bad argument (null operands)", who);
    if (!layout_ok(layout) || !layout_ok(out_layout)) return fail(PM_ERR_ARG, "%s: the layout must be PM_JONES_AOS or PM_JONES_PLANES", who);
    if (const int rc = check_shape(who, rows, cols)) return rc < 0 ? rc : 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        if (const int rc = check_view(who, out, out_layout, vector_tail ? 2 : 4, rows, cols, out_ld, out_pstride, 2 * sizeof(T))) return rc;
        Operand<T> ops[PM_JONES_MAX_CHAIN] = {};
        for (int i = 0; i < count; ++i) {
            const pm_jones_operand& o = operands[i];
            const int ncomp = vector_tail && i == count - 1 ? 2 : 4;
            if (o.map)
                if (const int rc = check_view(who, o.map, layout, ncomp, rows, cols, o.ld, o.pstride, 2 * sizeof(T))) return rc;
            ops[i] = Operand<T>{static_cast<const cx<T>*>(o.map), o.ld, o.pstride, int(aligned(o.map, 16)), {}};
            for (int j = 0; j < 4; ++j) ops[i].k[j] = cx<T>{T(o.c[2 * j]), T(o.c[2 * j + 1])};
        }
        return by_layout(layout, [&](auto pin) {
            return by_layout(out_layout, [&](auto pout) {
                constexpr bool PI = decltype(pin)::value, PO = decltype(pout)::value;
                auto run = [&](auto vec) {
                    constexpr bool V = decltype(vec)::value;
                    ChainOp<T, PI, PO, V> op;
                    op.count = count;
                    for (int i = 0; i < PM_JONES_MAX_CHAIN; ++i) op.op[i] = ops[i];
                    op.out = view_of<T, V ? 2 : 4, PO>(out, out_ld, out_pstride);
                    return sweep_heavy(rows, cols, PM_STREAM(stream), op);
                };
                return vector_tail ? run(std::true_type{}) : run(std::false_type{});
            });
        });
    });
}

int pm_jones_scale(int32_t dtype, int32_t ncomp, int64_t rows, int64_t cols, const void* in, int32_t layout, int64_t ld, int64_t pstride,
                   int32_t field_kind, const void* field, int64_t field_ld, void* out, int32_t out_layout, int64_t out_ld, int64_t out_pstride,
                   void* stream) {
    const char* who = "pm_jones_scale";
    if (ncomp != 2 && ncomp != 4) return fail(PM_ERR_ARG, "%s: the components per pixel must be 4 (a matrix) or 2 (a vector)", who);
    if (!layout_ok(layout) || !layout_ok(out_layout)) return fail(PM_ERR_ARG, "%s: the layout must be PM_JONES_AOS or PM_JONES_PLANES", who);
    if (field_kind != PM_JONES_FIELD_NONE && field_kind != PM_JONES_FIELD_REAL && field_kind != PM_JONES_FIELD_COMPLEX)
        return fail(PM_ERR_ARG, "%s: field_kind must be PM_JONES_FIELD_NONE, PM_JONES_FIELD_REAL or PM_JONES_FIELD_COMPLEX", who);
    if (const int rc = check_shape(who, rows, cols)) return rc < 0 ? rc : 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        if (const int rc = check_view(who, in, layout, ncomp, rows, cols, ld, pstride, 2 * sizeof(T))) return rc;
        if (const int rc = check_view(who, out, out_layout, ncomp, rows, cols, out_ld, out_pstride, 2 * sizeof(T))) return rc;
        if (field_kind != PM_JONES_FIELD_NONE) {
            if (!field) return fail(PM_ERR_ARG, "%s: the field is missing (null pointer)", who);
            PM_CHECK_LD("pm_jones_scale", ld_ok(rows, cols, field_ld));
            if (!aligned(field, field_kind == PM_JONES_FIELD_REAL ? sizeof(T) : 2 * sizeof(T)))
                return fail(PM_ERR_ARG, "%s: an array is not aligned like its elements", who);
        }
        if (in == out && (layout != out_layout || ld != out_ld || (layout == PM_JONES_PLANES && pstride != out_pstride)))
            return fail(PM_ERR_ARG, "%s: in place needs the same layout and strides on both sides", who);
        return by_layout(layout, [&](auto pin) {
            return by_layout(out_layout, [&](auto pout) {
                constexpr bool PI = decltype(pin)::value, PO = decltype(pout)::value;
                auto run = [&](auto nc) {
                    constexpr int NC = decltype(nc)::value;
                    ScaleOp<T, NC, PI, PO> op{view_of<T, NC, PI>(in, ld, pstride), int(field_kind), field, field_ld, view_of<T, NC, PO>(out, out_ld, out_pstride)};
                    return sweep(rows, cols, PM_STREAM(stream), op);
                };
                return ncomp == 4 ? run(std::integral_constant<int, 4>{}) : run(std::integral_constant<int, 2>{});
            });
        });
    });
}

int pm_jones_to_mueller(int32_t dtype, int64_t rows, int64_t cols, const void* jones, int32_t layout, int64_t ld, int64_t pstride, void* out,
                        int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream) {
    const char* who = "pm_jones_to_mueller";
    if (!layout_ok(layout) || !layout_ok(out_layout)) return fail(PM_ERR_ARG, "%s: the layout must be PM_JONES_AOS or PM_JONES_PLANES", who);
    if (const int rc = check_shape(who, rows, cols)) return rc < 0 ? rc : 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        if (const int rc = check_view(who, jones, layout, 4, rows, cols, ld, pstride, 2 * sizeof(T))) return rc;
        if (const int rc = check_view(who, out, out_layout, 16, rows, cols, out_ld, out_pstride, sizeof(T))) return rc;
        return by_layout(layout, [&](auto pin) {
            return by_layout(out_layout, [&](auto pout) {
                constexpr bool PI = decltype(pin)::value, PO = decltype(pout)::value;
                MuellerOp<T, PI, PO> op{view_of<T, 4, PI>(jones, ld, pstride), static_cast<T*>(out), out_ld, out_pstride, int(aligned(out, 16))};
                return sweep(rows, cols, PM_STREAM(stream), op);
            });
        });
    });
}

int pm_pauli_coefficients(int32_t dtype, int64_t rows, int64_t cols, const void* jones, int32_t layout, int64_t ld, int64_t pstride, void* out,
                          int64_t out_ld, int64_t out_pstride, void* stream) {
    const char* who = "pm_pauli_coefficients";
    if (!layout_ok(layout)) return fail(PM_ERR_ARG, "%s: the layout must be PM_JONES_AOS or PM_JONES_PLANES", who);
    if (const int rc = check_shape(who, rows, cols)) return rc < 0 ? rc : 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        if (const int rc = check_view(who, jones, layout, 4, rows, cols, ld, pstride, 2 * sizeof(T))) return rc;
        if (const int rc = check_view(who, out, PM_JONES_PLANES, 4, rows, cols, out_ld, out_pstride, 2 * sizeof(T))) return rc;
        return by_layout(layout, [&](auto pin) {
            constexpr bool PI = decltype(pin)::value;
            PauliOp<T, PI> op{view_of<T, 4, PI>(jones, ld, pstride), view_of<T, 4, true>(out, out_ld, out_pstride)};
            return sweep(rows, cols, PM_STREAM(stream), op);
        });
    });
}

}  // extern "C"
