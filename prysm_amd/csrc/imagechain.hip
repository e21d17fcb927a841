// The image chain between the PSF and the detector (prysm/objects.py, prysm/degradations.py, prysm/psf.py,
// prysm/coordinates.py uniform_cart_to_polar) (gfx950):
//
//  - pm_object_render: a target (slit, pinhole, Siemens star, tilted square, slanted edge) from a kind code and a small parameter
//    record, one launch, each sample stored once.  The coordinates come from the pixel index, from two vectors or from two arrays
//    and are read once; polar targets take (r, t) arrays as they are or form them from x and y in registers.
//  - pm_tf_product: H = the product of up to 16 analytic transfer functions and user maps, walked per sample from a table in the
//    kernel arguments (scalar loads, the same for every lane) and stored once, complex or real, with its origin at [0, 0]: centred
//    inputs are reached through an index rotation.  The frequencies come from (dx, n) as fttools.forward_ft_unit makes them -- the
//    integer of the bin times 1 / (n dx) in double, rounded once to the working precision -- or from vectors or arrays.
//  - pm_polar_resample: the bilinear gather of uniform_cart_to_polar.
//  - pm_centroid: sum d, sum row d, sum col d in double; pm_psf_size: the maximum of a polar map, the threshold crossing of each
//    row (one wavefront per row) and their mean.  Partials per workgroup in a workspace, folded in a fixed order by a second launch
//    (both stages: pm_reduce.h): no atomics, the same bits every run, nothing read on the host.
//
// The pointwise kernels ride on pm_sweep.h.  The unit is compiled with -ffp-contract=off (csrc/Makefile): every product and sum is
// rounded by itself, in the order written, which prysm_amd/imagechain_plan.py restates in numpy.  J1 is the Chebyshev series of
// csrc/fibers_coefs.h (for x <= 8 the series J1S is J1(x) / x itself).
#include <cmath>

#include "fibers_coefs.h"
#include "pm_entry.h"
#include "pm_math.h"
#include "pm_reduce.h"
#include "pm_sweep.h"

namespace pm {
namespace {

constexpr double kPi = 3.141592653589793;

// sum_k c_k T_k(t) by Clenshaw, the first N32 terms in float (the walk of csrc/fibers.hip over the same tables)
#define PM_IC_SERIES(NAME)                                                                                             \
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
PM_IC_SERIES(J1S)
PM_IC_SERIES(P1)
PM_IC_SERIES(Q1)
#undef PM_IC_SERIES

// J1(x) / x, even in x; 0.5 below 1e-8 as the reference sets it (the series gives 0.5 there to within one rounding)
template <typename T>
__device__ __forceinline__ T jinc_(T x) {
    const T ax = abs_(x);
    if (ax < T(1e-8)) return T(0.5);
    if (ax <= T(8)) return cheb_J1S(ax * ax * T(0.03125) - T(1));
    const T z = T(8) / ax;
    const T t = T(2) * (z * z) - T(1);
    T s, c;
    sincos_(ax, &s, &c);
    const T amp = sqrt_(T(0.6366197723675814) / ax);
    const T c0 = (c + s) * T(0.7071067811865476), s0 = (s - c) * T(0.7071067811865476);
    return amp * (cheb_P1(t) * s0 + z * cheb_Q1(t) * c0) / ax;
}

// numpy's sinc: sin(pi a) / (pi a), 1 at 0
template <typename T>
__device__ __forceinline__ T sinc_(T a) {
    if (a == T(0)) return T(1);
    const T y = T(kPi) * a;
    return sin_(y) / y;
}

// ---------------------------------------------------------------- targets
// where the two coordinates of sample (r, c) come from
template <typename T>
struct Coords {
    int mode;
    const T* a;      // x, or r when the arrays are polar
    const T* b;      // y, or t
    int64_t lda, ldb;      // POINTWISE: elements between rows; SEPARABLE: ldb = elements between the values of y
    int64_t ox, oy;
    T dx;
    __device__ __forceinline__ T first(int64_t r, int64_t c) const {
        return mode == PM_COORDS_GRID ? T(c - ox) * dx : mode == PM_COORDS_SEPARABLE ? a[c] : a[r * lda + c];
    }
    __device__ __forceinline__ T second(int64_t r, int64_t c) const {
        return mode == PM_COORDS_GRID ? T(r - oy) * dx : mode == PM_COORDS_SEPARABLE ? b[r * ldb] : b[r * ldb + c];
    }
};

// The polar coordinates a target forms in registers are formed, and used, in double whatever the working precision: a Siemens
// star's cosine is zero along whole lines of a grid (the diagonals, for a multiple of four spokes), where a float angle times
// spokes / 2 decides the sample by its last bit.  (r, t) arrays given by the caller are used in their own precision.
__device__ __forceinline__ double radius_of(double x, double y) { return hypot(x, y); }
__device__ __forceinline__ double angle_of(double x, double y) { return atan2(y, x); }

// O = uint8_t: slit and pinhole masks; O = T: the others
template <typename T, typename O>
struct ObjectOp {
    Coords<T> co;
    int kind, flags, polar;     // polar: the arrays hold (r, t)
    T p[8];
    int64_t n;                  // the square grid of the crossed edge
    O* out;
    int64_t ld;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ bool edge(int64_t r, int64_t c) const {
        return co.first(r, c) * p[0] - co.second(r, c) * p[1] > T(0);
    }

    // the star at (rho, t), computed in C
    template <typename C>
    __device__ __forceinline__ T star(C rho, C t) const {
        C a = C(p[1]) * cos_(C(p[0]) * t);
        a = (a + C(1)) / C(2);
        if (rho > C(p[2]) || rho < C(p[3])) a = C(p[4]);
        if (flags & PM_OBJECT_BINARY) {       // after the background, as the reference does: a black background becomes `bottom`
            if (a < C(0.5)) a = C(p[5]);
            if (a > C(0.5)) a = C(p[6]);
        }
        return T(a);
    }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        O v;
        if constexpr (sizeof(O) == 1) {
            if (kind == PM_OBJECT_SLIT) {
                bool in = false;
                if (flags & PM_OBJECT_SLIT_X) in = abs_(co.first(r, c)) <= p[0];
                if (flags & PM_OBJECT_SLIT_Y) in = in || abs_(co.second(r, c)) <= p[1];
                v = O(in);
            } else {
                v = polar ? O(co.first(r, c) <= p[0]) : O(radius_of(co.first(r, c), co.second(r, c)) <= double(p[0]));
            }
        } else {
            switch (kind) {
            case PM_OBJECT_SIEMENSSTAR: {
                const T x = co.first(r, c), y = co.second(r, c);
                v = polar ? star<T>(x, y) : star<double>(radius_of(x, y), angle_of(x, y));
            } break;
            case PM_OBJECT_TILTEDSQUARE: {
                const T x = co.first(r, c), y = co.second(r, c);
                const T xp = x * p[0] - y * p[1], yp = x * p[1] + y * p[0];
                v = (abs_(xp) <= p[2] && abs_(yp) <= p[2]) ? p[3] : p[4];
            } break;
            default: {      // PM_OBJECT_SLANTEDEDGE
                bool m;
                if (flags & PM_OBJECT_CROSSED) {
                    const int64_t last = n - 1;
                    m = (edge(r, c) && edge(c, last - r)) || (edge(last - r, last - c) && edge(last - c, r));
                } else {
                    m = edge(r, c);
                }
                v = m ? p[2] : p[3];
            } break;
            }
        }
        out[r * ld + c] = v;
    }
};

// ---------------------------------------------------------------- transfer functions
template <typename T>
struct TfOp {
    int nrec;
    pm_tf_record rec[PM_TF_MAX_RECORDS];
    int fmode;
    const T* fx;
    const T* fy;
    const T* fr;
    int64_t ldx, ldy, ldr;
    double valx, valy;   // 1 / (n dx), 1 / (m dx): numpy's fftfreq forms the frequency as integer * that
    int64_t m, n, sy, sx;     // the inputs' origin: (sy, sx) = (m / 2, n / 2) when they are centred, else 0
    int need_x, need_y, need_r;      // which frequencies the records read: each is formed once per sample
    int out_complex;
    void* out;
    int64_t ld;

    struct Col {
        int64_t sc;
    };

    // the frequencies at SOURCE index i (the order the inputs are in)
    __device__ __forceinline__ T gen(int64_t i, int64_t s, int64_t len, double v) const {
        int64_t o = i - s;
        if (o < 0) o += len;
        const int64_t k = o < (len + 1) / 2 ? o : o - len;
        return T(double(k) * v);
    }
    __device__ __forceinline__ T freq_x(int64_t sr, int64_t sc) const {
        return fmode == PM_FREQ_GRID ? gen(sc, sx, n, valx) : fmode == PM_FREQ_VECTORS ? fx[sc] : fx[sr * ldx + sc];
    }
    __device__ __forceinline__ T freq_y(int64_t sr, int64_t sc) const {
        return fmode == PM_FREQ_GRID ? gen(sr, sy, m, valy) : fmode == PM_FREQ_VECTORS ? fy[sr * ldy] : fy[sr * ldy + sc];
    }
    __device__ __forceinline__ Col column(int64_t c) const {
        int64_t sc = c + sx;
        if (sc >= n) sc -= n;
        return {sc};
    }

    __device__ __forceinline__ void point(int64_t r, int64_t c, Col col) const {
        const int64_t sc = col.sc;
        int64_t sr = r + sy;
        if (sr >= m) sr -= m;
        const T fxv = need_x ? freq_x(sr, sc) : T(0), fyv = need_y ? freq_y(sr, sc) : T(0);
        T frv = T(0);
        if (need_r) frv = (fmode == PM_FREQ_POINTWISE && fr) ? fr[sr * ldr + sc] : hypot_(fxv, fyv);
        T re = T(1), im = T(0);
        for (int i = 0; i < nrec; ++i) {
            const pm_tf_record& q = rec[i];
            T v = T(1);
            switch (q.kind) {
            case PM_TFP_SINC_X: v = sinc_(fxv * T(q.p[0])); break;
            case PM_TFP_SINC_Y: v = sinc_(fyv * T(q.p[0])); break;
            case PM_TFP_COS_X: v = cos_(T(q.p[0]) * fxv); break;
            case PM_TFP_COS_Y: v = cos_(T(q.p[0]) * fyv); break;
            case PM_TFP_GAUSS_R: {
                const T core = T(q.p[0]) * frv;
                v = exp_(T(-2) * core * core);
            } break;
            case PM_TFP_JINC_R: v = jinc_(frv * T(q.p[0])); break;
            case PM_TFP_AIRY_FT_R: {
                T s = abs_(frv) / T(q.p[0]);
                if (s > T(1)) s = T(1);
                v = T(2 / kPi) * (acos_(s) - s * sqrt_(T(1) - s * s));
            } break;
            case PM_TFP_AIRY_R:
            case PM_TFP_AIRY_EFIELD_R: {
                const T u = frv * T(kPi) / T(q.p[0]) / T(q.p[1]);
                const T e = T(2) * jinc_(u);
                v = q.kind == PM_TFP_AIRY_R ? abs_(e) * abs_(e) : e;
            } break;
            case PM_TFP_SLIT_FT: {
                const T wx = T(q.p[0]), wy = T(q.p[1]);
                if (q.flags == (PM_OBJECT_SLIT_X | PM_OBJECT_SLIT_Y)) {
                    // the grid lengths from the spacing of the first two frequencies, as the reference recovers them
                    const T Lx = T(1) / (freq_x(0, 1) - freq_x(0, 0)), Ly = T(1) / (freq_y(1, 0) - freq_y(0, 0));
                    const T sx_ = sinc_(fxv * wx), sy_ = sinc_(fyv * wy);
                    const T bx = (wx * Ly) * sx_ * T(fyv == T(0)), by = (wy * Lx) * sy_ * T(fxv == T(0));
                    const T ov = T(q.p[0] * q.p[1]) * sx_ * sy_;
                    const T area = wx * Ly + wy * Lx - T(q.p[0] * q.p[1]);
                    v = (bx + by - ov) / area;
                } else if (q.flags == PM_OBJECT_SLIT_X) {
                    v = sinc_(fxv * wx) * T(fyv == T(0));
                } else {
                    v = sinc_(fyv * wy) * T(fxv == T(0));
                }
            } break;
            case PM_TFP_MAP_REAL: v = static_cast<const T*>(q.ptr)[sr * q.ld + sc]; break;
            case PM_TFP_MAP_COMPLEX: {
                const cx<T> w = static_cast<const cx<T>*>(q.ptr)[sr * q.ld + sc];
                const T nr = re * w.x - im * w.y, ni = re * w.y + im * w.x;
                re = nr;
                im = ni;
                continue;
            }
            default: break;
            }
            re = re * v;
            im = im * v;
        }
        if (out_complex)
            static_cast<cx<T>*>(out)[r * ld + c] = cx<T>{re, im};
        else
            static_cast<T*>(out)[r * ld + c] = re;
    }
};

// ---------------------------------------------------------------- uniform_cart_to_polar
// the cell of q on a sorted, regular axis g of len values: the guess from the spacing, then at most one step either way, so that
// g[i] <= q < g[i + 1] (the last cell is closed above)
template <typename T>
__device__ __forceinline__ int64_t cell_of(const T* __restrict__ g, int64_t len, T inv, T q) {
    int64_t i = int64_t((q - g[0]) * inv);
    i = i < 0 ? 0 : (i > len - 2 ? len - 2 : i);
    if (i > 0 && q < g[i]) --i;
    if (i < len - 2 && q >= g[i + 1]) ++i;
    return i;
}

template <typename T>
struct PolarOp {
    const T* x;      // nx
    const T* y;      // ny
    const T* rho;    // nx
    const T* phi;    // ny
    T invx, invy;
    int64_t ny, nx;
    const T* data;
    int64_t dld;
    T* out;
    int64_t ld;

    __device__ __forceinline__ T column(int64_t c) const { return rho[c]; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, T rv) const {
        T sn, cs;
        sincos_(phi[r], &sn, &cs);
        const T xq = rv * cs, yq = rv * sn;
        T v = T(0);
        // outside [min, max] of either axis is the fill value; the boundary is inside.  !(a && b) also sends NaN there
        if (xq >= x[0] && xq <= x[nx - 1] && yq >= y[0] && yq <= y[ny - 1]) {
            const int64_t ix = cell_of(x, nx, invx, xq), iy = cell_of(y, ny, invy, yq);
            const T tx = (xq - x[ix]) / (x[ix + 1] - x[ix]), ty = (yq - y[iy]) / (y[iy + 1] - y[iy]);
            const T* __restrict__ d0 = data + iy * dld + ix;
            const T* __restrict__ d1 = d0 + dld;
            const T ux = T(1) - tx, uy = T(1) - ty;
            v = d0[0] * (uy * ux);
            v = v + d0[1] * (uy * tx);
            v = v + d1[0] * (ty * ux);
            v = v + d1[1] * (ty * tx);
        }
        out[r * ld + c] = v;
    }
};

// ---------------------------------------------------------------- reductions
constexpr int kRedThreads = 256;
constexpr int kRedWgs = 1024;        // most workgroups of a reduction pass: as many partials per sum
constexpr int kCrossWaves = kRedThreads / 64;
constexpr int kCrossWgs = 1024;      // most workgroups of the crossing pass, kCrossWaves rows each per trip

int red_groups(int64_t n) { return reduce_groups(n, kRedThreads, kRedWgs); }
int cross_groups(int64_t rows) { return reduce_groups(rows, kCrossWaves, kCrossWgs); }

// pass A over an m x n array (rows ld apart): MAX: the maximum; else sum d, sum row d, sum col d.  partial[wg * NS + k]
template <typename T, bool MAX>
__global__ __launch_bounds__(kRedThreads) void reduce_kernel(int64_t m, int64_t n, const T* __restrict__ d, int64_t ld,
                                                             double* __restrict__ partial) {
    constexpr int NS = MAX ? 1 : 3;
    using Op = std::conditional_t<MAX, FoldMax, FoldSum>;
    double a[NS];
    a[0] = MAX ? -INFINITY : 0.0;
    if constexpr (!MAX) a[1] = a[2] = 0.0;
    const int64_t total = m * n, stride = int64_t(gridDim.x) * kRedThreads;
    for (int64_t i = int64_t(blockIdx.x) * kRedThreads + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / n, c = i - r * n;
        const double v = double(d[r * ld + c]);
        if constexpr (MAX) {
            a[0] = v > a[0] ? v : a[0];
        } else {
            a[0] = a[0] + v;
            a[1] = a[1] + double(r) * v;
            a[2] = a[2] + double(c) * v;
        }
    }
    wg_fold<kRedThreads, Op>(threadIdx.x, a, partial + int64_t(blockIdx.x) * NS);
}

// pass B, one workgroup: the partials in a fixed order.  Centroid: out = (sum row d / sum d, sum col d / sum d).
__global__ __launch_bounds__(kRedThreads) void centroid_fold_kernel(int nparts, const double* __restrict__ partial, double* __restrict__ out) {
    double tot[3];
    fold_partials<kRedThreads, FoldSum>(threadIdx.x, nparts, partial, 0.0, tot);
    if (threadIdx.x == 0) {
        out[0] = tot[1] / tot[0];
        out[1] = tot[2] / tot[0];
    }
}

// pass B of the maximum: the threshold hm in T, as a double, to sc[0].  relative: hm = T(value) * max, else hm = T(value)
template <typename T>
__global__ __launch_bounds__(kRedThreads) void threshold_fold_kernel(int nparts, const double* __restrict__ partial, int relative, double value,
                                                                     double* __restrict__ sc) {
    double tot[1];
    fold_partials<kRedThreads, FoldMax>(threadIdx.x, nparts, partial, -INFINITY, tot);
    if (threadIdx.x == 0) sc[0] = relative ? double(T(value) * T(tot[0])) : double(T(value));
}

// one wavefront per row of the polar map: the first (last = 0) or last index i where (p[i] > hm) != (p[i + 1] > hm), and the radius
// interpolated there, r[i] + frac (r[i + 1] - r[i]) in double with frac = (hm - p[i]) / (p[i + 1] - p[i]) in T (0 when the two are
// equal).  cross[row] = the radius, has[row] = 1, or both 0 where the row has no crossing.
template <typename T>
__global__ __launch_bounds__(kRedThreads) void crossing_kernel(int64_t rows, int64_t cols, const T* __restrict__ polar, int64_t ld,
                                                               const T* __restrict__ rad, int last, const double* __restrict__ sc,
                                                               double* __restrict__ cross, double* __restrict__ has) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const T hm = T(sc[0]);
    for (int64_t row = int64_t(blockIdx.x) * kCrossWaves + wave; row < rows; row += int64_t(gridDim.x) * kCrossWaves) {
        const T* __restrict__ p = polar + row * ld;
        int64_t best = -1;
        for (int64_t j = lane; j + 1 < cols; j += 64) {
            if ((p[j] > hm) != (p[j + 1] > hm)) {
                if (last)
                    best = j;
                else if (best < 0)
                    best = j;
            }
        }
        // -1 is "none": the last crossing is the largest index; the first the smallest one that is not -1
        for (int off = 32; off > 0; off >>= 1) {
            const int64_t other = __shfl_xor(best, off, 64);
            if (last)
                best = other > best ? other : best;
            else
                best = best < 0 ? other : (other >= 0 && other < best ? other : best);
        }
        if (lane == 0) {
            double rc = 0.0, h = 0.0;
            if (best >= 0) {
                const T y0 = p[best], y1 = p[best + 1];
                const T frac = y1 == y0 ? T(0) : (hm - y0) / (y1 - y0);
                const double r0 = double(rad[best]), r1 = double(rad[best + 1]);
                rc = r0 + double(frac) * (r1 - r0);
                h = 1.0;
            }
            cross[row] = rc;
            has[row] = h;
        }
    }
}

// one workgroup: out = (mean of the crossings, their count); a mean of 0 when there is none
__global__ __launch_bounds__(kRedThreads) void crossing_mean_kernel(int64_t rows, const double* __restrict__ cross, const double* __restrict__ has,
                                                                    double* __restrict__ out) {
    double a[2] = {0.0, 0.0}, tot[2];
    for (int64_t i = threadIdx.x; i < rows; i += kRedThreads) {
        a[0] = a[0] + cross[i];
        a[1] = a[1] + has[i];
    }
    wg_total<kRedThreads, FoldSum>(threadIdx.x, a, tot);
    if (threadIdx.x == 0) {
        out[0] = tot[1] > 0.0 ? tot[0] / tot[1] : 0.0;
        out[1] = tot[1];
    }
}

// workspace of pm_psf_size in doubles: [hm | maximum partials (kRedWgs) | cross (rows) | has (rows)]
size_t size_doubles(int64_t rows) { return size_t(1) + size_t(kRedWgs) + 2 * size_t(rows); }

bool too_large(int64_t m, int64_t n) { return m > INT32_MAX || n > INT32_MAX; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_object_render(int32_t dtype, int32_t coords, int32_t polar, int64_t ny, int64_t nx, const void* a, int64_t lda, const void* b,
                     int64_t ldb, double dx, const pm_object* obj, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_object_render";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (coords != PM_COORDS_GRID && coords != PM_COORDS_SEPARABLE && coords != PM_COORDS_POINTWISE)
        return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID, PM_COORDS_SEPARABLE or PM_COORDS_POINTWISE", who);
    if (ny < 0 || nx < 0 || !obj || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    const int kind = obj->kind, flags = obj->flags;
    if (kind < PM_OBJECT_SLIT || kind > PM_OBJECT_SLANTEDEDGE) return fail(PM_ERR_ARG, "%s: unknown target kind %d", who, kind);
    // which of the two coordinates the target reads
    const bool pinhole_rho = kind == PM_OBJECT_PINHOLE && polar;
    bool need_a = true, need_b = !pinhole_rho;
    if (kind == PM_OBJECT_SLIT) {
        if (!(flags & (PM_OBJECT_SLIT_X | PM_OBJECT_SLIT_Y))) need_a = need_b = false;
        else need_a = flags & PM_OBJECT_SLIT_X, need_b = flags & PM_OBJECT_SLIT_Y;
    }
    if (polar && (coords != PM_COORDS_POINTWISE || (kind != PM_OBJECT_PINHOLE && kind != PM_OBJECT_SIEMENSSTAR)))
        return fail(PM_ERR_ARG, "%s: (r, t) arrays are for the pinhole and the Siemens star, as PM_COORDS_POINTWISE", who);
    if (coords != PM_COORDS_GRID && ((need_a && !a) || (need_b && !b))) return fail(PM_ERR_ARG, "%s: coordinate arrays are missing (null pointer)", who);
    if (coords == PM_COORDS_GRID && !std::isfinite(dx)) return fail(PM_ERR_ARG, "%s: the grid spacing must be finite", who);
    if (coords == PM_COORDS_POINTWISE) PM_CHECK_LD("pm_object_render", (!need_a || ld_ok(ny, nx, lda)) && (!need_b || ld_ok(ny, nx, ldb)));
    PM_CHECK_LD("pm_object_render", ld_ok(ny, nx, out_ld));
    if (kind == PM_OBJECT_SLANTEDEDGE && (flags & PM_OBJECT_CROSSED) && ny != nx)
        return fail(PM_ERR_ARG, "%s: crossed edges need a square grid, got %lld x %lld", who, (long long)ny, (long long)nx);
    if (too_large(ny, nx)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)ny, (long long)nx);
    if (ny == 0 || nx == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        Coords<T> co{coords, static_cast<const T*>(a), static_cast<const T*>(b), lda, ldb, nx / 2, ny / 2, T(dx)};
        auto run = [&](auto o) {
            using O = decltype(o);
            ObjectOp<T, O> op;
            op.co = co, op.kind = kind, op.flags = flags, op.polar = polar != 0, op.n = nx, op.out = static_cast<O*>(out), op.ld = out_ld;
            for (int k = 0; k < 8; ++k) op.p[k] = T(obj->p[k]);
            return sweep_heavy(ny, nx, PM_STREAM(stream), op);
        };
        return (kind == PM_OBJECT_SLIT || kind == PM_OBJECT_PINHOLE) ? run(uint8_t{}) : run(T{});
    });
}

int pm_tf_product(int32_t dtype, int64_t m, int64_t n, const pm_tf_freq* freq, const pm_tf_record* records, int64_t nrec, int32_t out_complex,
                  void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_tf_product";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (m < 0 || n < 0 || nrec < 0 || !freq || !out || (nrec && !records)) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (nrec > PM_TF_MAX_RECORDS) return fail(PM_ERR_ARG, "%s: %lld records, at most %d", who, (long long)nrec, PM_TF_MAX_RECORDS);
    const int fmode = freq->mode;
    if (fmode != PM_FREQ_GRID && fmode != PM_FREQ_VECTORS && fmode != PM_FREQ_POINTWISE)
        return fail(PM_ERR_ARG, "%s: the frequency mode must be PM_FREQ_GRID, PM_FREQ_VECTORS or PM_FREQ_POINTWISE", who);
    if (fmode == PM_FREQ_GRID && !(std::isfinite(freq->dx) && freq->dx != 0)) return fail(PM_ERR_ARG, "%s: the sample spacing must be finite and nonzero", who);
    PM_CHECK_LD("pm_tf_product", ld_ok(m, n, out_ld));
    bool need_x = false, need_y = false, need_r = false;
    for (int64_t i = 0; i < nrec; ++i) {
        const pm_tf_record& q = records[i];
        switch (q.kind) {
        case PM_TFP_SINC_X: case PM_TFP_COS_X: need_x = true; break;
        case PM_TFP_SINC_Y: case PM_TFP_COS_Y: need_y = true; break;
        case PM_TFP_GAUSS_R: case PM_TFP_JINC_R: case PM_TFP_AIRY_FT_R: case PM_TFP_AIRY_R: case PM_TFP_AIRY_EFIELD_R: need_r = true; break;
        case PM_TFP_SLIT_FT:
            need_x = need_y = true;
            if (!(q.flags & (PM_OBJECT_SLIT_X | PM_OBJECT_SLIT_Y)) || (q.flags & ~(PM_OBJECT_SLIT_X | PM_OBJECT_SLIT_Y)))
                return fail(PM_ERR_ARG, "%s: record %lld: a slit needs a width in x, in y or in both", who, (long long)i);
            if (q.flags == (PM_OBJECT_SLIT_X | PM_OBJECT_SLIT_Y) && (m < 2 || n < 2))
                return fail(PM_ERR_ARG, "%s: record %lld: crossed slits recover the grid lengths from two frequencies per axis", who, (long long)i);
            break;
        case PM_TFP_MAP_REAL: case PM_TFP_MAP_COMPLEX:
            if (!q.ptr) return fail(PM_ERR_ARG, "%s: record %lld: the map is a null pointer", who, (long long)i);
            PM_CHECK_LD("pm_tf_product", ld_ok(m, n, q.ld));
            if (q.kind == PM_TFP_MAP_COMPLEX && !out_complex) return fail(PM_ERR_ARG, "%s: record %lld: a complex map needs a complex output", who, (long long)i);
            break;
        default: return fail(PM_ERR_ARG, "%s: record %lld: unknown kind %d", who, (long long)i, int(q.kind));
        }
    }
    if (fmode == PM_FREQ_POINTWISE && need_r && !freq->fr) need_x = need_y = true;
    if (fmode != PM_FREQ_POINTWISE && need_r) need_x = need_y = true;
    if (fmode != PM_FREQ_GRID && ((need_x && !freq->fx) || (need_y && !freq->fy)))
        return fail(PM_ERR_ARG, "%s: a record reads a frequency array that is missing (null pointer)", who);
    if (fmode == PM_FREQ_POINTWISE)
        PM_CHECK_LD("pm_tf_product", (!need_x || ld_ok(m, n, freq->ldx)) && (!need_y || ld_ok(m, n, freq->ldy)) && (!freq->fr || ld_ok(m, n, freq->ldr)));
    if (too_large(m, n)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)m, (long long)n);
    if (m == 0 || n == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        TfOp<T> op;
        op.nrec = int(nrec);
        for (int64_t i = 0; i < nrec; ++i) op.rec[i] = records[i];
        op.fmode = fmode;
        op.fx = static_cast<const T*>(freq->fx), op.fy = static_cast<const T*>(freq->fy), op.fr = static_cast<const T*>(freq->fr);
        op.ldx = freq->ldx, op.ldy = freq->ldy, op.ldr = freq->ldr;
        op.valx = fmode == PM_FREQ_GRID ? 1.0 / (double(n) * freq->dx) : 0.0;
        op.valy = fmode == PM_FREQ_GRID ? 1.0 / (double(m) * freq->dx) : 0.0;
        op.m = m, op.n = n, op.sy = freq->shift ? m / 2 : 0, op.sx = freq->shift ? n / 2 : 0;
        op.need_x = need_x, op.need_y = need_y, op.need_r = need_r;
        op.out_complex = out_complex != 0, op.out = out, op.ld = out_ld;
        return sweep_heavy(m, n, PM_STREAM(stream), op);
    });
}

int pm_polar_resample(int32_t dtype, int64_t ny, int64_t nx, const void* x, const void* y, double x_step, double y_step, const void* rho,
                      const void* phi, const void* data, int64_t data_ld, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_polar_resample";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (ny < 0 || nx < 0 || !x || !y || !rho || !phi || !data || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if ((ny > 0 && ny < 2) || (nx > 0 && nx < 2)) return fail(PM_ERR_ARG, "%s: an axis needs at least two samples to interpolate between", who);
    if (!(std::isfinite(x_step) && x_step > 0 && std::isfinite(y_step) && y_step > 0))
        return fail(PM_ERR_ARG, "%s: the axes must ascend: their spacings must be finite and positive", who);
    PM_CHECK_LD("pm_polar_resample", ld_ok(ny, nx, data_ld) && ld_ok(ny, nx, out_ld));
    if (too_large(ny, nx)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)ny, (long long)nx);
    if (ny == 0 || nx == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        PolarOp<T> op{static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const T*>(rho), static_cast<const T*>(phi),
                      T(1.0 / x_step), T(1.0 / y_step), ny, nx, static_cast<const T*>(data), data_ld, static_cast<T*>(out), out_ld};
        return sweep(ny, nx, PM_STREAM(stream), op);
    });
}

size_t pm_centroid_workspace(int64_t m, int64_t n) {
    if (m <= 0 || n <= 0 || too_large(m, n)) return 0;
    return size_t(red_groups(m * n)) * 3 * sizeof(double);
}

int pm_centroid(int32_t dtype, int64_t m, int64_t n, const void* data, int64_t ld, void* out, void* workspace, size_t workspace_bytes,
                void* stream) {
    const char* who = "pm_centroid";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (m <= 0 || n <= 0 || !data || !out || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    PM_CHECK_LD("pm_centroid", ld_ok(m, n, ld));
    if (too_large(m, n)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)m, (long long)n);
    if (workspace_bytes < pm_centroid_workspace(m, n)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_centroid_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(out, 8)) return fail(PM_ERR_ARG, "%s: out and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        const int wgs = red_groups(m * n);
        double* part = static_cast<double*>(workspace);
        hipLaunchKernelGGL((reduce_kernel<T, false>), dim3(wgs), dim3(kRedThreads), 0, PM_STREAM(stream), m, n, static_cast<const T*>(data), ld, part);
        hipLaunchKernelGGL(centroid_fold_kernel, dim3(1), dim3(kRedThreads), 0, PM_STREAM(stream), wgs, part, static_cast<double*>(out));
        return int(hipGetLastError());
    });
}

size_t pm_psf_size_workspace(int64_t rows) { return rows <= 0 || rows > INT32_MAX ? 0 : size_doubles(rows) * sizeof(double); }

int64_t pm_psf_size_groups(int64_t rows) { return rows <= 0 ? 0 : cross_groups(rows); }

int pm_psf_size(int32_t dtype, int64_t rows, int64_t cols, const void* polar, int64_t ld, const void* r, int32_t relative, double value,
                int32_t last, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_psf_size";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (rows <= 0 || cols <= 0 || !polar || !r || !out || !workspace) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or empty array)", who);
    PM_CHECK_LD("pm_psf_size", ld_ok(rows, cols, ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (workspace_bytes < pm_psf_size_workspace(rows)) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_psf_size_workspace()", who);
    if (!aligned(workspace, 8) || !aligned(out, 8)) return fail(PM_ERR_ARG, "%s: out and the workspace hold doubles (8-byte alignment)", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        double* sc = static_cast<double*>(workspace);
        double* part = sc + 1;
        double* cross = part + kRedWgs;
        double* has = cross + rows;
        const int wgs = red_groups(rows * cols);
        const T* p = static_cast<const T*>(polar);
        hipLaunchKernelGGL((reduce_kernel<T, true>), dim3(wgs), dim3(kRedThreads), 0, st, rows, cols, p, ld, part);
        hipLaunchKernelGGL(threshold_fold_kernel<T>, dim3(1), dim3(kRedThreads), 0, st, wgs, part, relative != 0, value, sc);
        hipLaunchKernelGGL(crossing_kernel<T>, dim3(cross_groups(rows)), dim3(kRedThreads), 0, st, rows, cols, p, ld, static_cast<const T*>(r),
                           last != 0, sc, cross, has);
        hipLaunchKernelGGL(crossing_mean_kernel, dim3(1), dim3(kRedThreads), 0, st, rows, cross, has, static_cast<double*>(out));
        return int(hipGetLastError());
    });
}

}  // extern "C"
