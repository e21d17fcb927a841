// Coordinates and aperture geometry (prysm/coordinates.py, prysm/geometry.py) (gfx950):
//
//  - pm_xy_grid: make_xy_grid, both outputs from one launch (meshgrids or vectors).
//  - pm_cart_to_polar / pm_polar_to_cart: both outputs from one launch.
//  - pm_sdf_render: a whole aperture -- a tree of signed-distance shapes combined by union (min), intersect (max) and subtract
//    (max(d1, -d2)) -- evaluated per pixel in ONE launch and written once, as the distance, the `<= 0` mask or antialias's coverage.
//
// The aperture is a table of steps built on the host (prysm_amd/geometry_plan.py), the same for every lane: its index comes from
// kernel arguments, blockIdx and the loop counter only, so each step is read through the scalar cache and costs no vector memory
// traffic.  The tree is flattened at plan time: a step computes (part of) a primitive -- one polygon edge, one spider vane, or a
// whole circle / rectangle / ellipse -- and, at the primitive's last step, combines it into one of four NAMED accumulators chosen
// by a switch over constants, so there is no runtime-indexed register array and no scratch.  An OP_MERGE step combines accumulator
// slot + 1 into accumulator slot (a composite child of a composite).  The result is accumulator 0.
//
// A wave owns 256 consecutive x of one row; a lane 4 of them, in runs of 16 bytes of the output type (4 float / bool, 2 double), so
// float stores are 16 bytes and bool stores 4 bytes wide, each wave instruction covering one contiguous piece of the row.  In grid
// and separable mode y is one value per thread and everything that depends on y alone is computed once for the 4 points.
//
// This unit is compiled with -ffp-contract=off (csrc/Makefile): every product and sum is rounded by itself, in the order written, so
// the numpy walk of the same table (geometry_plan.evaluate) does the same arithmetic.  No LDS, no atomics.
#include <cmath>

#include "pm_entry.h"
#include "pm_math.h"

namespace pm {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kV = 4, kTileX = 64 * kV;
// the walk has four named accumulators a0 .. a3: the depth of nested composites a program may have (geometry_plan.MAX_SLOTS)

// geometry_plan.py: OPS, COMBS, FLAGS
enum { OP_NOP = 0, OP_CIRCLE = 1, OP_ANNULUS = 2, OP_RCIRCLE = 3, OP_RANNULUS = 4, OP_RECT = 5, OP_ELLIPSE = 6, OP_EDGE = 7, OP_VANE = 8,
       OP_GAUSS = 9, OP_MERGE = 10 };
enum { CB_SET = 0, CB_MIN = 1, CB_MAX = 2, CB_MAXNEG = 3 };
enum { FL_BEGIN = 1, FL_END = 2, FL_ROT = 4, FL_UP = 8 };

// one step of the table (geometry_plan.step_dtype)
template <typename T>
struct GStep {
    int32_t op, comb, slot, flags;
    T f[8];
};
static_assert(sizeof(GStep<float>) == 48 && sizeof(GStep<double>) == 80, "GStep layout is shared with geometry_plan.step_dtype");

template <typename T> __device__ __forceinline__ T min_(T a, T b) { return a < b ? a : b; }
template <typename T> __device__ __forceinline__ T max_(T a, T b) { return a > b ? a : b; }

// The walk of one program over the lane's kV points.  VY = 1: y is one value for all of them; VY = kV: a y per point.
template <typename T, int VY>
__device__ __forceinline__ void sdf_walk(const GStep<T>* __restrict__ table, int nsteps, const T X[kV], const T Y[VY], T d[kV]) {
    T a0[kV], a1[kV], a2[kV], a3[kV], run[kV];
    bool par[kV];
#pragma unroll
    for (int q = 0; q < kV; ++q) {
        a0[q] = a1[q] = a2[q] = a3[q] = run[q] = T(0);
        par[q] = false;
    }
    for (int s = 0; s < nsteps; ++s) {
        const GStep<T>& st = table[s];
        const int op = st.op, flags = st.flags, slot = st.slot, comb = st.comb;
        const bool begin = flags & FL_BEGIN;
        T p[kV];
#pragma unroll
        for (int q = 0; q < kV; ++q) p[q] = T(0);
        switch (op) {
        case OP_CIRCLE:
        case OP_ANNULUS: {
            const T cx = st.f[0], cy = st.f[1], r0 = st.f[2], hw = st.f[3];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T xx = X[q] - cx, yy = Y[q % VY] - cy;
                const T r = sqrt_(xx * xx + yy * yy) - r0;
                p[q] = op == OP_CIRCLE ? r : fabs(r) - hw;
            }
        } break;
        case OP_RCIRCLE:
        case OP_RANNULUS: {
            const T r0 = st.f[2], hw = st.f[3];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T r = X[q] - r0;
                p[q] = op == OP_RCIRCLE ? r : fabs(r) - hw;
            }
        } break;
        case OP_RECT: {
            const T c = st.f[0], sn = st.f[1], cx = st.f[2], cy = st.f[3], hw = st.f[4], hh = st.f[5], fr = st.f[6];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                T xx = X[q], yy = Y[q % VY];
                if (flags & FL_ROT) {
                    const T xr = xx * c - yy * sn;
                    yy = xx * sn + yy * c;
                    xx = xr;
                }
                const T qx = fabs(xx - cx) - hw, qy = fabs(yy - cy) - hh;
                const T ox = max_(qx, T(0)), oy = max_(qy, T(0));
                p[q] = sqrt_(ox * ox + oy * oy) + min_(max_(qx, qy), T(0)) - fr;
            }
        } break;
        case OP_ELLIPSE: {
            const T c = st.f[0], sn = st.f[1], a = st.f[2], b = st.f[3], aa = st.f[4], bb = st.f[5];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T xx = X[q], yy = Y[q % VY];
                const T xr = xx * c + yy * sn, yr = xx * sn - yy * c;
                const T u = xr / a, v = yr / b;
                const T F = u * u + v * v - T(1);
                const T gx = T(2) * xr / aa, gy = T(2) * yr / bb;
                p[q] = F / max_(sqrt_(gx * gx + gy * gy), T(1e-15));
            }
        } break;
        case OP_EDGE: {
            const T x0 = st.f[0], y0 = st.f[1], ex = st.f[2], ey = st.f[3], rinv = st.f[4], y1 = st.f[5];
            const bool up = flags & FL_UP;
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T y = Y[q % VY];
                const T wx = X[q] - x0, wy = y - y0;
                T t = (wx * ex + wy * ey) * rinv;
                t = min_(max_(t, T(0)), T(1));
                const T px = wx - t * ex, py = wy - t * ey;
                const T seg = px * px + py * py;
                const bool crosses = ((y0 > y) != (y1 > y)) && ((wx * ey < ex * wy) == up);
                run[q] = begin ? seg : min_(run[q], seg);
                par[q] = begin ? crosses : (par[q] != crosses);
                if (flags & FL_END) {
                    const T dd = sqrt_(run[q]);
                    p[q] = par[q] ? -dd : dd;
                }
            }
        } break;
        case OP_VANE: {
            const T c = st.f[0], sn = st.f[1], cx = st.f[2], cy = st.f[3], hw = st.f[4];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T xx = X[q] - cx, yy = Y[q % VY] - cy;
                const T al = min_(xx * c - yy * sn, T(0)), ac = xx * sn + yy * c;
                const T vane = sqrt_(al * al + ac * ac) - hw;
                run[q] = begin ? vane : min_(run[q], vane);
                p[q] = run[q];
            }
        } break;
        case OP_GAUSS: {
            const T cx = st.f[0], cy = st.f[1], k = st.f[2], s2 = st.f[3];
#pragma unroll
            for (int q = 0; q < kV; ++q) {
                const T xx = X[q] - cx, yy = Y[q % VY] - cy;
                p[q] = exp_(k * (xx * xx + yy * yy) / s2);
            }
        } break;
        case OP_MERGE: {
#pragma unroll
            for (int q = 0; q < kV; ++q) p[q] = slot == 0 ? a1[q] : slot == 1 ? a2[q] : a3[q];
        } break;
        default: break;
        }
        if (!(flags & FL_END)) continue;
#define PM_COMBINE(A)                                                                                        \
    _Pragma("unroll") for (int q = 0; q < kV; ++q) {                                                         \
        const T v = comb == CB_MAXNEG ? -p[q] : p[q];                                                        \
        A[q] = comb == CB_SET ? v : comb == CB_MIN ? min_(A[q], v) : max_(A[q], v);                          \
    }
        switch (slot) {
        case 0: PM_COMBINE(a0) break;
        case 1: PM_COMBINE(a1) break;
        case 2: PM_COMBINE(a2) break;
        case 3: PM_COMBINE(a3) break;
        default: break;
        }
#undef PM_COMBINE
    }
#pragma unroll
    for (int q = 0; q < kV; ++q) d[q] = a0[q];
}

template <typename T>
struct RenderArgs {
    int64_t ny, nx;
    const T* x;
    const T* y;
    int64_t ox, oy;
    T dx, dy;
    const GStep<T>* table;
    int nsteps;
    int out_kind;
    T aa_dx;
    void* out;
    int64_t out_ld, out_bstride;
    int64_t tiles_per_row;
    int vec_in, vec_out;
};

// the lane's q-th point of the wave tile starting at column xt: runs of W consecutive points, run r at r * 64 * W
template <int W>
__device__ __forceinline__ int64_t col_of(int64_t xt, int lane, int q) { return xt + (q / W) * 64 * W + lane * W + q % W; }

// W consecutive elements at p (all inside the array): as 16-byte pieces (or one piece of W elements when that is smaller) when fast
template <typename E, int W>
__device__ __forceinline__ void load_run(const E* __restrict__ p, bool fast, int64_t left, E* v) {
    constexpr int C = (W * sizeof(E) >= 16) ? int(16 / sizeof(E)) : W;
    using cv = E __attribute__((ext_vector_type(C)));
    if (fast) {
#pragma unroll
        for (int c = 0; c < W / C; ++c) {
            const cv t = *reinterpret_cast<const cv*>(p + c * C);
#pragma unroll
            for (int e = 0; e < C; ++e) v[c * C + e] = t[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = e < left ? p[e] : E(0);
    }
}

template <typename E, int W>
__device__ __forceinline__ void store_run(E* __restrict__ p, bool fast, int64_t left, const E* v) {
    constexpr int C = (W * sizeof(E) >= 16) ? int(16 / sizeof(E)) : W;
    using cv = E __attribute__((ext_vector_type(C)));
    if (fast) {
#pragma unroll
        for (int c = 0; c < W / C; ++c) {
            cv t;
#pragma unroll
            for (int e = 0; e < C; ++e) t[e] = v[c * C + e];
            *reinterpret_cast<cv*>(p + c * C) = t;
        }
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (e < left) p[e] = v[e];
    }
}

enum { MODE_GRID = PM_COORDS_GRID, MODE_SEPARABLE = PM_COORDS_SEPARABLE, MODE_POINTWISE = PM_COORDS_POINTWISE };

// O = T: distance or coverage; O = uint8_t: the mask.  grid.x: groups of kWaves wave tiles (row-major over rows x tiles_per_row),
// grid.y: the program of a stack.
template <typename T, typename O, int MODE>
__global__ __launch_bounds__(kThreads) void sdf_render_kernel(RenderArgs<T> a) {
    constexpr int W = sizeof(O) == 8 ? 2 : 4, R = kV / W, VY = MODE == MODE_POINTWISE ? kV : 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = int64_t(blockIdx.x) * kWaves + wave;
    const int64_t row = tile / a.tiles_per_row;
    if (row >= a.ny) return;
    const int64_t xt = (tile - row * a.tiles_per_row) * kTileX;

    T X[kV], Y[VY];
    if (MODE == MODE_GRID) {
#pragma unroll
        for (int q = 0; q < kV; ++q) X[q] = T(col_of<W>(xt, lane, q) - a.ox) * a.dx;
        Y[0] = T(row - a.oy) * a.dy;
    } else {
        const T* __restrict__ xp = MODE == MODE_POINTWISE ? a.x + row * a.nx : a.x;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t c0 = col_of<W>(xt, lane, r * W), left = a.nx - c0;
            if (left <= 0) {
#pragma unroll
                for (int e = 0; e < W; ++e) X[r * W + e] = T(0);
                if (MODE == MODE_POINTWISE) {
#pragma unroll
                    for (int e = 0; e < W; ++e) Y[(r * W + e) % VY] = T(0);
                }
                continue;
            }
            const bool fast = a.vec_in && left >= W;
            load_run<T, W>(xp + c0, fast, left, X + r * W);
            if (MODE == MODE_POINTWISE) load_run<T, W>(a.y + row * a.nx + c0, fast, left, Y + (r * W) % VY);
        }
        if (MODE == MODE_SEPARABLE) Y[0] = a.y[row];
    }

    T d[kV];
    sdf_walk<T, VY>(a.table + int64_t(blockIdx.y) * a.nsteps, a.nsteps, X, Y, d);

    O* __restrict__ op = static_cast<O*>(a.out) + int64_t(blockIdx.y) * a.out_bstride + row * a.out_ld;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t c0 = col_of<W>(xt, lane, r * W), left = a.nx - c0;
        if (left <= 0) continue;
        O v[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
            const T dd = d[r * W + e];
            if (sizeof(O) == 1)
                v[e] = O(dd <= T(0) ? 1 : 0);
            else if (a.out_kind == PM_SDF_COVERAGE)
                v[e] = O(min_(max_(T(0.5) - dd / a.aa_dx, T(0)), T(1)));
            else
                v[e] = O(dd);
        }
        store_run<O, W>(op + c0, a.vec_out && left >= W, left, v);
    }
}

// ---------------------------------------------------------------- coordinates
// make_xy_grid: meshgrids (grid != 0: x and y of ny x nx) or vectors (x of nx, y of ny), element = T(index - n / 2) * T(dx)
template <typename T>
__global__ __launch_bounds__(kThreads) void xy_grid_kernel(int64_t ny, int64_t nx, T dx, int grid, T* __restrict__ x, T* __restrict__ y) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (grid) {
        if (i >= ny * nx) return;
        const int64_t r = i / nx, c = i - r * nx;
        x[i] = T(c - nx / 2) * dx;
        y[i] = T(r - ny / 2) * dx;
    } else {
        if (i < nx) x[i] = T(i - nx / 2) * dx;
        if (i < ny) y[i] = T(i - ny / 2) * dx;
    }
}

// separable: x has nx values and y ny values, the outputs ny x nx; else all four hold ny x nx values
template <typename T>
__global__ __launch_bounds__(kThreads) void cart_to_polar_kernel(int64_t ny, int64_t nx, int separable, const T* __restrict__ x,
                                                                 const T* __restrict__ y, T* __restrict__ rho, T* __restrict__ phi) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= ny * nx) return;
    T xx, yy;
    if (separable) {
        const int64_t r = i / nx;
        xx = x[i - r * nx];
        yy = y[r];
    } else {
        xx = x[i];
        yy = y[i];
    }
    rho[i] = hypot_(xx, yy);
    phi[i] = atan2_(yy, xx);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void polar_to_cart_kernel(int64_t n, const T* __restrict__ rho, const T* __restrict__ phi,
                                                                 T* __restrict__ x, T* __restrict__ y) {
    const int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    T s, c;
    sincos_(phi[i], &s, &c);
    x[i] = rho[i] * c;
    y[i] = rho[i] * s;
}

int64_t blocks_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

template <typename T, typename O>
void launch_render_mode(int32_t coords, const RenderArgs<T>& a, dim3 grid, hipStream_t st) {
    const dim3 block{kThreads};
    if (coords == PM_COORDS_GRID)
        hipLaunchKernelGGL((sdf_render_kernel<T, O, MODE_GRID>), grid, block, 0, st, a);
    else if (coords == PM_COORDS_SEPARABLE)
        hipLaunchKernelGGL((sdf_render_kernel<T, O, MODE_SEPARABLE>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((sdf_render_kernel<T, O, MODE_POINTWISE>), grid, block, 0, st, a);
}

template <typename T>
void launch_render(int32_t coords, int64_t ny, int64_t nx, const void* x, const void* y, int64_t ox, int64_t oy, double dx, double dy,
                   const void* table, int nsteps, int64_t batch, int32_t out_kind, double aa_dx, void* out, int64_t out_ld, int64_t out_bstride,
                   hipStream_t st) {
    RenderArgs<T> a;
    a.ny = ny, a.nx = nx, a.x = static_cast<const T*>(x), a.y = static_cast<const T*>(y), a.ox = ox, a.oy = oy, a.dx = T(dx), a.dy = T(dy);
    a.table = static_cast<const GStep<T>*>(table), a.nsteps = nsteps, a.out_kind = out_kind, a.aa_dx = T(aa_dx);
    a.out = out, a.out_ld = out_ld, a.out_bstride = out_bstride;
    a.tiles_per_row = (nx + kTileX - 1) / kTileX;
    // 16-byte pieces: every row of every array starts on a 16-byte boundary (4 bytes for the mask's 4-byte pieces)
    const size_t es = sizeof(T);
    a.vec_in = coords == PM_COORDS_GRID ? 0
               : coords == PM_COORDS_SEPARABLE ? aligned(x, 16)
                                               : (aligned(x, 16) && aligned(y, 16) && (nx * es) % 16 == 0);
    if (out_kind == PM_SDF_MASK)
        a.vec_out = aligned(out, 4) && out_ld % 4 == 0 && out_bstride % 4 == 0;
    else
        a.vec_out = aligned(out, 16) && (out_ld * es) % 16 == 0 && (out_bstride * es) % 16 == 0;
    const int64_t tiles = ny * a.tiles_per_row;
    const dim3 grid{unsigned((tiles + kWaves - 1) / kWaves), unsigned(batch)};
    if (out_kind == PM_SDF_MASK)
        launch_render_mode<T, uint8_t>(coords, a, grid, st);
    else
        launch_render_mode<T, T>(coords, a, grid, st);
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_xy_grid(int32_t dtype, int64_t ny, int64_t nx, double dx, int32_t grid, void* x, void* y, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_xy_grid: dtype must be PM_F32 or PM_F64");
    if (ny < 0 || nx < 0 || !x || !y) return fail(PM_ERR_ARG, "pm_xy_grid: bad argument (null pointer or negative size)");
    const int64_t n = grid ? ny * nx : std::max(ny, nx);
    if (ny > INT32_MAX || nx > INT32_MAX || blocks_of(n) > INT32_MAX) return fail(PM_ERR_ARG, "pm_xy_grid: %lld x %lld is too large", (long long)ny, (long long)nx);
    if (n == 0) return 0;
    return by_rdtype(dtype, "pm_xy_grid", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(xy_grid_kernel<T>, dim3(unsigned(blocks_of(n))), dim3(kThreads), 0, PM_STREAM(stream), ny, nx, T(dx), grid != 0,
                           static_cast<T*>(x), static_cast<T*>(y));
        return int(hipGetLastError());
    });
}

int pm_cart_to_polar(int32_t dtype, int64_t ny, int64_t nx, int32_t separable, const void* x, const void* y, void* rho, void* phi, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_cart_to_polar: dtype must be PM_F32 or PM_F64");
    if (ny < 0 || nx < 0 || !x || !y || !rho || !phi) return fail(PM_ERR_ARG, "pm_cart_to_polar: bad argument (null pointer or negative size)");
    if (ny > INT32_MAX || nx > INT32_MAX || blocks_of(ny * nx) > INT32_MAX)
        return fail(PM_ERR_ARG, "pm_cart_to_polar: %lld x %lld is too large", (long long)ny, (long long)nx);
    if (ny * nx == 0) return 0;
    return by_rdtype(dtype, "pm_cart_to_polar", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(cart_to_polar_kernel<T>, dim3(unsigned(blocks_of(ny * nx))), dim3(kThreads), 0, PM_STREAM(stream), ny, nx,
                           separable != 0, static_cast<const T*>(x), static_cast<const T*>(y), static_cast<T*>(rho), static_cast<T*>(phi));
        return int(hipGetLastError());
    });
}

int pm_polar_to_cart(int32_t dtype, int64_t n, const void* rho, const void* phi, void* x, void* y, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_polar_to_cart: dtype must be PM_F32 or PM_F64");
    if (n < 0 || !rho || !phi || !x || !y) return fail(PM_ERR_ARG, "pm_polar_to_cart: bad argument (null pointer or negative size)");
    if (blocks_of(n) > INT32_MAX) return fail(PM_ERR_ARG, "pm_polar_to_cart: %lld points is too many", (long long)n);
    if (n == 0) return 0;
    return by_rdtype(dtype, "pm_polar_to_cart", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(polar_to_cart_kernel<T>, dim3(unsigned(blocks_of(n))), dim3(kThreads), 0, PM_STREAM(stream), n,
                           static_cast<const T*>(rho), static_cast<const T*>(phi), static_cast<T*>(x), static_cast<T*>(y));
        return int(hipGetLastError());
    });
}

int pm_sdf_render(int32_t dtype, int32_t coords, int64_t ny, int64_t nx, const void* x, const void* y, int64_t ox, int64_t oy, double dx,
                  double dy, const void* table, int64_t nsteps, int64_t batch, int32_t out_kind, double aa_dx, void* out, int64_t out_ld,
                  int64_t out_bstride, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_sdf_render: dtype must be PM_F32 or PM_F64");
    if (coords != PM_COORDS_GRID && coords != PM_COORDS_SEPARABLE && coords != PM_COORDS_POINTWISE)
        return fail(PM_ERR_ARG, "pm_sdf_render: coords must be PM_COORDS_GRID, PM_COORDS_SEPARABLE or PM_COORDS_POINTWISE");
    if (out_kind != PM_SDF_MASK && out_kind != PM_SDF_DISTANCE && out_kind != PM_SDF_COVERAGE)
        return fail(PM_ERR_ARG, "pm_sdf_render: out_kind must be PM_SDF_MASK, PM_SDF_DISTANCE or PM_SDF_COVERAGE");
    if (ny < 0 || nx < 0 || nsteps < 0 || batch < 0 || !table || !out)
        return fail(PM_ERR_ARG, "pm_sdf_render: bad argument (null pointer or negative size)");
    if (coords != PM_COORDS_GRID && (!x || !y)) return fail(PM_ERR_ARG, "pm_sdf_render: coordinate arrays are missing (null pointer)");
    if (coords == PM_COORDS_GRID && !(std::isfinite(dx) && std::isfinite(dy)))
        return fail(PM_ERR_ARG, "pm_sdf_render: the grid spacing must be finite");
    if (out_kind == PM_SDF_COVERAGE && !(std::isfinite(aa_dx) && aa_dx > 0))
        return fail(PM_ERR_ARG, "pm_sdf_render: coverage needs a sample spacing aa_dx > 0");
    if (out_ld < nx) return fail(PM_ERR_ARG, "pm_sdf_render: out_ld %lld is smaller than the row of %lld", (long long)out_ld, (long long)nx);
    if (!stack_ok(batch, ny, out_ld, out_bstride)) return fail(PM_ERR_ARG, "pm_sdf_render: out_bstride: the outputs of a stack would overlap");
    if (nsteps > INT32_MAX || batch > 65535) return fail(PM_ERR_ARG, "pm_sdf_render: too many steps or programs (batch <= 65535)");
    const int64_t tpr = (nx + kTileX - 1) / kTileX;
    if (nx > INT32_MAX || ny > INT32_MAX || (ny * tpr + kWaves - 1) / kWaves > INT32_MAX)
        return fail(PM_ERR_ARG, "pm_sdf_render: %lld x %lld is too large", (long long)ny, (long long)nx);
    if (ny == 0 || nx == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_sdf_render", [&](auto real) {
        launch_render<decltype(real)>(coords, ny, nx, x, y, ox, oy, dx, dy, table, int(nsteps), batch, out_kind, aa_dx, out, out_ld, out_bstride,
                                      PM_STREAM(stream));
        return int(hipGetLastError());
    });
}

}  // extern "C"
