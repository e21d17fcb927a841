// The two pieces of the deformable-mirror model (prysm/x/dm.py) that are not FFT chains (gfx950):
//
//  - pm_lattice: the actuator lattice.  SCATTER writes the whole poke grid (zeros included, so no memset precedes it) with
//    scale * a[i][j] at (y0 + i sy, x0 + j sx); GATHER reads the lattice samples back out (the last line of DM.render_adjoint).
//  - pm_warp: scipy.ndimage.map_coordinates(img, (y', x'), order=3, mode='constant', cval=0) at the pull coordinates of a 3x3
//    homography (coordinates.warp / apply_homography), times `scale`, through an output window (pad2d / crop_center fused).
//
// The spline prefilter.  scipy runs a causal + anticausal recursion along each axis on the mirror-extended signal; its impulse
// response on that signal is exactly the symmetric FIR h[k] = sqrt(3) z^|k|, z = sqrt(3) - 2 (|z|^k < 1e-16 from k = 28), so the
// prefilter is LOCAL: one launch filters a tile along both axes in LDS from a mirrored halo of K samples (K = 30 for fp64, 14 for
// fp32: |z|^14 = 1e-8) and writes the coefficient image into the workspace; a second launch evaluates the 4 x 4 tap B-spline per
// output pixel.  A coordinate outside [0, n - 1] on either axis gives exactly 0 (scipy's constant mode has no tolerance there);
// inside, taps past an edge read the coefficients mirrored about it.  Coordinates are computed in fp64 in both precisions.
#include "pm_entry.h"

namespace pm {
namespace {

constexpr int kLatticeBlockX = 64, kLatticeBlockY = 4;
constexpr int kFirTX = 32, kFirTY = 16, kFirThreads = 256;
constexpr int kMaxGridZ = 65535;
constexpr int kMaxGridY = 65535;        // as csrc/pm_sweep.h: at most 65535 workgroups down the rows, more rows by the grid-stride step

// the rows of a thread of a (x, y) block: its own, then every gridDim.y * blockDim.y-th after it
__device__ __forceinline__ int64_t row_first() { return int64_t(blockIdx.y) * blockDim.y + threadIdx.y; }
__device__ __forceinline__ int64_t row_step() { return int64_t(gridDim.y) * blockDim.y; }

template <typename T> struct FirK;
template <> struct FirK<float> { static constexpr int K = 14; };
template <> struct FirK<double> { static constexpr int K = 30; };

// whole-sample mirror (scipy 'mirror': period 2n - 2, the edge samples are not repeated)
__device__ __forceinline__ int mirror_index(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i > n - 1 ? p - i : i;
}

// an element of the input read as real: a REAL array of T, or the real part of an interleaved complex one (IS_CX)
template <typename T, bool IS_CX>
__device__ __forceinline__ T load_re(const T* base, int64_t idx) {
    return IS_CX ? base[2 * idx] : base[idx];
}

// ---------------------------------------------------------------- lattice
template <typename T>
__global__ void lattice_scatter_kernel(int64_t batch, int rows, int cols, int nact_y, int nact_x, int y0, int x0, int sy, int sx,
                                       T scale, const T* __restrict__ in, int64_t in_ld, int64_t in_bstride, T* __restrict__ out,
                                       int64_t out_ld, int64_t out_bstride) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    const int dx = c - x0;
    const int j = dx / sx;
    const bool hit_x = dx >= 0 && dx == j * sx && j < nact_x;
    for (int64_t r = row_first(); r < rows; r += row_step()) {
        const int dy = int(r) - y0;
        const int i = dy / sy;
        const bool hit = hit_x && dy >= 0 && dy == i * sy && i < nact_y;
        for (int64_t b = blockIdx.z; b < batch; b += gridDim.z)
            out[b * out_bstride + r * out_ld + c] = hit ? scale * in[b * in_bstride + i * in_ld + j] : T(0);
    }
}

template <typename T, bool IS_CX>
__global__ void lattice_gather_kernel(int64_t batch, int nact_y, int nact_x, int y0, int x0, int sy, int sx, T scale,
                                      const T* __restrict__ in, int64_t in_ld, int64_t in_bstride, T* __restrict__ out, int64_t out_ld,
                                      int64_t out_bstride) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nact_x) return;
    for (int64_t i = row_first(); i < nact_y; i += row_step())
        for (int64_t b = blockIdx.z; b < batch; b += gridDim.z)
            out[b * out_bstride + i * out_ld + j] = scale * load_re<T, IS_CX>(in, b * in_bstride + (y0 + i * sy) * in_ld + (x0 + j * sx));
}

// ---------------------------------------------------------------- warp: prefilter
// One workgroup filters a kFirTY x kFirTX tile of one field along both axes: the (TY + 2K) x (TX + 2K) mirrored input footprint goes
// to LDS, the row FIR of its TY + 2K rows goes to registers and back over the footprint's first TX columns, the column FIR of those
// gives the tile.  fp64: 76 x 92 doubles = 55.9 KiB of LDS.
template <typename T, bool IS_CX>
__global__ __launch_bounds__(kFirThreads) void spline_fir_kernel(int64_t batch, int rows, int cols, const T* __restrict__ in, int64_t in_ld,
                                                                 int64_t in_bstride, T* __restrict__ coeff) {
    constexpr int K = FirK<T>::K;
    constexpr int HH = kFirTY + 2 * K, HW = kFirTX + 2 * K;
    constexpr int NV = (HH * kFirTX + kFirThreads - 1) / kFirThreads;
    __shared__ T s[HH * HW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kFirTX;
    const T sqrt3 = T(1.7320508075688772), z = T(-0.2679491924311228);
    // tile rows past kMaxGridY * kFirTY rows are this workgroup's next trips (rows <= INT32_MAX / 2, so y0 + the step stays an int)
    for (int y0 = blockIdx.y * kFirTY; y0 < rows; y0 += gridDim.y * kFirTY)
    for (int64_t b = blockIdx.z; b < batch; b += gridDim.z) {
        for (int e = tid; e < HH * HW; e += kFirThreads) {
            const int hr = e / HW, hc = e - hr * HW;
            const int r = mirror_index(y0 - K + hr, rows), c = mirror_index(x0 - K + hc, cols);
            s[e] = load_re<T, IS_CX>(in, b * in_bstride + int64_t(r) * in_ld + c);
        }
        __syncthreads();
        T v[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int e = tid + q * kFirThreads;
            v[q] = T(0);
            if (e < HH * kFirTX) {
                const int hr = e / kFirTX, tc = e - hr * kFirTX;
                const T* row = s + hr * HW + K + tc;
                T acc = row[0], p = T(1);
#pragma unroll 2
                for (int k = 1; k <= K; ++k) {
                    p *= z;
                    acc += p * (row[-k] + row[k]);
                }
                v[q] = sqrt3 * acc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int e = tid + q * kFirThreads;
            if (e < HH * kFirTX) {
                const int hr = e / kFirTX, tc = e - hr * kFirTX;
                s[hr * HW + tc] = v[q];
            }
        }
        __syncthreads();
        T* dst = coeff + b * int64_t(rows) * cols;
        for (int e = tid; e < kFirTY * kFirTX; e += kFirThreads) {
            const int ty = e / kFirTX, tc = e - ty * kFirTX;
            const int r = y0 + ty, c = x0 + tc;
            if (r < rows && c < cols) {
                const T* col = s + (K + ty) * HW + tc;
                T acc = col[0], p = T(1);
#pragma unroll 2
                for (int k = 1; k <= K; ++k) {
                    p *= z;
                    acc += p * (col[-k * HW] + col[k * HW]);
                }
                dst[int64_t(r) * cols + c] = sqrt3 * acc;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- warp: sample
struct Homography {
    double m[9];
};

__device__ __forceinline__ void bspline3_weights(double t, double w[4]) {
    // taps at floor - 1 .. floor + 2 for the fractional part t in [0, 1)
    const double u = 1.0 - t;
    w[0] = u * u * u * (1.0 / 6.0);
    w[1] = (2.0 / 3.0) - t * t + 0.5 * t * t * t;
    w[2] = (2.0 / 3.0) - u * u + 0.5 * u * u * u;
    w[3] = t * t * t * (1.0 / 6.0);
}

template <typename T>
__global__ void spline_sample_kernel(int64_t batch, int rows, int cols, const T* __restrict__ coeff, Homography H, double scale, int out_rows,
                                     int out_cols, int off_y, int off_x, T* __restrict__ out, int64_t out_ld, int64_t out_bstride) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= out_cols) return;
    for (int64_t r64 = row_first(); r64 < out_rows; r64 += row_step()) {
        const int r = int(r64);
        const int R = r + off_y, C = c + off_x;
        bool inside = R >= 0 && R < rows && C >= 0 && C < cols;
        int iy[4], ix[4];
        double wy[4], wx[4];
        if (inside) {
            // apply_homography (prysm/coordinates.py:545-570): (x', y', w) = H (C, R, 1), then x'/w, y'/w -- all fp64
            const double xc = double(C), yr = double(R);
            const double xp = H.m[0] * xc + H.m[1] * yr + H.m[2];
            const double yp = H.m[3] * xc + H.m[4] * yr + H.m[5];
            const double w = H.m[6] * xc + H.m[7] * yr + H.m[8];
            const double x = xp / w, y = yp / w;
            inside = x >= 0.0 && x <= double(cols - 1) && y >= 0.0 && y <= double(rows - 1);
            if (inside) {
                const double fy = floor(y), fx = floor(x);
                bspline3_weights(y - fy, wy);
                bspline3_weights(x - fx, wx);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    iy[k] = mirror_index(int(fy) - 1 + k, rows);
                    ix[k] = mirror_index(int(fx) - 1 + k, cols);
                }
            }
        }
        for (int64_t b = blockIdx.z; b < batch; b += gridDim.z) {
            T v = T(0);
            if (inside) {
                const T* cb = coeff + b * int64_t(rows) * cols;
                T acc = T(0);
#pragma unroll
                for (int ky = 0; ky < 4; ++ky) {
                    const T* crow = cb + int64_t(iy[ky]) * cols;
                    T racc = T(0);
#pragma unroll
                    for (int kx = 0; kx < 4; ++kx) racc += T(wx[kx]) * crow[ix[kx]];
                    acc += T(wy[ky]) * racc;
                }
                v = T(scale) * acc;
            }
            out[b * out_bstride + int64_t(r) * out_ld + c] = v;
        }
    }
}

size_t warp_ws_bytes(int32_t dtype, int64_t batch, int64_t rows, int64_t cols) {
    const size_t es = (dtype == PM_F32 || dtype == PM_C64) ? 4 : 8;
    return size_t(batch) * size_t(rows) * size_t(cols) * es;
}

bool real_or_complex(int32_t dtype) { return dtype == PM_F32 || dtype == PM_F64 || dtype == PM_C64 || dtype == PM_C128; }

// every kernel here steps over the rows (row_step, the tile loop of spline_fir_kernel) and the stack members that the caps leave out
dim3 grid_of(int64_t cols, int64_t rows, int64_t batch, dim3 block) {
    const int64_t gy = (rows + block.y - 1) / block.y;
    return dim3(unsigned((cols + block.x - 1) / block.x), unsigned(gy < kMaxGridY ? gy : kMaxGridY),
                unsigned(batch < kMaxGridZ ? batch : kMaxGridZ));
}

// Calls f(real, cx) for a dtype that real_or_complex() has passed: real is a value of the dtype's real type, cx std::true_type for
// the two complex dtypes (the kernels then read the real part of interleaved complex elements)
template <typename F>
int by_real_part(int32_t dtype, F&& f) {
    switch (dtype) {
        case PM_F32: return f(float{}, std::false_type{});
        case PM_F64: return f(double{}, std::false_type{});
        case PM_C64: return f(float{}, std::true_type{});
        default: return f(double{}, std::true_type{});
    }
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_lattice(int32_t dtype, int32_t op, int64_t batch, int64_t rows, int64_t cols, int64_t nact_y, int64_t nact_x, int64_t y0, int64_t x0,
               int64_t sy, int64_t sx, double scale, const void* in, int64_t in_ld, int64_t in_bstride, void* out, int64_t out_ld,
               int64_t out_bstride, void* stream) {
    if (op != PM_LATTICE_SCATTER && op != PM_LATTICE_GATHER)
        return fail(PM_ERR_ARG, "pm_lattice: op must be PM_LATTICE_SCATTER or PM_LATTICE_GATHER");
    if (op == PM_LATTICE_SCATTER ? (dtype != PM_F32 && dtype != PM_F64) : !real_or_complex(dtype))
        return fail(PM_ERR_ARG, "pm_lattice: dtype must be PM_F32 or PM_F64 (GATHER also reads the real part of PM_C64 / PM_C128)");
    if (!in || !out || batch < 0 || rows < 1 || cols < 1 || nact_y < 1 || nact_x < 1 || sy < 1 || sx < 1 || rows > INT32_MAX ||
        cols > INT32_MAX)
        return fail(PM_ERR_ARG, "pm_lattice: bad argument (null pointer, empty grid or lattice, separation < 1)");
    if (y0 < 0 || x0 < 0 || y0 + (nact_y - 1) * sy >= rows || x0 + (nact_x - 1) * sx >= cols)
        return fail(PM_ERR_ARG,
                    "pm_lattice: the %lld x %lld lattice at (%lld, %lld) with separation (%lld, %lld) does not fit inside the %lld x %lld grid",
                    (long long)nact_y, (long long)nact_x, (long long)y0, (long long)x0, (long long)sy, (long long)sx, (long long)rows,
                    (long long)cols);
    const int64_t irows = op == PM_LATTICE_SCATTER ? nact_y : rows, icols = op == PM_LATTICE_SCATTER ? nact_x : cols;
    const int64_t orows = op == PM_LATTICE_SCATTER ? rows : nact_y, ocols = op == PM_LATTICE_SCATTER ? cols : nact_x;
    if ((irows > 1 && in_ld < icols) || in_bstride < 0)
        return fail(PM_ERR_ARG, "pm_lattice: in_ld must be >= %lld and in_bstride >= 0", (long long)icols);
    if ((orows > 1 && out_ld < ocols) || (batch > 1 && out_bstride < (orows - 1) * out_ld + ocols))
        return fail(PM_ERR_ARG, "pm_lattice: out_ld / out_bstride make the outputs overlap (need out_ld >= %lld, out_bstride >= rows * out_ld)",
                    (long long)ocols);
    if (batch == 0) return 0;
    hipStream_t st = PM_STREAM(stream);
    const dim3 block(kLatticeBlockX, kLatticeBlockY);
    if (op == PM_LATTICE_SCATTER)
        return by_rdtype(dtype, "pm_lattice", [&](auto real) {
            using T = decltype(real);
            hipLaunchKernelGGL(lattice_scatter_kernel<T>, grid_of(cols, rows, batch, block), block, 0, st, batch, int(rows), int(cols), int(nact_y),
                               int(nact_x), int(y0), int(x0), int(sy), int(sx), T(scale), static_cast<const T*>(in), in_ld, in_bstride,
                               static_cast<T*>(out), out_ld, out_bstride);
            return int(hipGetLastError());
        });
    return by_real_part(dtype, [&](auto real, auto cx) {
        using T = decltype(real);
        hipLaunchKernelGGL((lattice_gather_kernel<T, decltype(cx)::value>), grid_of(nact_x, nact_y, batch, block), block, 0, st, batch, int(nact_y),
                           int(nact_x), int(y0), int(x0), int(sy), int(sx), T(scale), static_cast<const T*>(in), in_ld, in_bstride,
                           static_cast<T*>(out), out_ld, out_bstride);
        return int(hipGetLastError());
    });
}

size_t pm_warp_workspace(int32_t dtype, int64_t batch, int64_t rows, int64_t cols) {
    if (!real_or_complex(dtype) || batch < 0 || rows < 1 || cols < 1) return 0;
    return warp_ws_bytes(dtype, batch, rows, cols);
}

int pm_warp(int32_t dtype, int32_t order, int64_t batch, int64_t rows, int64_t cols, const void* in, int64_t in_ld, int64_t in_bstride,
            const double* homography, double scale, int64_t out_rows, int64_t out_cols, int64_t off_y, int64_t off_x, void* out,
            int64_t out_ld, int64_t out_bstride, void* workspace, size_t workspace_bytes, void* stream) {
    if (!real_or_complex(dtype)) return fail(PM_ERR_ARG, "pm_warp: dtype must be PM_F32, PM_F64, PM_C64 or PM_C128");
    if (order != 3) return fail(PM_ERR_UNSUPPORTED, "pm_warp: spline order %d is not implemented (order 3 is)", int(order));
    if (!in || !out || !homography || batch < 0 || rows < 1 || cols < 1 || out_rows < 0 || out_cols < 0 || rows > INT32_MAX / 2 ||
        cols > INT32_MAX / 2 || out_rows > INT32_MAX / 2 || out_cols > INT32_MAX / 2 || off_y < -(INT32_MAX / 2) || off_y > INT32_MAX / 2 ||
        off_x < -(INT32_MAX / 2) || off_x > INT32_MAX / 2)
        return fail(PM_ERR_ARG, "pm_warp: bad argument (null pointer or size out of range)");
    if ((rows > 1 && in_ld < cols) || in_bstride < 0) return fail(PM_ERR_ARG, "pm_warp: in_ld must be >= cols and in_bstride >= 0");
    if ((out_rows > 1 && out_ld < out_cols) || (batch > 1 && out_bstride < (out_rows - 1) * out_ld + out_cols))
        return fail(PM_ERR_ARG, "pm_warp: out_ld / out_bstride make the outputs overlap (need out_ld >= out_cols, out_bstride >= out_rows * out_ld)");
    if (batch == 0 || out_rows == 0 || out_cols == 0) return 0;
    const size_t need = warp_ws_bytes(dtype, batch, rows, cols);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "pm_warp: workspace of %zu bytes is smaller than the %zu pm_warp_workspace asks for", workspace_bytes, need);
    Homography H;
    for (int k = 0; k < 9; ++k) H.m[k] = homography[k];
    return by_real_part(dtype, [&](auto real, auto cx) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        T* coeff = static_cast<T*>(workspace);
        hipLaunchKernelGGL((spline_fir_kernel<T, decltype(cx)::value>), grid_of(cols, rows, batch, dim3(kFirTX, kFirTY)), dim3(kFirThreads), 0, st,
                           batch, int(rows), int(cols), static_cast<const T*>(in), in_ld, in_bstride, coeff);
        const dim3 block(kLatticeBlockX, kLatticeBlockY);
        hipLaunchKernelGGL(spline_sample_kernel<T>, grid_of(out_cols, out_rows, batch, block), block, 0, st, batch, int(rows), int(cols), coeff, H,
                           scale, int(out_rows), int(out_cols), int(off_y), int(off_x), static_cast<T*>(out), out_ld, out_bstride);
        return int(hipGetLastError());
    });
}

}  // extern "C"
