// Polynomial families defined by a three-term recurrence, without a stored basis (prysm/polynomials/jacobi.py, cheby.py, legendre.py,
// hermite.py, laguerre.py, dickson.py, xy.py) (gfx950):
//
//  - pm_recur_basis: the planes P_k(u) and / or P_k'(u) of the orders a table asks for, one launch.
//  - pm_recur_sum: sum_k c[b][k] P_k(u) and its derivative(s) for B coefficient vectors, up to 8 vectors per walk.
//  - pm_recur_project: sum_p g[b][p] P_k(u_p) (or P_k'), the adjoint of the sum with respect to c.
//  - pm_recur2_sum: z[i][j] = sum_{n,m} C[n][m] Py_n(y_i) Px_m(x_j) on a rows x cols grid with dz/dx and dz/dy, one launch, factored.
//  - pm_recur2_project: Cbar[n][m] = sum_{i,j} g[i][j] Fy_n(y_i) Fx_m(x_j), the adjoint of one of the three maps, two launches.
//  - pm_recur2_outer: out[k] = ty[n_k] (x) tx[m_k] from two stored 1-D tables.
//
// One table of steps built on the host (prysm_amd/polynomials/recur_plan.py) describes a family: record k holds (a, b, c) of
//     P_k = (a + b x) P_{k-1} - c P_{k-2},      D_k = b P_{k-1} + (a + b x) D_{k-1} - c D_{k-2}        (D = dP/dx)
// walked from P_{-1} = 1, P_{-2} = 0, D = 0 -- record 0 is (P_0, 0, 0) and record 1 has c = 0 -- and the output plane of order k
// (slot, -1: walked, not written).  The step index is uniform, so the table is read through the scalar cache.
//
// The reductions are deterministic as in zernike.hip: partials in a fixed order into the caller's workspace, then a fixed-order sum.
// The tile, the 1-D projection's reduction around rwalk, its second stage and its launcher are modal_tile.h's.
#include "modal_tile.h"

namespace pm {
namespace {

// one step of the table (recur_plan.step_dtype)
template <typename T>
struct RStep {
    T a, b, c;
    int32_t slot;
};
static_assert(sizeof(RStep<float>) == 16 && sizeof(RStep<double>) == 32, "RStep layout is shared with recur_plan.step_dtype");

// the recurrence state of one point and one step of it
template <typename T, bool DER = true>
struct RState {
    T p = T(1), pm = T(0), d = T(0), dm = T(0);
    __device__ __forceinline__ void step(const RStep<T>& st, T x) {
        const T lin = st.a + st.b * x;
        const T n = lin * p - st.c * pm;
        if (DER) {
            const T nd = st.b * p + lin * d - st.c * dm;
            dm = d;
            d = nd;
        }
        pm = p;
        p = n;
    }
};

// the argument of the walk at the lane's points: u itself, or 2 (u^2 + v^2) / R^2 - 1
template <typename T>
__device__ __forceinline__ void recur_arg(int r2, T inv_r2, const T u[kVec], const T v[kVec], T X[kVec]) {
#pragma unroll
    for (int q = 0; q < kVec; ++q) X[q] = r2 ? T(2) * (u[q] * u[q] + v[q] * v[q]) * inv_r2 - T(1) : u[q];
}

// The walk over kVec points, E steps at a time: emit(j, slot, P, D) at the j-th step of a group when it writes, flush() after every
// group (the projection batches E reductions so that they overlap).
template <int E, bool DER, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void rwalk(const T X[kVec], const RStep<T>* __restrict__ table, int nsteps, int nout, Emit&& emit, Flush&& flush) {
    RState<T, DER> s[kVec];
    for (int s0 = 0; s0 < nsteps; s0 += E) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (s0 + j >= nsteps) break;
            const RStep<T> st = table[s0 + j];
            T p[kVec], d[kVec];
#pragma unroll
            for (int q = 0; q < kVec; ++q) {
                s[q].step(st, X[q]);
                p[q] = s[q].p;
                d[q] = s[q].d;
            }
            if (unsigned(st.slot) < unsigned(nout)) emit(j, st.slot, p, d);
        }
        flush();
    }
}

// ---------------------------------------------------------------- basis: planes of values and / or derivatives, write-bound
template <typename T>
__global__ __launch_bounds__(kThreads) void recur_basis_kernel(int64_t npts, int r2, T inv_r2, const T* __restrict__ u, const T* __restrict__ v,
                                                               const RStep<T>* __restrict__ table, int nsteps, int nout, T* __restrict__ out,
                                                               T* __restrict__ out_der, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T uu[kVec], vv[kVec] = {}, X[kVec];
    load_pts(u, base, lane, npts, full, uu);
    if (r2) load_pts(v, base, lane, npts, full, vv);
    recur_arg(r2, inv_r2, uu, vv, X);
    rwalk<1, true>(X, table, nsteps, nout,
                   [&](int, int k, const T p[kVec], const T d[kVec]) {
                       if (out) store_pts<true>(out + int64_t(k) * npts, base, lane, npts, full, p);
                       if (out_der) store_pts<true>(out_der + int64_t(k) * npts, base, lane, npts, full, d);
                   },
                   [] {});
}

// ---------------------------------------------------------------- sum: NB coefficient vectors per walk
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void recur_sum_kernel(int64_t npts, int r2, T inv_r2, const T* __restrict__ u, const T* __restrict__ v,
                                                             const RStep<T>* __restrict__ table, int nsteps, int ncoef,
                                                             const T* __restrict__ coefs, int accumulate, T* __restrict__ out,
                                                             T* __restrict__ out_dx, T* __restrict__ out_dy, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    const bool der = out_dx || out_dy;
    T uu[kVec], vv[kVec] = {}, X[kVec], acc[NB][kVec], dacc[NB][kVec];
    load_pts(u, base, lane, npts, full, uu);
    if (r2) load_pts(v, base, lane, npts, full, vv);
    recur_arg(r2, inv_r2, uu, vv, X);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < kVec; ++q) acc[b][q] = dacc[b][q] = T(0);
    rwalk<1, true>(X, table, nsteps, ncoef,
                   [&](int, int k, const T p[kVec], const T d[kVec]) {
#pragma unroll
                       for (int b = 0; b < NB; ++b) {
                           const T c = coefs[int64_t(b) * ncoef + k];
#pragma unroll
                           for (int q = 0; q < kVec; ++q) {
                               acc[b][q] += c * p[q];
                               dacc[b][q] += c * d[q];
                           }
                       }
                   },
                   [] {});
    auto put = [&](T* dst, T val[kVec]) {
        if (accumulate) {
            T old[kVec];
            load_pts(dst, base, lane, npts, full, old);
#pragma unroll
            for (int q = 0; q < kVec; ++q) val[q] += old[q];
        }
        store_pts<false>(dst, base, lane, npts, full, val);
    };
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (out) put(out + int64_t(b) * npts, acc[b]);
        if (!der) continue;
        if (r2) {      // dz/dx = dz/du 4 x / R^2, dz/dy = dz/du 4 y / R^2 (jacobi.py:392-413)
            T gx[kVec], gy[kVec];
#pragma unroll
            for (int q = 0; q < kVec; ++q) {
                gx[q] = dacc[b][q] * (T(4) * uu[q] * inv_r2);
                gy[q] = dacc[b][q] * (T(4) * vv[q] * inv_r2);
            }
            if (out_dx) put(out_dx + int64_t(b) * npts, gx);
            if (out_dy) put(out_dy + int64_t(b) * npts, gy);
        } else {
            put(out_dx + int64_t(b) * npts, dacc[b]);
        }
    }
}

// ---------------------------------------------------------------- projection: one partial per (workgroup, b, k)
// The reduction of modal_tile.h around rwalk(): partial[group][b0 + b][k], row length ld = B * nout.  With der the derivative track
// is projected, g first multiplied by the chain factor of the R2 form (g 4 x / R^2 + g2 4 y / R^2).
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void recur_project_kernel(int64_t npts, int r2, T inv_r2, const T* __restrict__ u, const T* __restrict__ v,
                                                                 const RStep<T>* __restrict__ table, int nsteps, int nout, int der,
                                                                 const T* __restrict__ g, const T* __restrict__ g2, T* __restrict__ partial,
                                                                 int64_t ld, int vec) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nacc = NB * nout;
    T* sacc = project_begin<T>(smem, nacc, tid);
    T* wacc = sacc + wave * nacc;
    for (int64_t base = wave_tile(wave); base < npts; base += int64_t(gridDim.x) * kThreads * kVec) {
        const bool full = vec && base + 64 * kVec <= npts;
        T uu[kVec], vv[kVec] = {}, X[kVec], gg[NB][kVec];
        ProjectStep<T, NB> step;
        load_pts(u, base, lane, npts, full, uu);
        if (r2) load_pts(v, base, lane, npts, full, vv);
        recur_arg(r2, inv_r2, uu, vv, X);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            load_pts(g + int64_t(b) * npts, base, lane, npts, full, gg[b]);
            if (der && r2) {
                T hh[kVec] = {};
                if (g2) load_pts(g2 + int64_t(b) * npts, base, lane, npts, full, hh);
#pragma unroll
                for (int q = 0; q < kVec; ++q) gg[b][q] = (gg[b][q] * uu[q] + hh[q] * vv[q]) * (T(4) * inv_r2);
            }
        }
        step.clear();
        rwalk<ProjectStep<T, NB>::E, true>(
            X, table, nsteps, nout,
            [&](int j, int k, const T p[kVec], const T d[kVec]) { step.emit_each(j, k, gg, [&](int q) { return der ? d[q] : p[q]; }); },
            [&] { step.flush(wacc, nout, lane); });
    }
    project_end(sacc, nacc, tid, [&](int o, T s) { partial[int64_t(blockIdx.x) * ld + o] = s; });
}

// ---------------------------------------------------------------- separable sum on a rows x cols grid
// A workgroup owns kCols columns (lane = column) and `chunk` rows of one member of the stack.  Stage A: wave w walks the x table at its
// column once per 8 rows n = w, w + 4, ... of C and leaves t[n][j] = sum_m C[n][m] Px_m(x_j) in LDS, and tx[n][j] from the derivative
// track when dz/dx is asked for (C is read at uniform addresses, through the scalar cache).  Stage B: a wave takes kRowsB rows of the
// chunk at a time, walks the y table at their y_i and forms every output asked for from one pass over t / tx: consecutive lanes read
// consecutive LDS words and store consecutive elements of a row.  No basis is stored anywhere.
constexpr int kCols = 64, kMaxOrder = 64, kRowsB = 4, kGroup = 8, kSubRows = 64;
constexpr size_t kSumLds = 64 * 1024;

template <typename T>
struct PD {
    T p, d;
};

// the LDS of a workgroup of the sum: t, tx when dz/dx is asked for and, with the y walk hoisted, (P, D) of kSubRows rows
template <typename T>
size_t sum_lds(int ny, bool want_zx, bool hoist) { return size_t(ny) * sizeof(T) * (kCols * (want_zx ? 2 : 1) + (hoist ? 2 * kSubRows : 0)); }

template <typename T, bool HOIST>
__global__ __launch_bounds__(kThreads) void recur2_sum_kernel(int rows, int cols, int chunk, const T* __restrict__ x, const T* __restrict__ y,
                                                              const RStep<T>* __restrict__ xt, int nx, const RStep<T>* __restrict__ yt, int ny,
                                                              const T* __restrict__ C, int what, T inv_xn, T inv_yn, T* __restrict__ z,
                                                              T* __restrict__ zx, T* __restrict__ zy, int64_t ld, int64_t bstride) {
    extern __shared__ __align__(16) unsigned char smem[];
    T* t = reinterpret_cast<T*>(smem);
    T* tx = t + ny * kCols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.x * kCols + lane;
    const bool incol = col < cols;
    const bool want_zx = (what & PM_RECUR2_ZX) != 0;
    const T xv = incol ? x[col] : T(0);
    const T* Cb = C + int64_t(blockIdx.z) * ny * nx;
    for (int n0 = wave; n0 < ny; n0 += kWaves * kGroup) {
        T acc[kGroup], accd[kGroup];
#pragma unroll
        for (int e = 0; e < kGroup; ++e) acc[e] = accd[e] = T(0);
        RState<T> s;
        for (int m = 0; m < nx; ++m) {
            s.step(xt[m], xv);
#pragma unroll
            for (int e = 0; e < kGroup; ++e) {
                const int n = n0 + e * kWaves;
                if (n < ny) {
                    const T c = Cb[n * nx + m];
                    acc[e] += c * s.p;
                    accd[e] += c * s.d;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < kGroup; ++e) {
            const int n = n0 + e * kWaves;
            if (n < ny) {
                t[n * kCols + lane] = acc[e];
                if (want_zx) tx[n * kCols + lane] = accd[e];
            }
        }
    }
    __syncthreads();
    const int row0 = blockIdx.y * chunk, row_end = min(rows, row0 + chunk);
    auto store = [&](int i, T vz, T vx, T vy) {
        const int64_t o = int64_t(blockIdx.z) * bstride + int64_t(i) * ld + col;
        if (z) __builtin_nontemporal_store(vz, z + o);
        if (zx) __builtin_nontemporal_store(vx * inv_xn, zx + o);
        if (zy) __builtin_nontemporal_store(vy * inv_yn, zy + o);
    };
    if (HOIST) {
        // the y walk depends on the row alone: one thread per row of a block of kSubRows rows leaves (P_n, D_n)(y_i) in LDS, and the
        // waves read them at uniform addresses (broadcast) -- three multiply-adds per point and order instead of a walk per lane
        PD<T>* fy = reinterpret_cast<PD<T>*>(t + ny * kCols * (want_zx ? 2 : 1));
        for (int sub = row0; sub < row_end; sub += kSubRows) {
            __syncthreads();
            if (tid < kSubRows) {
                const T yv = sub + tid < row_end ? y[sub + tid] : T(0);
                RState<T> s;
                for (int n = 0; n < ny; ++n) {
                    s.step(yt[n], yv);
                    fy[tid * ny + n] = PD<T>{s.p, s.d};
                }
            }
            __syncthreads();
            for (int q = 0; q < kSubRows / (kWaves * kRowsB); ++q) {
                const int r0 = (q * kWaves + wave) * kRowsB;
                if (sub + r0 >= row_end) break;
                T az[kRowsB], ax[kRowsB], ay[kRowsB];
#pragma unroll
                for (int r = 0; r < kRowsB; ++r) az[r] = ax[r] = ay[r] = T(0);
#pragma unroll 2
                for (int n = 0; n < ny; ++n) {
                    const T tn = t[n * kCols + lane];
                    const T txn = want_zx ? tx[n * kCols + lane] : T(0);
#pragma unroll
                    for (int r = 0; r < kRowsB; ++r) {
                        const PD<T> f = fy[(r0 + r) * ny + n];
                        az[r] += f.p * tn;
                        ax[r] += f.p * txn;
                        ay[r] += f.d * tn;
                    }
                }
                if (!incol) continue;
#pragma unroll
                for (int r = 0; r < kRowsB; ++r)
                    if (sub + r0 + r < row_end) store(sub + r0 + r, az[r], ax[r], ay[r]);
            }
        }
        return;
    }
    for (int i0 = row0 + wave * kRowsB; i0 < row_end; i0 += kWaves * kRowsB) {
        T yv[kRowsB], az[kRowsB], ax[kRowsB], ay[kRowsB];
        RState<T> s[kRowsB];
#pragma unroll
        for (int r = 0; r < kRowsB; ++r) {
            yv[r] = i0 + r < row_end ? y[i0 + r] : T(0);
            az[r] = ax[r] = ay[r] = T(0);
        }
        for (int n = 0; n < ny; ++n) {
            const RStep<T> st = yt[n];
            const T tn = t[n * kCols + lane];
            const T txn = want_zx ? tx[n * kCols + lane] : T(0);
#pragma unroll
            for (int r = 0; r < kRowsB; ++r) {
                s[r].step(st, yv[r]);
                az[r] += s[r].p * tn;
                ax[r] += s[r].p * txn;
                ay[r] += s[r].d * tn;
            }
        }
        if (!incol) continue;
#pragma unroll
        for (int r = 0; r < kRowsB; ++r)
            if (i0 + r < row_end) store(i0 + r, az[r], ax[r], ay[r]);
    }
}

// ---------------------------------------------------------------- separable adjoint, launch 1: reduce the rows of a chunk
// part[b][chunk][n][j] = sum over the chunk's kPRows rows i of Fy_n(y_i) g[b][i][j] (F the value or the derivative track).  The walk
// depends on the row alone, so one thread per row walks the y table once and leaves F[row][n] in LDS.  Then lane = column: wave w holds
// g of its rows w, w + 4, ... in registers and takes 8 orders n per pass, reading F at uniform addresses (broadcast, 8 consecutive
// values), and the four waves are added in order through LDS.  Columns past `cols` and rows past `rows` count as zeros.
constexpr int kPRows = 64, kPRowsPerWave = kPRows / kWaves;

int padded_orders(int ny) { return (ny + kGroup - 1) / kGroup * kGroup; }
template <typename T>
size_t project_cols_lds(int ny) { return (size_t(kPRows) * padded_orders(ny) + size_t(kWaves) * kGroup * kCols) * sizeof(T); }

template <typename T>
__global__ __launch_bounds__(kThreads) void recur2_project_cols_kernel(int rows, int cols, const T* __restrict__ y,
                                                                       const RStep<T>* __restrict__ yt, int ny, int nyp, int yder,
                                                                       const T* __restrict__ g, int64_t ld, int64_t bstride,
                                                                       T* __restrict__ part, int colpad) {
    extern __shared__ __align__(16) unsigned char smem[];
    T* F = reinterpret_cast<T*>(smem);             // [kPRows][nyp]
    T* sw = F + kPRows * nyp;                      // [kWaves][kGroup][kCols]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = blockIdx.x * kCols + lane;
    const bool incol = col < cols;
    const int row0 = blockIdx.y * kPRows;
    const T* gb = g + int64_t(blockIdx.z) * bstride;
    T* pb = part + (int64_t(blockIdx.z) * gridDim.y + blockIdx.y) * ny * int64_t(colpad) + int64_t(blockIdx.x) * kCols;
    if (tid < kPRows) {
        const bool inrow = row0 + tid < rows;
        const T yv = inrow ? y[row0 + tid] : T(0);
        RState<T> s;
        for (int n = 0; n < nyp; ++n) {
            if (n < ny) s.step(yt[n], yv);
            F[tid * nyp + n] = inrow && n < ny ? (yder ? s.d : s.p) : T(0);
        }
    }
    T gv[kPRowsPerWave];
#pragma unroll
    for (int q = 0; q < kPRowsPerWave; ++q) {
        const int i = row0 + wave + q * kWaves;
        gv[q] = incol && i < rows ? gb[int64_t(i) * ld + col] : T(0);
    }
    __syncthreads();
    for (int n0 = 0; n0 < ny; n0 += kGroup) {
        T acc[kGroup];
#pragma unroll
        for (int e = 0; e < kGroup; ++e) acc[e] = T(0);
#pragma unroll
        for (int q = 0; q < kPRowsPerWave; ++q) {
            const T* f = F + (wave + q * kWaves) * nyp + n0;
#pragma unroll
            for (int e = 0; e < kGroup; ++e) acc[e] += f[e] * gv[q];
        }
#pragma unroll
        for (int e = 0; e < kGroup; ++e) sw[(wave * kGroup + e) * kCols + lane] = acc[e];
        __syncthreads();
        for (int o = tid; o < kGroup * kCols; o += kThreads) {
            const int e = o / kCols, l = o % kCols;
            if (n0 + e < ny) {
                T t = sw[e * kCols + l];
                for (int w = 1; w < kWaves; ++w) t += sw[(w * kGroup + e) * kCols + l];
                pb[int64_t(n0 + e) * colpad + l] = t;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- separable adjoint, launch 2: sum the chunks, contract the columns
// out[b][n][m] (+)= scale * sum_j Fx_m(x_j) (sum over chunks, in order, of part[b][chunk][n][j]).  A workgroup of 1024 threads takes
// one n and 8 orders m; each thread its columns in order, then the butterfly over the wave and the 16 waves in order.
constexpr int kRowsThreads = 1024, kRowsWaves = kRowsThreads / 64;

template <typename T>
__global__ __launch_bounds__(kRowsThreads) void recur2_project_rows_kernel(int cols, int nchunks, const T* __restrict__ x,
                                                                           const RStep<T>* __restrict__ xt, int nx, int xder, T scale,
                                                                           const T* __restrict__ part, int colpad, int ny, int accumulate,
                                                                           T* __restrict__ out) {
    __shared__ T sw[kRowsWaves][kGroup];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x, m0 = blockIdx.y * kGroup, b = blockIdx.z;
    const int64_t cstride = int64_t(ny) * colpad;
    T acc[kGroup];
#pragma unroll
    for (int e = 0; e < kGroup; ++e) acc[e] = T(0);
    for (int j = tid; j < cols; j += kRowsThreads) {
        const T* pj = part + (int64_t(b) * nchunks * ny + n) * int64_t(colpad) + j;
        T uj = T(0);
#pragma unroll 8
        for (int c = 0; c < nchunks; ++c) uj += pj[c * cstride];
        const T xv = x[j];
        RState<T> s;
        for (int k = 0; k < m0; ++k) s.step(xt[k], xv);
#pragma unroll
        for (int e = 0; e < kGroup; ++e) {
            if (m0 + e < nx) {
                s.step(xt[m0 + e], xv);
                acc[e] += (xder ? s.d : s.p) * uj;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kGroup; ++e) {
        acc[e] = wave_sum(acc[e]);
        if (lane == 0) sw[wave][e] = acc[e];
    }
    __syncthreads();
    if (tid < kGroup && m0 + tid < nx) {
        T t = sw[0][tid];
        for (int w = 1; w < kRowsWaves; ++w) t += sw[w][tid];
        t *= scale;
        T* dst = out + (int64_t(b) * ny + n) * nx + m0 + tid;
        *dst = accumulate ? *dst + t : t;
    }
}

// ---------------------------------------------------------------- outer products of two stored tables, write-bound
constexpr int kOuterRows = 16;

template <typename T>
__global__ __launch_bounds__(kThreads) void recur2_outer_kernel(int rows, int cols, const T* __restrict__ ty, int nty, const T* __restrict__ tx,
                                                                int ntx, const int32_t* __restrict__ pairs, T* __restrict__ out) {
    const int k = blockIdx.z;
    const int m = pairs[2 * k], n = pairs[2 * k + 1];
    const int col = blockIdx.x * kThreads + threadIdx.x;
    if (unsigned(m) >= unsigned(ntx) || unsigned(n) >= unsigned(nty) || col >= cols) return;
    const T xv = tx[int64_t(m) * cols + col];
    const int row0 = blockIdx.y * kOuterRows, row_end = min(rows, row0 + kOuterRows);
    for (int i = row0; i < row_end; ++i)
        __builtin_nontemporal_store(ty[int64_t(n) * rows + i] * xv, out + (int64_t(k) * rows + i) * cols + col);
}

// ---------------------------------------------------------------- host
int64_t col_tiles(int64_t cols) { return (cols + kCols - 1) / kCols; }

// rows of a workgroup's chunk: the largest of 128 .. 32 that still leaves 1024 workgroups, else 16
int recur2_chunk(int64_t rows, int64_t cols, int64_t batch) {
    const int64_t tiles = col_tiles(cols) * std::max<int64_t>(batch, 1);
    for (int c = 128; c > 16; c >>= 1)
        if (tiles * ((rows + c - 1) / c) >= 1024) return c;
    return 16;
}

int check_1d(const char* who, int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table,
             int64_t nsteps, int64_t nout) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (form != PM_RECUR_X && form != PM_RECUR_R2) return fail(PM_ERR_ARG, "%s: form must be PM_RECUR_X or PM_RECUR_R2", who);
    if (!u || (form == PM_RECUR_R2 && !v) || !table || npts < 0 || nsteps < 0 || nout < 0 || nsteps > INT32_MAX || nout > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (form == PM_RECUR_R2 && !(radius > 0)) return fail(PM_ERR_ARG, "%s: the normalisation radius must be positive", who);
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld points is too many", who, (long long)npts);
    return 0;
}

int check_2d(const char* who, int32_t dtype, int64_t rows, int64_t cols, const void* x, const void* y, const void* xtable, int64_t nx,
             const void* ytable, int64_t ny, int64_t batch) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!x || !y || !xtable || !ytable || rows < 0 || cols < 0 || nx < 0 || ny < 0 || batch < 0)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (rows > 65535 * 16 || cols > INT32_MAX / 2 || batch > 65535)      // grid.y: chunks of at least 16 rows
        return fail(PM_ERR_ARG, "%s: the grid or the stack is too large", who);
    if (nx > kMaxOrder || ny > kMaxOrder)
        return fail(PM_ERR_UNSUPPORTED, "%s: %lld x %lld orders; an axis takes at most %d", who, (long long)ny, (long long)nx, kMaxOrder);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_recur_basis(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                   int64_t nout, void* out, void* out_der, void* stream) {
    if (int rc = check_1d("pm_recur_basis", dtype, form, npts, u, v, radius, table, nsteps, nout)) return rc;
    if (!out && !out_der) return fail(PM_ERR_ARG, "pm_recur_basis: bad argument (neither out nor out_der given)");
    if (npts == 0 || nout == 0 || nsteps == 0) return 0;
    return by_rdtype(dtype, "pm_recur_basis", [&](auto real) {
        using T = decltype(real);
        const int r2 = form == PM_RECUR_R2;
        hipLaunchKernelGGL(recur_basis_kernel<T>, dim3(unsigned(tiles_of(npts))), dim3(kThreads), 0, PM_STREAM(stream), npts, r2,
                           T(r2 ? 1.0 / (radius * radius) : 1.0), static_cast<const T*>(u), static_cast<const T*>(v),
                           static_cast<const RStep<T>*>(table), int(nsteps), int(nout), static_cast<T*>(out), static_cast<T*>(out_der),
                           vec_ok(npts, {u, v, out, out_der}));
        return int(hipGetLastError());
    });
}

int pm_recur_sum(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                 int64_t ncoef, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* out_dx, void* out_dy, void* stream) {
    if (int rc = check_1d("pm_recur_sum", dtype, form, npts, u, v, radius, table, nsteps, ncoef)) return rc;
    if ((!out && !out_dx && !out_dy) || !coefs || batch < 0)
        return fail(PM_ERR_ARG, "pm_recur_sum: bad argument (null pointer, no output or negative batch)");
    if (form == PM_RECUR_X && out_dy) return fail(PM_ERR_ARG, "pm_recur_sum: out_dy needs form PM_RECUR_R2");
    if (npts == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_recur_sum", [&](auto real) {
        using T = decltype(real);
        const int r2 = form == PM_RECUR_R2;
        const T *up = static_cast<const T*>(u), *vp = static_cast<const T*>(v), *c = static_cast<const T*>(coefs);
        const RStep<T>* steps = static_cast<const RStep<T>*>(table);
        T *o = static_cast<T*>(out), *ox = static_cast<T*>(out_dx), *oy = static_cast<T*>(out_dy);
        const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
        const int vec = vec_ok(npts, {u, v, out, out_dx, out_dy});
        const T inv_r2 = T(r2 ? 1.0 / (radius * radius) : 1.0);
        for (int64_t b0 = 0; b0 < batch;)
            b0 += by_nb(batch - b0, 8, [&](auto nb) {
                hipLaunchKernelGGL((recur_sum_kernel<T, decltype(nb)::value>), grid, block, 0, PM_STREAM(stream), npts, r2, inv_r2, up, vp, steps,
                                   int(nsteps), int(ncoef), c + b0 * ncoef, accumulate != 0, o ? o + b0 * npts : nullptr,
                                   ox ? ox + b0 * npts : nullptr, oy ? oy + b0 * npts : nullptr, vec);
            });
        return int(hipGetLastError());
    });
}

size_t pm_recur_project_workspace(int32_t dtype, int64_t npts, int64_t nout, int64_t batch) {
    if (!real_dtype(dtype) || npts < 0 || nout < 0 || batch < 0) return 0;
    return project_workspace_bytes(dtype, npts, size_t(batch) * size_t(nout));
}

int pm_recur_project(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                     int64_t nout, int64_t batch, int32_t der, const void* databar, const void* databar2, int32_t accumulate, void* out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_1d("pm_recur_project", dtype, form, npts, u, v, radius, table, nsteps, nout)) return rc;
    if (!out || !databar || batch < 0) return fail(PM_ERR_ARG, "pm_recur_project: bad argument (null pointer or negative batch)");
    if (databar2 && !(der && form == PM_RECUR_R2))
        return fail(PM_ERR_ARG, "pm_recur_project: databar2 is the dy adjoint of form PM_RECUR_R2 with der set");
    const int r2 = form == PM_RECUR_R2, vec = vec_ok(npts, {u, v, databar, databar2});
    return launch_project("pm_recur_project", "nout", "orders", dtype, npts, nout, batch, nout, accumulate, out, workspace, workspace_bytes, stream,
                          kMaxProjectGroups, [&](auto real, auto nb, int64_t b0, int64_t groups, size_t lds, hipStream_t st) {
                              using T = decltype(real);
                              const T *g = static_cast<const T*>(databar), *g2 = static_cast<const T*>(databar2);
                              hipLaunchKernelGGL((recur_project_kernel<T, decltype(nb)::value>), dim3(unsigned(groups)), dim3(kThreads), lds, st,
                                                 npts, r2, T(r2 ? 1.0 / (radius * radius) : 1.0), static_cast<const T*>(u),
                                                 static_cast<const T*>(v), static_cast<const RStep<T>*>(table), int(nsteps), int(nout), der != 0,
                                                 g + b0 * npts, g2 ? g2 + b0 * npts : nullptr, static_cast<T*>(workspace) + b0 * nout,
                                                 batch * nout, vec);
                          });
}

int pm_recur2_sum(int32_t dtype, int64_t rows, int64_t cols, const void* x, const void* y, const void* xtable, int64_t nx, const void* ytable,
                  int64_t ny, int64_t batch, const void* coefs, int32_t what, double inv_xnorm, double inv_ynorm, void* z, void* zx, void* zy,
                  int64_t ld, int64_t bstride, void* stream) {
    if (int rc = check_2d("pm_recur2_sum", dtype, rows, cols, x, y, xtable, nx, ytable, ny, batch)) return rc;
    if (!coefs) return fail(PM_ERR_ARG, "pm_recur2_sum: bad argument (null pointer)");
    if (what <= 0 || what > (PM_RECUR2_Z | PM_RECUR2_ZX | PM_RECUR2_ZY))
        return fail(PM_ERR_ARG, "pm_recur2_sum: what must be a mask of PM_RECUR2_Z, PM_RECUR2_ZX, PM_RECUR2_ZY");
    if (((what & PM_RECUR2_Z) && !z) || ((what & PM_RECUR2_ZX) && !zx) || ((what & PM_RECUR2_ZY) && !zy))
        return fail(PM_ERR_ARG, "pm_recur2_sum: bad argument (an output asked for in what is a null pointer)");
    PM_CHECK_LD("pm_recur2_sum", ld_ok(rows, cols, ld));
    if (!stack_ok(batch, rows, ld, bstride)) return fail(PM_ERR_ARG, "pm_recur2_sum: the batch stride is smaller than rows * ld");
    if (rows == 0 || cols == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_recur2_sum", [&](auto real) {
        using T = decltype(real);
        const int chunk = recur2_chunk(rows, cols, batch);
        const dim3 grid(unsigned(col_tiles(cols)), unsigned((rows + chunk - 1) / chunk), unsigned(batch));
        const bool want_zx = (what & PM_RECUR2_ZX) != 0, hoist = sum_lds<T>(int(ny), want_zx, true) <= kSumLds;
        auto launch = [&](auto kernel) {       // at most 64 KiB of LDS either way: 64 orders of fp64 with dz/dx fill it without the hoist
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), sum_lds<T>(int(ny), want_zx, hoist), PM_STREAM(stream), int(rows), int(cols), chunk,
                               static_cast<const T*>(x), static_cast<const T*>(y), static_cast<const RStep<T>*>(xtable), int(nx),
                               static_cast<const RStep<T>*>(ytable), int(ny), static_cast<const T*>(coefs), what, T(inv_xnorm), T(inv_ynorm),
                               (what & PM_RECUR2_Z) ? static_cast<T*>(z) : nullptr, want_zx ? static_cast<T*>(zx) : nullptr,
                               (what & PM_RECUR2_ZY) ? static_cast<T*>(zy) : nullptr, ld, bstride);
        };
        if (hoist)
            launch(recur2_sum_kernel<T, true>);
        else
            launch(recur2_sum_kernel<T, false>);
        return int(hipGetLastError());
    });
}

size_t pm_recur2_project_workspace(int32_t dtype, int64_t rows, int64_t cols, int64_t ny, int64_t batch) {
    if (!real_dtype(dtype) || rows < 0 || cols < 0 || ny < 0 || batch < 0) return 0;
    return size_t(batch) * size_t((rows + kPRows - 1) / kPRows) * size_t(ny) * size_t(col_tiles(cols) * kCols) * elem_of(dtype);
}

int pm_recur2_project(int32_t dtype, int64_t rows, int64_t cols, const void* x, const void* y, const void* xtable, int64_t nx,
                      const void* ytable, int64_t ny, int64_t batch, int32_t what, double inv_xnorm, double inv_ynorm, const void* databar,
                      int64_t ld, int64_t bstride, int32_t accumulate, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_2d("pm_recur2_project", dtype, rows, cols, x, y, xtable, nx, ytable, ny, batch)) return rc;
    if (!databar || !out) return fail(PM_ERR_ARG, "pm_recur2_project: bad argument (null pointer)");
    if (what != PM_RECUR2_Z && what != PM_RECUR2_ZX && what != PM_RECUR2_ZY)
        return fail(PM_ERR_ARG, "pm_recur2_project: what must be one of PM_RECUR2_Z, PM_RECUR2_ZX, PM_RECUR2_ZY");
    PM_CHECK_LD("pm_recur2_project", ld_ok(rows, cols, ld));
    if (!stack_ok(batch, rows, ld, bstride)) return fail(PM_ERR_ARG, "pm_recur2_project: the batch stride is smaller than rows * ld");
    if (batch == 0 || nx == 0 || ny == 0) return 0;
    const size_t need = pm_recur2_project_workspace(dtype, rows, cols, ny, batch);
    if (need && (!workspace || workspace_bytes < need))
        return fail(PM_ERR_WORKSPACE, "pm_recur2_project: workspace of %zu bytes is smaller than the %zu pm_recur2_project_workspace asks for",
                    workspace_bytes, need);
    return by_rdtype(dtype, "pm_recur2_project", [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        const int nchunks = rows && cols ? int((rows + kPRows - 1) / kPRows) : 0, colpad = int(col_tiles(cols) * kCols);
        T* part = static_cast<T*>(workspace);
        if (nchunks)
            hipLaunchKernelGGL(recur2_project_cols_kernel<T>, dim3(unsigned(col_tiles(cols)), unsigned(nchunks), unsigned(batch)), dim3(kThreads),
                               project_cols_lds<T>(int(ny)), st, int(rows), int(cols), static_cast<const T*>(y),
                               static_cast<const RStep<T>*>(ytable), int(ny), padded_orders(int(ny)), what == PM_RECUR2_ZY,
                               static_cast<const T*>(databar), ld, bstride, part, colpad);
        const double scale = what == PM_RECUR2_ZX ? inv_xnorm : what == PM_RECUR2_ZY ? inv_ynorm : 1.0;
        hipLaunchKernelGGL(recur2_project_rows_kernel<T>, dim3(unsigned(ny), unsigned((nx + kGroup - 1) / kGroup), unsigned(batch)),
                           dim3(kRowsThreads), 0, st, nchunks ? int(cols) : 0, nchunks, static_cast<const T*>(x),
                           static_cast<const RStep<T>*>(xtable), int(nx), what == PM_RECUR2_ZX, T(scale), part, colpad, int(ny),
                           accumulate != 0, static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

int pm_recur2_outer(int32_t dtype, int64_t rows, int64_t cols, int64_t nk, const void* ty, int64_t nty, const void* tx, int64_t ntx,
                    const void* pairs, void* out, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_recur2_outer: dtype must be PM_F32 or PM_F64");
    if (!ty || !tx || !pairs || !out || rows < 0 || cols < 0 || nk < 0 || nty < 0 || ntx < 0)
        return fail(PM_ERR_ARG, "pm_recur2_outer: bad argument (null pointer or negative size)");
    if (rows > INT32_MAX / 2 || cols > INT32_MAX / 2 || nk > 65535 || nty > INT32_MAX || ntx > INT32_MAX ||
        (rows + kOuterRows - 1) / kOuterRows > 65535)
        return fail(PM_ERR_ARG, "pm_recur2_outer: the grid or the pair list is too large");
    if (rows == 0 || cols == 0 || nk == 0) return 0;
    return by_rdtype(dtype, "pm_recur2_outer", [&](auto real) {
        using T = decltype(real);
        const dim3 grid(unsigned((cols + kThreads - 1) / kThreads), unsigned((rows + kOuterRows - 1) / kOuterRows), unsigned(nk));
        hipLaunchKernelGGL(recur2_outer_kernel<T>, grid, dim3(kThreads), 0, PM_STREAM(stream), int(rows), int(cols), static_cast<const T*>(ty),
                           int(nty), static_cast<const T*>(tx), int(ntx), static_cast<const int32_t*>(pairs), static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

}  // extern "C"
