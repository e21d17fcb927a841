// Zernike polynomials without a stored basis (prysm/polynomials/zernike.py, fitting.py) (gfx950):
//
//  - pm_zernike_basis: the K planes of zernike_nm_seq, one launch.
//  - pm_zernike_sum: sum_k c[b][k] Z_k for B coefficient vectors (zernike_sum), the basis evaluated once per point per group of up to
//    8 vectors and never stored.
//  - pm_zernike_project: sum_p g[b][p] Z_k[p] (the adjoint of zernike_sum with respect to c), same walk.
//  - pm_modes_dot: sum_p modes[k][p] g[p] over a stored basis (sum_of_2d_modes_adjoint).
//
// Every point walks one table of steps built on the host (prysm_amd/polynomials/zernike_plan.py): modes sorted by |m| then by Jacobi
// order j = (n - |m|) // 2; the Jacobi recurrence P_j^(0,|m|)(2 r^2 - 1) and z^|m| (z = x + i y) stay in registers, so
// r^|m| cos(|m| t) = Re z^|m| and r^|m| sin(|m| t) = Im z^|m| need no trigonometry in the loop.  The step index is uniform, so the
// table is read through the scalar cache.  A step whose slot is outside [0, nmodes) writes nothing.
//
// The two reductions (project, modes dot) are deterministic: each workgroup reduces its points in a fixed order (lane sums, a
// butterfly over the wave, waves in LDS slots of their own) and stores one partial per output into the caller's workspace; a second
// launch sums the partials of each output in a fixed order.  No atomics, so every run and every graph replay gives the same bits.
#include "zernike_walk.h"

#include "pm_entry.h"

namespace pm {
namespace {

constexpr int kMaxProjectGroups = 1024;                 // workgroups of a projection (grid-stride beyond): the partial count per output
constexpr int kDotIt = 2, kDotChunk = kThreads * kVec * kDotIt, kDotModes = 16;
constexpr size_t kProjectLds = 64 * 1024;               // per-wave accumulators of a projection workgroup

// ---------------------------------------------------------------- basis: K planes, write-bound
template <typename T>
__global__ __launch_bounds__(kThreads) void zernike_basis_kernel(int64_t npts, int polar, const T* __restrict__ u, const T* __restrict__ v,
                                                                 const ZStep<T>* __restrict__ table, int nsteps, int nmodes, T* __restrict__ out,
                                                                 int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T uu[kVec], vv[kVec];
    load_pts(u, base, lane, npts, full, uu);
    load_pts(v, base, lane, npts, full, vv);
    walk<1>(polar != 0, uu, vv, table, nsteps, nmodes,
            [&](int, int k, const T z[kVec]) { store_pts<true>(out + int64_t(k) * npts, base, lane, npts, full, z); }, [] {});
}

// ---------------------------------------------------------------- sum: NB coefficient vectors per walk
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void zernike_sum_kernel(int64_t npts, int polar, const T* __restrict__ u, const T* __restrict__ v,
                                                               const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                               const T* __restrict__ coefs, int accumulate, T* __restrict__ out, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T uu[kVec], vv[kVec], acc[NB][kVec];
    load_pts(u, base, lane, npts, full, uu);
    load_pts(v, base, lane, npts, full, vv);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < kVec; ++q) acc[b][q] = T(0);
    walk<1>(polar != 0, uu, vv, table, nsteps, nmodes,
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
// Each wave sums its 64 x kVec points per step, reduces over its lanes and adds the total into an LDS slot of its own, (wave, b, k);
// the workgroup adds its waves in order at the end and stores partial[group][b0 + b][k] (row length ld = B * nmodes).  The butterfly
// reductions of E = 8 / NB consecutive steps run together, 8 independent chains at a time.
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void zernike_project_kernel(int64_t npts, int polar, const T* __restrict__ u, const T* __restrict__ v,
                                                                   const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                                   const T* __restrict__ g, T* __restrict__ partial, int64_t ld, int vec) {
    constexpr int E = 8 / NB;
    extern __shared__ __align__(16) unsigned char smem[];
    T* sacc = reinterpret_cast<T*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nacc = NB * nmodes;
    for (int e = tid; e < kWaves * nacc; e += kThreads) sacc[e] = T(0);
    __syncthreads();
    T* wacc = sacc + wave * nacc;
    // the wave stays together through the loop (a shuffle needs every lane) and masks its own tail
    for (int64_t base = wave_tile(wave); base < npts; base += int64_t(gridDim.x) * kThreads * kVec) {
        const bool full = vec && base + 64 * kVec <= npts;
        T uu[kVec], vv[kVec], gg[NB][kVec], red[NB][E];
        int slot[E];
        load_pts(u, base, lane, npts, full, uu);
        load_pts(v, base, lane, npts, full, vv);
#pragma unroll
        for (int b = 0; b < NB; ++b) load_pts(g + int64_t(b) * npts, base, lane, npts, full, gg[b]);
#pragma unroll
        for (int j = 0; j < E; ++j) slot[j] = -1;
        walk<E>(polar != 0, uu, vv, table, nsteps, nmodes,
                [&](int j, int k, const T z[kVec]) {
                    slot[j] = k;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        T s = T(0);
#pragma unroll
                        for (int q = 0; q < kVec; ++q) s += gg[b][q] * z[q];
                        red[b][j] = s;
                    }
                },
                [&] {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                        for (int j = 0; j < E; ++j)
#pragma unroll
                            for (int b = 0; b < NB; ++b) red[b][j] += __shfl_xor(red[b][j], off);
#pragma unroll
                    for (int j = 0; j < E; ++j) {
                        if (slot[j] >= 0 && lane == 0)
#pragma unroll
                            for (int b = 0; b < NB; ++b) wacc[b * nmodes + slot[j]] += red[b][j];
                        slot[j] = -1;
                    }
                });
    }
    __syncthreads();
    for (int o = tid; o < nacc; o += kThreads) {
        T s = sacc[o];
        for (int w = 1; w < kWaves; ++w) s += sacc[w * nacc + o];
        partial[int64_t(blockIdx.x) * ld + o] = s;
    }
}

// ---------------------------------------------------------------- modes dot: partial[chunk][k] = sum over the chunk of modes[k] * g
// A workgroup takes kDotIt wave tiles per wave (kDotChunk points) and kDotModes modes; g of the chunk stays in registers.
template <typename T>
__global__ __launch_bounds__(kThreads) void modes_dot_kernel(int64_t npts, int nmodes, const T* __restrict__ modes, int64_t mstride,
                                                             const T* __restrict__ g, T* __restrict__ partial, int vec) {
    __shared__ T sw[kWaves][kDotModes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k0 = blockIdx.y * kDotModes;
    const int kn = min(kDotModes, nmodes - k0);
    int64_t base[kDotIt];
    bool full[kDotIt];
    T gg[kDotIt][kVec];
#pragma unroll
    for (int it = 0; it < kDotIt; ++it) {
        base[it] = int64_t(blockIdx.x) * kDotChunk + int64_t(it * kWaves + wave) * 64 * kVec;
        full[it] = vec && base[it] + 64 * kVec <= npts;
        load_pts(g, base[it], lane, npts, full[it], gg[it]);
    }
    for (int kk = 0; kk < kn; ++kk) {
        const T* mk = modes + int64_t(k0 + kk) * mstride;
        T s = T(0);
#pragma unroll
        for (int it = 0; it < kDotIt; ++it) {
            T m[kVec];
            load_pts<true>(mk, base[it], lane, npts, full[it], m);
#pragma unroll
            for (int q = 0; q < kVec; ++q) s += m[q] * gg[it][q];
        }
        s = wave_sum(s);
        if (lane == 0) sw[wave][kk] = s;
    }
    __syncthreads();
    if (tid < kn) {
        T s = sw[0][tid];
        for (int w = 1; w < kWaves; ++w) s += sw[w][tid];
        partial[int64_t(blockIdx.x) * nmodes + k0 + tid] = s;
    }
}

size_t elem_of(int32_t dtype) { return dtype == PM_F32 ? 4 : 8; }

// 16-byte vectors: every plane of npts points starts on a 16-byte boundary, and so does every pointer given
int vec_ok(int64_t npts, size_t elem, std::initializer_list<const void*> ptrs) {
    if (npts % kVec) return 0;
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 16) return 0;
    return 1;
}

int64_t tiles_of(int64_t npts) { return (npts + int64_t(kThreads) * kVec - 1) / (int64_t(kThreads) * kVec); }

int64_t project_groups(int64_t npts) { return std::max<int64_t>(1, std::min<int64_t>(tiles_of(npts), kMaxProjectGroups)); }

int64_t dot_chunks(int64_t npts) { return std::max<int64_t>(1, (npts + kDotChunk - 1) / kDotChunk); }

// the largest of 8, 4, 2, 1 coefficient vectors per projection walk whose per-wave accumulators fit kProjectLds
int project_nb(int32_t dtype, int64_t nmodes, int64_t batch) {
    for (int nb = 8; nb > 1; nb >>= 1)
        if (nb <= batch && size_t(kWaves) * nb * size_t(nmodes) * elem_of(dtype) <= kProjectLds) return nb;
    return 1;
}

int check_walk(const char* who, int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
               int64_t nmodes) {
    if (dtype != PM_F32 && dtype != PM_F64) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (coords != PM_ZERNIKE_CARTESIAN && coords != PM_ZERNIKE_POLAR)
        return fail(PM_ERR_ARG, "%s: coords must be PM_ZERNIKE_CARTESIAN or PM_ZERNIKE_POLAR", who);
    if (!u || !v || !table || npts < 0 || nsteps < 0 || nmodes < 0 || nsteps > INT32_MAX || nmodes > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    return 0;
}

template <typename T>
void launch_sum(int64_t npts, int polar, const void* u, const void* v, const void* table, int nsteps, int nmodes, int64_t batch,
                const void* coefs, int accumulate, void* out, hipStream_t st) {
    const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
    const int vec = vec_ok(npts, sizeof(T), {u, v, out});
    for (int64_t b0 = 0; b0 < batch;) {
        const int64_t left = batch - b0;
        const T* c = (const T*)coefs + b0 * nmodes;
        T* o = (T*)out + b0 * npts;
#define PM_ZSUM(NB)                                                                                                                 \
    hipLaunchKernelGGL((zernike_sum_kernel<T, NB>), grid, block, 0, st, npts, polar, (const T*)u, (const T*)v, (const ZStep<T>*)table, \
                       nsteps, nmodes, c, accumulate, o, vec);                                                                           \
    b0 += NB
        if (left >= 8) { PM_ZSUM(8); }
        else if (left >= 4) { PM_ZSUM(4); }
        else if (left >= 2) { PM_ZSUM(2); }
        else { PM_ZSUM(1); }
#undef PM_ZSUM
    }
}

template <typename T>
void launch_project(int64_t npts, int polar, const void* u, const void* v, const void* table, int nsteps, int nmodes, int64_t batch,
                    const void* g, void* out, void* ws, int nb, hipStream_t st) {
    const int64_t groups = project_groups(npts);
    const dim3 grid{unsigned(groups)}, block{kThreads};
    T* partial = (T*)ws;
    const int vec = vec_ok(npts, sizeof(T), {u, v, g});
    for (int64_t b0 = 0; b0 < batch;) {
        const int64_t left = batch - b0;
        const T* gb = (const T*)g + b0 * npts;
        T* pb = partial + b0 * nmodes;
#define PM_ZPROJ(NB)                                                                                                                \
    hipLaunchKernelGGL((zernike_project_kernel<T, NB>), grid, block, size_t(kWaves) * NB * nmodes * sizeof(T), st, npts, polar,      \
                       (const T*)u, (const T*)v, (const ZStep<T>*)table, nsteps, nmodes, gb, pb, batch * nmodes, vec);                      \
    b0 += NB
        if (nb >= 8 && left >= 8) { PM_ZPROJ(8); }
        else if (nb >= 4 && left >= 4) { PM_ZPROJ(4); }
        else if (nb >= 2 && left >= 2) { PM_ZPROJ(2); }
        else { PM_ZPROJ(1); }
#undef PM_ZPROJ
    }
    hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3(unsigned(batch * nmodes)), block, 0, st, groups, batch * nmodes, (const T*)partial,
                       (T*)out);
}

template <typename T>
void launch_dot(int64_t nmodes, int64_t npts, const void* modes, int64_t mstride, const void* g, void* out, void* ws, hipStream_t st) {
    const int64_t chunks = dot_chunks(npts);
    const dim3 grid(unsigned(chunks), unsigned((nmodes + kDotModes - 1) / kDotModes)), block(kThreads);
    const int vec = vec_ok(npts, sizeof(T), {modes, g}) && mstride % kVec == 0;
    hipLaunchKernelGGL(modes_dot_kernel<T>, grid, block, 0, st, npts, int(nmodes), (const T*)modes, mstride, (const T*)g, (T*)ws, vec);
    hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3(unsigned(nmodes)), block, 0, st, chunks, nmodes, (const T*)ws, (T*)out);
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_zernike_basis(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                     int64_t nmodes, void* out, void* stream) {
    if (int rc = check_walk("pm_zernike_basis", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out) return fail(PM_ERR_ARG, "pm_zernike_basis: bad argument (null pointer)");
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "pm_zernike_basis: %lld points is too many", (long long)npts);
    if (npts == 0 || nmodes == 0) return 0;
    hipStream_t st = PM_STREAM(stream);
    const int polar = coords == PM_ZERNIKE_POLAR;
    const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
    const int vec = vec_ok(npts, elem_of(dtype), {u, v, out});
    if (dtype == PM_F32)
        hipLaunchKernelGGL(zernike_basis_kernel<float>, grid, block, 0, st, npts, polar, (const float*)u, (const float*)v,
                           (const ZStep<float>*)table, int(nsteps), int(nmodes), (float*)out, vec);
    else
        hipLaunchKernelGGL(zernike_basis_kernel<double>, grid, block, 0, st, npts, polar, (const double*)u, (const double*)v,
                           (const ZStep<double>*)table, int(nsteps), int(nmodes), (double*)out, vec);
    return int(hipGetLastError());
}

int pm_zernike_sum(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                   int64_t nmodes, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream) {
    if (int rc = check_walk("pm_zernike_sum", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !coefs || batch < 0) return fail(PM_ERR_ARG, "pm_zernike_sum: bad argument (null pointer or negative batch)");
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "pm_zernike_sum: %lld points is too many", (long long)npts);
    if (npts == 0 || batch == 0) return 0;
    hipStream_t st = PM_STREAM(stream);
    const int polar = coords == PM_ZERNIKE_POLAR;
    if (dtype == PM_F32)
        launch_sum<float>(npts, polar, u, v, table, int(nsteps), int(nmodes), batch, coefs, accumulate != 0, out, st);
    else
        launch_sum<double>(npts, polar, u, v, table, int(nsteps), int(nmodes), batch, coefs, accumulate != 0, out, st);
    return int(hipGetLastError());
}

size_t pm_zernike_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch) {
    if ((dtype != PM_F32 && dtype != PM_F64) || npts < 0 || nmodes < 0 || batch < 0) return 0;
    return size_t(project_groups(npts)) * size_t(batch) * size_t(nmodes) * elem_of(dtype);
}

int pm_zernike_project(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                       int64_t nmodes, int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_walk("pm_zernike_project", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !databar || batch < 0) return fail(PM_ERR_ARG, "pm_zernike_project: bad argument (null pointer or negative batch)");
    if (batch * nmodes > INT32_MAX) return fail(PM_ERR_ARG, "pm_zernike_project: batch * nmodes is too large");
    if (size_t(kWaves) * size_t(nmodes) * elem_of(dtype) > kProjectLds)
        return fail(PM_ERR_UNSUPPORTED, "pm_zernike_project: %lld modes do not fit the workgroup's accumulators", (long long)nmodes);
    if (batch == 0 || nmodes == 0) return 0;
    const size_t need = pm_zernike_project_workspace(dtype, npts, nmodes, batch);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "pm_zernike_project: workspace of %zu bytes is smaller than the %zu pm_zernike_project_workspace asks for",
                    workspace_bytes, need);
    hipStream_t st = PM_STREAM(stream);
    const int polar = coords == PM_ZERNIKE_POLAR;
    const int nb = project_nb(dtype, nmodes, batch);
    if (dtype == PM_F32)
        launch_project<float>(npts, polar, u, v, table, int(nsteps), int(nmodes), batch, databar, out, workspace, nb, st);
    else
        launch_project<double>(npts, polar, u, v, table, int(nsteps), int(nmodes), batch, databar, out, workspace, nb, st);
    return int(hipGetLastError());
}

size_t pm_modes_dot_workspace(int32_t dtype, int64_t nmodes, int64_t npts) {
    if ((dtype != PM_F32 && dtype != PM_F64) || nmodes < 0 || npts < 0) return 0;
    return size_t(dot_chunks(npts)) * size_t(nmodes) * elem_of(dtype);
}

int pm_modes_dot(int32_t dtype, int64_t nmodes, int64_t npts, const void* modes, int64_t mode_stride, const void* v, void* out, void* workspace,
                 size_t workspace_bytes, void* stream) {
    if (dtype != PM_F32 && dtype != PM_F64) return fail(PM_ERR_ARG, "pm_modes_dot: dtype must be PM_F32 or PM_F64");
    if (!modes || !v || !out || nmodes < 0 || npts < 0 || (nmodes > 1 && mode_stride < npts) || nmodes > 65535 * int64_t(kDotModes) ||
        dot_chunks(npts) > INT32_MAX)
        return fail(PM_ERR_ARG, "pm_modes_dot: bad argument (null pointer, negative size or mode_stride < npts)");
    if (nmodes == 0) return 0;
    const size_t need = pm_modes_dot_workspace(dtype, nmodes, npts);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "pm_modes_dot: workspace of %zu bytes is smaller than the %zu pm_modes_dot_workspace asks for",
                    workspace_bytes, need);
    hipStream_t st = PM_STREAM(stream);
    if (dtype == PM_F32)
        launch_dot<float>(nmodes, npts, modes, mode_stride, v, out, workspace, st);
    else
        launch_dot<double>(nmodes, npts, modes, mode_stride, v, out, workspace, st);
    return int(hipGetLastError());
}

}  // extern "C"
