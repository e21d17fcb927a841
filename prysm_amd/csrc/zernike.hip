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
// The projection's reduction and its launcher are modal_tile.h's, shared with qpoly.hip, recur.hip and segmented.hip.
#include "zernike_walk.h"

namespace pm {
namespace {

constexpr int kDotIt = 2, kDotChunk = kThreads * kVec * kDotIt, kDotModes = 16;

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
// The reduction of modal_tile.h around walk(): partial[group][b0 + b][k], row length ld = B * nmodes.
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void zernike_project_kernel(int64_t npts, int polar, const T* __restrict__ u, const T* __restrict__ v,
                                                                   const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                                   const T* __restrict__ g, T* __restrict__ partial, int64_t ld, int vec) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nacc = NB * nmodes;
    T* sacc = project_begin<T>(smem, nacc, tid);
    T* wacc = sacc + wave * nacc;
    for (int64_t base = wave_tile(wave); base < npts; base += int64_t(gridDim.x) * kThreads * kVec) {
        const bool full = vec && base + 64 * kVec <= npts;
        T uu[kVec], vv[kVec], gg[NB][kVec];
        ProjectStep<T, NB> step;
        load_pts(u, base, lane, npts, full, uu);
        load_pts(v, base, lane, npts, full, vv);
#pragma unroll
        for (int b = 0; b < NB; ++b) load_pts(g + int64_t(b) * npts, base, lane, npts, full, gg[b]);
        step.clear();
        walk<ProjectStep<T, NB>::E>(polar != 0, uu, vv, table, nsteps, nmodes, [&](int j, int k, const T z[kVec]) { step.emit(j, k, gg, z); },
                     [&] { step.flush(wacc, nmodes, lane); });
    }
    project_end(sacc, nacc, tid, [&](int o, T s) { partial[int64_t(blockIdx.x) * ld + o] = s; });
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

int64_t dot_chunks(int64_t npts) { return std::max<int64_t>(1, (npts + kDotChunk - 1) / kDotChunk); }

int check_walk(const char* who, int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
               int64_t nmodes) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (coords != PM_ZERNIKE_CARTESIAN && coords != PM_ZERNIKE_POLAR)
        return fail(PM_ERR_ARG, "%s: coords must be PM_ZERNIKE_CARTESIAN or PM_ZERNIKE_POLAR", who);
    if (!u || !v || !table || npts < 0 || nsteps < 0 || nmodes < 0 || nsteps > INT32_MAX || nmodes > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    return 0;
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
    return by_rdtype(dtype, "pm_zernike_basis", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(zernike_basis_kernel<T>, dim3(unsigned(tiles_of(npts))), dim3(kThreads), 0, PM_STREAM(stream), npts,
                           coords == PM_ZERNIKE_POLAR, static_cast<const T*>(u), static_cast<const T*>(v), static_cast<const ZStep<T>*>(table),
                           int(nsteps), int(nmodes), static_cast<T*>(out), vec_ok(npts, {u, v, out}));
        return int(hipGetLastError());
    });
}

int pm_zernike_sum(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                   int64_t nmodes, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream) {
    if (int rc = check_walk("pm_zernike_sum", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !coefs || batch < 0) return fail(PM_ERR_ARG, "pm_zernike_sum: bad argument (null pointer or negative batch)");
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "pm_zernike_sum: %lld points is too many", (long long)npts);
    if (npts == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_zernike_sum", [&](auto real) {
        using T = decltype(real);
        const T *up = static_cast<const T*>(u), *vp = static_cast<const T*>(v), *c = static_cast<const T*>(coefs);
        const ZStep<T>* steps = static_cast<const ZStep<T>*>(table);
        T* o = static_cast<T*>(out);
        const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
        const int vec = vec_ok(npts, {u, v, out});
        for (int64_t b0 = 0; b0 < batch;)
            b0 += by_nb(batch - b0, 8, [&](auto nb) {
                hipLaunchKernelGGL((zernike_sum_kernel<T, decltype(nb)::value>), grid, block, 0, PM_STREAM(stream), npts,
                                   coords == PM_ZERNIKE_POLAR, up, vp, steps, int(nsteps), int(nmodes), c + b0 * nmodes, accumulate != 0,
                                   o + b0 * npts, vec);
            });
        return int(hipGetLastError());
    });
}

size_t pm_zernike_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch) {
    if (!real_dtype(dtype) || npts < 0 || nmodes < 0 || batch < 0) return 0;
    return project_workspace_bytes(dtype, npts, size_t(batch) * size_t(nmodes));
}

int pm_zernike_project(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                       int64_t nmodes, int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_walk("pm_zernike_project", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !databar || batch < 0) return fail(PM_ERR_ARG, "pm_zernike_project: bad argument (null pointer or negative batch)");
    const int vec = vec_ok(npts, {u, v, databar});
    return launch_project("pm_zernike_project", "nmodes", "modes", dtype, npts, nmodes, batch, nmodes, 0, out, workspace, workspace_bytes, stream,
                          kMaxProjectGroups, [&](auto real, auto nb, int64_t b0, int64_t groups, size_t lds, hipStream_t st) {
                              using T = decltype(real);
                              hipLaunchKernelGGL((zernike_project_kernel<T, decltype(nb)::value>), dim3(unsigned(groups)), dim3(kThreads), lds, st,
                                                 npts, coords == PM_ZERNIKE_POLAR, static_cast<const T*>(u), static_cast<const T*>(v),
                                                 static_cast<const ZStep<T>*>(table), int(nsteps), int(nmodes),
                                                 static_cast<const T*>(databar) + b0 * npts, static_cast<T*>(workspace) + b0 * nmodes,
                                                 batch * nmodes, vec);
                          });
}

size_t pm_modes_dot_workspace(int32_t dtype, int64_t nmodes, int64_t npts) {
    if (!real_dtype(dtype) || nmodes < 0 || npts < 0) return 0;
    return size_t(dot_chunks(npts)) * size_t(nmodes) * elem_of(dtype);
}

int pm_modes_dot(int32_t dtype, int64_t nmodes, int64_t npts, const void* modes, int64_t mode_stride, const void* v, void* out, void* workspace,
                 size_t workspace_bytes, void* stream) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "pm_modes_dot: dtype must be PM_F32 or PM_F64");
    if (!modes || !v || !out || nmodes < 0 || npts < 0 || (nmodes > 1 && mode_stride < npts) || nmodes > 65535 * int64_t(kDotModes) ||
        dot_chunks(npts) > INT32_MAX)
        return fail(PM_ERR_ARG, "pm_modes_dot: bad argument (null pointer, negative size or mode_stride < npts)");
    if (nmodes == 0) return 0;
    const size_t need = pm_modes_dot_workspace(dtype, nmodes, npts);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "pm_modes_dot: workspace of %zu bytes is smaller than the %zu pm_modes_dot_workspace asks for",
                    workspace_bytes, need);
    return by_rdtype(dtype, "pm_modes_dot", [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        T* partial = static_cast<T*>(workspace);
        const int64_t chunks = dot_chunks(npts);
        const dim3 grid(unsigned(chunks), unsigned((nmodes + kDotModes - 1) / kDotModes)), block(kThreads);
        const int vec = vec_ok(npts, {modes, v}) && mode_stride % kVec == 0;
        hipLaunchKernelGGL(modes_dot_kernel<T>, grid, block, 0, st, npts, int(nmodes), static_cast<const T*>(modes), mode_stride,
                           static_cast<const T*>(v), partial, vec);
        hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3(unsigned(nmodes)), block, 0, st, chunks, nmodes, partial, 0,
                           static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

}  // extern "C"
