// Forbes Q polynomials without a stored basis (prysm/polynomials/qpoly.py: Qbfs, Qcon, Q2D) (gfx950):
//
//  - pm_qpoly_basis: the K planes of Qbfs_seq / Qcon_seq / Q2d_seq, one launch.
//  - pm_qpoly_sum: sum_k c[b][k] Q_k for B coefficient vectors (Q2d_sum, Qcon_sum, compute_z_Qbfs, compute_z_Q2d), the basis
//    evaluated once per point per group of up to 8 vectors and never stored.
//  - pm_qpoly_project: sum_p g[b][p] Q_k[p] (the adjoint of pm_qpoly_sum with respect to c), same walk.
//
// Every point walks one table of steps built on the host (prysm_amd/polynomials/qpoly_plan.py): modes grouped by |m|, one step per
// order n.  The auxiliary polynomial P (a three-term recurrence in x = u^2, or a cubic seed), the orthogonalised Q (Q_n = (P_n -
// g Q_{n-1} - h Q_{n-2}) / f) and z^|m| (z = x + i y) stay in registers, so u^|m| cos(|m| t) = Re z^|m| and u^|m| sin(|m| t) =
// Im z^|m| need no trigonometry in the loop.  Radial tables (Qbfs, Qcon) take PM_QPOLY_RADIAL points: u only, no angle read.  The
// step index is uniform, so the table is read through the scalar cache.  A step whose slot is outside [0, nmodes) writes nothing.
//
// The tile, its 16-byte loads and stores, the projection's reduction around qwalk, its fixed-order second stage and the host's launch
// helpers are modal_tile.h's: per-workgroup partials in the caller's workspace, then a fixed-order sum.  No atomics, so every run and
// every graph replay gives the same bits.
#include "modal_tile.h"

namespace pm {
namespace {

enum { QS_RESET = 1, QS_SEED = 2, QS_ADV = 4 };
enum { QP_NONE = 0, QP_BFS = 1, QP_CON = 2, QP_COS = 3, QP_SIN = 4 };

// one step of the table (qpoly_plan.step_dtype)
template <typename T>
struct QStep {
    T a, b, c, d, g, h, rf, w;
    int32_t op, part, slot, dm;
};
static_assert(sizeof(QStep<float>) == 48 && sizeof(QStep<double>) == 80, "QStep layout is shared with qpoly_plan.step_dtype");

// The walk of the step table over kVec points, E steps at a time: emit(j, slot, values) at the j-th step of a group that writes, then
// flush() after every group of E steps.  coords: PM_ZERNIKE_CARTESIAN (u, v) = (x, y), PM_ZERNIKE_POLAR (r, t), PM_QPOLY_RADIAL u
// only (z = u, angle 0).
template <int E, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void qwalk(int coords, const T u[kVec], const T v[kVec], const QStep<T>* __restrict__ table, int nsteps, int nmodes,
                                      Emit&& emit, Flush&& flush) {
    T X[kVec], zx[kVec], zy[kVec], pr[kVec], pi[kVec], p[kVec], pm[kVec], q1[kVec], q2[kVec];
#pragma unroll
    for (int q = 0; q < kVec; ++q) {
        if (coords == PM_ZERNIKE_POLAR) {
            T s, c;
            sincos_(v[q], &s, &c);
            zx[q] = u[q] * c;
            zy[q] = u[q] * s;
            X[q] = u[q] * u[q];
        } else if (coords == PM_ZERNIKE_CARTESIAN) {
            zx[q] = u[q];
            zy[q] = v[q];
            X[q] = u[q] * u[q] + v[q] * v[q];
        } else {
            zx[q] = u[q];
            zy[q] = T(0);
            X[q] = u[q] * u[q];
        }
        pr[q] = T(1);
        pi[q] = T(0);
        p[q] = pm[q] = q1[q] = q2[q] = T(0);
    }
    for (int s0 = 0; s0 < nsteps; s0 += E) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (s0 + j >= nsteps) break;
            const QStep<T> st = table[s0 + j];
            if (st.op & QS_RESET) {
                for (int d = 0; d < st.dm; ++d) {
#pragma unroll
                    for (int q = 0; q < kVec; ++q) {
                        const T r = pr[q] * zx[q] - pi[q] * zy[q];
                        pi[q] = pr[q] * zy[q] + pi[q] * zx[q];
                        pr[q] = r;
                    }
                }
#pragma unroll
                for (int q = 0; q < kVec; ++q) p[q] = pm[q] = q1[q] = q2[q] = T(0);
            }
            if (st.op & QS_SEED) {
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    pm[q] = p[q];
                    p[q] = st.a + X[q] * (st.b + X[q] * (st.c + X[q] * st.d));
                }
            } else if (st.op & QS_ADV) {
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    const T n = (st.a + st.b * X[q]) * p[q] - st.c * pm[q];
                    pm[q] = p[q];
                    p[q] = n;
                }
            }
            if (st.op & (QS_SEED | QS_ADV)) {
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    const T n = (p[q] - st.g * q1[q] - st.h * q2[q]) * st.rf;
                    q2[q] = q1[q];
                    q1[q] = n;
                }
            }
            if (st.part != QP_NONE && unsigned(st.slot) < unsigned(nmodes)) {
                T z[kVec];
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    const T wq = st.w * q1[q];
                    const T pre = st.part == QP_BFS ? X[q] * (T(1) - X[q])
                                  : st.part == QP_CON ? X[q] * X[q]
                                  : st.part == QP_COS ? pr[q] : pi[q];
                    z[q] = wq * pre;
                }
                emit(j, st.slot, z);
            }
        }
        flush();
    }
}

// the coordinates of the lane's points: v is not read for radial points
template <typename T>
__device__ __forceinline__ void load_coords(int coords, const T* __restrict__ u, const T* __restrict__ v, int64_t base, int lane, int64_t npts,
                                            bool full, T uu[kVec], T vv[kVec]) {
    load_pts(u, base, lane, npts, full, uu);
    if (coords != PM_QPOLY_RADIAL)
        load_pts(v, base, lane, npts, full, vv);
    else
#pragma unroll
        for (int q = 0; q < kVec; ++q) vv[q] = T(0);
}

// ---------------------------------------------------------------- basis: K planes, write-bound
template <typename T>
__global__ __launch_bounds__(kThreads) void qpoly_basis_kernel(int64_t npts, int coords, const T* __restrict__ u, const T* __restrict__ v,
                                                               const QStep<T>* __restrict__ table, int nsteps, int nmodes, T* __restrict__ out,
                                                               int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T uu[kVec], vv[kVec];
    load_coords(coords, u, v, base, lane, npts, full, uu, vv);
    qwalk<1>(coords, uu, vv, table, nsteps, nmodes,
             [&](int, int k, const T z[kVec]) { store_pts<true>(out + int64_t(k) * npts, base, lane, npts, full, z); }, [] {});
}

// ---------------------------------------------------------------- sum: NB coefficient vectors per walk
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void qpoly_sum_kernel(int64_t npts, int coords, const T* __restrict__ u, const T* __restrict__ v,
                                                             const QStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                             const T* __restrict__ coefs, int accumulate, T* __restrict__ out, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T uu[kVec], vv[kVec], acc[NB][kVec];
    load_coords(coords, u, v, base, lane, npts, full, uu, vv);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < kVec; ++q) acc[b][q] = T(0);
    qwalk<1>(coords, uu, vv, table, nsteps, nmodes,
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
// The reduction of modal_tile.h around qwalk(): partial[group][b0 + b][k], row length ld = B * nmodes.
template <typename T, int NB>
__global__ __launch_bounds__(kThreads) void qpoly_project_kernel(int64_t npts, int coords, const T* __restrict__ u, const T* __restrict__ v,
                                                                 const QStep<T>* __restrict__ table, int nsteps, int nmodes,
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
        load_coords(coords, u, v, base, lane, npts, full, uu, vv);
#pragma unroll
        for (int b = 0; b < NB; ++b) load_pts(g + int64_t(b) * npts, base, lane, npts, full, gg[b]);
        step.clear();
        qwalk<ProjectStep<T, NB>::E>(coords, uu, vv, table, nsteps, nmodes, [&](int j, int k, const T z[kVec]) { step.emit(j, k, gg, z); },
                                     [&] { step.flush(wacc, nmodes, lane); });
    }
    project_end(sacc, nacc, tid, [&](int o, T s) { partial[int64_t(blockIdx.x) * ld + o] = s; });
}

int check_walk(const char* who, int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
               int64_t nmodes) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (coords != PM_ZERNIKE_CARTESIAN && coords != PM_ZERNIKE_POLAR && coords != PM_QPOLY_RADIAL)
        return fail(PM_ERR_ARG, "%s: coords must be PM_ZERNIKE_CARTESIAN, PM_ZERNIKE_POLAR or PM_QPOLY_RADIAL", who);
    if (!u || (!v && coords != PM_QPOLY_RADIAL) || !table || npts < 0 || nsteps < 0 || nmodes < 0 || nsteps > INT32_MAX ||
        nmodes > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (tiles_of(npts) > INT32_MAX) return fail(PM_ERR_ARG, "%s: %lld points is too many", who, (long long)npts);
    return 0;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_qpoly_basis(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                   int64_t nmodes, void* out, void* stream) {
    if (int rc = check_walk("pm_qpoly_basis", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out) return fail(PM_ERR_ARG, "pm_qpoly_basis: bad argument (null pointer)");
    if (npts == 0 || nmodes == 0) return 0;
    return by_rdtype(dtype, "pm_qpoly_basis", [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(qpoly_basis_kernel<T>, dim3(unsigned(tiles_of(npts))), dim3(kThreads), 0, PM_STREAM(stream), npts, coords,
                           static_cast<const T*>(u), static_cast<const T*>(v), static_cast<const QStep<T>*>(table), int(nsteps), int(nmodes),
                           static_cast<T*>(out), vec_ok(npts, {u, v, out}));
        return int(hipGetLastError());
    });
}

int pm_qpoly_sum(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                 int64_t nmodes, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream) {
    if (int rc = check_walk("pm_qpoly_sum", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !coefs || batch < 0) return fail(PM_ERR_ARG, "pm_qpoly_sum: bad argument (null pointer or negative batch)");
    if (npts == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_qpoly_sum", [&](auto real) {
        using T = decltype(real);
        const T *up = static_cast<const T*>(u), *vp = static_cast<const T*>(v), *c = static_cast<const T*>(coefs);
        const QStep<T>* steps = static_cast<const QStep<T>*>(table);
        T* o = static_cast<T*>(out);
        const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
        const int vec = vec_ok(npts, {u, v, out});
        for (int64_t b0 = 0; b0 < batch;)
            b0 += by_nb(batch - b0, 8, [&](auto nb) {
                hipLaunchKernelGGL((qpoly_sum_kernel<T, decltype(nb)::value>), grid, block, 0, PM_STREAM(stream), npts, coords, up, vp, steps,
                                   int(nsteps), int(nmodes), c + b0 * nmodes, accumulate != 0, o + b0 * npts, vec);
            });
        return int(hipGetLastError());
    });
}

size_t pm_qpoly_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch) {
    if (!real_dtype(dtype) || npts < 0 || nmodes < 0 || batch < 0) return 0;
    return project_workspace_bytes(dtype, npts, size_t(batch) * size_t(nmodes));
}

int pm_qpoly_project(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                     int64_t nmodes, int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_walk("pm_qpoly_project", dtype, coords, npts, u, v, table, nsteps, nmodes)) return rc;
    if (!out || !databar || batch < 0) return fail(PM_ERR_ARG, "pm_qpoly_project: bad argument (null pointer or negative batch)");
    const int vec = vec_ok(npts, {u, v, databar});
    return launch_project("pm_qpoly_project", "nmodes", "modes", dtype, npts, nmodes, batch, nmodes, 0, out, workspace, workspace_bytes, stream,
                          kMaxProjectGroups, [&](auto real, auto nb, int64_t b0, int64_t groups, size_t lds, hipStream_t st) {
                              using T = decltype(real);
                              hipLaunchKernelGGL((qpoly_project_kernel<T, decltype(nb)::value>), dim3(unsigned(groups)), dim3(kThreads), lds, st,
                                                 npts, coords, static_cast<const T*>(u), static_cast<const T*>(v),
                                                 static_cast<const QStep<T>*>(table), int(nsteps), int(nmodes),
                                                 static_cast<const T*>(databar) + b0 * npts, static_cast<T*>(workspace) + b0 * nmodes,
                                                 batch * nmodes, vec);
                          });
}

}  // extern "C"
