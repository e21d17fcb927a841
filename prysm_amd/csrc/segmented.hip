// Segmented apertures: the per-segment OPD of CompositeHexagonalAperture.compose_opd (prysm/segmented.py:178-285) and its adjoint with
// respect to the segment coefficients (gfx950):
//
//  - pm_segment_compose: out[b][p] (+)= sum over the segments s covering p of mask_s[p] * sum_k c[b][s][k] Z_{s,k}[p], one launch for up
//    to 8 coefficient stacks.  Pixel-major: each point reads its cover list (the segments whose window covers it with a non-zero mask,
//    in segment order, at most ncover of them) one pass at a time; a pass's lanes hold different segments, but the mode index stays
//    wave-uniform, so the Zernike walk (zernike_walk.h) is shared by the whole wave.  A wave whose points have no segment left in a
//    pass stops there (the lists are packed to the front).
//  - pm_segment_project: out[b][s][k] = sum over the window of s of mask_s[p] Z_{s,k}[p] g[b][p].  Segment-major: workgroup (i, s)
//    takes slice i of segment s's window, so the segment is uniform; the reduction, the second launch that sums the per-workgroup
//    partials in a fixed order and the launcher are modal_tile.h's, as for pm_zernike_project.  No atomics: bitwise reproducible.
//
// Z_{s,k} comes from one of two sources, a template parameter of both kernels: the Zernike table walk at the local coordinates of the
// segment's grid source ((x - cx) / nr, (y - cy) / nr at the same position in the source's window), or a strided read of a stored
// (K, h, w) basis of the grid source.  The plan (SegDesc per segment, the packed masks, the cover planes) is built on the host by
// prysm_amd/segmented.py and checked by pm_segment_plan_check before it is uploaded.
#include "zernike_walk.h"

namespace pm {
namespace {

constexpr int kSegGroups = 256;                          // workgroups per segment of a projection (grid-stride beyond)

// one segment of the plan (prysm_amd/segmented.py: _DESC_DTYPE)
struct SegDesc {
    int32_t y0, x0, h, w;         // the segment's window in the grid
    int32_t gy0, gx0, pad0, pad1; // the window of its grid source (same h, w)
    int64_t moff, boff;           // its mask in the packed masks; the (K, h, w) stored basis of its grid source
    double cx, cy, nr, pad2;      // the grid source's centre and the normalisation radius
};
static_assert(sizeof(SegDesc) == 80, "SegDesc layout is shared with segmented._DESC_DTYPE");

// Z_k of a stored basis: point q reads bp[q][k * hw[q]] (hw = 0 for a point of no segment: it rereads one valid element)
template <int E, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void stored_walk(const T* const bp[kVec], const int64_t hw[kVec], int nmodes, Emit&& emit, Flush&& flush) {
    for (int k0 = 0; k0 < nmodes; k0 += E) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (k0 + j >= nmodes) break;
            T z[kVec];
#pragma unroll
            for (int q = 0; q < kVec; ++q) z[q] = bp[q][int64_t(k0 + j) * hw[q]];
            emit(j, k0 + j, z);
        }
        flush();
    }
}

template <int SRC, int E, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void seg_modes(const T u[kVec], const T v[kVec], const T* const bp[kVec], const int64_t hw[kVec],
                                          const ZStep<T>* __restrict__ table, int nsteps, int nmodes, Emit&& emit, Flush&& flush) {
    if constexpr (SRC == PM_SEGMENT_ZERNIKE)
        walk<E>(false, u, v, table, nsteps, nmodes, emit, flush);
    else
        stored_walk<E, T>(bp, hw, nmodes, emit, flush);
}

// point (wr, wc) of segment d's window (li = wr * w + wc): its local coordinates, or its stored-basis pointer
template <int SRC, typename T>
__device__ __forceinline__ void seg_point(const SegDesc& d, int wr, int wc, int li, int cols, const T* __restrict__ x,
                                          const T* __restrict__ y, const T* __restrict__ basis, T& u, T& v, const T*& bp, int64_t& hw) {
    if constexpr (SRC == PM_SEGMENT_ZERNIKE) {
        const int64_t gp = int64_t(d.gy0 + wr) * cols + d.gx0 + wc;
        const T nr = T(d.nr);
        u = (x[gp] - T(d.cx)) / nr;
        v = (y[gp] - T(d.cy)) / nr;
    } else {
        bp = basis + d.boff + li;
        hw = int64_t(d.h) * d.w;
    }
}

// ---------------------------------------------------------------- compose: pixel-major, NB coefficient stacks per walk
template <int SRC, typename T, int NB>
__global__ __launch_bounds__(kThreads) void segment_compose_kernel(int rows, int cols, const T* __restrict__ x, const T* __restrict__ y,
                                                                   int nseg, const SegDesc* __restrict__ plan, const T* __restrict__ masks,
                                                                   int ncover, const int16_t* __restrict__ cover,
                                                                   const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                                   const T* __restrict__ basis, const T* __restrict__ coefs, int accumulate,
                                                                   T* __restrict__ out, int vec) {
    using RT = Runs<T>;
    const int lane = threadIdx.x & 63;
    const int64_t npts = int64_t(rows) * cols;
    const int64_t base = wave_tile(threadIdx.x >> 6);
    if (base >= npts) return;
    const bool full = vec && base + 64 * kVec <= npts;
    T tot[NB][kVec];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (accumulate)
            load_pts(out + int64_t(b) * npts, base, lane, npts, full, tot[b]);
        else
#pragma unroll
            for (int q = 0; q < kVec; ++q) tot[b][q] = T(0);
    }
    for (int pass = 0; pass < ncover; ++pass) {
        int sid[kVec];
        int any = 0;
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
            const int64_t i = RT::at(base, lane, q);
            sid[q] = i < npts ? int(cover[int64_t(pass) * npts + i]) : -1;
            any |= sid[q] >= 0;
        }
        if (!__any(any)) break;             // the lists are packed to the front: no later pass has a segment here either
        T u[kVec], v[kVec], m[kVec], acc[NB][kVec];
        const T* bp[kVec];
        int64_t hw[kVec];
        int crow[kVec];
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
            u[q] = v[q] = m[q] = T(0);
            bp[q] = basis;
            hw[q] = 0;
            crow[q] = 0;
            if (sid[q] >= 0) {
                const SegDesc d = plan[sid[q]];
                const int i = int(RT::at(base, lane, q));
                const int r = i / cols, c = i - r * cols;
                const int wr = r - d.y0, wc = c - d.x0, li = wr * d.w + wc;
                m[q] = masks[d.moff + li];
                seg_point<SRC>(d, wr, wc, li, cols, x, y, basis, u[q], v[q], bp[q], hw[q]);
                crow[q] = sid[q] * nmodes;
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < kVec; ++q) acc[b][q] = T(0);
        seg_modes<SRC, 1>(u, v, bp, hw, table, nsteps, nmodes,
                          [&](int, int k, const T z[kVec]) {
#pragma unroll
                              for (int b = 0; b < NB; ++b) {
                                  const T* cb = coefs + int64_t(b) * nseg * nmodes + k;
#pragma unroll
                                  for (int q = 0; q < kVec; ++q) acc[b][q] += cb[crow[q]] * z[q];
                              }
                          },
                          [] {});
        // out[win] += tile * mask, segment by segment in segment order (compose_opd)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < kVec; ++q)
                if (sid[q] >= 0) tot[b][q] += acc[b][q] * m[q];
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) store_pts<false>(out + int64_t(b) * npts, base, lane, npts, full, tot[b]);
}

// ---------------------------------------------------------------- projection: segment-major, one partial per (workgroup, b, s, k)
// Workgroup (blockIdx.x, s) walks its slice of the window of s with the reduction of modal_tile.h around seg_modes(); g is weighted
// by the mask as it is loaded.  The partials go to partial[blockIdx.x][b0 + b][s][k] (row length ld = B * nseg * nmodes).
template <int SRC, typename T, int NB>
__global__ __launch_bounds__(kThreads) void segment_project_kernel(int rows, int cols, const T* __restrict__ x, const T* __restrict__ y,
                                                                   int nseg, const SegDesc* __restrict__ plan, const T* __restrict__ masks,
                                                                   const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                                                   const T* __restrict__ basis, const T* __restrict__ g,
                                                                   T* __restrict__ partial, int64_t ld) {
    using RT = Runs<T>;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.y;
    const SegDesc d = plan[s];
    const int64_t npts = int64_t(rows) * cols, hwin = int64_t(d.h) * d.w;
    const int nacc = NB * nmodes;
    T* sacc = project_begin<T>(smem, nacc, tid);
    T* wacc = sacc + wave * nacc;
    for (int64_t base = wave_tile(wave); base < hwin; base += int64_t(gridDim.x) * kThreads * kVec) {
        T u[kVec], v[kVec], wg[NB][kVec];
        const T* bp[kVec];
        int64_t hw[kVec];
        ProjectStep<T, NB> step;
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
            const int64_t i = RT::at(base, lane, q);
            u[q] = v[q] = T(0);
            bp[q] = basis;
            hw[q] = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b) wg[b][q] = T(0);
            if (i < hwin) {
                const int li = int(i), wr = li / d.w, wc = li - wr * d.w;
                const T m = masks[d.moff + li];
                const int64_t gp = int64_t(d.y0 + wr) * cols + d.x0 + wc;
#pragma unroll
                for (int b = 0; b < NB; ++b) wg[b][q] = m * g[int64_t(b) * npts + gp];
                seg_point<SRC>(d, wr, wc, li, cols, x, y, basis, u[q], v[q], bp[q], hw[q]);
            }
        }
        step.clear();
        seg_modes<SRC, ProjectStep<T, NB>::E>(u, v, bp, hw, table, nsteps, nmodes, [&](int j, int k, const T z[kVec]) { step.emit(j, k, wg, z); },
                                              [&] { step.flush(wacc, nmodes, lane); });
    }
    project_end(sacc, nacc, tid, [&](int o, T sum) {
        const int b = o / nmodes, k = o - b * nmodes;
        partial[int64_t(blockIdx.x) * ld + (int64_t(b) * nseg + s) * nmodes + k] = sum;
    });
}

int check_common(const char* who, int32_t dtype, int32_t source, int64_t rows, int64_t cols, const void* x, const void* y, int64_t nseg,
                 const void* plan, const void* masks, const void* table, int64_t nsteps, int64_t nmodes, const void* basis, int64_t batch) {
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (source != PM_SEGMENT_ZERNIKE && source != PM_SEGMENT_STORED)
        return fail(PM_ERR_ARG, "%s: source must be PM_SEGMENT_ZERNIKE or PM_SEGMENT_STORED", who);
    if (rows < 0 || cols < 0 || nseg < 0 || nmodes < 0 || batch < 0 || nsteps < 0)
        return fail(PM_ERR_ARG, "%s: bad argument (negative size)", who);
    if (rows * cols > INT32_MAX || nseg > 32767 || nmodes > INT32_MAX || nsteps > INT32_MAX)
        return fail(PM_ERR_ARG, "%s: grid of %lld x %lld, %lld segments or %lld modes is too large", who, (long long)rows, (long long)cols,
                    (long long)nseg, (long long)nmodes);
    if (!plan || !masks) return fail(PM_ERR_ARG, "%s: bad argument (null plan or masks)", who);
    if (source == PM_SEGMENT_ZERNIKE && (!x || !y || !table))
        return fail(PM_ERR_ARG, "%s: the Zernike source needs x, y and the step table", who);
    if (source == PM_SEGMENT_STORED && !basis) return fail(PM_ERR_ARG, "%s: the stored source needs the basis", who);
    return 0;
}

// calls f with the source of Z_{s,k} (checked before) as a std::integral_constant, the template parameter of both kernels
template <typename F>
int by_source(int32_t source, F&& f) {
    if (source == PM_SEGMENT_ZERNIKE) return f(std::integral_constant<int, PM_SEGMENT_ZERNIKE>{});
    return f(std::integral_constant<int, PM_SEGMENT_STORED>{});
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_segment_plan_check(int64_t rows, int64_t cols, int64_t nseg, const void* plan, int64_t mask_elems, int64_t nmodes,
                          int64_t basis_elems) {
    if (!plan || rows < 0 || cols < 0 || nseg < 0 || nmodes < 0 || mask_elems < 0)
        return fail(PM_ERR_ARG, "pm_segment_plan_check: bad argument (null plan or negative size)");
    const SegDesc* d = static_cast<const SegDesc*>(plan);
    for (int64_t s = 0; s < nseg; ++s) {
        const SegDesc& e = d[s];
        const int64_t hw = int64_t(e.h) * e.w;
        if (e.h < 0 || e.w < 0 || e.y0 < 0 || e.x0 < 0 || e.y0 + int64_t(e.h) > rows || e.x0 + int64_t(e.w) > cols)
            return fail(PM_ERR_ARG, "pm_segment_plan_check: segment %lld: window outside the %lld x %lld grid", (long long)s, (long long)rows,
                        (long long)cols);
        if (e.gy0 < 0 || e.gx0 < 0 || e.gy0 + int64_t(e.h) > rows || e.gx0 + int64_t(e.w) > cols)
            return fail(PM_ERR_ARG, "pm_segment_plan_check: segment %lld: grid source window outside the grid", (long long)s);
        if (e.moff < 0 || e.moff + hw > mask_elems)
            return fail(PM_ERR_ARG, "pm_segment_plan_check: segment %lld: mask outside the %lld packed elements", (long long)s,
                        (long long)mask_elems);
        if (basis_elems >= 0 && (e.boff < 0 || e.boff + nmodes * hw > basis_elems))
            return fail(PM_ERR_ARG, "pm_segment_plan_check: segment %lld: stored basis outside the %lld elements", (long long)s,
                        (long long)basis_elems);
        if (!(e.nr > 0.0)) return fail(PM_ERR_ARG, "pm_segment_plan_check: segment %lld: normalization radius must be > 0", (long long)s);
    }
    return 0;
}

int pm_segment_compose(int32_t dtype, int32_t source, int64_t rows, int64_t cols, const void* x, const void* y, int64_t nseg, const void* plan,
                       const void* masks, int64_t ncover, const void* cover, const void* table, int64_t nsteps, int64_t nmodes,
                       const void* basis, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream) {
    if (int rc = check_common("pm_segment_compose", dtype, source, rows, cols, x, y, nseg, plan, masks, table, nsteps, nmodes, basis, batch))
        return rc;
    if (!out || !coefs || ncover < 0 || ncover > nseg || (ncover && !cover))
        return fail(PM_ERR_ARG, "pm_segment_compose: bad argument (null out, coefs or cover, or ncover outside [0, nseg])");
    if (rows * cols == 0 || batch == 0) return 0;
    return by_rdtype(dtype, "pm_segment_compose", [&](auto real) {
        return by_source(source, [&](auto src) {
            using T = decltype(real);
            const T *xp = static_cast<const T*>(x), *yp = static_cast<const T*>(y), *mp = static_cast<const T*>(masks);
            const T *bp = static_cast<const T*>(basis), *c = static_cast<const T*>(coefs);
            const ZStep<T>* steps = static_cast<const ZStep<T>*>(table);
            T* o = static_cast<T*>(out);
            const int64_t npts = rows * cols;
            const dim3 grid{unsigned(tiles_of(npts))}, block{kThreads};
            const int vec = vec_ok(npts, {out});
            for (int64_t b0 = 0; b0 < batch;)
                b0 += by_nb(batch - b0, 8, [&](auto nb) {
                    hipLaunchKernelGGL((segment_compose_kernel<decltype(src)::value, T, decltype(nb)::value>), grid, block, 0, PM_STREAM(stream),
                                       int(rows), int(cols), xp, yp, int(nseg), static_cast<const SegDesc*>(plan), mp, int(ncover),
                                       static_cast<const int16_t*>(cover), steps, int(nsteps), int(nmodes), bp, c + b0 * nseg * nmodes,
                                       accumulate != 0, o + b0 * npts, vec);
                });
            return int(hipGetLastError());
        });
    });
}

size_t pm_segment_project_workspace(int32_t dtype, int64_t window_pts, int64_t nseg, int64_t nmodes, int64_t batch) {
    if (!real_dtype(dtype) || window_pts < 0 || nseg < 0 || nmodes < 0 || batch < 0) return 0;
    return project_workspace_bytes(dtype, window_pts, size_t(batch) * size_t(nseg) * size_t(nmodes), kSegGroups);
}

int pm_segment_project(int32_t dtype, int32_t source, int64_t rows, int64_t cols, const void* x, const void* y, int64_t nseg, const void* plan,
                       const void* masks, int64_t window_pts, const void* table, int64_t nsteps, int64_t nmodes, const void* basis,
                       int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_common("pm_segment_project", dtype, source, rows, cols, x, y, nseg, plan, masks, table, nsteps, nmodes, basis, batch))
        return rc;
    if (!out || !databar || window_pts < 0 || window_pts > rows * cols)
        return fail(PM_ERR_ARG, "pm_segment_project: bad argument (null out or databar, or window_pts outside [0, rows * cols])");
    return launch_project(
        "pm_segment_project", "nseg * nmodes", "modes", dtype, window_pts, nmodes, batch, nseg * nmodes, 0, out, workspace, workspace_bytes, stream,
        kSegGroups, [&](auto real, auto nb, int64_t b0, int64_t groups, size_t lds, hipStream_t st) {
            by_source(source, [&](auto src) {
                using T = decltype(real);
                hipLaunchKernelGGL((segment_project_kernel<decltype(src)::value, T, decltype(nb)::value>), dim3(unsigned(groups), unsigned(nseg)),
                                   dim3(kThreads), lds, st, int(rows), int(cols), static_cast<const T*>(x), static_cast<const T*>(y), int(nseg),
                                   static_cast<const SegDesc*>(plan), static_cast<const T*>(masks), static_cast<const ZStep<T>*>(table),
                                   int(nsteps), int(nmodes), static_cast<const T*>(basis), static_cast<const T*>(databar) + b0 * rows * cols,
                                   static_cast<T*>(workspace) + b0 * nseg * nmodes, batch * nseg * nmodes);
                return 0;
            });
        });
}

}  // extern "C"
