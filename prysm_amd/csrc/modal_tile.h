// What the modal units csrc/zernike.hip, csrc/qpoly.hip, csrc/recur.hip and csrc/segmented.hip share (gfx950): the wave tile of points
// with its 16-byte loads and stores, the wave reduction, the skeleton of the deterministic projection around a unit's own table walk,
// the fixed-order second stage, and what the host halves need to launch over the tile (grids, the 16-byte test, the projection's
// checks, workspace and launches).  The walks, their step tables and the kernels stay with their units.
#pragma once
#include <initializer_list>

#include "pm_entry.h"
#include "pm_math.h"

namespace pm {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kVec = 4;

// A wave's tile is 64 * kVec consecutive points.  Lane l holds kVec / W runs of W = 16 / sizeof(T) consecutive points, run r at
// r * 64 * W + l * W, so every 16-byte vector load or store of the wave covers one contiguous KiB (fp64 lanes holding 4 consecutive
// points would store 32 bytes apart, half a line per instruction: 0.4 of copy bandwidth against 0.8-1.0 measured for fp32).
template <typename T>
struct Runs {
    static constexpr int W = 16 / sizeof(T), R = kVec / W;
    using vec = T __attribute__((ext_vector_type(W)));
    static __device__ __forceinline__ int64_t at(int64_t base, int lane, int q) { return base + (q / W) * 64 * W + lane * W + q % W; }
};

template <typename T>
__device__ __forceinline__ T wave_sum(T s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// the lane's kVec points of the wave tile at `base`; 0 past n (never stored).  full: the whole tile is inside and 16-byte aligned
template <bool NT = false, typename T>
__device__ __forceinline__ void load_pts(const T* __restrict__ p, int64_t base, int lane, int64_t n, bool full, T out[kVec]) {
    using RT = Runs<T>;
    if (full) {
#pragma unroll
        for (int r = 0; r < RT::R; ++r) {
            const auto* src = reinterpret_cast<const typename RT::vec*>(p + RT::at(base, lane, r * RT::W));
            const typename RT::vec q = NT ? __builtin_nontemporal_load(src) : *src;
#pragma unroll
            for (int e = 0; e < RT::W; ++e) out[r * RT::W + e] = q[e];
        }
    } else {
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
            const int64_t i = RT::at(base, lane, q);
            out[q] = i < n ? p[i] : T(0);
        }
    }
}

template <bool NT, typename T>
__device__ __forceinline__ void store_pts(T* __restrict__ p, int64_t base, int lane, int64_t n, bool full, const T z[kVec]) {
    using RT = Runs<T>;
    if (full) {
#pragma unroll
        for (int r = 0; r < RT::R; ++r) {
            typename RT::vec q;
#pragma unroll
            for (int e = 0; e < RT::W; ++e) q[e] = z[r * RT::W + e];
            auto* dst = reinterpret_cast<typename RT::vec*>(p + RT::at(base, lane, r * RT::W));
            if (NT)
                __builtin_nontemporal_store(q, dst);
            else
                *dst = q;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kVec; ++q) {
            const int64_t i = RT::at(base, lane, q);
            if (i < n) p[i] = z[q];
        }
    }
}

__device__ __forceinline__ int64_t wave_tile(int wave) { return (int64_t(blockIdx.x) * kWaves + wave) * 64 * kVec; }

// ---------------------------------------------------------------- projection: the reduction around a unit's table walk
// out[b][k] = sum_p g[b][p] F_k[p], the adjoint of a modal sum with respect to its coefficients, for NB vectors g per walk.  A walk
// visits its steps E = 8 / NB at a time: emit(j, k, ...) at the j-th step of a group when it writes mode k, flush() after every group.
// Each wave sums its 64 x kVec points per step (emit), reduces over its lanes -- the butterflies of the E steps of a group run
// together, 8 independent chains at a time -- and lane 0 adds the totals into LDS accumulators of the wave's own, (wave, b, k) (flush);
// at the end the workgroup adds its waves in order and hands one partial per (b, k) to the kernel's `put`.  reduce_partials_kernel
// then sums the workgroups' partials in a fixed order.  No atomics, so every run and every graph replay gives the same bits.
//
// A kernel: project_begin, then per wave tile -- the wave stays together through that loop (a shuffle needs every lane) and masks its
// own tail -- load the coordinates and g, clear() a ProjectStep, call its walk with emit and flush forwarded to it; project_end last.

// zeroes the kWaves * nacc accumulators of the workgroup (nacc = NB * nmodes) and returns them; the wave's own start at wave * nacc
template <typename T>
__device__ __forceinline__ T* project_begin(unsigned char* smem, int nacc, int tid) {
    T* sacc = reinterpret_cast<T*>(smem);
    for (int e = tid; e < kWaves * nacc; e += kThreads) sacc[e] = T(0);
    __syncthreads();
    return sacc;
}

template <typename T, int NB>
struct ProjectStep {
    static constexpr int E = 8 / NB;
    int slot[E];          // before red: with the arrays in the other order the compiler lays the NB = 1 and 2 kernels out differently
    T red[NB][E];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < E; ++j) slot[j] = -1;
    }
    // the lane sums of step j of the group, which writes mode k: sum_q gg[b][q] * value(q), or * z[q]
    template <typename Value>
    __device__ __forceinline__ void emit_each(int j, int k, const T (&gg)[NB][kVec], Value&& value) {
        slot[j] = k;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            T s = T(0);
#pragma unroll
            for (int q = 0; q < kVec; ++q) s += gg[b][q] * value(q);
            red[b][j] = s;
        }
    }
    __device__ __forceinline__ void emit(int j, int k, const T (&gg)[NB][kVec], const T z[kVec]) {
        emit_each(j, k, gg, [&](int q) { return z[q]; });
    }
    // the group's butterflies, then lane 0's adds into the wave's accumulators wacc[b * nmodes + k]
    __device__ __forceinline__ void flush(T* wacc, int nmodes, int lane) {
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
    }
};

// the waves' accumulators added in order: put(o, sum) for o = b * nmodes + k
template <typename T, typename Put>
__device__ __forceinline__ void project_end(const T* sacc, int nacc, int tid, Put&& put) {
    __syncthreads();
    for (int o = tid; o < nacc; o += kThreads) {
        T s = sacc[o];
        for (int w = 1; w < kWaves; ++w) s += sacc[w * nacc + o];
        put(o, s);
    }
}

// ---------------------------------------------------------------- second stage: out[o] (+)= sum over groups of partial[group][o]
template <typename T>
__global__ __launch_bounds__(kThreads) void reduce_partials_kernel(int64_t ngroups, int64_t nout, const T* __restrict__ partial, int accumulate,
                                                                   T* __restrict__ out) {
    __shared__ T sw[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o = blockIdx.x;
    T s = T(0);
    for (int64_t gi = tid; gi < ngroups; gi += kThreads) s += partial[gi * nout + o];
    s = wave_sum(s);
    if (lane == 0) sw[wave] = s;
    __syncthreads();
    if (tid == 0) {
        T t = sw[0];
        for (int w = 1; w < kWaves; ++w) t += sw[w];
        out[o] = accumulate ? out[o] + t : t;
    }
}

// ---------------------------------------------------------------- host: launching over the wave tile
constexpr int kMaxProjectGroups = 1024;                 // workgroups of a projection (grid-stride beyond): the partial count per output
constexpr size_t kProjectLds = 64 * 1024;               // per-wave accumulators of a projection workgroup

// 16-byte vectors: every plane of npts points starts on a 16-byte boundary, and so does every pointer given (null: not read)
int vec_ok(int64_t npts, std::initializer_list<const void*> ptrs) {
    if (npts % kVec) return 0;
    for (const void* p : ptrs)
        if (!aligned(p, 16)) return 0;
    return 1;
}

int64_t tiles_of(int64_t npts) { return (npts + int64_t(kThreads) * kVec - 1) / (int64_t(kThreads) * kVec); }

int64_t project_groups(int64_t npts, int64_t most = kMaxProjectGroups) { return std::max<int64_t>(1, std::min(tiles_of(npts), most)); }

// the LDS of a projection workgroup: an accumulator per (wave, coefficient vector, mode)
size_t project_lds(int64_t nb, int64_t nmodes, size_t elem) { return size_t(kWaves) * size_t(nb) * size_t(nmodes) * elem; }

// the largest of 8, 4, 2, 1 coefficient vectors per projection walk whose per-wave accumulators fit kProjectLds
int project_nb(int32_t dtype, int64_t nmodes, int64_t batch) {
    for (int nb = 8; nb > 1; nb >>= 1)
        if (nb <= batch && project_lds(nb, nmodes, elem_of(dtype)) <= kProjectLds) return nb;
    return 1;
}

// the workspace of a projection over `pts` points: one partial per (workgroup, output), `outputs` = batch * outputs of one vector
size_t project_workspace_bytes(int32_t dtype, int64_t pts, size_t outputs, int64_t most_groups = kMaxProjectGroups) {
    return size_t(project_groups(pts, most_groups)) * outputs * elem_of(dtype);
}

// What the pm_*_project entry points do once their own arguments are checked: the three checks every projection shares, with the
// empty-shape return between the second and the third, then the two stages.  `per_vector` is the number of outputs of one of the
// `batch` vectors -- `outputs` spells that product in the first refusal -- each of them one of `nmodes` accumulators (`noun`: what a
// mode is called) of a workgroup.  piece(real, nb, b0, groups, lds, stream) launches the unit's kernel<T, NB> for the vectors
// b0 .. b0 + NB - 1 over `groups` workgroups with `lds` bytes of LDS; its partials have the row length batch * per_vector.
template <typename Piece>
int launch_project(const char* name, const char* outputs, const char* noun, int32_t dtype, int64_t pts, int64_t nmodes, int64_t batch,
                   int64_t per_vector, int32_t accumulate, void* out, void* workspace, size_t workspace_bytes, void* stream,
                   int64_t most_groups, Piece&& piece) {
    const int64_t nout = batch * per_vector;
    if (nout > INT32_MAX) return fail(PM_ERR_ARG, "%s: batch * %s is too large", name, outputs);
    if (project_lds(1, nmodes, elem_of(dtype)) > kProjectLds)
        return fail(PM_ERR_UNSUPPORTED, "%s: %lld %s do not fit the workgroup's accumulators", name, (long long)nmodes, noun);
    if (nout == 0) return 0;
    const size_t need = project_workspace_bytes(dtype, pts, size_t(nout), most_groups);
    if (!workspace || workspace_bytes < need)
        return fail(PM_ERR_WORKSPACE, "%s: workspace of %zu bytes is smaller than the %zu %s_workspace asks for", name, workspace_bytes, need,
                    name);
    return by_rdtype(dtype, name, [&](auto real) {
        using T = decltype(real);
        hipStream_t st = PM_STREAM(stream);
        const int64_t groups = project_groups(pts, most_groups);
        for (int64_t b0 = 0; b0 < batch;)
            b0 += by_nb(batch - b0, project_nb(dtype, nmodes, batch),
                        [&](auto nb) { piece(real, nb, b0, groups, project_lds(nb, nmodes, sizeof(T)), st); });
        hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3(unsigned(nout)), dim3(kThreads), 0, st, groups, nout,
                           static_cast<const T*>(workspace), accumulate != 0, static_cast<T*>(out));
        return int(hipGetLastError());
    });
}

}  // namespace
}  // namespace pm
