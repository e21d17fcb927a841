// The Zernike table walk shared by csrc/zernike.hip and csrc/segmented.hip (gfx950): the step layout, the wave tile of points, its
// 16-byte loads and stores, the walk itself and the fixed-order second stage of the deterministic reductions.  See zernike.hip for
// the table and prysm_amd/polynomials/zernike_plan.py for how it is built.  csrc/qpoly.hip walks a table of its own over the same tile.
// At the end: what the host halves of the three units need to launch over that tile (grids, the 16-byte test, the projection's LDS).
#pragma once
#include <initializer_list>

#include "pm_entry.h"

namespace pm {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kVec = 4;

enum { ZS_RESET = 1, ZS_ADV = 2 };
enum { ZP_NONE = 0, ZP_RADIAL = 1, ZP_COS = 2, ZP_SIN = 3 };

// one step of the table (zernike_plan.step_dtype)
template <typename T>
struct ZStep {
    T a, b, c, w;
    int32_t op, part, slot, dm;
};
static_assert(sizeof(ZStep<float>) == 32 && sizeof(ZStep<double>) == 48, "ZStep layout is shared with zernike_plan.step_dtype");

// A wave's tile is 64 * kVec consecutive points.  Lane l holds kVec / W runs of W = 16 / sizeof(T) consecutive points, run r at
// r * 64 * W + l * W, so every 16-byte vector load or store of the wave covers one contiguous KiB (fp64 lanes holding 4 consecutive
// points would store 32 bytes apart, half a line per instruction: 0.4 of copy bandwidth against 0.8-1.0 measured for fp32).
template <typename T>
struct Runs {
    static constexpr int W = 16 / sizeof(T), R = kVec / W;
    using vec = T __attribute__((ext_vector_type(W)));
    static __device__ __forceinline__ int64_t at(int64_t base, int lane, int q) { return base + (q / W) * 64 * W + lane * W + q % W; }
};

__device__ __forceinline__ void sincos_(float t, float* s, float* c) { sincosf(t, s, c); }
__device__ __forceinline__ void sincos_(double t, double* s, double* c) { sincos(t, s, c); }

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

// The walk of the step table over kVec points, E steps at a time: emit(j, slot, values) at the j-th step of a group that writes, then
// flush() after every group of E steps (the projection batches E reductions so that they overlap).
template <int E, typename T, typename Emit, typename Flush>
__device__ __forceinline__ void walk(bool polar, const T u[kVec], const T v[kVec], const ZStep<T>* __restrict__ table, int nsteps, int nmodes,
                                     Emit&& emit, Flush&& flush) {
    T X[kVec], zx[kVec], zy[kVec], pr[kVec], pi[kVec], p[kVec], pm[kVec];
#pragma unroll
    for (int q = 0; q < kVec; ++q) {
        if (polar) {
            T s, c;
            sincos_(v[q], &s, &c);
            zx[q] = u[q] * c;
            zy[q] = u[q] * s;
            X[q] = T(2) * (u[q] * u[q]) - T(1);
        } else {
            zx[q] = u[q];
            zy[q] = v[q];
            X[q] = T(2) * (u[q] * u[q] + v[q] * v[q]) - T(1);
        }
        pr[q] = T(1);
        pi[q] = T(0);
        p[q] = T(1);
        pm[q] = T(0);
    }
    for (int s0 = 0; s0 < nsteps; s0 += E) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            if (s0 + j >= nsteps) break;
            const ZStep<T> st = table[s0 + j];
            if (st.op & ZS_RESET) {
                for (int d = 0; d < st.dm; ++d) {
#pragma unroll
                    for (int q = 0; q < kVec; ++q) {
                        const T r = pr[q] * zx[q] - pi[q] * zy[q];
                        pi[q] = pr[q] * zy[q] + pi[q] * zx[q];
                        pr[q] = r;
                    }
                }
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    p[q] = T(1);
                    pm[q] = T(0);
                }
            }
            if (st.op & ZS_ADV) {
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    const T n = (st.a * X[q] + st.b) * p[q] - st.c * pm[q];
                    pm[q] = p[q];
                    p[q] = n;
                }
            }
            if (st.part != ZP_NONE && unsigned(st.slot) < unsigned(nmodes)) {
                T z[kVec];
#pragma unroll
                for (int q = 0; q < kVec; ++q) {
                    const T wp = st.w * p[q];
                    z[q] = st.part == ZP_RADIAL ? wp : wp * (st.part == ZP_COS ? pr[q] : pi[q]);
                }
                emit(j, st.slot, z);
            }
        }
        flush();
    }
}

__device__ __forceinline__ int64_t wave_tile(int wave) { return (int64_t(blockIdx.x) * kWaves + wave) * 64 * kVec; }

// ---------------------------------------------------------------- second stage: out[o] = sum over groups of partial[group][o]
template <typename T>
__global__ __launch_bounds__(kThreads) void reduce_partials_kernel(int64_t ngroups, int64_t nout, const T* __restrict__ partial,
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
        out[o] = t;
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

}  // namespace
}  // namespace pm
