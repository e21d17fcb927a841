// The two-pass reduction of the kernel units (csrc/optym.hip, csrc/imagechain.hip, csrc/bayer.hip, csrc/thinfilm.hip, csrc/ee.hip): a
// first launch leaves one partial per workgroup and value in a workspace, partial[wg * NS + k], and a second launch of ONE workgroup
// combines the partials.  Both stages end in the same tree over LDS, red[tid] = op(red[tid], red[tid + s]) for s = THREADS / 2 .. 1,
// so a launch shape combines the same numbers in the same order run after run: no atomics, the same bits every run.
//
// A unit keeps its first-stage element loop and the tail of its second stage; the tree, the loop over the partials and the barriers
// between them are here, once.  First stages that combine across lanes with shuffles add in another order and are not on this header.
#pragma once
#include <algorithm>

#include "pm_internal.h"

namespace pm {

// the combining operations.  The two maxima differ on purpose: FoldMax never takes a NaN, FoldNanMax hands one through as numpy's max does
struct FoldSum {
    template <typename V> static __device__ __forceinline__ V of(V u, V w) { return u + w; }
};
struct FoldMax {
    template <typename V> static __device__ __forceinline__ V of(V u, V w) { return w > u ? w : u; }
};
struct FoldNanMax {
    template <typename V> static __device__ __forceinline__ V of(V u, V w) { return (u != u || u > w) ? u : w; }
};

// The tree: red[k][0] is the combination of a[k] over the workgroup's THREADS threads.  Every thread has passed the barrier that
// follows the last step when this returns, so every thread may read red[k][0]; `tid` is the caller's numbering of its threads
template <int THREADS, typename Op, int NS, typename V>
__device__ __forceinline__ auto& wg_tree(int tid, const V (&a)[NS]) {
    __shared__ V red[NS][THREADS];
#pragma unroll
    for (int k = 0; k < NS; ++k) red[k][tid] = a[k];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int k = 0; k < NS; ++k) red[k][tid] = Op::of(red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    return red;
}

// first stage: the workgroup's combination of a[k] to dst[k], thread k storing it
template <int THREADS, typename Op, int NS, typename V, typename D>
__device__ __forceinline__ void wg_fold(int tid, const V (&a)[NS], D* __restrict__ dst) {
    const auto& red = wg_tree<THREADS, Op>(tid, a);
    if (tid < NS) dst[tid] = D(red[tid][0]);
}

// the same, handed to every thread
template <int THREADS, typename Op, int NS, typename V>
__device__ __forceinline__ void wg_total(int tid, const V (&a)[NS], V (&total)[NS]) {
    const auto& red = wg_tree<THREADS, Op>(tid, a);
#pragma unroll
    for (int k = 0; k < NS; ++k) total[k] = red[k][0];
}

// second stage, one workgroup: total[k] = the combination of partial[i * NS + k] over i < nparts, starting from `init`, in every thread.
// One value after the other, so a thread holds one running value at a time whatever NS is; N, int or int64_t, is the caller's count
template <int THREADS, typename Op, int NS, typename N>
__device__ __forceinline__ void fold_partials(int tid, N nparts, const double* __restrict__ partial, double init, double (&total)[NS]) {
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        a[k] = init;
        for (N i = tid; i < nparts; i += THREADS) a[k] = Op::of(a[k], partial[int64_t(i) * NS + k]);
    }
    wg_total<THREADS, Op>(tid, a, total);
}

// workgroups of a first stage over n elements, `threads` of them per workgroup and trip: at most `most`, as many partials per value
inline int reduce_groups(int64_t n, int threads, int most) { return int(std::min<int64_t>(most, (n + threads - 1) / threads)); }

}  // namespace pm
