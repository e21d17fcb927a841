// The row sweep of the pointwise kernels (csrc/pointwise.hip, csrc/bayer.hip): 2-D row-major work, one element per thread at a time.  A
// thread owns a column (64 adjacent columns per wavefront, so a row is read and written in whole lines) and strides over the rows,
// 64 x 4 threads per workgroup and at most 65535 workgroups down the rows; more rows are reached by the grid-stride step.
//
// An operation is a functor F.  F::column(c) is evaluated once per thread (what the operation hoists out of the row loop; NoColumn
// where there is nothing).  The per-element part comes in two forms, chosen at compile time by the sweep() that is called:
//     sweep(rows, cols, st, f)          F::point(r, c, column)       one array, grid.z unused (blockIdx.z is not read)
//     sweep(batch, rows, cols, st, f)   F::point(b, r, c, column)    a stack, member b = blockIdx.z (batch <= 65535)
//     sweep_heavy(rows, cols, st, f)    as the first, compiled for the 256 threads it is launched with
#pragma once
#include "pm_internal.h"

namespace pm {

struct NoColumn {};

template <bool STACK, typename F>
__device__ __forceinline__ void sweep_body(int64_t rows, int64_t cols, const F& f) {
    const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    if constexpr (STACK) {
        const int64_t b = blockIdx.z;
        const auto col = f.column(c);
        for (int64_t r = int64_t(blockIdx.y) * blockDim.y + threadIdx.y; r < rows; r += int64_t(gridDim.y) * blockDim.y) f.point(b, r, c, col);
    } else {
        const auto col = f.column(c);
        for (int64_t r = int64_t(blockIdx.y) * blockDim.y + threadIdx.y; r < rows; r += int64_t(gridDim.y) * blockDim.y) f.point(r, c, col);
    }
}

template <bool STACK, typename F>
__global__ void sweep_kernel(int64_t rows, int64_t cols, const F f) {
    sweep_body<STACK>(rows, cols, f);
}

// the same sweep for functors with a long per-element part (csrc/imagechain.hip: transcendental functions in double): the workgroup
// size is stated, so the register allocator may use what 256 threads leave it instead of spilling at the 128 of an unstated one
template <bool STACK, typename F>
__global__ __launch_bounds__(256) void sweep_kernel_heavy(int64_t rows, int64_t cols, const F f) {
    sweep_body<STACK>(rows, cols, f);
}

template <bool STACK, bool HEAVY = false, typename F>
int sweep_launch(int64_t batch, int64_t rows, int64_t cols, hipStream_t st, const F& f) {
    const dim3 block(64, 4);
    const int64_t gx = (cols + block.x - 1) / block.x;
    int64_t gy = (rows + block.y - 1) / block.y;
    if (gy > 65535) gy = 65535;
    if constexpr (HEAVY)
        hipLaunchKernelGGL((sweep_kernel_heavy<STACK, F>), dim3((unsigned)gx, (unsigned)gy, (unsigned)batch), block, 0, st, rows, cols, f);
    else
        hipLaunchKernelGGL((sweep_kernel<STACK, F>), dim3((unsigned)gx, (unsigned)gy, (unsigned)batch), block, 0, st, rows, cols, f);
    return int(hipGetLastError());
}

template <typename F>
int sweep(int64_t rows, int64_t cols, hipStream_t st, const F& f) { return sweep_launch<false>(1, rows, cols, st, f); }
template <typename F>
int sweep(int64_t batch, int64_t rows, int64_t cols, hipStream_t st, const F& f) { return sweep_launch<true>(batch, rows, cols, st, f); }
template <typename F>
int sweep_heavy(int64_t rows, int64_t cols, hipStream_t st, const F& f) { return sweep_launch<false, true>(1, rows, cols, st, f); }

}  // namespace pm
