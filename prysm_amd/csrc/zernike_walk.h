// The Zernike table walk shared by csrc/zernike.hip and csrc/segmented.hip (gfx950): the step layout and the walk itself, over the wave
// tile of modal_tile.h.  See zernike.hip for the table and prysm_amd/polynomials/zernike_plan.py for how it is built.
#pragma once
#include "modal_tile.h"

namespace pm {
namespace {

enum { ZS_RESET = 1, ZS_ADV = 2 };
enum { ZP_NONE = 0, ZP_RADIAL = 1, ZP_COS = 2, ZP_SIN = 3 };

// one step of the table (zernike_plan.step_dtype)
template <typename T>
struct ZStep {
    T a, b, c, w;
    int32_t op, part, slot, dm;
};
static_assert(sizeof(ZStep<float>) == 32 && sizeof(ZStep<double>) == 48, "ZStep layout is shared with zernike_plan.step_dtype");

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

}  // namespace
}  // namespace pm
