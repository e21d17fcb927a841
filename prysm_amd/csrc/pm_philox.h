// Philox4x32-10 (Salmon et al., SC'11), integer arithmetic only, and the exact word-to-float rules of the units that draw from it
// (csrc/detector.hip, csrc/psdsynth.hip).  prysm_amd/detector_plan.py philox4x32 / uniform53 are the same in numpy; the detector
// tests pin the words.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace pm {

struct Words {
    uint32_t w[4];
};

__device__ __forceinline__ Words philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c1 = uint32_t(p1), c3 = uint32_t(p0), c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

// two words -> [0, 1) with 53 random bits, every step exact
__device__ __forceinline__ double uniform53(uint32_t hi, uint32_t lo) {
    return (double(hi >> 5) * 67108864.0 + double(lo >> 6)) * 0x1p-53;
}

// one word -> [0, 1) with 24 random bits, every step exact
__device__ __forceinline__ float uniform24(uint32_t w) { return float(w >> 8) * 0x1p-24f; }

}  // namespace pm
