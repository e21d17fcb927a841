// The library functions a kernel template calls on T = float or double: one overload set, so that a unit writes sqrt_(v) and gets
// sqrtf or sqrt.  Users: csrc/imagechain.hip, csrc/geometry.hip, csrc/fibers.hip, csrc/modal_tile.h and the modal units behind it.
#pragma once
#include <cmath>

#include "pm_internal.h"

namespace pm {

__device__ __forceinline__ float sqrt_(float v) { return sqrtf(v); }
__device__ __forceinline__ double sqrt_(double v) { return sqrt(v); }
__device__ __forceinline__ float exp_(float v) { return expf(v); }
__device__ __forceinline__ double exp_(double v) { return exp(v); }
__device__ __forceinline__ float log_(float v) { return logf(v); }
__device__ __forceinline__ double log_(double v) { return log(v); }
__device__ __forceinline__ float sin_(float v) { return sinf(v); }
__device__ __forceinline__ double sin_(double v) { return sin(v); }
__device__ __forceinline__ float cos_(float v) { return cosf(v); }
__device__ __forceinline__ double cos_(double v) { return cos(v); }
__device__ __forceinline__ float acos_(float v) { return acosf(v); }
__device__ __forceinline__ double acos_(double v) { return acos(v); }
__device__ __forceinline__ float abs_(float v) { return fabsf(v); }
__device__ __forceinline__ double abs_(double v) { return fabs(v); }
__device__ __forceinline__ float hypot_(float a, float b) { return hypotf(a, b); }
__device__ __forceinline__ double hypot_(double a, double b) { return hypot(a, b); }
__device__ __forceinline__ float atan2_(float a, float b) { return atan2f(a, b); }
__device__ __forceinline__ double atan2_(double a, double b) { return atan2(a, b); }
__device__ __forceinline__ void sincos_(float t, float* s, float* c) { sincosf(t, s, c); }
__device__ __forceinline__ void sincos_(double t, double* s, double* c) { sincos(t, s, c); }

}  // namespace pm
