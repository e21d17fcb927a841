// What the extern "C" entry points of the kernel units share: the stream cast, the leading-dimension and stack-overlap rules, and the
// dispatch from a runtime value (a dtype code, a byte width, what is left of a batch) to a compile-time type or constant
#pragma once
#include <algorithm>
#include <type_traits>

#include "pm_internal.h"

#define PM_STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace pm {

// rows of a rows x cols window lie `ld` elements apart: with more than one row a leading dimension below cols would make rows overlap
// (and an output race); one row takes any value (the wrappers pass the length there)
static inline bool ld_ok(int64_t rows, int64_t cols, int64_t ld) { return rows <= 1 || ld >= cols; }
#define PM_CHECK_LD(name, cond)                                                                                        \
    do {                                                                                                               \
        if (!(cond)) return fail(PM_ERR_ARG, name ": a leading dimension is smaller than the number of columns");      \
    } while (0)

// the members of a stack of `batch` arrays of `rows` rows lie `bstride` elements apart: below rows * ld they would overlap; one member
// takes any value.  The caller words the refusal
static inline bool stack_ok(int64_t batch, int64_t rows, int64_t ld, int64_t bstride) { return batch <= 1 || bstride >= rows * ld; }

static inline bool real_dtype(int32_t dtype) { return dtype == PM_F32 || dtype == PM_F64; }
static inline size_t elem_of(int32_t dtype) { return dtype == PM_F32 ? 4 : 8; }      // of a real dtype
static inline bool aligned(const void* p, size_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// Calls f with a value of the dtype's REAL type -- float for PM_C64, double for PM_C128 -- so that a generic lambda names it:
//     return by_cdtype(dtype, "pm_name", [&](auto real) { using T = decltype(real); ... return status; });
// Any other dtype is refused under `name`.  The refusal happens HERE: an entry point places this call where its dtype check belongs
// among its other checks (most look at the dtype only after the empty-shape return).
template <typename F>
int by_cdtype(int32_t dtype, const char* name, F&& f) {
    if (dtype == PM_C64) return f(float{});
    if (dtype == PM_C128) return f(double{});
    return fail(PM_ERR_ARG, "%s: dtype must be PM_C64 or PM_C128", name);
}

// the same for the real dtypes: float for PM_F32, double for PM_F64.  The units that take them look at the dtype FIRST, with a check of
// their own at the top, and call this last, around the launch: the refusal here is then never reached
template <typename F>
int by_rdtype(int32_t dtype, const char* name, F&& f) {
    if (dtype == PM_F32) return f(float{});
    if (dtype == PM_F64) return f(double{});
    return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", name);
}

// the same with an element type of 1, 4, 8 or 16 bytes, for kernels that only move elements
template <typename F>
int by_elem_bytes(int32_t elem_bytes, const char* name, F&& f) {
    switch (elem_bytes) {
        case 1: return f((unsigned char)0);
        case 4: return f(float{});
        case 8: return f(double{});
        case 16: return f(double2{});
    }
    return fail(PM_ERR_ARG, "%s: elem_bytes must be 1, 4, 8 or 16", name);
}

// the same with the unsigned integer of 1, 2, 4 or 8 bytes, for kernels that store samples in their final width
template <typename F>
int by_uint_bytes(int32_t bytes, const char* name, F&& f) {
    switch (bytes) {
        case 1: return f(uint8_t{});
        case 2: return f(uint16_t{});
        case 4: return f(uint32_t{});
        case 8: return f(uint64_t{});
    }
    return fail(PM_ERR_ARG, "%s: the width must be 1, 2, 4 or 8 bytes", name);
}

// A batch is launched in pieces of 8, 4, 2 or 1 members, the piece a template parameter of the kernel.  Calls f with the largest of
// them that is neither above `left` nor above `cap` as a std::integral_constant<int, NB>, and returns NB:
//     for (int64_t b0 = 0; b0 < batch;)
//         b0 += by_nb(batch - b0, 8, [&](auto nb) { hipLaunchKernelGGL((kernel<T, decltype(nb)::value>), ... offsets from b0 ...); });
template <typename F>
int by_nb(int64_t left, int cap, F&& f) {
    const int64_t n = std::min<int64_t>(left, cap);
    if (n >= 8) return f(std::integral_constant<int, 8>{}), 8;
    if (n >= 4) return f(std::integral_constant<int, 4>{}), 4;
    if (n >= 2) return f(std::integral_constant<int, 2>{}), 2;
    return f(std::integral_constant<int, 1>{}), 1;
}

}  // namespace pm
