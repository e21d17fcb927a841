// What the extern "C" entry points of the kernel units share: the stream cast, the leading-dimension rule and the dispatch from a
// runtime dtype code to a compile-time type
#pragma once
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

}  // namespace pm
