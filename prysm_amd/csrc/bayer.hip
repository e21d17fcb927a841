// Bayer mosaics (prysm/bayer.py) (gfx950):
//
//  - pm_bayer_demosaic: demosaic_malvar fused.  The reference runs four full 5 x 5 convolutions, ten strided assignments and a stack;
//    here one kernel reads the mosaic once (fp32, fp64, or the detector's uint8 / uint16 / uint32 DN converted in registers) and
//    stores the RGB image once.
//      tile: one workgroup of 256 threads (4 waves) owns 16 rows x 64 columns.  The tile and its 2-sample halo, 20 x 68 samples, are
//        staged in LDS (5.4 KB fp32, 10.9 KB fp64), every sample fetched once per tile through the reflect map; 64 columns because a
//        wave then reads an LDS row and writes an output row as whole lines, 16 rows because with the output staging below the
//        workgroup stays under 18 KB (fp32) / 35 KB (fp64) of LDS, i.e. 8 / 4 workgroups per CU, at a halo overhead of 1.33 on the
//        quarter of the traffic that is loads.  LDS rows of 68 elements read by 64 adjacent lanes are conflict-free.
//      taps: a lane owns a column and wave w the rows w, w + 4, ...; a pixel evaluates the two filters its colour needs out of the
//        13 samples of the radius-2 diamond.
//      store: interleaved output -- the three values of a pixel go to an LDS staging row at 3 * column + channel (stride 3: no bank
//        conflict), and after a barrier each wave stores its rows as 3 instructions of 64 consecutive elements: 768 contiguous bytes
//        per 64 fp32 pixels, every element stored once, no 12-byte-strided partial lines.  Planar output needs no staging: three
//        stores of 64 consecutive elements straight from registers.
//    Sum order of every filter: the taps in row-major order of the 5 x 5 footprint (north-2; north-west, north, north-east; west-2,
//    west, centre, east, east-2; south-west, south, south-east; south-2), zero weights skipped, one running sum that starts at 0, each
//    product rounded by itself (power-of-two weights are exact).  Boundary: scipy's mode='reflect' (the edge sample repeated).
//  - pm_bayer_weave / pm_bayer_deinterlace / pm_bayer_assemble / pm_bayer_scale: row sweeps (pm_sweep.h: 64 adjacent columns per wave,
//    64 x 4 threads, threads striding down the rows) in its stacked form, grid.z the member of a stack.
//  - pm_bayer_class_max: the maxima of the parity classes of a mosaic or of the channels of an RGB image, two launches (partials per
//    workgroup, then one workgroup; both stages: pm_reduce.h), comparisons only: no atomics, deterministic, NaN propagates as numpy's
//    max does.
//
// prysm_amd/bayer_plan.py is this file in numpy.  The unit is compiled with -ffp-contract=off (csrc/Makefile) so that every product and
// sum is rounded by itself, as numpy does.
#include <algorithm>
#include <cmath>

#include "pm_entry.h"
#include "pm_reduce.h"
#include "pm_sweep.h"

namespace pm {
namespace {

constexpr int kTileW = 64, kTileH = 16, kHalo = 2, kDemThreads = 256;
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;
constexpr int kMaxPartials = 4096;      // workgroups of the first stage of pm_bayer_class_max

// scipy's mode='reflect': (d c b a | a b c d | d c b a)
__device__ __forceinline__ int64_t reflect(int64_t i, int64_t n) {
    const int64_t p = 2 * n;
    int64_t j = i % p;
    if (j < 0) j += p;
    return j >= n ? p - 1 - j : j;
}

template <typename T, typename In, bool PLANAR>
__global__ __launch_bounds__(kDemThreads) void demosaic_kernel(int64_t m, int64_t n, int cfa, const In* __restrict__ in, int64_t ld,
                                                               int64_t bstride, T* __restrict__ out) {
    __shared__ T tile[kLdsH][kLdsW];
    __shared__ T stage[PLANAR ? 1 : kTileH][PLANAR ? 1 : 3 * kTileW];
    const int tid = threadIdx.y * kTileW + threadIdx.x;
    const int64_t r0 = int64_t(blockIdx.y) * kTileH, c0 = int64_t(blockIdx.x) * kTileW, b = blockIdx.z;
    const In* __restrict__ src = in + b * bstride;
    for (int i = tid; i < kLdsH * kLdsW; i += kDemThreads) {
        const int ty = i / kLdsW, tx = i - ty * kLdsW;
        tile[ty][tx] = T(src[reflect(r0 - kHalo + ty, m) * ld + reflect(c0 - kHalo + tx, n)]);
    }
    __syncthreads();
    const int lx = threadIdx.x;
    const int64_t c = c0 + lx;
    const int px = int(c & 1);
    T* __restrict__ obase = out + b * m * n * 3;
    for (int ly = threadIdx.y; ly < kTileH; ly += 4) {
        const int64_t r = r0 + ly;
        const int py = int(r & 1);
#define TAP(dy, dx) tile[ly + kHalo + (dy)][lx + kHalo + (dx)]
        const T ctr = TAP(0, 0);
        const T n2 = TAP(-2, 0), s2 = TAP(2, 0), w2 = TAP(0, -2), e2 = TAP(0, 2);
        T first, green, second;      // first: the colour of the (even, even) sites
        if (py == px) {
            // an R or B site: G_at_R_or_B and R_at_B_in_BB
            const T n1 = TAP(-1, 0), s1 = TAP(1, 0), w1 = TAP(0, -1), e1 = TAP(0, 1);
            const T nw = TAP(-1, -1), ne = TAP(-1, 1), sw = TAP(1, -1), se = TAP(1, 1);
            T g = T(0) + T(-0.125) * n2;
            g = g + T(0.25) * n1;
            g = g + T(-0.125) * w2;
            g = g + T(0.25) * w1;
            g = g + T(0.5) * ctr;
            g = g + T(0.25) * e1;
            g = g + T(-0.125) * e2;
            g = g + T(0.25) * s1;
            g = g + T(-0.125) * s2;
            T d = T(0) + T(-0.1875) * n2;
            d = d + T(0.25) * nw;
            d = d + T(0.25) * ne;
            d = d + T(-0.1875) * w2;
            d = d + T(0.75) * ctr;
            d = d + T(-0.1875) * e2;
            d = d + T(0.25) * sw;
            d = d + T(0.25) * se;
            d = d + T(-0.1875) * s2;
            green = g;
            first = py == 0 ? ctr : d;
            second = py == 0 ? d : ctr;
        } else {
            // a G site: R_at_G_in_RB (the like colour left and right) and R_at_G_in_BR (above and below)
            const T n1 = TAP(-1, 0), s1 = TAP(1, 0), w1 = TAP(0, -1), e1 = TAP(0, 1);
            const T nw = TAP(-1, -1), ne = TAP(-1, 1), sw = TAP(1, -1), se = TAP(1, 1);
            T h = T(0) + T(0.0625) * n2;
            h = h + T(-0.125) * nw;
            h = h + T(-0.125) * ne;
            h = h + T(-0.125) * w2;
            h = h + T(0.5) * w1;
            h = h + T(0.625) * ctr;
            h = h + T(0.5) * e1;
            h = h + T(-0.125) * e2;
            h = h + T(-0.125) * sw;
            h = h + T(-0.125) * se;
            h = h + T(0.0625) * s2;
            T v = T(0) + T(-0.125) * n2;
            v = v + T(-0.125) * nw;
            v = v + T(0.5) * n1;
            v = v + T(-0.125) * ne;
            v = v + T(0.0625) * w2;
            v = v + T(0.625) * ctr;
            v = v + T(0.0625) * e2;
            v = v + T(-0.125) * sw;
            v = v + T(0.5) * s1;
            v = v + T(-0.125) * se;
            v = v + T(-0.125) * s2;
            green = ctr;
            first = py == 0 ? h : v;
            second = py == 0 ? v : h;
        }
#undef TAP
        const T red = cfa == 0 ? first : second, blue = cfa == 0 ? second : first;
        if constexpr (PLANAR) {
            if (r < m && c < n) {
                T* __restrict__ o = obase + r * n + c;
                o[0] = red;
                o[m * n] = green;
                o[2 * m * n] = blue;
            }
        } else {
            stage[ly][3 * lx] = red;
            stage[ly][3 * lx + 1] = green;
            stage[ly][3 * lx + 2] = blue;
        }
    }
    if constexpr (!PLANAR) {
        __syncthreads();
        const int64_t wv = n - c0 < kTileW ? n - c0 : kTileW;      // valid columns of this tile
        for (int ly = threadIdx.y; ly < kTileH; ly += 4) {
            const int64_t r = r0 + ly;
            if (r >= m) break;
            T* __restrict__ o = obase + (r * n + c0) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = k * kTileW + lx;
                if (e < 3 * wv) o[e] = stage[ly][e];
            }
        }
    }
}

// a plane of a stack: element (b, r, c) at p[b * bs + r * rs + c * es]
template <typename T>
struct Plane {
    const T* p; int64_t rs, es, bs;
    __device__ __forceinline__ T at(int64_t b, int64_t r, int64_t c) const { return p[b * bs + r * rs + c * es]; }
};

// composite (half = 0): out[r][c] = plane(parity)[r][c]; recomposite (half = 1): out[r][c] = plane(parity)[r / 2][c / 2]
template <typename T>
struct Weave {
    Plane<T> pl[4];      // by parity class 2 * (r & 1) + (c & 1)
    int half; T* o; int64_t ldo, bso;
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t b, int64_t r, int64_t c, NoColumn) const {
        const int64_t sr = half ? r >> 1 : r, sc = half ? c >> 1 : c;
        const int k = int(r & 1) * 2 + int(c & 1);
        const T v = k == 0 ? pl[0].at(b, sr, sc) : k == 1 ? pl[1].at(b, sr, sc) : k == 2 ? pl[2].at(b, sr, sc) : pl[3].at(b, sr, sc);
        o[b * bso + r * ldo + c] = v;
    }
};

// (m, n) -> (m / 2, n / 2, 3): r, (g1 + g2) / 2, b; the sweep runs over the OUTPUT pixels
template <typename T>
struct Deinterlace {
    const T* in; int64_t ld, bs; int cfa; int64_t orows, ocols; T* o;
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t b, int64_t r, int64_t c, NoColumn) const {
        const T* __restrict__ p = in + b * bs + 2 * r * ld + 2 * c;
        const T a = p[0], g1 = p[1], g2 = p[ld], d = p[ld + 1];
        T* __restrict__ q = o + ((b * orows + r) * ocols + c) * 3;
        q[0] = cfa == 0 ? a : d;
        q[1] = (g1 + g2) / T(2);
        q[2] = cfa == 0 ? d : a;
    }
};

// (m, n, 3) from four planes: r, (g2 + g1) / 2, b
template <typename T>
struct Assemble {
    Plane<T> r_, g1, g2, b_; int64_t rows, cols; T* o;
    __device__ NoColumn column(int64_t) const { return {}; }
    __device__ void point(int64_t b, int64_t r, int64_t c, NoColumn) const {
        T* __restrict__ q = o + ((b * rows + r) * cols + c) * 3;
        q[0] = r_.at(b, r, c);
        q[1] = (g2.at(b, r, c) + g1.at(b, r, c)) / T(2);
        q[2] = b_.at(b, r, c);
    }
};

// The class of element (r, c): mosaic (nclass 4) 2 * (r & 1) + (c & 1); RGB rows of 3 n values (nclass 3) c % 3.
__device__ __forceinline__ int class_of(int nclass, int64_t r, int64_t c) { return nclass == 4 ? int(r & 1) * 2 + int(c & 1) : int(c % 3); }

// stage 1: the sweep's launch shape; every workgroup leaves its four maxima (-inf where it saw no element) in partial[workgroup][4]
template <typename T>
__global__ __launch_bounds__(256) void class_max_kernel(int nclass, int64_t batch, int64_t rows, int64_t cols, const T* __restrict__ in,
                                                        int64_t ld, int64_t bs, double* __restrict__ partial) {
    const int64_t c = int64_t(blockIdx.x) * 64 + threadIdx.x;
    T a0 = -INFINITY, a1 = -INFINITY;      // even rows, odd rows
    if (c < cols)
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t r = int64_t(blockIdx.y) * 4 + threadIdx.y; r < rows; r += int64_t(gridDim.y) * 4) {
                const T v = in[b * bs + r * ld + c];
                if (r & 1) a1 = FoldNanMax::of(a1, v);      // numpy's max: NaN wins
                else a0 = FoldNanMax::of(a0, v);
            }
    const int k0 = class_of(nclass, 0, c), k1 = class_of(nclass, 1, c);
    T a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        T v = -INFINITY;
        if (k == k0) v = FoldNanMax::of(v, a0);
        if (k == k1) v = FoldNanMax::of(v, a1);
        a[k] = v;
    }
    wg_fold<256, FoldNanMax>(int(threadIdx.y * 64 + threadIdx.x), a, partial + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 4);
}

// stage 2: one workgroup
__global__ __launch_bounds__(256) void class_max_final_kernel(int64_t nparts, const double* __restrict__ partial, double* __restrict__ out) {
    double a[4];
    fold_partials<256, FoldNanMax>(threadIdx.x, nparts, partial, -INFINITY, a);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = a[k];
}

// In place: element (r, c) times the gain of its class.  With `safe` the gains are first divided by the reference's ratio, formed in T
// from the class maxima: ratio = 1; per class in the reference's order rat = max * gain / sat, taken when rat > 1 and rat > ratio.
struct Gains {
    double gain[4], sat[4];      // in the reference's order: r, g1, g2, b (mosaic) or r, g, b (RGB)
    int cls[4];                  // the class each of them scales
};
template <typename T>
struct GainPair {
    T even, odd;
};
template <typename T>
struct Scale {
    int nclass, safe; Gains g; const double* __restrict__ maxima; T* data; int64_t ld, bs;
    __device__ GainPair<T> column(int64_t c) const {
        T w[4] = {T(g.gain[0]), T(g.gain[1]), T(g.gain[2]), T(g.gain[3])};
        if (safe) {
            T ratio = T(1);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nclass) {
                    const int cl = g.cls[k];
                    const double mx = cl == 0 ? maxima[0] : cl == 1 ? maxima[1] : cl == 2 ? maxima[2] : maxima[3];
                    const T rat = T(mx) * w[k] / T(g.sat[k]);
                    if (rat > T(1) && rat > ratio) ratio = rat;
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = w[k] / ratio;
        }
        const int k0 = class_of(nclass, 0, c), k1 = class_of(nclass, 1, c);
        GainPair<T> p = {T(0), T(0)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < nclass && g.cls[k] == k0) p.even = w[k];
            if (k < nclass && g.cls[k] == k1) p.odd = w[k];
        }
        return p;
    }
    __device__ void point(int64_t b, int64_t r, int64_t c, GainPair<T> p) const {
        T* __restrict__ q = data + b * bs + r * ld + c;
        *q = *q * ((r & 1) ? p.odd : p.even);
    }
};

// what every entry point checks of (batch, m, n) read through a row stride and a batch stride of `row` elements per row
int check_stack(const char* who, int64_t batch, int64_t m, int64_t n, int64_t row, int64_t ld, int64_t bstride) {
    if (batch < 1 || m < 1 || n < 1) return fail(PM_ERR_ARG, "%s: batch, m and n must be at least 1, got %lld, %lld, %lld", who, (long long)batch, (long long)m, (long long)n);
    if (m > INT32_MAX || n > INT32_MAX / 4 || batch > 65535) return fail(PM_ERR_ARG, "%s: %lld x %lld x %lld is too large", who, (long long)batch, (long long)m, (long long)n);
    if (ld < row) return fail(PM_ERR_ARG, "%s: the row stride %lld is smaller than the row of %lld", who, (long long)ld, (long long)row);
    if (!stack_ok(batch, m, ld, bstride)) return fail(PM_ERR_ARG, "%s: bstride: the members of a stack would overlap", who);
    return 0;
}
int check_cfa(const char* who, int32_t cfa) {
    if (cfa != PM_CFA_RGGB && cfa != PM_CFA_BGGR) return fail(PM_ERR_ARG, "%s: cfa must be PM_CFA_RGGB or PM_CFA_BGGR, got %d", who, int(cfa));
    return 0;
}

template <typename T, typename In>
void launch_demosaic(int planar, int64_t batch, int64_t m, int64_t n, int cfa, const void* in, int64_t ld, int64_t bs, void* out, hipStream_t st) {
    const dim3 grid(unsigned((n + kTileW - 1) / kTileW), unsigned((m + kTileH - 1) / kTileH), unsigned(batch)), block(kTileW, 4);
    if (planar)
        hipLaunchKernelGGL((demosaic_kernel<T, In, true>), grid, block, 0, st, m, n, cfa, static_cast<const In*>(in), ld, bs, static_cast<T*>(out));
    else
        hipLaunchKernelGGL((demosaic_kernel<T, In, false>), grid, block, 0, st, m, n, cfa, static_cast<const In*>(in), ld, bs, static_cast<T*>(out));
}

template <typename T>
int demosaic_by_input(int32_t in_dtype, int planar, int64_t batch, int64_t m, int64_t n, int cfa, const void* in, int64_t ld, int64_t bs, void* out,
                      hipStream_t st) {
    switch (in_dtype) {
    case PM_U8: launch_demosaic<T, uint8_t>(planar, batch, m, n, cfa, in, ld, bs, out, st); break;
    case PM_U16: launch_demosaic<T, uint16_t>(planar, batch, m, n, cfa, in, ld, bs, out, st); break;
    case PM_U32: launch_demosaic<T, uint32_t>(planar, batch, m, n, cfa, in, ld, bs, out, st); break;
    default: launch_demosaic<T, T>(planar, batch, m, n, cfa, in, ld, bs, out, st); break;
    }
    return int(hipGetLastError());
}

template <typename T>
Plane<T> plane_of(const void* p, int64_t rs, int64_t es, int64_t bs) { return Plane<T>{static_cast<const T*>(p), rs, es, bs}; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_bayer_demosaic(int32_t in_dtype, int32_t out_dtype, int32_t cfa, int32_t planar, int64_t batch, int64_t m, int64_t n, const void* in,
                      int64_t in_ld, int64_t in_bstride, void* out, void* stream) {
    const char* who = "pm_bayer_demosaic";
    if (!real_dtype(out_dtype)) return fail(PM_ERR_ARG, "%s: out dtype must be PM_F32 or PM_F64", who);
    const bool integer = in_dtype == PM_U8 || in_dtype == PM_U16 || in_dtype == PM_U32;
    if (!integer && in_dtype != out_dtype)
        return fail(PM_ERR_ARG, "%s: in dtype must be the out dtype (a float mosaic keeps its precision) or PM_U8, PM_U16, PM_U32", who);
    if (int rc = check_cfa(who, cfa)) return rc;
    if (int rc = check_stack(who, batch, m, n, n, in_ld, in_bstride)) return rc;
    if ((m + kTileH - 1) / kTileH > 65535) return fail(PM_ERR_ARG, "%s: %lld rows are too many", who, (long long)m);
    if (!in || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    return by_rdtype(out_dtype, who, [&](auto real) {
        return demosaic_by_input<decltype(real)>(in_dtype, planar != 0, batch, m, n, cfa, in, in_ld, in_bstride, out, PM_STREAM(stream));
    });
}

int pm_bayer_weave(int32_t dtype, int32_t mode, int32_t cfa, int64_t batch, int64_t m, int64_t n, const void* r, int64_t r_rs, int64_t r_es,
                   int64_t r_bs, const void* g1, int64_t g1_rs, int64_t g1_es, int64_t g1_bs, const void* g2, int64_t g2_rs, int64_t g2_es,
                   int64_t g2_bs, const void* b, int64_t b_rs, int64_t b_es, int64_t b_bs, void* out, int64_t out_ld, int64_t out_bstride,
                   void* stream) {
    const char* who = "pm_bayer_weave";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (mode != PM_BAYER_COMPOSITE && mode != PM_BAYER_RECOMPOSITE) return fail(PM_ERR_ARG, "%s: mode must be PM_BAYER_COMPOSITE or PM_BAYER_RECOMPOSITE", who);
    if (int rc = check_cfa(who, cfa)) return rc;
    if (int rc = check_stack(who, batch, m, n, n, out_ld, out_bstride)) return rc;
    if (mode == PM_BAYER_RECOMPOSITE && ((m | n) & 1)) return fail(PM_ERR_ARG, "%s: recomposite needs even m and n, got %lld x %lld", who, (long long)m, (long long)n);
    if (!r || !g1 || !g2 || !b || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    const void* first = cfa == PM_CFA_RGGB ? r : b;
    const void* last = cfa == PM_CFA_RGGB ? b : r;
    const int64_t f_rs = cfa == PM_CFA_RGGB ? r_rs : b_rs, f_es = cfa == PM_CFA_RGGB ? r_es : b_es, f_bs = cfa == PM_CFA_RGGB ? r_bs : b_bs;
    const int64_t l_rs = cfa == PM_CFA_RGGB ? b_rs : r_rs, l_es = cfa == PM_CFA_RGGB ? b_es : r_es, l_bs = cfa == PM_CFA_RGGB ? b_bs : r_bs;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        Weave<T> w;
        w.pl[0] = plane_of<T>(first, f_rs, f_es, f_bs), w.pl[1] = plane_of<T>(g1, g1_rs, g1_es, g1_bs);
        w.pl[2] = plane_of<T>(g2, g2_rs, g2_es, g2_bs), w.pl[3] = plane_of<T>(last, l_rs, l_es, l_bs);
        w.half = mode == PM_BAYER_RECOMPOSITE, w.o = static_cast<T*>(out), w.ldo = out_ld, w.bso = out_bstride;
        return sweep(batch, m, n, PM_STREAM(stream), w);
    });
}

int pm_bayer_deinterlace(int32_t dtype, int32_t cfa, int64_t batch, int64_t m, int64_t n, const void* in, int64_t in_ld, int64_t in_bstride,
                         void* out, void* stream) {
    const char* who = "pm_bayer_deinterlace";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (int rc = check_cfa(who, cfa)) return rc;
    if (int rc = check_stack(who, batch, m, n, n, in_ld, in_bstride)) return rc;
    if ((m | n) & 1) return fail(PM_ERR_ARG, "%s: m and n must be even, got %lld x %lld", who, (long long)m, (long long)n);
    if (!in || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return sweep(batch, m / 2, n / 2, PM_STREAM(stream), Deinterlace<T>{static_cast<const T*>(in), in_ld, in_bstride, cfa, m / 2, n / 2, static_cast<T*>(out)});
    });
}

int pm_bayer_assemble(int32_t dtype, int64_t batch, int64_t m, int64_t n, const void* r, int64_t r_rs, int64_t r_es, int64_t r_bs, const void* g1,
                      int64_t g1_rs, int64_t g1_es, int64_t g1_bs, const void* g2, int64_t g2_rs, int64_t g2_es, int64_t g2_bs, const void* b,
                      int64_t b_rs, int64_t b_es, int64_t b_bs, void* out, void* stream) {
    const char* who = "pm_bayer_assemble";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (int rc = check_stack(who, batch, m, n, n, n, m * n)) return rc;
    if (!r || !g1 || !g2 || !b || !out) return fail(PM_ERR_ARG, "%s: null pointer", who);
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return sweep(batch, m, n, PM_STREAM(stream),
                     Assemble<T>{plane_of<T>(r, r_rs, r_es, r_bs), plane_of<T>(g1, g1_rs, g1_es, g1_bs), plane_of<T>(g2, g2_rs, g2_es, g2_bs),
                                 plane_of<T>(b, b_rs, b_es, b_bs), m, n, static_cast<T*>(out)});
    });
}

size_t pm_bayer_class_max_workspace(void) { return size_t(kMaxPartials) * 4 * sizeof(double); }

int pm_bayer_class_max(int32_t dtype, int32_t classes, int64_t batch, int64_t m, int64_t n, const void* in, int64_t in_ld, int64_t in_bstride,
                       void* maxima, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "pm_bayer_class_max";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (classes != PM_BAYER_MOSAIC && classes != PM_BAYER_RGB) return fail(PM_ERR_ARG, "%s: classes must be PM_BAYER_MOSAIC or PM_BAYER_RGB", who);
    const int nclass = classes == PM_BAYER_MOSAIC ? 4 : 3;
    const int64_t cols = classes == PM_BAYER_MOSAIC ? n : 3 * n;
    if (int rc = check_stack(who, batch, m, n, cols, in_ld, in_bstride)) return rc;
    const int64_t gx = (cols + 63) / 64;
    if (gx > kMaxPartials) return fail(PM_ERR_ARG, "%s: rows of %lld values are too long", who, (long long)cols);
    if (!in || !maxima || !workspace) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (workspace_bytes < pm_bayer_class_max_workspace()) return fail(PM_ERR_WORKSPACE, "%s: the workspace is smaller than pm_bayer_class_max_workspace()", who);
    int64_t gy = std::min<int64_t>((m + 3) / 4, kMaxPartials / gx);
    if (gy < 1) gy = 1;
    hipStream_t st = PM_STREAM(stream);
    const dim3 grid{unsigned(gx), unsigned(gy)}, block(64, 4);
    double* part = static_cast<double*>(workspace);
    const int rc = by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        hipLaunchKernelGGL(class_max_kernel<T>, grid, block, 0, st, nclass, batch, m, cols, static_cast<const T*>(in), in_ld, in_bstride, part);
        return int(hipGetLastError());
    });
    if (rc) return rc;
    hipLaunchKernelGGL(class_max_final_kernel, dim3{1}, dim3{256}, 0, st, gx * gy, part, static_cast<double*>(maxima));
    return int(hipGetLastError());
}

int pm_bayer_scale(int32_t dtype, int32_t classes, int32_t cfa, int64_t batch, int64_t m, int64_t n, void* data, int64_t ld, int64_t bstride,
                   const double* gains, int32_t safe, const double* saturation, const void* maxima, void* stream) {
    const char* who = "pm_bayer_scale";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (classes != PM_BAYER_MOSAIC && classes != PM_BAYER_RGB) return fail(PM_ERR_ARG, "%s: classes must be PM_BAYER_MOSAIC or PM_BAYER_RGB", who);
    if (int rc = check_cfa(who, cfa)) return rc;
    const int nclass = classes == PM_BAYER_MOSAIC ? 4 : 3;
    const int64_t cols = classes == PM_BAYER_MOSAIC ? n : 3 * n;
    if (int rc = check_stack(who, batch, m, n, cols, ld, bstride)) return rc;
    if (!data || !gains) return fail(PM_ERR_ARG, "%s: null pointer", who);
    if (safe && (!saturation || !maxima)) return fail(PM_ERR_ARG, "%s: safe scaling needs the saturations and the class maxima", who);
    Gains g;
    for (int k = 0; k < 4; ++k) {
        g.gain[k] = k < nclass ? gains[k] : 1.0;
        g.sat[k] = safe && k < nclass ? saturation[k] : 1.0;
        g.cls[k] = k;
        if (safe && k < nclass && !(g.sat[k] > 0.0)) return fail(PM_ERR_ARG, "%s: saturation must be positive", who);
    }
    if (nclass == 4 && cfa == PM_CFA_BGGR) g.cls[0] = 3, g.cls[3] = 0;      // r sits at (odd, odd), b at (even, even)
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        return sweep(batch, m, cols, PM_STREAM(stream), Scale<T>{nclass, safe != 0, g, static_cast<const double*>(maxima), static_cast<T*>(data), ld, bstride});
    });
}

}  // extern "C"
