// The wavefront sensors (prysm/x/psi.py, prysm/x/shack_hartmann.py, prysm/x/pdi.py, prysm/x/sri.py) (gfx950):
//
//  - pm_psi: K phase-shifted frames (float32, float64, uint8 or uint16, each with its own base pointer, the table of pointers and
//    weights in the kernel arguments) to the numerator sum_k s[k] g_k, the denominator sum_k c[k] g_k and the wrapped phase
//    atan2(num, den).  Every frame is read once, with 16-byte loads where the frames' alignment allows and scalar accesses for the
//    head and the tail of each row; the sums run over k in ascending order in double for every frame dtype.
//  - pm_lenslet_screen: the Shack-Hartmann screen in one launch.  A sample tests the 3 x 3 lenslets around the nearest centre, adds
//    ((x - xc)^2 + (y - yc)^2) / (2 efl) of those whose aperture holds it, in the reference's order, and stores exp(i k total).
//  - pm_grating (field x amplitude grating), pm_beam_combine (|ca a + cb b|^2 and optionally the total field) and pm_fiber_scale
//    (Efib sqrt(P eta) exp(i phi) with P and eta read from device scalars): the pointwise steps of the two interferometers.
//
// The pointwise kernels ride on pm_sweep.h; pm_psi has its own row sweep of the same shape (64 x 4 threads, a grid-stride step over
// the rows) whose threads own 16 bytes of a row instead of one element.  No atomics and no reductions: every output sample is a
// function of its own inputs.  The unit is compiled with -ffp-contract=off (csrc/Makefile): every product and sum is rounded by
// itself, in the order written, which prysm_amd/x/sensors_plan.py restates in numpy.
#include <cmath>

#include "pm_entry.h"
#include "pm_math.h"
#include "pm_sweep.h"

namespace pm {
namespace {

// ---------------------------------------------------------------- phase-shifting interferometry
struct PsiTable {
    const void* frame[PM_PSI_MAX_FRAMES];
    double s[PM_PSI_MAX_FRAMES];
    double c[PM_PSI_MAX_FRAMES];
};

// V samples side by side, on a 16-byte boundary when they fill 16 bytes or more (a longer pack moves as several 16-byte accesses)
template <typename F, int V>
struct alignas(sizeof(F) * V < 16 ? sizeof(F) * V : 16) Pack {
    F v[V];
};

// One thread owns V adjacent samples of a row (V * sizeof(F) = 16 bytes), or one (V = 1).  A row is [head | chunks of V | tail]:
// `head` scalar samples bring the frames to a 16-byte boundary, the same in every row and frame (the entry point checks it), the
// chunks are read wide, and what is left is the tail.  Thread q < nq of a row takes chunk q; thread nq + e takes the e-th of the
// head and tail samples.  wide_st: the outputs are on a 16-byte boundary where the chunks are, so their stores are wide as well.
template <typename F, typename O, int V>
__global__ __launch_bounds__(256) void psi_kernel(int K, int64_t rows, int64_t cols, const PsiTable t, int64_t ld, int64_t head, int64_t nq,
                                                  O* __restrict__ num, O* __restrict__ den, O* __restrict__ phase, int64_t old, int wide_st) {
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t edge = cols - nq * V;      // head + tail samples
    if (q >= nq + edge) return;
    for (int64_t r = int64_t(blockIdx.y) * blockDim.y + threadIdx.y; r < rows; r += int64_t(gridDim.y) * blockDim.y) {
        if (q < nq) {
            const int64_t at = r * ld + head + q * V;
            double n[V], d[V];
#pragma unroll
            for (int j = 0; j < V; ++j) n[j] = d[j] = 0.0;
            for (int k = 0; k < K; ++k) {
                const Pack<F, V> g = *reinterpret_cast<const Pack<F, V>*>(static_cast<const F*>(t.frame[k]) + at);
                const double sk = t.s[k], ck = t.c[k];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const double gv = double(g.v[j]);
                    n[j] = n[j] + sk * gv;
                    d[j] = d[j] + ck * gv;
                }
            }
            const int64_t to = r * old + head + q * V;
            Pack<O, V> pn, pd, pp;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                pn.v[j] = O(n[j]);
                pd.v[j] = O(d[j]);
                pp.v[j] = atan2_(pn.v[j], pd.v[j]);
            }
            if (wide_st) {
                if (num) *reinterpret_cast<Pack<O, V>*>(num + to) = pn;
                if (den) *reinterpret_cast<Pack<O, V>*>(den + to) = pd;
                if (phase) *reinterpret_cast<Pack<O, V>*>(phase + to) = pp;
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    if (num) num[to + j] = pn.v[j];
                    if (den) den[to + j] = pd.v[j];
                    if (phase) phase[to + j] = pp.v[j];
                }
            }
        } else {
            const int64_t e = q - nq;
            const int64_t col = e < head ? e : nq * V + e;
            double n = 0.0, d = 0.0;
            for (int k = 0; k < K; ++k) {
                const double gv = double(static_cast<const F*>(t.frame[k])[r * ld + col]);
                n = n + t.s[k] * gv;
                d = d + t.c[k] * gv;
            }
            const O on = O(n), od = O(d);
            if (num) num[r * old + col] = on;
            if (den) den[r * old + col] = od;
            if (phase) phase[r * old + col] = atan2_(on, od);
        }
    }
}

template <typename F, typename O, int V>
int psi_launch(int K, int64_t rows, int64_t cols, const PsiTable& t, int64_t ld, int64_t head, void* num, void* den, void* phase, int64_t old,
               int wide_st, hipStream_t st) {
    const int64_t nq = V == 1 ? cols : (cols > head ? (cols - head) / V : 0);
    if (V == 1) head = 0;
    const int64_t threads = nq + (cols - nq * V);
    const dim3 block(64, 4);
    const int64_t gx = (threads + block.x - 1) / block.x;
    int64_t gy = (rows + block.y - 1) / block.y;
    if (gy > 65535) gy = 65535;
    hipLaunchKernelGGL((psi_kernel<F, O, V>), dim3((unsigned)gx, (unsigned)gy), block, 0, st, K, rows, cols, t, ld, head, nq, static_cast<O*>(num),
                       static_cast<O*>(den), static_cast<O*>(phase), old, wide_st);
    return int(hipGetLastError());
}

// ---------------------------------------------------------------- Shack-Hartmann
// where the two coordinates of sample (r, c) come from (the three forms of csrc/imagechain.hip)
template <typename T>
struct Coords {
    int mode;
    const T* a;
    const T* b;
    int64_t lda, ldb;      // POINTWISE: elements between rows; SEPARABLE: ldb = elements between the values of y
    int64_t ox, oy;
    T dx;
    __device__ __forceinline__ T first(int64_t r, int64_t c) const {
        return mode == PM_COORDS_GRID ? T(c - ox) * dx : mode == PM_COORDS_SEPARABLE ? a[c] : a[r * lda + c];
    }
    __device__ __forceinline__ T second(int64_t r, int64_t c) const {
        return mode == PM_COORDS_GRID ? T(r - oy) * dx : mode == PM_COORDS_SEPARABLE ? b[r * ldb] : b[r * ldb + c];
    }
};

template <typename T>
struct LensletOp {
    Coords<T> co;
    int kind;
    int nxc, nyc;          // centres along x and along y
    T pitch, shx, shy;     // centre i along x: T(i - nxc / 2) * pitch + shx, each operation rounded (make_xy_grid, then the shift)
    T hw, hh;              // rectangle: half width and half height; circle: hw = radius^2
    T two_efl, k;          // phase = rsq / two_efl; out = exp(i k total)
    double inv_pitch;
    cx<T>* out;
    int64_t ld;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    // the index of the centre nearest to v, clamped into the array
    __device__ __forceinline__ int nearest(T v, T sh, int n) const {
        const double u = (double(v) - double(sh)) * inv_pitch + double(n / 2);
        const double f = floor(u + 0.5);
        return f >= 0.0 ? (f > double(n - 1) ? n - 1 : int(f)) : 0;      // a NaN coordinate lands on 0
    }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        const T x = co.first(r, c), y = co.second(r, c);
        const int i0 = nearest(x, shx, nxc), j0 = nearest(y, shy, nyc);
        T total = T(0);
        // rows of lenslets outermost, ascending: the order in which the reference adds its windows
        for (int j = j0 - 1; j <= j0 + 1; ++j) {
            if (j < 0 || j >= nyc) continue;
            const T ly = y - (T(j - nyc / 2) * pitch + shy);
            for (int i = i0 - 1; i <= i0 + 1; ++i) {
                if (i < 0 || i >= nxc) continue;
                const T lx = x - (T(i - nxc / 2) * pitch + shx);
                const T rsq = lx * lx + ly * ly;
                bool in;
                if (kind == PM_LENSLET_CIRCLE)
                    in = rsq - hw <= T(0);
                else
                    in = abs_(lx) - hw <= T(0) && abs_(ly) - hh <= T(0);
                if (in) total = total + rsq / two_efl;
            }
        }
        T s, cs;
        sincos_(k * total, &s, &cs);
        out[r * ld + c] = cx<T>{cs, s};
    }
};

// ---------------------------------------------------------------- the interferometers' pointwise steps
// numpy's mod: the sign of the divisor
template <typename T>
__device__ __forceinline__ T npmod_(T a, T b) {
    T m = sizeof(T) == 4 ? T(fmodf(float(a), float(b))) : T(fmod(double(a), double(b)));
    if (m != T(0)) {
        if ((b < T(0)) != (m < T(0))) m = m + b;
    } else {
        m = copysign(T(0), b);
    }
    return m;
}

template <typename T>
struct GratingOp {
    Coords<T> co;
    int kind, add_shift;
    T shift;
    T p[5];      // SIN_AMP: prefix.  PULSE: period, duty * period, hi, lo, mid
    T eps;
    const cx<T>* field;      // null: the grating itself, real
    int64_t fld;
    void* out;
    int64_t ld;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        T x = co.first(r, c);
        if (add_shift) x = x + shift;
        T g;
        if (kind == PM_GRATING_SIN_AMP) {
            const T sh = (sin_(p[0] * x) + T(1)) / T(2);
            g = T(1) - sh * T(0.1);
        } else {
            const T xw = npmod_(x, p[0]);
            g = xw < p[1] ? p[2] : p[3];
            if (abs_(xw) < eps) g = p[4];
        }
        if (field) {
            const cx<T> f = field[r * fld + c];
            static_cast<cx<T>*>(out)[r * ld + c] = cx<T>{f.x * g, f.y * g};
        } else {
            static_cast<T*>(out)[r * ld + c] = g;
        }
    }
};

template <typename T>
struct CombineOp {
    const cx<T>* a;
    const cx<T>* b;
    int64_t lda, ldb;
    T ca, cb;
    T* inten;
    cx<T>* total;
    int64_t ldi, ldt;

    __device__ __forceinline__ NoColumn column(int64_t) const { return {}; }

    __device__ __forceinline__ void point(int64_t r, int64_t c, NoColumn) const {
        const cx<T> u = a[r * lda + c], w = b[r * ldb + c];
        const T re = u.x * ca + w.x * cb, im = u.y * ca + w.y * cb;
        if (total) total[r * ldt + c] = cx<T>{re, im};
        if (inten) inten[r * ldi + c] = re * re + im * im;
    }
};

template <typename T>
struct FiberScaleOp {
    const T* efib;
    int64_t lde;
    const T* power;
    const T* eta;
    T cs, sn;
    cx<T>* out;
    int64_t ld;

    __device__ __forceinline__ T column(int64_t) const { return sqrt_(power[0] * eta[0]); }

    __device__ __forceinline__ void point(int64_t r, int64_t c, T scale) const {
        const T e = efib[r * lde + c] * scale;
        out[r * ld + c] = cx<T>{e * cs, e * sn};
    }
};

bool too_large(int64_t m, int64_t n) { return m > INT32_MAX || n > INT32_MAX; }

size_t frame_bytes(int32_t dtype) { return dtype == PM_U8 ? 1 : dtype == PM_U16 ? 2 : dtype == PM_F32 ? 4 : 8; }

bool coords_ok(int32_t coords) { return coords == PM_COORDS_GRID || coords == PM_COORDS_SEPARABLE || coords == PM_COORDS_POINTWISE; }

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" {

int pm_psi(int32_t frame_dtype, int32_t out_dtype, int64_t K, int64_t rows, int64_t cols, const pm_psi_frames* frames, int64_t ld, void* num,
           void* den, void* phase, int64_t out_ld, void* stream) {
    const char* who = "pm_psi";
    if (frame_dtype != PM_F32 && frame_dtype != PM_F64 && frame_dtype != PM_U8 && frame_dtype != PM_U16)
        return fail(PM_ERR_ARG, "%s: the frames' dtype must be PM_F32, PM_F64, PM_U8 or PM_U16", who);
    if (!real_dtype(out_dtype)) return fail(PM_ERR_ARG, "%s: the outputs' dtype must be PM_F32 or PM_F64", who);
    if (real_dtype(frame_dtype) && out_dtype != frame_dtype) return fail(PM_ERR_ARG, "%s: float frames give outputs of their own dtype", who);
    if (K < 1 || K > PM_PSI_MAX_FRAMES) return fail(PM_ERR_ARG, "%s: %lld frames, between 1 and %d are taken", who, (long long)K, PM_PSI_MAX_FRAMES);
    if (rows < 0 || cols < 0 || !frames) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (!num && !den && !phase) return fail(PM_ERR_ARG, "%s: no output (num, den and phase are all null)", who);
    PM_CHECK_LD("pm_psi", ld_ok(rows, cols, ld) && ld_ok(rows, cols, out_ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    const size_t fb = frame_bytes(frame_dtype), ob = elem_of(out_dtype);
    for (int64_t k = 0; k < K; ++k) {
        if (!frames->frame[k]) return fail(PM_ERR_ARG, "%s: frame %lld is a null pointer", who, (long long)k);
        if (!aligned(frames->frame[k], fb)) return fail(PM_ERR_ARG, "%s: frame %lld is not aligned to its element", who, (long long)k);
    }
    for (const void* o : {num, den, phase})
        if (o && !aligned(o, ob)) return fail(PM_ERR_ARG, "%s: an output is not aligned to its element", who);
    if (rows == 0 || cols == 0) return 0;
    PsiTable t;
    for (int64_t k = 0; k < PM_PSI_MAX_FRAMES; ++k) {
        t.frame[k] = k < K ? frames->frame[k] : nullptr;
        t.s[k] = k < K ? frames->s[k] : 0.0;
        t.c[k] = k < K ? frames->c[k] : 0.0;
    }
    // wide loads: every frame at the same offset from a 16-byte boundary, and rows a multiple of 16 bytes apart (or one row)
    const uintptr_t mis = reinterpret_cast<uintptr_t>(frames->frame[0]) % 16;
    bool wide = rows == 1 || (size_t(ld) * fb) % 16 == 0;
    for (int64_t k = 1; k < K && wide; ++k) wide = reinterpret_cast<uintptr_t>(frames->frame[k]) % 16 == mis;
    const int64_t head = wide ? int64_t(((16 - mis) % 16) / fb) : 0;
    // wide stores: every output on a 16-byte boundary at column `head`, rows a multiple of 16 bytes apart
    bool wide_st = wide && (rows == 1 || (size_t(out_ld) * ob) % 16 == 0);
    for (const void* o : {num, den, phase})
        if (o && (reinterpret_cast<uintptr_t>(o) + size_t(head) * ob) % 16 != 0) wide_st = false;
    hipStream_t st = PM_STREAM(stream);
    auto run = [&](auto f, auto o) {
        using F = decltype(f);
        using O = decltype(o);
        constexpr int V = int(16 / sizeof(F));
        if (wide) return psi_launch<F, O, V>(int(K), rows, cols, t, ld, head, num, den, phase, out_ld, wide_st, st);
        return psi_launch<F, O, 1>(int(K), rows, cols, t, ld, 0, num, den, phase, out_ld, 0, st);
    };
    if (frame_dtype == PM_F32) return run(float{}, float{});
    if (frame_dtype == PM_F64) return run(double{}, double{});
    if (frame_dtype == PM_U8) return out_dtype == PM_F32 ? run(uint8_t{}, float{}) : run(uint8_t{}, double{});
    return out_dtype == PM_F32 ? run(uint16_t{}, float{}) : run(uint16_t{}, double{});
}

int pm_lenslet_screen(int32_t dtype, int32_t coords, int64_t ny, int64_t nx, const void* x, int64_t ldx, const void* y, int64_t ldy, double dx,
                      const pm_lenslets* lens, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_lenslet_screen";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (!coords_ok(coords)) return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID, PM_COORDS_SEPARABLE or PM_COORDS_POINTWISE", who);
    if (ny < 0 || nx < 0 || !lens || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (coords != PM_COORDS_GRID && (!x || !y)) return fail(PM_ERR_ARG, "%s: coordinate arrays are missing (null pointer)", who);
    if (coords == PM_COORDS_GRID && !std::isfinite(dx)) return fail(PM_ERR_ARG, "%s: the grid spacing must be finite", who);
    if (lens->kind != PM_LENSLET_RECTANGLE && lens->kind != PM_LENSLET_CIRCLE) return fail(PM_ERR_ARG, "%s: unknown aperture kind %d", who, lens->kind);
    if (lens->nx < 1 || lens->ny < 1 || lens->nx > 32768 || lens->ny > 32768)
        return fail(PM_ERR_ARG, "%s: %d x %d lenslets, between 1 and 32768 per axis are taken", who, lens->nx, lens->ny);
    if (!(std::isfinite(lens->pitch) && lens->pitch > 0)) return fail(PM_ERR_ARG, "%s: the pitch must be finite and positive", who);
    if (!(std::isfinite(lens->efl) && lens->efl != 0)) return fail(PM_ERR_ARG, "%s: the focal length must be finite and nonzero", who);
    if (!std::isfinite(lens->k)) return fail(PM_ERR_ARG, "%s: the wavenumber must be finite", who);
    // the 3 x 3 neighbourhood holds every lenslet whose aperture can reach a sample only while the aperture stays within one pitch
    if (lens->kind == PM_LENSLET_RECTANGLE && !(lens->half_width >= 0 && lens->half_width <= lens->pitch && lens->half_height >= 0 && lens->half_height <= lens->pitch))
        return fail(PM_ERR_ARG, "%s: the aperture's half width and half height must lie in [0, pitch]", who);
    if (lens->kind == PM_LENSLET_CIRCLE && !(lens->half_width >= 0 && lens->half_width <= lens->pitch * lens->pitch))
        return fail(PM_ERR_ARG, "%s: the aperture's squared radius must lie in [0, pitch^2]", who);
    if (coords == PM_COORDS_POINTWISE) PM_CHECK_LD("pm_lenslet_screen", ld_ok(ny, nx, ldx) && ld_ok(ny, nx, ldy));
    PM_CHECK_LD("pm_lenslet_screen", ld_ok(ny, nx, out_ld));
    if (too_large(ny, nx)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)ny, (long long)nx);
    if (ny == 0 || nx == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        LensletOp<T> op;
        op.co = Coords<T>{coords, static_cast<const T*>(x), static_cast<const T*>(y), ldx, ldy, nx / 2, ny / 2, T(dx)};
        op.kind = lens->kind, op.nxc = lens->nx, op.nyc = lens->ny;
        op.pitch = T(lens->pitch), op.shx = T(lens->shift_x), op.shy = T(lens->shift_y);
        op.hw = T(lens->half_width), op.hh = T(lens->half_height);
        op.two_efl = T(2 * lens->efl), op.k = T(lens->k);
        op.inv_pitch = 1.0 / lens->pitch;
        op.out = static_cast<cx<T>*>(out), op.ld = out_ld;
        return sweep_heavy(ny, nx, PM_STREAM(stream), op);
    });
}

int pm_grating(int32_t dtype, int32_t kind, int32_t coords, int64_t rows, int64_t cols, const void* x, int64_t ldx, double dx, double shift,
               const double* p, const void* field, int64_t field_ld, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_grating";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (kind != PM_GRATING_SIN_AMP && kind != PM_GRATING_PULSE) return fail(PM_ERR_ARG, "%s: kind must be PM_GRATING_SIN_AMP or PM_GRATING_PULSE", who);
    if (!coords_ok(coords)) return fail(PM_ERR_ARG, "%s: coords must be PM_COORDS_GRID, PM_COORDS_SEPARABLE or PM_COORDS_POINTWISE", who);
    if (rows < 0 || cols < 0 || !p || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (coords != PM_COORDS_GRID && !x) return fail(PM_ERR_ARG, "%s: the coordinate array is missing (null pointer)", who);
    if (coords == PM_COORDS_GRID && !std::isfinite(dx)) return fail(PM_ERR_ARG, "%s: the grid spacing must be finite", who);
    if (kind == PM_GRATING_PULSE && !(std::isfinite(p[0]) && p[0] != 0)) return fail(PM_ERR_ARG, "%s: the period must be finite and nonzero", who);
    if (coords == PM_COORDS_POINTWISE) PM_CHECK_LD("pm_grating", ld_ok(rows, cols, ldx));
    PM_CHECK_LD("pm_grating", ld_ok(rows, cols, out_ld) && (!field || ld_ok(rows, cols, field_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        GratingOp<T> op;
        op.co = Coords<T>{coords, static_cast<const T*>(x), nullptr, ldx, 0, cols / 2, rows / 2, T(dx)};
        op.kind = kind, op.add_shift = shift != 0, op.shift = T(shift);
        for (int i = 0; i < 5; ++i) op.p[i] = T(p[i]);
        op.eps = sizeof(T) == 4 ? T(1.1920928955078125e-07) : T(2.220446049250313e-16);
        op.field = static_cast<const cx<T>*>(field), op.fld = field_ld, op.out = out, op.ld = out_ld;
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

int pm_beam_combine(int32_t dtype, int64_t rows, int64_t cols, const void* a, int64_t lda, double ca, const void* b, int64_t ldb, double cb,
                    void* intensity, int64_t intensity_ld, void* total, int64_t total_ld, void* stream) {
    const char* who = "pm_beam_combine";
    if (dtype != PM_C64 && dtype != PM_C128) return fail(PM_ERR_ARG, "%s: dtype must be PM_C64 or PM_C128", who);
    if (rows < 0 || cols < 0 || !a || !b) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    if (!intensity && !total) return fail(PM_ERR_ARG, "%s: no output (intensity and total are both null)", who);
    PM_CHECK_LD("pm_beam_combine", ld_ok(rows, cols, lda) && ld_ok(rows, cols, ldb) && (!intensity || ld_ok(rows, cols, intensity_ld)) &&
                                       (!total || ld_ok(rows, cols, total_ld)));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return 0;
    return by_cdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        CombineOp<T> op{static_cast<const cx<T>*>(a), static_cast<const cx<T>*>(b), lda, ldb, T(ca), T(cb), static_cast<T*>(intensity),
                        static_cast<cx<T>*>(total), intensity_ld, total_ld};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

int pm_fiber_scale(int32_t dtype, int64_t rows, int64_t cols, const void* efib, int64_t efib_ld, const void* power, const void* eta, double cos_phi,
                   double sin_phi, void* out, int64_t out_ld, void* stream) {
    const char* who = "pm_fiber_scale";
    if (!real_dtype(dtype)) return fail(PM_ERR_ARG, "%s: dtype must be PM_F32 or PM_F64", who);
    if (rows < 0 || cols < 0 || !efib || !power || !eta || !out) return fail(PM_ERR_ARG, "%s: bad argument (null pointer or negative size)", who);
    PM_CHECK_LD("pm_fiber_scale", ld_ok(rows, cols, efib_ld) && ld_ok(rows, cols, out_ld));
    if (too_large(rows, cols)) return fail(PM_ERR_ARG, "%s: %lld x %lld is too large", who, (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return 0;
    return by_rdtype(dtype, who, [&](auto real) {
        using T = decltype(real);
        FiberScaleOp<T> op{static_cast<const T*>(efib), efib_ld, static_cast<const T*>(power), static_cast<const T*>(eta), T(cos_phi), T(sin_phi),
                           static_cast<cx<T>*>(out), out_ld};
        return sweep(rows, cols, PM_STREAM(stream), op);
    });
}

}  // extern "C"
