// Internal interface between the translation units behind the extern "C" surface (round 6: capi.hip was one 2000-line file):
//   capi_core.hip  error text, twiddle / plan tables, tuning knobs, device queries   (+ pm_version, pm_set_tuning*, pm_last_error, pm_plan_prepare, pm_shutdown)
//   capi_plan.hip  host-only planning: which route a descriptor takes, workspace sizes, argument checks  (+ the workspace queries, pm_plan_explain)
//   capi_run.hip   the routes themselves: parameter blocks and kernel launches per plan
//   capi.hip       the transform entry points (pm_fft2, pm_fft2_spectral, pm_fft2_mul_ifft2, pm_fft1*, pm_czt_axis, pm_fft1_ramp, pm_fft2_time_passes)
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "bluestein.h"
#include "fft_mixed.h"
#include "pm_internal.h"
#include "ws_layout.h"
#include "fft_r2c_types.h"
#include "fft_hermt_types.h"
#include "fft_conv1_types.h"
#include "fft_spectral_types.h"
#include "fft_c2r_types.h"

namespace pm {

inline size_t elem_size(int dtype) { return dtype == PM_C64 ? 8 : 16; }      // bytes of a complex element

// ---------------------------------------------------------------- what the three plans share
struct PlanBase {
    int logn = -1, logm = -1;   // engine log2 sizes or -1
    TiledLayout lay;      // the tiled intermediate (ws_layout.h): lay.tc is the column-pass tile width when both passes run on the engine,
                          // else 0 (natural intermediate)
    bool fold = false;    // one radix-2 step of the column transform is taken in the row pass (RowStoreFold): the column
                          // pass then runs two planes of M/2-point tiles; on the transposed Hermitian form (r2c_t) in the column pass's load
    size_t ws_bytes = 0;  // total workspace
    // launch choices (the runner reads these, not the knobs): sibling groups, streaming loads / stores
    int row_log_g = 0, col_log_g = 0, nt_in = 0, nt_out = 0;
};

// ---------------------------------------------------------------- 2-D transform
struct Fft2Plan : PlanBase {
    bool r2c = false;     // real input on the Hermitian path (fft_r2c.h): N/2-point row transforms, N/2 + 1 columns, mirrored stores
    bool r2c_t = false;   // ... in its transposed form (fft_hermt.h, round 6): real-input COLUMN transforms into an M/2 x N natural intermediate,
                          // then full-length row transforms that store every row and its mirror image as whole lines
    int col_var = 0;      // column-pass tiling (ColCfgSel): 2 = 128 B tiles for the planes of a folded 4096-row complex128 transform
    size_t ws_field = 0;  // bytes of intermediate per field (256 B aligned)
    int64_t wstride = 0;  // ... in elements: from one field's intermediate to the next
    int64_t nbatch = 1;   // fields
    int64_t chunk = 1;    // fields per launch pair: the intermediates of one chunk stay resident in the 256 MiB
                          // Infinity Cache between the two passes, consecutive chunks reuse the same workspace
    bool mix_n = false, mix_m = false;    // the row / column transforms take the mixed-radix kernel (composite lengths, fft_mixed.hip)
    int64_t w_ld = 0;     // row pitch of the NATURAL intermediate (lay.tc == 0), in elements: N, or N rounded up to whole 128 B lines when the
                          // column pass is the mixed-radix kernel -- its 32 / 64 B pieces then share lines only inside one XCD group
                          // (3000 complex64 columns: rows of 24000 B put every other row half a line off and the pass read 1.52x its bytes)
    bool blue_n = false, blue_m = false;  // the row / column transforms take the Bluestein path (non-power-of-two lengths, bluestein.hip)
    size_t blue_off = 0;  // its scratch sits behind the intermediates in the workspace (shared by the two passes)
    int big_rn = 0, big_rm = 0;   // power-of-two lengths above the engine's: radix of the extra step per axis (1 = none), 0 = not this path
    bool blue_big = false;        // blue2d whose convolution length exceeds the engine's: two big power-of-two transforms around the multiply
    bool blue2d = false;  // both axes: chirp multiply -> ONE fused fft2 x (B1 (x) B2) ifft2 chain of size MB1 x MB2 -> chirp multiply
                          // (blue2d_run); the workspace is then Blue2dWs
    bool blue_fuse = false;       // ... with the chirp multiplies inside the chain's first / last row pass (blue2d_fused_run)
    int hermt_row_var = 0;        // r2c_t: tiling of its row pass at 4096 complex64 points (launch_row_hermt): 4 two rows per thread, 0 one row per workgroup
};

// ---------------------------------------------------------------- fused fft2 -> multiply -> ifft2
// [W1 | W2] PER FIELD: stored input rows x N, and M x N; one shared block when every row is stored (the chain then runs in place)
struct FusedWs {
    size_t w1 = 0, w2 = 0;      // 256 B aligned; w2 == 0: shared
    size_t w2_off() const { return w2 ? w1 : 0; }
    size_t field() const { return w1 + w2; }
};
inline FusedWs fused_ws(size_t w1_raw, size_t w2_raw, bool inplace) { return {align256(w1_raw), inplace ? 0 : align256(w2_raw)}; }
struct FusedPlan : PlanBase {
    FusedWs cut;
    int64_t wstride = 0;         // elements from one field's block to the next
    bool inplace = false;
    int64_t nbatch = 1, chunk = 1;   // fields, fields per launch triple
    bool mixmid = false;         // composite column length: natural intermediates of pitch w_ld, the mixed-radix middle pass (fft_mixed.h)
    int64_t w_ld = 0;
    int colmul_mode = 0;         // knob of launch_col_mul
};

// ---- real object, real result: the chain on half spectra (fft_c2r.h)
struct HermConvPlan : PlanBase {};

// ---------------------------------------------------------------- workspaces made of several buffers: offsets and total, for the query and the route
// [first | second], arrays of a x b elements each (both false: the first alone).  big2d_run: [Z: R_n planes of M x N/R_n | F (and the
// pre-processed rows before it)]; fft1_big: rows [Y | Z] of batch x n, columns one array
struct PairWs { size_t second, total; };
inline PairWs pair_ws(size_t es, int64_t a, int64_t b, bool both = true) {
    const size_t arr = align256(size_t(a) * size_t(b) * es);
    return {arr, both ? 2 * arr : arr};
}
// blue2d_run: [a (M x N) | c (M x N) | workspace of the fused chain]; blue_big: [a | c | spectrum (MB1 x MB2) | workspace of the big transforms]
struct Blue2dWs { size_t c, chain, big, total; };
size_t blue2d_fused_ws(int dtype, int64_t M, int64_t N);
inline Blue2dWs blue2d_ws(int dtype, int64_t M, int64_t N, bool big) {
    const size_t es = elem_size(dtype), arr = align256(size_t(M) * size_t(N) * es);
    if (!big) return {arr, 2 * arr, 0, 2 * arr + blue2d_fused_ws(dtype, M, N)};
    const size_t spec = align256(size_t(blue_conv_len(M)) * size_t(blue_conv_len(N)) * es);
    return {arr, 2 * arr, 2 * arr + spec, 2 * arr + spec + 2 * spec};
}

// ---- capi_plan.hip / capi_run.hip
inline AxisMap to_map(const pm_axis& a) { return AxisMap{int(a.n), int(a.len), int(a.off), int(a.shift)}; }
int64_t batch_chunk(int64_t nb, size_t ws_field);
Fft2Plan plan_fft2(const pm_fft2_desc* d, bool allow_r2c = true);
bool plan_fused_mix(const pm_fft2_desc* d, FusedPlan& p);
bool plan_fused(const pm_fft2_desc* d, FusedPlan& p);
bool fused_mix_pass_a(const pm_fft2_desc* d, int64_t w_ld, pm_fft2_desc& da, Fft2Plan& pa);
void blue2d_desc(pm_fft2_desc& dd, int dtype, int64_t M, int64_t N);
int check_fft2(const pm_fft2_desc* d);
bool ce_rows_axis(const pm_fft2_desc* d, const Fft2Plan& p);
bool ce_cols_axis(const pm_fft2_desc* d, const Fft2Plan& p);
bool ce_both_axes_stack(const pm_fft2_desc* d, const Fft2Plan& p);
inline bool fft1_big_ok(const pm_axis* ti) { return big_split(ti->n) > 1 && ti->shift == 0; }
bool herm_conv_plan(const pm_fft2_desc* d, HermConvPlan& p);
bool spectral_fast(const pm_fft2_desc* d, const Fft2Plan& p);
int spectral_group(int32_t count);
int check_fft1(int32_t dtype, int32_t direction, int32_t axis, int64_t batch, const pm_axis* t_in, const pm_axis* t_out);
template <typename T>
int fft2_run(const pm_fft2_desc* d, const Fft2Plan& p, const void* in, void* out, void* ws, hipStream_t st);
template <typename T>
int fused_run(const pm_fft2_desc* d, const FusedPlan& p, const void* in, void* out, void* ws, hipStream_t st);
template <typename T>
int fft1_run(int direction, int axis, int64_t batch, const pm_axis* ti, const pm_axis* to, double scale,
                    const void* in, int64_t in_ld, void* out, int64_t out_ld, hipStream_t st, void* blue_ws = nullptr);
template <typename T>
int czt_axis_run(int32_t axis, int64_t nseq, int64_t K, int64_t in_len, int64_t in_off, int64_t out_len, int64_t out_off,
                        const void* pre, int pre_conj, const void* H, int h_conj, const void* post, int post_conj, double scale,
                        const void* in, int64_t in_ld, void* out, int64_t out_ld, hipStream_t st, int single = 0);
template <typename T>
int herm_conv_run(const pm_fft2_desc* d, const HermConvPlan& p, const void* in, void* out, void* ws, hipStream_t st);
template <typename T>
int fft2_spectral_group(const pm_fft2_desc* d, const Fft2Plan& p, const Spectral& w, const void* in, void* out, void* ws, hipStream_t st);

}  // namespace pm
