/* prysm_amd -- C ABI of the MI355X (gfx950) physical-optics propagation engine.
 *
 * This is the drop-in boundary for the ONE hot path of brandondube/prysm v0.22
 * named in BASELINE.json: pupil<->focus FFT propagation, angular-spectrum free
 * space propagation, the matrix-DFT fixed-sampling focus and the |.|^2
 * intensity / incoherent polychromatic sum.  The reference is pure Python and has
 * no FFI; its plug surface is the `prysm.mathops` backend shim
 * (prysm/mathops.py:11-45) through which every hot-path module reaches
 * numpy / scipy.fft / BLAS.  Each entry point below names the reference call
 * site(s) whose arithmetic it replaces.  The host-side mirror of the reference's
 * Python interface (same names, arguments, error behaviour) is the `prysm_amd`
 * package, which binds these symbols with ctypes; INTEGRATION.md shows the
 * binding a prysm maintainer would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (HBM) unless stated otherwise; buffers are
 *    owned by the caller (PyTorch allocates them).  The library allocates only
 *    immutable per-(N, dtype, device) twiddle tables in a plan cache.
 *  - Arrays are row-major `a[y][x]` (prysm convention), leading dimension in
 *    ELEMENTS.  Complex values are interleaved (re, im).
 *  - Every function only ENQUEUES work on `stream` (a hipStream_t; NULL = the
 *    default stream) and never synchronises.
 *  - Return value: 0 = ok, < 0 = argument error (see pm_last_error()),
 *    > 0 = a hipError_t.
 *  - gfx950 only.  There is no CPU path: without a GPU every compute entry
 *    point fails with a hipError_t.
 */
#ifndef PRYSM_AMD_H
#define PRYSM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_VERSION 107 /* 0.1.0 */

/* dtype codes */
enum { PM_C64 = 0, PM_C128 = 1, PM_F32 = 2, PM_F64 = 3, PM_BOOL = 4, PM_U8 = 5, PM_U16 = 6, PM_U32 = 7 };

/* error codes (negative) */
enum {
    PM_OK = 0,
    PM_ERR_ARG = -1,         /* bad argument (null pointer, negative size, bad enum) */
    PM_ERR_UNSUPPORTED = -2, /* size / dtype combination not implemented */
    PM_ERR_WORKSPACE = -3    /* workspace too small; query with pm_fft2_workspace() */
};

/* epilogues of the last FFT pass */
enum {
    PM_EPI_NONE = 0,       /* complex output */
    PM_EPI_ABS2 = 1,       /* real output  |scale * X|^2           (Wavefront.intensity fused) */
    PM_EPI_ABS2_ACCUM = 2, /* real output  out += weight*|scale*X|^2 (incoherent polychromatic sum) */
    PM_EPI_ABS = 3,        /* real output  |scale * X|    (otf.mtf_from_psf, prysm/otf.py:77-103)  -- real-input transforms only */
    PM_EPI_ARG = 4         /* real output  angle(scale*X) (otf.ptf_from_psf, prysm/otf.py:106-135) -- real-input transforms only */
};

/* multiplier applied to the complex result before it is stored */
enum { PM_MUL_NONE = 0, PM_MUL_FULL = 1, PM_MUL_SEPARABLE = 2 };

/* flags */
enum {
    PM_FLAG_PASS1_ONLY = 1, /* profiling: run only the row pass    */
    PM_FLAG_PASS2_ONLY = 2, /* profiling: run only the column pass */
    PM_FLAG_SYNTH_INPUT = 8, /* `in` is the real OPD map (float); the transformed field is synth_amp * exp(i synth_k opd),
                             * synthesised while the row pass loads it -- Wavefront.from_amp_and_phase
                             * (prysm/propagation/wavefront.py:58-79) fused into focus: the complex pupil never exists in
                             * memory.  `in` is float for PM_C64, double for PM_C128 (fp64 sincospi per sample: 4096^2 329 -> 255 us
                             * against synthesis + transform).  Row lengths: powers of two (the engine's row loader) and composites of primes
                             * <= 19 up to 8192 (the mixed-radix row kernel's first stage, round 4); PM_ERR_UNSUPPORTED otherwise. */
    PM_FLAG_SYNTH_PACKED = 32, /* with PM_FLAG_SYNTH_INPUT: `in` holds (amplitude, OPD) float / double PAIRS (in_ld in pairs), synth_amp is ignored.
                             * One 8-byte load per element instead of two 4-byte loads from two arrays: a loop over wavelengths packs
                             * its two maps once (the polychromatic recipe: 133 -> 101 us per wavelength at 4096^2) */
    PM_FLAG_NORM_DC = 16,   /* divide the result by its DC bin X[0][0] before the epilogue -- the centre normalisation
                             * `data / data[cy, cx]` of the OTF routines (prysm/otf.py:62-74).  Real-input transforms on the
                             * Hermitian path only (see PM_FLAG_REAL_INPUT), where that bin is real; PM_ERR_UNSUPPORTED otherwise */
    PM_FLAG_REAL_OUTPUT = 64, /* pm_fft2_mul_ifft2 with PM_FLAG_REAL_INPUT: `out` is a REAL array (out_ld in real elements) that receives
                             * the REAL PART of the result -- what convolution.conv / apply_transfer_functions keep for a real object
                             * (prysm/convolution.py:29-31, 110-113).  The chain then runs on half spectra end to end (real rows as
                             * N/2 packed complex points, the Hermitian part of the multiplier, N/2-point inverse row transforms):
                             * 32 instead of 56 bytes per sample.  A full (PM_MUL_FULL) multiplier, unpadded power-of-two sizes from
                             * 2048^2 samples (rows of 64 .. 8192; smaller fields: tuning key "r2c" = 2), rotations by 0 or N/2 along x,
                             * unwindowed output, one field;
                             * PM_ERR_UNSUPPORTED otherwise (the caller takes the real part of the complex chain instead). */
    PM_FLAG_REAL_INPUT = 4  /* `in` is a REAL array of the precision that goes with dtype (float / double); in_ld and
                             * in_bstride count real elements.  fft2 of a real PSF / object / actuator map
                             * (prysm/otf.py:31, prysm/convolution.py:27-28,82-85) without a complex copy: pass 1 reads
                             * half the bytes.  A FORWARD transform of an unpadded real field with power-of-two lengths (>= 32
                             * per row) and an unwindowed output takes the Hermitian path: half the spectrum is computed and each
                             * result stored twice (at (u, k) and, conjugated, at (-u, -k)) -- along x (half-length row transforms,
                             * N/2 + 1 columns through the column pass) or, where every rotation is 0 or half a length and it
                             * measured faster, along y (real-input column transforms, then M/2 row transforms that store each
                             * row and its mirror image as whole lines; tuning key "herm_t");
                             * PM_EPI_ABS / PM_EPI_ARG / PM_FLAG_NORM_DC exist on that path */
};

/* One axis of a windowed, rotated view.  A logical (transform-sized) axis of
 * length n is related to memory by
 *     position p = (i + shift) mod n,   memory index q = p - off,   0 <= q < len.
 * On the INPUT side logical element i reads mem[q] (zero outside the window):
 *     fft.ifftshift            -> shift = n/2            (prysm/propagation/fft.py:24)
 *     fttools.pad2d            -> off = ceil((n-len)/2)  (prysm/fttools.py:88-94), never materialised
 * On the OUTPUT side transform bin k is written to mem[q] (dropped outside):
 *     fft.fftshift             -> shift = n/2
 *     fttools.crop_center      -> off = ceil((n-len)/2)  (prysm/fttools.py:122-124)
 */
typedef struct pm_axis {
    int64_t n;
    int64_t len;
    int64_t off;
    int64_t shift;
} pm_axis;

/* 2-D complex transform with fused pad / shift / crop / scale / multiply / |.|^2.
 * Replaces, in one call:
 *   fft.fftshift(fft.fft2(fft.ifftshift(pad2d(x, Q)), norm=...))      prysm/propagation/fft.py:23-25 (focus)
 *   ... ifft2 ...                                                      fft.py:44,65,84 (unfocus, adjoints) + crop_center
 *   fft.fft2(field) * tf  and  fft.ifft2(.)                            prysm/propagation/angular_spectrum.py:35,41-42,76
 *   re*re + im*im of the result                                        prysm/propagation/wavefront.py:146-151
 *   fft.fftshift(fft.fft2(fft.ifftshift(psf)))                         prysm/otf.py:31
 */
typedef struct pm_fft2_desc {
    int32_t dtype;      /* PM_C64 or PM_C128 */
    int32_t direction;  /* -1: exp(-2 pi i ..) (fft2), +1: exp(+2 pi i ..) (ifft2, unnormalised) */
    int32_t epilogue;   /* PM_EPI_* */
    int32_t flags;      /* PM_FLAG_* */
    double scale;       /* multiplies the complex result: 1/sqrt(MN) for norm='ortho', 1/(MN) for ifft2 */
    double weight;      /* PM_EPI_ABS2_ACCUM weight */
    pm_axis in_y, in_x;   /* input view  (rows, columns) */
    pm_axis out_y, out_x; /* output view (rows, columns) */
    int64_t in_ld, out_ld;
    int32_t mul_kind;   /* PM_MUL_*: result *= mul[k_y][k_x] (FULL) or mul_y[k_y]*mul_x[k_x] (SEPARABLE), */
    int32_t mul_conj;   /*           indexed by the unshifted transform bin; conj -> multiply by conj(mul) */
    const void* mul;    /* FULL: (M x N) complex array; SEPARABLE: length-M complex vector (rows) */
    const void* mul_x;  /* SEPARABLE: length-N complex vector (columns) */
    int64_t mul_ld;
    /* Batch of independent fields in ONE launch pair (wavelengths / field points of a polychromatic or
     * multi-field model -- the per-wavelength loop of docs/source/how-tos/Polychromatic Propagation.ipynb).
     * Field b reads in + b*in_bstride and writes out + b*out_bstride (elements of the respective array; for the
     * |.|^2 epilogues out elements are real).  batch = 0 means 1.  mul_bstride / mul_x_bstride: elements between
     * per-field multipliers (FULL: arrays; SEPARABLE: the row-factor and column-factor vectors), 0 = shared.
     * The workspace grows by the batch factor.  PM_EPI_ABS2_ACCUM needs distinct outputs per field. */
    int64_t batch;
    int64_t in_bstride, out_bstride;
    int64_t mul_bstride, mul_x_bstride;
    /* PM_FLAG_SYNTH_INPUT: amplitude array of the in window's shape (NULL: unit amplitude), its type (PM_F32, PM_F64,
     * PM_BOOL), leading dimension, and k = 2 pi / (wavelength_um * 1e3) for an OPD in nm */
    const void* synth_amp;
    int32_t synth_amp_dtype;
    int32_t synth_reserved;
    int64_t synth_amp_ld;
    double synth_k;
} pm_fft2_desc;

/* Transform lengths (per axis): powers of two from 2 to 8192 run on the Stockham engine; composite lengths from 32 to 8192 whose prime
 * factors are all <= 19 (1000, 1020, 1536, 2592, 3000, 6000 ...: what scipy.fft factors natively) run on their own factors in one LDS-resident
 * mixed-radix kernel per axis with no scratch (3000^2 complex64: 87 us; arrays of 4 GiB and more keep the routes below); 16384 and
 * 32768 take one radix-2 / radix-4 step around engine transforms (16384^2 complex64: 4.3 ms), and so do 3 / 5 / 7 x 2^k above 8192
 * (10240, 12288 ...: radix 3 / 5 / 7) and -- round 4 -- composites above 8192 whose cofactor of 2, 3, 4, 5 or 7 is a length the mixed-radix
 * kernel takes (10000 = 2 x 5000, 9000, 12000, 20000 ...: 10000^2 complex64 1.9 ms), when the other axis is a power of two, such a length
 * or a composite the mixed-radix kernel takes; other lengths from 96 to 4096 (a prime
 * factor above 19: 997, 1009 ...) run on the engine through Bluestein's identity (chirp multiply, power-of-two convolution of length >= 2n - 1, chirp multiply;
 * when both axes are such lengths the 2-D convolution is ONE fused fft2 x B ifft2 chain, and that form reaches 16384 per axis by
 * convolving at 16384 / 32768 points: 8000^2 complex64 8.6 ms); shorter lengths, and other lengths
 * up to 32768, run on a direct O(n^2) kernel with fp64 accumulation.  Anything else is PM_ERR_UNSUPPORTED.  The reference
 * takes any length through scipy.fft (prysm/propagation/fft.py:24).
 *
 * bytes of workspace pm_fft2 needs for this descriptor (the tiled intermediate, plus the Bluestein scratch) */
size_t pm_fft2_workspace(const pm_fft2_desc* d);

int pm_fft2(const pm_fft2_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
            void* stream);

/* The wavelength loop of a polychromatic PSF (docs/source/how-tos/Polychromatic Propagation.ipynb cell 3:
 *     for wvl, w in zip(wavelengths, weights): psf += w * abs(focus(amp * exp(1j * 2 pi / wvl * opd)))**2  ),
 * result-equivalent to `count` pm_fft2 calls with d->synth_k = k[b], d->weight = weight[b] on the same input and accumulator
 * (the descriptor must carry PM_FLAG_SYNTH_INPUT and PM_EPI_ABS2_ACCUM; its own synth_k / weight are ignored; k and weight
 * are HOST arrays).  With PM_FLAG_SYNTH_PACKED and engine lengths below 4096^2 bins (complex128: rows of up to 2048 samples) the loop
 * runs as one launch pair per group of wavelengths: the row pass reads the packed (amplitude, OPD) map once per group, the column
 * pass sums w_b |.|^2 over the group in registers and touches the accumulator once -- 16 + 16 / B bytes per sample and wavelength
 * instead of 32 in complex64 (B = 8: tuning keys "spectral", "spectral_area_log"; measured 1.8 - 2.5x the loop from 1024^2 to 2048^2,
 * no gain at 4096^2, which keeps the loop).  The sum runs in wavelength order; only its association differs from the loop's
 * (acc + (w_0 i_0 + w_1 i_1 + ..) per group).  Other descriptors run the plain loop.
 * Workspace: pm_fft2_spectral_workspace(d, count) bytes. */
size_t pm_fft2_spectral_workspace(const pm_fft2_desc* d, int32_t count);
int pm_fft2_spectral(const pm_fft2_desc* d, int32_t count, const double* k, const double* weight, const void* in, void* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Fused  out = window( ifft2( fft2( pad(in) ) * H ) )  in THREE passes (row FFT, column FFT x H x column IFFT
 * in registers, row IFFT): 6 N^2 s bytes of HBM traffic instead of the 8 N^2 s of two pm_fft2 calls.
 * Replaces fft.ifft2(fft.fft2(field) * tf) of angular_spectrum / angular_spectrum_adjoint
 * (prysm/propagation/angular_spectrum.py:35,41-42,76) and the fft2 * fft2 -> ifft2 core of convolution.conv
 * (prysm/convolution.py:27-30).  Transform lengths: powers of two <= 8192 on both axes, or (round 4: one field, complex output) a COLUMN
 * length from 32 to 8192 whose primes are <= 19 beside a row length of either kind -- the middle pass then keeps each column in LDS through
 * the forward stages of its factorisation, the multiplier and the same stages transposed (csrc/fft_mixed.h; angular spectrum 3000^2
 * complex128: 281 us against 369 for two pm_fft2 calls).  PM_ERR_UNSUPPORTED (workspace query: 0) otherwise: the caller composes two
 * pm_fft2 calls.  Uses the fields of pm_fft2_desc: dtype, scale (applied
 * once, at the end), in_* / out_* views, mul_* (required); direction / epilogue / weight are ignored. */
size_t pm_fft2_mul_ifft2_workspace(const pm_fft2_desc* d);
int pm_fft2_mul_ifft2(const pm_fft2_desc* d, const void* in, void* out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Batched 1-D complex transform along one axis of a 2-D array, zero padded or
 * truncated to n on input (numpy `fft.fft(x, n, axis=)` semantics).
 * Replaces fft.fft / fft.ifft at prysm/fttools.py:301-321,335-355,387,519-533 (CZT, FFTDFT).
 *   axis = 1: transform each row;  axis = 0: transform each column.
 *   `t` describes the transform axis on the input (zero pad: len < n) and `t_out` on the output
 *   (crop / shift); `batch` is the extent of the other axis.  */
int pm_fft1(int32_t dtype, int32_t direction, int32_t axis, int64_t batch, const pm_axis* t_in,
            const pm_axis* t_out, double scale, const void* in, int64_t in_ld, void* out, int64_t out_ld,
            void* stream);
/* The same with a workspace: pm_fft1_workspace() bytes (256 B aligned; 0 when none is needed) put 16384 / 32768 and 3 / 5 / 7 x 2^k
 * points on the FFT engine by one radix-R step (an unrotated input view), other lengths that are not powers of two (96 .. 4096)
 * through Bluestein's identity; without it (pm_fft1, or a smaller / NULL workspace) such lengths run on the direct O(n^2) kernel.  FFTDFT with K = 1 / (dx dfx) not a power of two
 * (prysm/fttools.py:484-533) is the caller that needs it. */
size_t pm_fft1_workspace(int32_t dtype, int32_t axis, int64_t batch, int64_t n);
int pm_fft1_ws(int32_t dtype, int32_t direction, int32_t axis, int64_t batch, const pm_axis* t_in,
               const pm_axis* t_out, double scale, const void* in, int64_t in_ld, void* out, int64_t out_ld,
               void* workspace, size_t workspace_bytes, void* stream);

/* One axis of a chirp-Z transform in ONE kernel (fttools.CZT.__call__ / .adjoint, prysm/fttools.py:297-361: per axis
 * `fft(x * b, K) -> * H -> ifft -> slice -> * a * phase`):
 *     out[.., m] = scale * post[m] * IFFT_K( FFT_K( pad_K(pre . in) ) . H )[out_off + m],     m < out_len,
 * the 1 / K of the inverse included.  axis = 1: the nseq sequences are rows of `in` (in_len samples each, placed at
 * [in_off, in_off + in_len) of the K-point sequence -- 0 for the forward transform, Mx - 1 ... for the adjoint's zero embedding);
 * axis = 0: columns.  pre (in_len), H (K) and post (out_len) are complex device vectors of `dtype`, each optionally conjugated
 * (the adjoint); pre and post may be NULL.  K: a power of two from 16 to 8192 (PM_ERR_UNSUPPORTED otherwise: the caller composes
 * pm_fft1 and pm_scale_sep).  The K-point sequence stays in the registers of its workgroup between the two transforms. */
int pm_czt_axis(int32_t dtype, int32_t axis, int64_t nseq, int64_t K, int64_t in_len, int64_t in_off, int64_t out_len, int64_t out_off,
                const void* pre, int32_t pre_conj, const void* H, int32_t h_conj, const void* post, int32_t post_conj, double scale,
                const void* in, int64_t in_ld, void* out, int64_t out_ld, void* stream);

/* One axis of fttools.FFTDFT (prysm/fttools.py:392-535: phase ramp, zero-padded FFT of length K, crop, phase ramp) in ONE kernel:
 *     out[.., m] = scale * post[m] * T_K( pad_K(pre . in) )[out_off + m],     m < out_len,
 * T_K the unnormalised K-point transform with exp(-2 pi i ..) (direction = -1) or exp(+2 pi i ..) (+1); windows, vectors and axis as
 * in pm_czt_axis (same kernel with the multiplier and the second transform switched off).  K: a power of two from 16 to 8192
 * (PM_ERR_UNSUPPORTED otherwise: compose pm_fft1_ws and pm_scale_sep). */
int pm_fft1_ramp(int32_t dtype, int32_t direction, int32_t axis, int64_t nseq, int64_t K, int64_t in_len, int64_t in_off, int64_t out_len,
                 int64_t out_off, const void* pre, int32_t pre_conj, const void* post, int32_t post_conj, double scale, const void* in,
                 int64_t in_ld, void* out, int64_t out_ld, void* stream);

/* --- pointwise / synthesis kernels -------------------------------------------------------- */
/* Every 2-D array of these entry points is row-major with a leading dimension in ELEMENTS (`*_ld`): element [r][c] lies at
 * base + r * ld + c, any ld >= cols and any element-aligned base.  A leading dimension below the number of columns is refused with
 * PM_ERR_ARG before anything is launched -- by pm_spline_prefilter, pm_encircled_energy and pm_encircled_energy_adjoint always, by
 * the others when the array has more than one row (for one row they take any value).  Nothing outside the rows x cols window of an
 * output is written (tests/test_gpu_pointwise.py). */

/* out = a * b (op 0), a * conj(b) (op 1); complex, same shape (rows x cols).
 * Wavefront.__mul__ (prysm/propagation/wavefront.py:360-411), _adjoint_multiply (_kernels.py:29-37). */
int pm_cmul(int32_t dtype, int32_t op, int64_t rows, int64_t cols, const void* a, int64_t a_ld, const void* b,
            int64_t b_ld, void* out, int64_t out_ld, void* stream);

/* out = scale * r * a: r REAL (float for PM_C64, double for PM_C128), a complex, same shape.
 * Wavefront.intensity_adjoint, Gbar = 2 * Ibar * E (prysm/propagation/wavefront.py:282-298), as one sweep. */
int pm_rmul(int32_t dtype, int64_t rows, int64_t cols, const void* r, int64_t r_ld, const void* a, int64_t a_ld, double scale,
            void* out, int64_t out_ld, void* stream);

/* out[i][j] = in[i][j] * ry[i] * cx[j] * scale, ry / cx optional complex vectors, each optionally conjugated.
 * The chirp / phase-ramp multiplies of CZT and FFTDFT (prysm/fttools.py:297-323,508-535). */
int pm_scale_sep(int32_t dtype, int64_t rows, int64_t cols, const void* in, int64_t in_ld, const void* ry,
                 int32_t ry_conj, const void* cx, int32_t cx_conj, double scale, void* out, int64_t out_ld,
                 void* stream);

/* out = re^2 + im^2 (accumulate = 0) or out += weight * (re^2 + im^2).  wavefront.py:146-151;
 * polynomials.sum_of_2d_modes (prysm/polynomials/fitting.py:7-37) as a running weighted sum. */
int pm_abs2(int32_t dtype, int64_t rows, int64_t cols, const void* in, int64_t in_ld, void* out, int64_t out_ld,
            int32_t accumulate, double weight, void* stream);

/* out_abs = |in|, out_arg = atan2(im, re) of a complex array in ONE sweep (either output may be NULL): the MTF and PTF of
 * otf.mtf_ptf_otf_from_psf (prysm/otf.py:167-203) from the centre-normalised OTF the transform already produced. */
int pm_abs_arg(int32_t dtype, int64_t rows, int64_t cols, const void* in, int64_t in_ld, void* out_abs, int64_t abs_ld, void* out_arg,
               int64_t arg_ld, void* stream);

/* out = sum_b weights[b] * modes[b] (accumulate = 0) or out += ...; REAL images of the precision that goes with
 * dtype (PM_C64: float, PM_C128: double), modes[b] at modes + b*mode_stride elements; weights is a HOST array.
 * polynomials.sum_of_2d_modes = tensordot(weights, modes, axes=(0, 0)) (prysm/polynomials/fitting.py:7-37), the
 * incoherent sum of the polychromatic recipe over a batch of intensities. */
int pm_sum_modes(int32_t dtype, int64_t nmodes, int64_t rows, int64_t cols, const void* modes, int64_t mode_stride,
                 int64_t modes_ld, const double* weights, int32_t accumulate, void* out, int64_t out_ld, void* stream);

/* Encircled energy of a PSF from its centre-normalised MTF (Baliga & Cohn 1988):
 *   out[r] = radius_r * df^2 * sum_ij mtf[i][j] * J1(2 pi radius_r nu_ij) / nu_ij,
 * nu = hypot of the FFT-centred frequency grid of spacing df (cy/mm; the zero bin is nudged to 1e-16 like the reference),
 * radii in mm in a HOST array (the reference divides its micron radii by 1e3), `out` a DEVICE array of nradii doubles.
 * Replaces otf._encircled_energy_geometry / _encircled_energy_core (prysm/otf.py:319-343,390-414) for every radius of
 * otf.encircled_energy (otf.py:346-387) in ceil(nradii / 8) passes over the MTF.  mtf is REAL (PM_C64: float, PM_C128: double);
 * J1 and the sums are fp64, reduced in a fixed order (reproducible).  workspace: pm_encircled_energy_workspace() bytes. */
size_t pm_encircled_energy_workspace(void);
int pm_encircled_energy(int32_t dtype, int64_t rows, int64_t cols, const void* mtf, int64_t mtf_ld, double df, int64_t nradii,
                        const double* radii_mm, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* MTF-plane gradient of the encircled energies: mtf_bar[i][j] = sum_r ee_bar[r] * radius_r * J1(2 pi radius_r nu_ij) / nu_ij * df^2
 * (otf.encircled_energy_adjoint, prysm/otf.py:417-472; the caller routes it through mtf_from_psf_adjoint).  radii_mm and
 * ee_bar are HOST arrays; mtf_bar is a REAL rows x cols device array of the precision that goes with dtype. */
int pm_encircled_energy_adjoint(int32_t dtype, int64_t rows, int64_t cols, double df, int64_t nradii, const double* radii_mm,
                                const double* ee_bar, void* mtf_bar, int64_t mtf_bar_ld, void* stream);

/* Resample a measured complex focal-plane-mask map at focal coordinates: scipy.ndimage.map_coordinates(order 0 | 1,
 * mode='nearest') of the real and imaginary parts at row = (yf - center_y)/dx + map_rows/2, col = (xf - center_x)/dx +
 * map_cols/2; points outside [0, n-1] on either axis take fill (a rows x cols complex array) or, with fill NULL, the
 * constant fill_re + i fill_im.  xf / yf are REAL arrays of the precision that goes with dtype, addressed as
 * xf[r*xf_sy + c*xf_sx] (a stride of 0 broadcasts a coordinate vector).  prepare_measured_fpm
 * (prysm/propagation/coronagraph.py:128-200).  Other spline orders: PM_ERR_UNSUPPORTED here, see pm_sample_spline. */
int pm_sample_map(int32_t dtype, int32_t order, int64_t map_rows, int64_t map_cols, const void* map, int64_t map_ld, double dx,
                  double center_x, double center_y, int64_t rows, int64_t cols, const void* xf, int64_t xf_sy, int64_t xf_sx,
                  const void* yf, int64_t yf_sy, int64_t yf_sx, const void* fill, int64_t fill_ld, double fill_re, double fill_im,
                  void* out, int64_t out_ld, void* stream);

/* Spline orders 2 .. 5 of the same resampling (scipy.ndimage.map_coordinates(order, mode='nearest') as prepare_measured_fpm
 * calls it, prysm/propagation/coronagraph.py:193-194): pm_spline_prefilter pads the map by 12 edge samples and runs scipy's
 * recursive B-spline prefilter along both axes in fp64 (once per measured map) into `coeff`, a complex128
 * (map_rows + 24) x (map_cols + 24) array; pm_sample_spline evaluates the tensor-product B-spline at the focal coordinates,
 * arguments as pm_sample_map with `coeff` in place of the map. */
int pm_spline_prefilter(int32_t dtype, int32_t order, int64_t map_rows, int64_t map_cols, const void* map, int64_t map_ld,
                        void* coeff, int64_t coeff_ld, void* stream);
int pm_sample_spline(int32_t dtype, int32_t order, int64_t map_rows, int64_t map_cols, const void* coeff, int64_t coeff_ld,
                     double dx, double center_x, double center_y, int64_t rows, int64_t cols, const void* xf, int64_t xf_sy,
                     int64_t xf_sx, const void* yf, int64_t yf_sy, int64_t yf_sx, const void* fill, int64_t fill_ld,
                     double fill_re, double fill_im, void* out, int64_t out_ld, void* stream);

/* --- deformable mirror (prysm/x/dm.py) ------------------------------------------------------ */
enum { PM_LATTICE_SCATTER = 0, PM_LATTICE_GATHER = 1 };

/* The actuator lattice of x.dm.DM (prepare_actuator_lattice, prysm/x/dm.py:18-61; geometry is the caller's) for a stack of `batch`
 * fields, lattice point (i, j) at grid sample (y0 + i sy, x0 + j sx):
 *   PM_LATTICE_SCATTER: out (rows x cols, REAL) = 0 everywhere, scale * in[i][j] at the lattice points -- the poke array of DM.render
 *                       (`poke_arr[iyy, ixx] = actuators`, dm.py:247); in is nact_y x nact_x.  dtype PM_F32 or PM_F64.
 *   PM_LATTICE_GATHER:  out (nact_y x nact_x, REAL) = scale * in at the lattice points -- `in_actuator_space[iyy, ixx]` of
 *                       DM.render_adjoint (dm.py:331); in is rows x cols, REAL (PM_F32 / PM_F64) or, with PM_C64 / PM_C128, the real
 *                       part of a complex array (in_ld and in_bstride in complex elements).
 * A lattice that does not fit inside the grid, or strides that make outputs overlap, are PM_ERR_ARG. */
int pm_lattice(int32_t dtype, int32_t op, int64_t batch, int64_t rows, int64_t cols, int64_t nact_y, int64_t nact_x, int64_t y0,
               int64_t x0, int64_t sy, int64_t sx, double scale, const void* in, int64_t in_ld, int64_t in_bstride, void* out,
               int64_t out_ld, int64_t out_bstride, void* stream);

/* Pull-warp of a REAL (batch, rows, cols) stack by a 3 x 3 homography H (row-major, 9 HOST doubles, passed to the kernels by value):
 * coordinates.warp (prysm/coordinates.py:644-672) at apply_homography's points (coordinates.py:545-570) as DM.render / render_adjoint
 * call it (dm.py:256, 326), i.e. for warp pixel (R, C):  (x', y', w) = H (C, R, 1);  value = scale * map_coordinates(img, (y'/w, x'/w),
 * order=3, mode='constant', cval=0), coordinates in fp64.  A coordinate outside [0, n - 1] on either axis gives exactly 0; inside, the
 * cubic B-spline of the mirror-prefiltered image.  The result goes through an output window: out (out_rows x out_cols) pixel (r, c) is
 * warp pixel (r + off_y, c + off_x), 0 outside the rows x cols warp domain (pad2d / crop_center, dm.py:267-271).  dtype PM_F32 /
 * PM_F64, or PM_C64 / PM_C128 to warp the real part of a complex stack (in_ld, in_bstride in complex elements); out is REAL.
 * order: 3 only (PM_ERR_UNSUPPORTED otherwise).  Two launches: the prefilter (a separable FIR of 2K + 1 taps, K = 30 fp64 / 14 fp32,
 * the exact impulse response of scipy's recursion) into the workspace, then the 4 x 4 tap evaluation. */
size_t pm_warp_workspace(int32_t dtype, int64_t batch, int64_t rows, int64_t cols);
int pm_warp(int32_t dtype, int32_t order, int64_t batch, int64_t rows, int64_t cols, const void* in, int64_t in_ld, int64_t in_bstride,
            const double* homography, double scale, int64_t out_rows, int64_t out_cols, int64_t off_y, int64_t off_x, void* out,
            int64_t out_ld, int64_t out_bstride, void* workspace, size_t workspace_bytes, void* stream);

/* Zernike polynomials without a stored basis (csrc/zernike.hip).  Points are npts contiguous REAL values per coordinate (dtype PM_F32 /
 * PM_F64, computed in that precision): coords PM_ZERNIKE_CARTESIAN reads (u, v) = (x, y), PM_ZERNIKE_POLAR reads (u, v) = (r, t).
 * `table` is a DEVICE array of nsteps steps built by prysm_amd/polynomials/zernike_plan.py (struct pm::ZStep: T a, b, c, w;
 * int32 op, part, slot, dm -- 32 bytes for PM_F32, 48 for PM_F64): modes sorted by |m| then Jacobi order, each step a Jacobi
 * recurrence step (DLMF 18.9, alpha = 0, beta = |m|) on 2 r^2 - 1, z^|m| (z = x + i y) advanced at each new |m|, and the output slot
 * in [0, nmodes), norm factor and cos / sin part of the mode written there.  Z_n^m = w P_{(n-|m|)//2}^(0,|m|)(2 r^2 - 1) {1, Re z^|m|,
 * Im z^|m|} is the reference's zernike_nm (prysm/polynomials/zernike.py:34-69) with r^|m| cos(m t) = Re z^|m|. */
enum { PM_ZERNIKE_CARTESIAN = 0, PM_ZERNIKE_POLAR = 1 };
/* Radial points for the Q-polynomial walk (pm_qpoly_*): u only, v is not read and may be NULL (angle 0).  The Zernike entry points
 * refuse it. */
enum { PM_QPOLY_RADIAL = 2 };

/* out (nmodes, npts): every mode of the table, one launch -- zernike_nm_seq / zernike_nm (zernike.py:72-163, 34-69). */
int pm_zernike_basis(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                     int64_t nmodes, void* out, void* stream);

/* out[b][p] (+)= sum_k coefs[b][k] Z_k[p] for batch coefficient vectors (coefs: DEVICE, batch x nmodes, read at launch time, so a
 * captured graph uses their current values); out is batch x npts, added to when accumulate != 0.  zernike_sum (zernike.py:166-181)
 * without materialising zernike_nm_seq; one walk of the table per point for each group of up to 8 vectors. */
int pm_zernike_sum(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                   int64_t nmodes, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream);

/* out[b][k] = sum_p databar[b][p] Z_k[p] (databar batch x npts, out batch x nmodes): the adjoint of pm_zernike_sum with respect to the
 * coefficients, i.e. sum_of_2d_modes_adjoint(zernike_nm_seq(...), databar) (fitting.py:40-57) without the basis.  Two launches: one
 * partial per (workgroup, b, k) into the workspace, then a fixed-order sum of the partials -- no atomics, bitwise reproducible. */
size_t pm_zernike_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch);
int pm_zernike_project(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                       int64_t nmodes, int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* out[k] = sum_p modes[k * mode_stride + p] v[p], k < nmodes, p < npts: np.tensordot(modes, databar) of sum_of_2d_modes_adjoint
 * (fitting.py:40-57).  REAL PM_F32 / PM_F64; two launches, deterministic as pm_zernike_project. */
size_t pm_modes_dot_workspace(int32_t dtype, int64_t nmodes, int64_t npts);
int pm_modes_dot(int32_t dtype, int64_t nmodes, int64_t npts, const void* modes, int64_t mode_stride, const void* v, void* out, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Forbes Q polynomials without a stored basis (csrc/qpoly.hip): Qbfs, Qcon and Q2D (prysm/polynomials/qpoly.py).  Points as for the
 * Zernike walk, plus coords PM_QPOLY_RADIAL (u only).  `table` is a DEVICE array of nsteps steps built by
 * prysm_amd/polynomials/qpoly_plan.py (struct pm::QStep: T a, b, c, d, g, h, rf, w; int32 op, part, slot, dm -- 48 bytes for PM_F32,
 * 80 for PM_F64): modes grouped by |m|, one step per order n.  With x = u^2 each step, by its op bits, may RESET the group (z^|m| *= z
 * dm times, P = Q = 0), SEED the auxiliary polynomial (P_{n-1} = P, P = a + b x + c x^2 + d x^3) or ADVance it (P_n = (a + b x) P_{n-1}
 * - c P_{n-2}); either of the last two is followed by the Q step Q_n = (P_n - g Q_{n-1} - h Q_{n-2}) * rf.  A step whose part is not
 * NONE (0) writes w Q_n times x (1 - x) (1, Qbfs), x^2 (2, Qcon), Re z^|m| (3) or Im z^|m| (4) into plane slot; a slot outside
 * [0, nmodes) writes nothing.  Replaces the reference's per-mode numpy loops: Qbfs (qpoly.py:65), Qbfs_seq (408), Qcon (621),
 * Qcon_seq (654), Q2d (893), Q2d_seq (1003), and the sums compute_z_Qbfs (349) and compute_z_Q2d (1888). */

/* out (nmodes, npts): every mode of the table, one launch -- Qbfs_seq, Qcon_seq, Q2d_seq and their single-mode forms. */
int pm_qpoly_basis(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                   int64_t nmodes, void* out, void* stream);

/* out[b][p] (+)= sum_k coefs[b][k] Q_k[p] for batch coefficient vectors (coefs: DEVICE, batch x nmodes, read at launch time);
 * out is batch x npts, added to when accumulate != 0.  compute_z_Qbfs / compute_z_Q2d (qpoly.py:349, 1888) and the package's
 * Q2d_sum / Qcon_sum without the basis; one walk of the table per point for each group of up to 8 vectors. */
int pm_qpoly_sum(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                 int64_t nmodes, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream);

/* out[b][k] = sum_p databar[b][p] Q_k[p]: the adjoint of pm_qpoly_sum with respect to the coefficients (the reference has none).  Two
 * launches as pm_zernike_project: per-workgroup partials into the workspace, then a fixed-order sum -- bitwise reproducible. */
size_t pm_qpoly_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch);
int pm_qpoly_project(int32_t dtype, int32_t coords, int64_t npts, const void* u, const void* v, const void* table, int64_t nsteps,
                     int64_t nmodes, int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* Polynomial families defined by a three-term recurrence, without a stored basis (csrc/recur.hip): Jacobi, Chebyshev of the four
 * kinds, Legendre, Hermite He / H, Laguerre, Dickson of both kinds and the XY monomials (prysm/polynomials/jacobi.py, cheby.py,
 * legendre.py, hermite.py, laguerre.py, dickson.py, xy.py).  `table` is a DEVICE array of nsteps = nmax + 1 records built by
 * prysm_amd/polynomials/recur_plan.py (struct pm::RStep: T a, b, c; int32 slot -- 16 bytes for PM_F32, 32 with padding for PM_F64).
 * Record k is order k: P_k = (a + b x) P_{k-1} - c P_{k-2} and, for the derivative, D_k = b P_{k-1} + (a + b x) D_{k-1} - c D_{k-2},
 * walked from P_{-1} = 1, P_{-2} = 0, D = 0, so record 0 is (P_0, 0, 0) and record 1 has c = 0; slot is the output plane (or the
 * coefficient) of order k, a slot outside [0, nout) writes nothing.  REAL dtypes PM_F32 / PM_F64, computed in that precision.
 * The argument of the walk: PM_RECUR_X, u[p] (v is not read and may be NULL); PM_RECUR_R2, 2 (u^2 + v^2) / radius^2 - 1 from the
 * Cartesian arrays u = x, v = y (jacobi.py:376-413). */
enum { PM_RECUR_X = 0, PM_RECUR_R2 = 1 };

/* out (nout, npts) = P_k and / or out_der (nout, npts) = dP_k / d(argument), either may be NULL, one launch: the *_seq and *_der_seq
 * of cheby.py:74-321, legendre.py:34-110, hermite.py:84-120, laguerre.py:65-140, dickson.py:87-275, jacobi.py:148-276 (jacobi_seq,
 * jacobi_der_seq, jacobi_seq_with_der) and their single-order forms. */
int pm_recur_basis(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                   int64_t nout, void* out, void* out_der, void* stream);

/* out[b][p] (+)= sum_k coefs[b][slot_k] P_k for batch coefficient vectors (coefs: DEVICE, batch x ncoef, read at launch time), up to 8
 * vectors per walk; any of the three outputs may be NULL.  PM_RECUR_X: out_dx = sum_k c D_k, out_dy must be NULL.  PM_RECUR_R2:
 * out_dx = dz/du 4 x / R^2, out_dy = dz/du 4 y / R^2.  jacobi_sum_clenshaw with dense orders (jacobi.py:279-316), jacobi_radial_sum
 * (376-389), jacobi_radial_sum_der_xy (392-413) without the basis. */
int pm_recur_sum(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                 int64_t ncoef, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* out_dx, void* out_dy, void* stream);

/* out[b][k] = sum_p databar[b][p] P_k(u_p), the adjoint of pm_recur_sum with respect to the coefficients (the reference has none).
 * der != 0: the derivative basis, for PM_RECUR_R2 with the chain factors: sum_p (databar 4 x / R^2 + databar2 4 y / R^2) D_k, databar
 * the adjoint of out_dx and databar2 (may be NULL) of out_dy; accumulate != 0 adds into out.  Two launches as pm_zernike_project: per-workgroup partials in a fixed
 * order into the workspace (pm_recur_project_workspace bytes), then a fixed-order sum -- no atomics, bitwise reproducible. */
size_t pm_recur_project_workspace(int32_t dtype, int64_t npts, int64_t nout, int64_t batch);
int pm_recur_project(int32_t dtype, int32_t form, int64_t npts, const void* u, const void* v, double radius, const void* table, int64_t nsteps,
                     int64_t nout, int64_t batch, int32_t der, const void* databar, const void* databar2, int32_t accumulate, void* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The separable sum on a rows x cols Cartesian grid: z[b][i][j] = sum_{n,m} coefs[b][n][m] Py_n(y[i]) Px_m(x[j]) with
 * zx = inv_xnorm dz/dx and zy = inv_ynorm dz/dy, the outputs chosen by the mask `what`; x[cols], y[rows], one table per axis (nx,
 * ny records, slot unused) and the dense DEVICE matrices coefs (batch, ny, nx), read at launch time.  One launch, factored through
 * t[n][j] = sum_m C[n][m] Px_m(x_j) in LDS; every output is stored once and no basis is stored.  Output rows lie ld elements apart,
 * members of the stack bstride.  An axis takes at most 64 orders (PM_ERR_UNSUPPORTED beyond).  cheby1_2d_sum[_der_xy]
 * (cheby.py:324-362, x_norm = 1 / inv_xnorm) and xy_sum[_der_xy] (xy.py:334-383, three matrix products over stored power tables). */
enum { PM_RECUR2_Z = 1, PM_RECUR2_ZX = 2, PM_RECUR2_ZY = 4 };
int pm_recur2_sum(int32_t dtype, int64_t rows, int64_t cols, const void* x, const void* y, const void* xtable, int64_t nx, const void* ytable,
                  int64_t ny, int64_t batch, const void* coefs, int32_t what, double inv_xnorm, double inv_ynorm, void* z, void* zx, void* zy,
                  int64_t ld, int64_t bstride, void* stream);

/* out[b][n][m] (+)= sum_{i,j} databar[b][i][j] Fy_n(y[i]) Fx_m(x[j]): the adjoint of ONE of the maps of pm_recur2_sum with respect to
 * coefs (the reference has none) -- what = PM_RECUR2_Z (F the values), PM_RECUR2_ZX (Fx the derivative, times inv_xnorm) or
 * PM_RECUR2_ZY (Fy the derivative, times inv_ynorm); accumulate != 0 adds into out, so the three adjoints can share one.  Two
 * launches: the rows of each chunk reduced per column into the workspace (pm_recur2_project_workspace bytes), then the chunks summed
 * in order and the columns contracted in a fixed order -- no atomics, bitwise reproducible. */
size_t pm_recur2_project_workspace(int32_t dtype, int64_t rows, int64_t cols, int64_t ny, int64_t batch);
int pm_recur2_project(int32_t dtype, int64_t rows, int64_t cols, const void* x, const void* y, const void* xtable, int64_t nx,
                      const void* ytable, int64_t ny, int64_t batch, int32_t what, double inv_xnorm, double inv_ynorm, const void* databar,
                      int64_t ld, int64_t bstride, int32_t accumulate, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* out[k][i][j] = ty[n_k][i] tx[m_k][j] for the nk DEVICE int32 pairs (m_k, n_k) of `pairs`, from two stored 1-D tables ty (nty, rows)
 * and tx (ntx, cols) (two small pm_recur_basis calls); a pair outside the tables writes nothing.  xy_seq, xy_der_x_seq, xy_der_y_seq,
 * xy_der_xy_seq (xy.py:166-300). */
int pm_recur2_outer(int32_t dtype, int64_t rows, int64_t cols, int64_t nk, const void* ty, int64_t nty, const void* tx, int64_t ntx,
                    const void* pairs, void* out, void* stream);

/* Coordinates (csrc/geometry.hip): REAL arrays of dtype PM_F32 / PM_F64, computed in that precision. */

/* make_xy_grid (prysm/coordinates.py:344-378) with fftrange (fttools.py:13-15): element j of an axis of n samples is (j - n / 2)
 * converted to dtype, times dx rounded once to dtype.  grid != 0: x and y are ny x nx meshgrids; grid == 0: x holds nx and y ny values.
 * Both outputs from one launch. */
int pm_xy_grid(int32_t dtype, int64_t ny, int64_t nx, double dx, int32_t grid, void* x, void* y, void* stream);

/* cart_to_polar (coordinates.py:73-102): rho = hypot(x, y), phi = atan2(y, x), ny x nx values each, one launch.  separable != 0: x
 * holds nx and y ny values (the reference's vec_to_grid); else x and y hold ny x nx values. */
int pm_cart_to_polar(int32_t dtype, int64_t ny, int64_t nx, int32_t separable, const void* x, const void* y, void* rho, void* phi,
                     void* stream);

/* polar_to_cart (coordinates.py:105-125): x = rho cos(phi), y = rho sin(phi) for n points, one launch. */
int pm_polar_to_cart(int32_t dtype, int64_t n, const void* rho, const void* phi, void* x, void* y, void* stream);

/* Aperture geometry (csrc/geometry.hip): a tree of the signed-distance shapes of prysm/geometry.py, combined on the distance and
 * turned into an array once, in ONE launch that writes every output element once.  Replaces the array sweeps of antialias
 * (geometry.py:11-34), union / intersect / subtract (37-93), gaussian (154-179), rectangle_sdf (182-222), rotated_ellipse_sdf
 * (251-290), circle_sdf (337-353), annulus_sdf (375-395), polygon_sdf (419-463), regular_polygon_sdf (466-491), spider_sdf (550-594),
 * offset_circle (627-653), rectangle_with_corner_fillets_sdf (656-696) and of the `<= 0` of their mask forms.
 *
 * `table` is a DEVICE array of batch x nsteps steps built by prysm_amd/geometry_plan.py (struct pm::GStep: int32 op, comb, slot, flags;
 * T f[8] -- 48 bytes for PM_F32, 80 for PM_F64), program b at table + b * nsteps.  A step evaluates (a part of) a primitive at the
 * point: op 1 circle / 2 annulus about (f0, f1) with radius f2 (half-width f3); 3 / 4 the same on a RADIAL coordinate taken from x;
 * 5 rectangle (coordinates rotated by (cos, sin) = (f0, f1) when flag ROT, then centre (f2, f3), half-sizes f4, f5, fillet f6);
 * 6 ellipse (cos f0, sin f1, axes f2, f3 and their squares f4, f5); 7 one polygon edge from (f0, f1) along (f2, f3), f4 = 1 / |e|^2,
 * f5 the end's y, flag UP = it rises; 8 one spider vane (cos f0, sin f1, root (f2, f3), half-width f4); 9 gaussian; 10 MERGE (the
 * value is accumulator slot + 1); 0 nothing.  Flag BEGIN starts a primitive of several steps (edges, vanes: running min / crossing
 * parity), flag END finishes it and combines it into accumulator `slot` (0 .. 3) by comb: 0 set, 1 min, 2 max, 3 max(acc, -value).
 * The result is accumulator 0.
 *
 * coords: PM_COORDS_GRID computes x = T(j - ox) * T(dx), y = T(i - oy) * T(dy) from the pixel index (x, y not read, may be NULL);
 * PM_COORDS_SEPARABLE reads x (nx values) and y (ny values); PM_COORDS_POINTWISE reads x and y of ny x nx values each (contiguous).
 * out_kind: PM_SDF_MASK writes 1-byte booleans d <= 0, PM_SDF_DISTANCE d, PM_SDF_COVERAGE min(max(0.5 - d / aa_dx, 0), 1) in dtype.
 * out: batch x ny x nx elements with out_ld elements between rows and out_bstride between programs. */
enum { PM_COORDS_GRID = 0, PM_COORDS_SEPARABLE = 1, PM_COORDS_POINTWISE = 2 };
enum { PM_SDF_MASK = 0, PM_SDF_DISTANCE = 1, PM_SDF_COVERAGE = 2 };
int pm_sdf_render(int32_t dtype, int32_t coords, int64_t ny, int64_t nx, const void* x, const void* y, int64_t ox, int64_t oy, double dx,
                  double dy, const void* table, int64_t nsteps, int64_t batch, int32_t out_kind, double aa_dx, void* out, int64_t out_ld,
                  int64_t out_bstride, void* stream);

/* The detector (csrc/detector.hip): prysm/detector.py's bindown (222-274), tile (277-339) and Detector.expose (83-148).
 *
 * pm_bindown: out (batch x my x nx) = the bins of fy x fx elements of in (batch x my fy x nx fx), summed (PM_BIN_SUM) or averaged
 * (PM_BIN_AVG: the sum divided by fy fx).  Each bin is one running sum in dtype, its rows in order and left to right within a row, so
 * the result is bitwise reproducible.  pm_tile is the adjoint: out (batch x my fy x nx fx) = every element of in (batch x my x nx)
 * repeated fy x fx times, times `scale`.  Leading dimensions and batch strides in elements; one launch each, no atomics. */
enum { PM_BIN_AVG = 0, PM_BIN_SUM = 1 };
int pm_bindown(int32_t dtype, int64_t batch, int64_t my, int64_t nx, int64_t fy, int64_t fx, int32_t mode, const void* in, int64_t in_ld,
               int64_t in_bstride, void* out, int64_t out_ld, int64_t out_bstride, void* stream);
int pm_tile(int32_t dtype, int64_t batch, int64_t my, int64_t nx, int64_t fy, int64_t fx, double scale, const void* in, int64_t in_ld,
            int64_t in_bstride, void* out, int64_t out_ld, int64_t out_bstride, void* stream);

/* The deterministic tail of an exposure, in fp64 whatever dtype the electrons have: + bias, clip at fwc, times 1 / conversion_gain,
 * clip to [0, 2^bits - 1], truncation toward zero, then lut[DN] when lut is not NULL (a DEVICE table of lut_len >= 2^bits elements
 * of out_bytes bytes each).  electrons: batch x ny x nx (PM_F32 / PM_F64) with ld elements between rows and bstride between
 * members; out: contiguous, elements of out_bytes (1, 2, 4 or 8) bytes; without a LUT 8 * out_bytes >= bits. */
int pm_detector_digitize(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* electrons, int64_t ld, int64_t bstride, double bias,
                         double fwc, double conversion_gain, int32_t bits, const void* lut, int64_t lut_len, int32_t out_bytes, void* out,
                         void* stream);

/* Detector.expose fused: `frames` noisy exposures of img (batch x ny x nx, strided like pm_detector_digitize's input) into out
 * (frames x batch x ny x nx, contiguous, out_bytes per element), one launch plus a one-thread launch that advances the state.
 * Per pixel: mean = img * exposure_time * prnu + dark_current * exposure_time * dcnu in fp64 (prnu, dcnu: DEVICE fp64 maps of ny x nx,
 * contiguous, shared by the members; NULL = 1); per frame: shot ~ Poisson(mean) (exact: inversion below a mean of 10, Hoermann's PTRS
 * from there), read = read_noise * N(0, 1) (nothing drawn when read_noise == 0), then the tail of pm_detector_digitize.  Random
 * words are Philox4x32-10 with key = seed and counter = (pixel low word, pixel high word, (state[0] + frame) mod 2^32, draw block);
 * pixel = pixel_offset + the row-major index into the stack.  `state` is a DEVICE array of two int64: [0] the exposure index (frames
 * exposed so far), read by the kernel and advanced by `frames` after it on the same stream; [1] a status word that is set to 1 when
 * a mean is negative, NaN or infinite (such a pixel gets 0 shot electrons).  prysm_amd/detector_plan.py is the same arithmetic in numpy. */
int pm_detector_expose(int32_t dtype, int64_t batch, int64_t ny, int64_t nx, const void* img, int64_t ld, int64_t bstride, const void* prnu,
                       const void* dcnu, double exposure_time, double dark_current, double read_noise, double bias, double fwc,
                       double conversion_gain, int32_t bits, const void* lut, int64_t lut_len, int32_t out_bytes, int64_t frames, int64_t seed,
                       int64_t pixel_offset, void* state, void* out, void* stream);

/* The four Philox words of draw block `block` of the pixels pixel0 .. pixel0 + npix - 1 at global frame index `frame`, to out (npix x 4
 * uint32): what the tests pin the kernels' generator with. */
int pm_detector_words(int64_t seed, int64_t pixel0, int64_t npix, int64_t frame, int32_t block, void* out, void* stream);

/* Bayer mosaics (csrc/bayer.hip): prysm/bayer.py.  The colour of a pixel is the parity of (row, col): PM_CFA_RGGB has R at (even, even),
 * G1 at (even, odd), G2 at (odd, even), B at (odd, odd); PM_CFA_BGGR swaps R and B.  Stacks are batch x m x n with a row stride and a
 * batch stride in elements; REAL data, PM_F32 or PM_F64.  prysm_amd/bayer_plan.py is the same arithmetic in numpy. */
enum { PM_CFA_RGGB = 0, PM_CFA_BGGR = 1 };
enum { PM_BAYER_COMPOSITE = 0, PM_BAYER_RECOMPOSITE = 1 };
enum { PM_BAYER_MOSAIC = 0, PM_BAYER_RGB = 1 };

/* demosaic_malvar (bayer.py:378-447, weights 344-375 divided by 8) as ONE kernel: in (batch x m x n; in_dtype PM_F32 / PM_F64 equal to
 * out_dtype, or PM_U8 / PM_U16 / PM_U32 read as stored and converted in registers) to out, contiguous: batch x m x n x 3 interleaved
 * R, G, B, or with planar != 0 batch x 3 x m x n.  Native sites are copies; every other value is one running sum over the taps of its
 * filter in row-major order of the 5 x 5 footprint.  Boundary: scipy's mode='reflect' (index i of an axis of length n reads
 * j = i mod 2n; j >= n ? 2n - 1 - j : j).  Any m, n >= 1. */
int pm_bayer_demosaic(int32_t in_dtype, int32_t out_dtype, int32_t cfa, int32_t planar, int64_t batch, int64_t m, int64_t n, const void* in,
                      int64_t in_ld, int64_t in_bstride, void* out, void* stream);

/* composite_bayer (bayer.py:130-171; PM_BAYER_COMPOSITE: out[r][c] = plane(parity)[r][c], planes of m x n) and recomposite_bayer
 * (bayer.py:213-257; PM_BAYER_RECOMPOSITE: out[2i + py][2j + px] = plane(parity)[i][j], planes of m/2 x n/2, m and n even).  out is
 * batch x m x n.  Each plane has its own row, element and batch stride (in elements), so the stride-2 views of decomposite_bayer
 * (bayer.py:174-210) go straight back in. */
int pm_bayer_weave(int32_t dtype, int32_t mode, int32_t cfa, int64_t batch, int64_t m, int64_t n, const void* r, int64_t r_rs, int64_t r_es,
                   int64_t r_bs, const void* g1, int64_t g1_rs, int64_t g1_es, int64_t g1_bs, const void* g2, int64_t g2_rs, int64_t g2_es,
                   int64_t g2_bs, const void* b, int64_t b_rs, int64_t b_es, int64_t b_bs, void* out, int64_t out_ld, int64_t out_bstride,
                   void* stream);

/* demosaic_deinterlace (bayer.py:260-282): in (batch x m x n, m and n even) to out (batch x m/2 x n/2 x 3, contiguous) as r, (g1 + g2) / 2, b. */
int pm_bayer_deinterlace(int32_t dtype, int32_t cfa, int64_t batch, int64_t m, int64_t n, const void* in, int64_t in_ld, int64_t in_bstride,
                         void* out, void* stream);

/* The last lines of assemble_superresolved (bayer.py:331-336): out (batch x m x n x 3, contiguous) = r, (g2 + g1) / 2, b from four planes
 * of m x n with their own row, element and batch strides (the real part of a complex plane is a plane of element stride 2). */
int pm_bayer_assemble(int32_t dtype, int64_t batch, int64_t m, int64_t n, const void* r, int64_t r_rs, int64_t r_es, int64_t r_bs, const void* g1,
                      int64_t g1_rs, int64_t g1_es, int64_t g1_bs, const void* g2, int64_t g2_rs, int64_t g2_es, int64_t g2_bs, const void* b,
                      int64_t b_rs, int64_t b_es, int64_t b_bs, void* out, void* stream);

/* White balance without a host round trip (wb_prescale bayer.py:13-75, wb_postscale bayer.py:78-127).
 * pm_bayer_class_max: the maxima of the classes of `in` to `maxima`, a DEVICE array of four doubles: PM_BAYER_MOSAIC the parity classes
 * 2 (row & 1) + (col & 1) of batch x m x n; PM_BAYER_RGB the channels of batch x m x n x 3 (row stride >= 3 n; maxima[3] = -inf).  Two
 * launches, comparisons only, deterministic; NaN propagates like numpy's max.  workspace: pm_bayer_class_max_workspace() DEVICE bytes.
 * pm_bayer_scale: data *= the gain of its class, in place.  gains / saturation are HOST arrays in the reference's order (r, g1, g2, b
 * for a mosaic, r, g, b for RGB).  With safe != 0 the kernel first divides the gains by `ratio`, computed in dtype from `maxima`:
 * ratio = 1, then per class in that order rat = max * gain / sat, taken when rat > 1 and rat > ratio. */
size_t pm_bayer_class_max_workspace(void);
int pm_bayer_class_max(int32_t dtype, int32_t classes, int64_t batch, int64_t m, int64_t n, const void* in, int64_t in_ld, int64_t in_bstride,
                       void* maxima, void* workspace, size_t workspace_bytes, void* stream);
int pm_bayer_scale(int32_t dtype, int32_t classes, int32_t cfa, int64_t batch, int64_t m, int64_t n, void* data, int64_t ld, int64_t bstride,
                   const double* gains, int32_t safe, const double* saturation, const void* maxima, void* stream);

/* Gradient-based optimisation (csrc/optym.hip): prysm/x/optym.  REAL data, PM_F32 or PM_F64; arrays of any shape are taken flat and
 * contiguous.  Nothing here reads a device value on the host, so an iteration (model, cost, adjoints, step) can be captured in a graph.
 * prysm_amd/x/optym_plan.py is the same arithmetic in numpy. */
enum { PM_COST_MSE = 0, PM_COST_BGI = 1, PM_COST_NLL = 2 };
enum { PM_OPT_GD = 0, PM_OPT_ADAGRAD = 1, PM_OPT_RMSPROP = 2, PM_OPT_ADAM = 3, PM_OPT_RADAM = 4, PM_OPT_ADAMOMENTUM = 5, PM_OPT_YOGI = 6 };
enum { PM_ACT_TANH = 0, PM_ACT_ARCTAN = 1, PM_ACT_SOFTPLUS = 2, PM_ACT_SIGMOID = 3 };
enum { PM_GRAD_FORWARD_X = 0, PM_GRAD_ADJOINT_X = 1, PM_GRAD_FORWARD_Y = 2, PM_GRAD_ADJOINT_Y = 3 };

/* mean_square_error (x/optym/cost.py:73-96), bias_and_gain_invariant_error (cost.py:30-70) and negative_loglikelihood (cost.py:99-125)
 * with the mask handling of cost.py:8-27: the cost to `cost`, a DEVICE cell of dtype, and d cost / d M to grad (n values of dtype, zero
 * where the mask is false).  M, D: n values; D may be NULL for PM_COST_NLL, whose target is then d_scalar.  mask: n bytes (ANY nonzero
 * byte keeps the element, 2 and 255 as 1 does) or NULL; an element the mask drops is never used, whatever it holds (NaN, infinity).
 * The mask is a predicate, nothing is compacted: the selected count N is one of the sums.  Every sum is
 * accumulated in double, per workgroup and then by one workgroup in a fixed order (no atomics: the result is the same bits run after
 * run), and 1/N, alpha, beta and R are formed in double on the device.  PM_COST_MSE and PM_COST_NLL are three launches (sums, fold,
 * gradient).  PM_COST_BGI is six: N, sum I, sum D and sum D^2 and their fold, which leaves the two means on the device; a second read
 * of I and D for sum (I - Imean)(D - Dmean) and sum (I - Imean)^2 -- the sums of CENTRED data, as the reference centres before it
 * multiplies, so that a pedestal on I or D costs no digits of alpha -- and the fold that forms alpha and beta; the gradient pass, which
 * carries sum(raw_err^2), and the fold that forms the cost, the reference's sum of squared residuals.  An all-false mask gives a
 * NaN cost and a zero gradient.  workspace: pm_optym_cost_workspace() DEVICE bytes, 8-byte aligned. */
size_t pm_optym_cost_workspace(void);
int pm_optym_cost(int32_t dtype, int32_t kind, int64_t n, const void* M, const void* D, double d_scalar, const void* mask, void* cost, void* grad,
                  void* workspace, size_t workspace_bytes, void* stream);

/* One step of GradientDescent, AdaGrad, RMSProp, Adam, RAdam, AdaMomentum or Yogi (x/optym/optimizers.py:205-500) as two launches.
 * pm_optym_advance (one thread): counter (a DEVICE int64, the reference's self.iter) += 1 = k, and coef (eight DEVICE doubles) =
 * 1 - beta1^k, 1 - beta2^k, RAdam's rho and r (optimizers.py:405-413), its branch (1 where rho >= 5), sqrt(1 - beta2^k), 0, 0.
 * pm_optym_step (one kernel over the n variables): the projected gradient (_project_gradient, optimizers.py:85-96), the moment update,
 * the step and the clamp (_project_bounds, optimizers.py:79-82), in dtype, each expression as the reference writes it.  x, s1 (m, or
 * the accumulator of AdaGrad / RMSProp; NULL for PM_OPT_GD) and s2 (v; from PM_OPT_ADAM on) are updated IN PLACE; the pre-step
 * iterate goes to x_prev.  beta1 is RMSProp's gamma.  lower / upper: n values each (infinite where a side is free) or both NULL; with
 * bounds the kernel also stores g_step (n values) and active (n bytes: the post-step iterate sits on a finite bound,
 * _store_bounded_step_metadata, optimizers.py:99-112).  coef is read from PM_OPT_ADAM on. */
int pm_optym_advance(int32_t kind, double beta1, double beta2, void* counter, void* coef, void* stream);
int pm_optym_step(int32_t dtype, int32_t kind, int64_t n, void* x, const void* g, void* s1, void* s2, const void* lower, const void* upper,
                  double alpha, double beta1, double beta2, double eps, const void* coef, void* x_prev, void* g_step, void* active, void* stream);

/* forward (backprop == 0) or backprop of Tanh, Arctan, Softplus and Sigmoid (x/optym/activation.py:207-252) with the affine parameters
 * a, x0, y0: one sweep, out may be x. */
int pm_optym_activation(int32_t dtype, int32_t kind, int32_t backprop, int64_t n, const void* x, double a, double x0, double y0, void* out,
                        void* stream);

/* Softmax.forward (activation.py:27-52) over rows x K, K last and contiguous: out = exp(x - max) / sum.  A row takes the smallest
 * power-of-two group of lanes that holds K, at most 64, and longer rows loop.  With u (rows x K uniform variates) the logits are
 * (x - log(-log(u + eps) + eps)) / tau, GumbelSoftmax.forward (activation.py:104-121), formed in the load, once per element (rows
 * longer than 64 stage their logits in out).
 * pm_optym_softmax_backprop (activation.py:54-83, 123-127): gin_k = y_k (grad_k S - sum_j grad_j y_j) / tau from the forward result y,
 * with S = sum_j y_j (1 up to the rounding of y), the two sums and the bracket in double: the reference's grad_k - sum_j grad_j y_j
 * cancels down to the rounding of y on a saturated row. */
int pm_optym_softmax(int32_t dtype, int64_t rows, int64_t K, const void* x, const void* u, double tau, double eps, void* out, void* stream);
int pm_optym_softmax_backprop(int32_t dtype, int64_t rows, int64_t K, const void* y, const void* grad, double tau, void* gin, void* stream);

/* SpatialGradient2D (x/optym/operators.py:5-48) on a contiguous m x n array: forward differences over the interior of an axis and
 * their adjoints, the adjoints as gathers.  in and out must differ. */
int pm_optym_spatial_gradient(int32_t dtype, int32_t op, int64_t m, int64_t n, const void* in, void* out, void* stream);

/* L-BFGS-B (csrc/lbfgsb.hip): the passes over the n variables of one step of PrysmLBFGSB (prysm/x/optym/_prysm_lbfgsb.py:206-1108).
 * REAL data, PM_F32 or PM_F64, arrays taken flat; sums in double, two-stage, no atomics.  The history S, Y is (ring, n) row-major,
 * rows `ld` apart, a ring in PHYSICAL order: logical pair j < k (oldest first) is row (start + j) % ring.  W = [Y, theta S] has 2k
 * rows q (q < k: Y's pair q; q >= k: S's pair q - k); results are in that order and WITHOUT theta.  k above PM_LBFGSB_MAX_MEMORY is
 * PM_ERR_UNSUPPORTED before any launch.  `record`: DEVICE doubles the pass's sums are left in (NULL: no fold launch, the partials stay in the workspace for pm_lbfgsb_small); `workspace`: pm_lbfgsb_workspace()
 * DEVICE bytes; both 8-byte aligned.  A pass is one launch over n and one fold launch.  prysm_amd/x/lbfgsb_plan.py is the same
 * arithmetic in numpy and unpacks the records. */
enum { PM_LBFGSB_MAX_MEMORY = 32, PM_LBFGSB_TILE = 8, PM_LBFGSB_THREADS = 256, PM_LBFGSB_WGS = 1024, PM_LBFGSB_GRAM_WGS = 256 };
enum { PM_LBFGSB_DIRECTION = 0, PM_LBFGSB_RESIDUAL = 1, PM_LBFGSB_SUBSPACE = 2 };
enum { PM_LBFGSB_SMALL_DIRECTION = 0, PM_LBFGSB_SMALL_BREAK = 1, PM_LBFGSB_SMALL_RESIDUAL = 2, PM_LBFGSB_SMALL_SUBSPACE = 3, PM_LBFGSB_SMALL_UPDATE = 4 };
size_t pm_lbfgsb_workspace(void);

/* The small algebra, everything of size 2k x 2k, in double, ONE single-workgroup launch per use (the compact form, lines 316-345;
 * _WM, 362-407; _Hg, 424-437; _subspace_solve, 856-899; _update_history, 979-1007).  `state`: pm_lbfgsb_state_doubles(memory) DEVICE
 * doubles that live as long as the optimizer, zero at the start except theta = 1 at [3 memory^2]: S S^T, S Y^T ([i][j] = s_i . y_j)
 * and Y Y^T, memory x memory each, in LOGICAL order, then theta.  The launch first adds the first-stage partials the pass before it
 * left in its workspace (that pass called with record = NULL: `partials` is that workspace, nparts its workgroups,
 * min(PM_LBFGSB_WGS, ceil(n / 256))), then by op:
 * DIRECTION (after pm_lbfgsb_dots of g): coef = the rows' weights of (1 / theta^2) W N^-1 W^T g, N = -M + W^T W / theta from the
 *   maintained Gram matrices; record[0] = g . g.
 * BREAK (after pm_lbfgsb_breakpoints): record = [row . d0 (2k) | d0 . d0, count t <= 0, count finite t > 0 | theta | M (2k x 2k)].
 * RESIDUAL (no pass before it): coef = the rows' weights of -W M^-1 c, c = c_in (2k DEVICE doubles).
 * SUBSPACE (after pm_lbfgsb_dots of r under the mask, and pm_lbfgsb_gram with record = NULL into `gram_partials`, gram_parts =
 *   min(PM_LBFGSB_GRAM_WGS, ceil(n / 256)) its workgroups, or 0 to take the maintained Gram: no variable is active): coef for dx.
 * UPDATE (after pm_lbfgsb_update): the curvature test, the new row and column of the three Gram matrices (a full history drops
 *   its oldest pair), theta rounded to dtype; record = [accepted, s . s, s . y, y . y, theta].  The ring's k and start are the caller's.
 * coef: 2k DEVICE doubles.  memory above PM_LBFGSB_MAX_MEMORY is PM_ERR_UNSUPPORTED. */
size_t pm_lbfgsb_state_doubles(int32_t memory);
int pm_lbfgsb_small(int32_t dtype, int32_t op, int32_t memory, int32_t k, int32_t nparts, int32_t gram_parts, void* state, const void* c_in,
                    void* coef, void* record, const void* partials, const void* gram_partials, void* stream);

/* row_q . v for the 2k rows (W^T g of _Hg, line 435; W_F^T r of _subspace_solve, line 887, under the byte mask `mask`, NULL = all)
 * and v . w (v . v with w NULL; phi' = g_new . p with k = 0).  record, per tile T of PM_LBFGSB_TILE rows, 9 doubles: the tile's 8
 * products, then (tile 0) v . w; max(1, ceil(2k / 8)) tiles. */
int pm_lbfgsb_dots(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* v,
                   const void* w, const void* mask, void* record, void* workspace, size_t workspace_bytes, void* stream);

/* _compute_breakpoints (lines 477-507) and the seed of _cauchy (lines 565-609) in one pass: t_i by the reference's sign and finiteness
 * rules (lower, upper: infinite where there is no bound), d0 = -g where t_i > 0 and 0 elsewhere -- the variables with t_i = 0 are
 * segments of zero length and leave the path at once -- both stored.  record, per tile 11 doubles: row . d0 of the tile's 8 rows, then
 * (tile 0) d0 . d0, the count of t_i <= 0, the count of finite t_i > 0. */
int pm_lbfgsb_breakpoints(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* x,
                          const void* g, const void* lower, const void* upper, void* t, void* d0, void* record, void* workspace,
                          size_t workspace_bytes, void* stream);

/* The history update (step, lines 1086-1096, and _update_history, lines 979-1007): s = alpha p (xt NULL) or s = xt - x (the clipped
 * trial point), y = g_new - g, formed in the pass and stored into row `slot` of S and Y (not a live row), dotted with every live row
 * and with each other.  record, per tile 19 doubles: (row . s, row . y) of the tile's 8 rows, then (tile 0) s . s, s . y, y . y.  The
 * curvature test and the ring's bookkeeping are the caller's. */
int pm_lbfgsb_update(int32_t dtype, int64_t n, void* S, void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, int32_t slot, const void* xt,
                     const void* x, const void* p, double alpha, const void* g_new, const void* g, void* record, void* workspace,
                     size_t workspace_bytes, void* stream);

/* W_F^T W_F (line 883) without theta: the products of all row pairs over the variables whose mask byte is set (NULL = all), in
 * 8 x 8 blocks.  record: 64 doubles per tile pair (ti <= tj, counted row by row), [r * 8 + c] = row (8 ti + r) . row (8 tj + c).
 * k >= 1. */
int pm_lbfgsb_gram(int32_t dtype, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k, const void* mask,
                   void* record, void* workspace, size_t workspace_bytes, void* stream);

/* out = a v + b (u1 - u2) + sum_q coef[q] row_q (coef: 2k DEVICE doubles), accumulated in double and rounded at the store.
 * PM_LBFGSB_DIRECTION: out = p, e.g. -H g (_Hg, lines 430-437).  PM_LBFGSB_RESIDUAL: out = r (lines 856-863), no record.
 * PM_LBFGSB_SUBSPACE: the value is dx on the free set (mask) and 0 elsewhere (lines 893-903); x_hat = xc + dx, x_bar = clip(x_hat),
 * out = x_bar - x, out2 = x_hat - x (lines 1045-1061).  record, 5 doubles: g . out, the count of out != 0, g . out2, the count of
 * out2 != 0, the minimum of _max_alpha_inside_box's bound_alpha for out2 (lines 906-926; the last three 0, 0, inf for DIRECTION). */
int pm_lbfgsb_combine(int32_t dtype, int32_t mode, int64_t n, const void* S, const void* Y, int64_t ld, int32_t ring, int32_t start, int32_t k,
                      double a, const void* v, double b, const void* u1, const void* u2, const void* coef, const void* mask, const void* xc,
                      const void* x, const void* lower, const void* upper, const void* g, void* out, void* out2, void* record, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The Cauchy point write (lines 746-775): visited (t_i <= t_last) variables get xc = x - t g and a 0 byte in free_mask, the others
 * xc = x + t_stop (-g) and a 1.  One launch. */
int pm_lbfgsb_cauchy_point(int32_t dtype, int64_t n, const void* x, const void* g, const void* t, double t_last, double t_stop, void* xc,
                           void* free_mask, void* stream);

/* The trial point xt = x + alpha p (_wolfe_eval, line 25).  With lower and upper it is clipped into the box: the reference clips
 * only the accepted point (lines 1088-1093) and evaluates the search's other trial points unclipped; here every trial point is
 * clipped, so the accepted one IS x_new and g_new belongs to it. */
int pm_lbfgsb_trial(int32_t dtype, int64_t n, const void* x, const void* p, double alpha, const void* lower, const void* upper, void* xt,
                    void* stream);

/* Thin-film multilayers (csrc/thinfilm.hip): prysm/thinfilm.py and the core of prysm/x/coatings (stack.py, diff.py).  One thread per
 * sample k < K walks the L layers (ambient side first) in registers.  dtype PM_C64 or PM_C128; real operands are of the matching real
 * type.  Operands, all DEVICE arrays: wvl (wavelength) and theta (the ambient angle, RADIANS), real; n0 (ambient index) and nsub
 * (substrate index), complex; the layer tables n (complex) and d (real, the unit of wvl).  Every operand has a sample stride `_ss` of
 * 0 (one value shared by all samples) or 1 (one per sample); layer j of a table starts `_ls` elements after layer j - 1 (at least K
 * where the table is per sample).  prysm_amd/thinfilm_plan.py is the same arithmetic in numpy. */
enum { PM_TF_S = 0, PM_TF_P = 1, PM_TF_BOTH = 2 };
enum { PM_TF_T_STACK = 0, PM_TF_T_THINFILM = 1 };

/* The characteristic-matrix sweep (x/coatings/stack.py:102-129, 174-203 and thinfilm.py:213-316): v = [1, eta_sub], v <- M_j v for
 * j = L - 1 .. 0 with cos(theta_j) by _cos_snell (thinfilm.py:75-80), then r = (eta0 B - C) / (eta0 B + C), t = 2 eta0 / (eta0 B + C)
 * from [B, C] = v.  pol selects s, p or both; with PM_TF_BOTH one sweep carries both vectors and every output has a leading axis of 2
 * (s, then p).  r, t: K complex values per polarisation, required.  Optional outputs, NULL when not wanted: R = |r|^2 and
 * T = Re eta_sub / Re eta0 |t|^2 (K reals; stack.py:304-334), the tangential fields E, H at the L + 1 boundaries ((L + 1) x K complex,
 * boundary-major, together or not at all; stack.py:229-249) and the per-layer absorptance A (L x K reals).  t_convention
 * PM_TF_T_THINFILM stores multilayer_stack_rt's t, which for p is t cos(theta_0) / cos(theta_sub) (from A00, thinfilm.py:297-311);
 * T, E, H and A are always the stack's.  One launch.  K = 0 returns 0 without a launch; L = 0 is the bare interface. */
int pm_tf_stack(int32_t dtype, int32_t pol, int32_t t_convention, int64_t K, int64_t L, const void* wvl, int64_t wvl_ss, const void* theta,
                int64_t theta_ss, const void* n, int64_t n_ls, int64_t n_ss, const void* d, int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss,
                const void* n0, int64_t n0_ss, void* r, void* t, void* R, void* T, void* E, void* H, void* A, void* stream);

/* thickness_gradient (x/coatings/diff.py:162-201, 233-308) for R / T seeds: grad[j] = sum_k dF/dd_j, L reals, from dR and dT (K reals
 * per polarisation, either may be NULL; with PM_TF_BOTH the seeds of p start seed_pstride elements after those of s, 0 = the same
 * seeds).  The cotangent of M_j is a_j b_{j+1}^H -- b the unnormalised boundary vectors of the sweep from the substrate (kept in the
 * workspace), a_0 = [Bbar, Cbar]^T, a_{j+1} = M_j^H a_j -- so no prefix or suffix product is stored and no matrix inverted.  The sum
 * over samples is in double: one partial per wavefront and layer, then one workgroup per layer adds them in a fixed order (no atomics,
 * the same bits run after run).  accumulate != 0 adds to grad.  Two launches.  K = 0 or L = 0 returns 0 without a launch.  workspace:
 * pm_tf_thickness_grad_workspace bytes (0 for a dtype or pol it does not know), DEVICE, 16-byte aligned. */
size_t pm_tf_thickness_grad_workspace(int32_t dtype, int32_t pol, int64_t K, int64_t L);
int pm_tf_thickness_grad(int32_t dtype, int32_t pol, int64_t K, int64_t L, const void* wvl, int64_t wvl_ss, const void* theta, int64_t theta_ss,
                         const void* n, int64_t n_ls, int64_t n_ss, const void* d, int64_t d_ls, int64_t d_ss, const void* nsub, int64_t nsub_ss,
                         const void* n0, int64_t n0_ss, const void* dR, const void* dT, int64_t seed_pstride, int32_t accumulate, void* grad,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Sequential ray trace (csrc/raytrace.hip): prysm/x/raytracing -- spencer_and_murty.raytrace (spencer_and_murty.py:500-622) around
 * Surface.interact (surfaces.py:1407-1482), with ray_plane_intersect and ray_conic_intersect (intersections.py:21-134),
 * ConicSeedMixin.intersect, _domain_corridor and _lipschitz_march_solve_s (intersections.py:169-477), newton_raphson_solve_s, refract
 * and reflect (spencer_and_murty.py:207-306, 424-479) and the conic and even-asphere sags and normals (sags.py:109-121, 413-483).  One
 * thread per ray walks the J surfaces with the ray in registers.  dtype PM_F32 or PM_F64 is the type of P, S and of the outputs and the
 * type the kernel computes in.  `table`: DEVICE, J records of PM_RT_RECORD doubles, 8-byte aligned, packed by
 * prysm_amd/x/raytrace_plan.py (pack_table; the layout is the enum at the top of csrc/raytrace.hip): interaction, shape and its
 * parameters (c, k, dx, dy, up to 8 even-asphere coefficients), vertex and rotation, the index after the surface, the aperture, the
 * conic-seed departure band, the first-surface and analytic flags.  n_launch is the index the rays start in; tol_sag the convergence
 * tolerance on |Z - sag| (resolve_tol_sag: 1e-12 for double, 100 eps for float).  P, S: DEVICE, N x 3, contiguous.
 * history = 1: P_out, S_out are (J + 1) x N x 3 and OPL_out (J + 1) x N, row 0 the launch (OPL 0), the reference's layout.
 * history = 0 (not in the reference): P_out, S_out N x 3 -- the last row -- and OPL_out N, the segments' lengths added in surface
 * order.  status_surface, status_code: N int32 each, the real and imaginary part of the reference's complex status -- the 1-based
 * surface and PM_RT_* code of a ray's FIRST failure, or J and PM_RT_OK; from the failing surface on the ray's P, S and OPL are NaN.
 * One launch.  N = 0 or J = 0 returns 0 without a launch (for J = 0 the caller fills row 0 and the status).
 * prysm_amd/x/raytrace_plan.py is the same arithmetic in numpy. */
enum { PM_RT_REFLECT = 0, PM_RT_REFRACT = 1, PM_RT_MEASURE = 2 };
enum { PM_RT_PLANE = 0, PM_RT_CONIC = 1, PM_RT_ASPHERE = 2 };
enum { PM_RT_OK = 0, PM_RT_NEWTON = 1, PM_RT_CLIP = 2, PM_RT_MISS = -1, PM_RT_TIR = -2 };
enum { PM_RT_RECORD = 48, PM_RT_MAX_SURFACES = 4096, PM_RT_MAX_COEFS = 8 };
int pm_rt_trace(int32_t dtype, int64_t N, int64_t J, const void* table, double n_launch, double tol_sag, int32_t history, const void* P,
                const void* S, void* P_out, void* S_out, void* OPL_out, void* status_surface, void* status_code, void* stream);

/* Step-index fibre LP modes without a stored basis (csrc/fibers.hip; prysm/x/fibers.py).  Points are npts contiguous REAL polar
 * coordinates r, t (dtype PM_F32 / PM_F64, computed in that precision); a is the core radius.  `table` is a DEVICE array of nrec records
 * built by prysm_amd/x/fibers_plan.py mode_table (struct pm::FRec: T U, W, invJ, invK; int32 l, slot_cos, slot_sin, flags -- 32 bytes
 * for PM_F32, 48 for PM_F64), one per radial function (|l|, m), sorted by |l|: U = V sqrt(1 - b), W = V sqrt(b), the normalisers
 * 1 / J_l(U) and 1 / (e^W K_l(W)) evaluated on the host AT the U, W the record holds, and the output slots in [0, nmodes) of the
 * cosine (+l, or l = 0) and sine (-l) mode (-1: not wanted).  The radial value is J_l(U r/a) / J_l(U) for r <= a, else
 * K_l(W r/a) / K_l(W) (compute_LP_modes, fibers.py:343-421); flags = 1 takes r (1/a) < 1 as the core (smf_mode_field, fibers.py:424-459,
 * whose J1 / K1 normalisers the record then holds).  J_l and K_l are the unit's own (the device library has no K_n and no J_n usable
 * below x = n).  prysm_amd/x/fibers_plan.py is the same arithmetic in numpy. */

/* out (nmodes, npts): every mode of the table, one launch -- compute_LP_modes (fibers.py:343-421) and smf_mode_field. */
int pm_fiber_modes(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                   void* out, void* stream);

/* out[b][p] (+)= sum_k coefs[b][k] mode_k[p] for batch coefficient vectors (coefs: DEVICE, batch x nmodes, read at launch time, so a
 * captured graph uses their current values), the modes evaluated once per point for every 8 vectors and never stored: the field at a
 * multimode fibre's exit face.  Complex coefficients are two real vectors (re, im) and come out as two planes.  Not in the reference
 * (it sums a stored compute_LP_modes dictionary). */
int pm_fiber_sum(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                 int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream);

/* out[b][k] = sum_p g[b][p] mode_k[p] for batch real vectors g (a complex incident field is Re E, Im E): the sums multimode_coupling
 * (fibers.py:551-588) forms from its stored modes, one per mode_overlap_integral call.  g = NULL (batch 1): sum_p mode_k[p]^2, the
 * other factor of its denominators.  Deterministic: one partial per (workgroup, output) in the workspace, summed in a fixed order by
 * a second launch; no atomics.  More modes than a workgroup has accumulators for (2048 in PM_F64) is PM_ERR_UNSUPPORTED. */
size_t pm_fiber_project_workspace(int32_t dtype, int64_t npts, int64_t nmodes, int64_t batch);
int pm_fiber_project(int32_t dtype, int64_t npts, const void* r, const void* t, double a, const void* table, int64_t nrec, int64_t nmodes,
                     int64_t batch, const void* g, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* mode_overlap_integral (fibers.py:505-548) in one pass over both fields: out (DEVICE, 5 reals of dtype PM_F32 / PM_F64) =
 * Re S, Im S, I1, I2, eta with S = sum E1 conj(E2), I1 = sum |E1|^2, I2 = sum |E2|^2, eta = |S|^2 / (I1 I2).  e1_complex / e2_complex:
 * the field is npts interleaved (re, im) pairs, aligned to the pair; else npts reals.  Nothing is read back, so the call can be
 * captured.  Deterministic as above (workspace: pm_overlap_workspace). */
size_t pm_overlap_workspace(int32_t dtype, int64_t npts);
int pm_overlap(int32_t dtype, int64_t npts, const void* e1, int32_t e1_complex, const void* e2, int32_t e2_complex, void* out,
               void* workspace, size_t workspace_bytes, void* stream);

/* The image chain (csrc/imagechain.hip): prysm/objects.py, prysm/degradations.py, prysm/psf.py and uniform_cart_to_polar of
 * prysm/coordinates.py.  REAL working precision, PM_F32 or PM_F64; every array is on the DEVICE, the small records are HOST structs read
 * at call time.  The unit is compiled without multiply-add contraction; prysm_amd/imagechain_plan.py is the same arithmetic in numpy. */
enum { PM_OBJECT_SLIT = 0, PM_OBJECT_PINHOLE = 1, PM_OBJECT_SIEMENSSTAR = 2, PM_OBJECT_TILTEDSQUARE = 3, PM_OBJECT_SLANTEDEDGE = 4 };
enum { PM_OBJECT_SLIT_X = 1, PM_OBJECT_SLIT_Y = 2, PM_OBJECT_BINARY = 4, PM_OBJECT_CROSSED = 8 };
/* kind, flags and parameters p (doubles, rounded once to the working precision):
 *   SLIT          flags SLIT_X / SLIT_Y: which slits; p = half width in x, in y.                          out: mask (1 byte per sample)
 *   PINHOLE       p = radius.                                                                             out: mask
 *   SIEMENSSTAR   flags BINARY; p = spokes / 2, contrast, outer radius, inner radius, background value (0 or 1), bottom, top
 *   TILTEDSQUARE  p = cos(angle), sin(angle), radius, value inside, value outside
 *   SLANTEDEDGE   flags CROSSED (square grids only); p = cos(angle), sin(angle), value where xp > 0, value elsewhere */
typedef struct pm_object {
    int32_t kind, flags;
    double p[8];
} pm_object;

/* slit, pinhole, siemensstar, tiltedsquare, slantededge (objects.py:8-37, 91-107, 130-181, 184-224, 227-258): out (ny x nx, rows out_ld
 * apart; uint8 0 / 1 for the masks, dtype otherwise), one launch, each sample stored once.  coords as pm_sdf_render: PM_COORDS_GRID
 * (a, b unused; x = (col - nx / 2) dx, y = (row - ny / 2) dx, make_xy_grid's elements), PM_COORDS_SEPARABLE (a = x, nx values; b = y, ny
 * values ldb elements apart) or PM_COORDS_POINTWISE (a, b: ny x nx arrays, rows lda / ldb apart).  polar != 0 (POINTWISE, pinhole and
 * Siemens star): a, b hold (r, t) as the reference takes them (b may be NULL for the pinhole); otherwise those two targets form
 * r = hypot(x, y), t = atan2(y, x) in registers.  The crossed edge evaluates the edge at (i, j), (j, N-1-i), (N-1-i, N-1-j), (N-1-j, i). */
int pm_object_render(int32_t dtype, int32_t coords, int32_t polar, int64_t ny, int64_t nx, const void* a, int64_t lda, const void* b,
                     int64_t ldb, double dx, const pm_object* obj, void* out, int64_t out_ld, void* stream);

/* Analytic transfer functions and their product.  A record is one factor:
 *   SINC_X / SINC_Y   sinc(f p0)                     pixel_ft (detector.py:174-194), smear_ft (degradations.py:7-39)
 *   COS_X / COS_Y     cos(p0 f)                      olpf_ft (detector.py:151-171), p0 = 2 width
 *   GAUSS_R           exp(-2 (p0 fr)^2)              jitter_ft (degradations.py:42-59), p0 = pi scale
 *   JINC_R            jinc(fr p0)                    pinhole_ft (objects.py:110-127), p0 = 2 pi radius
 *   AIRY_FT_R         2/pi (acos s - s sqrt(1 - s^2)), s = min(|fr| / p0, 1)      airydisk_ft (psf.py:268-292), p0 = 1 / (wavelength fno)
 *   AIRY_R / AIRY_EFIELD_R   |2 jinc(u)|^2 / 2 jinc(u), u = r pi / p0 / p1        airydisk, airydisk_efield (psf.py:240-265), p = wavelength, fno
 *   SLIT_FT           slit_ft (objects.py:40-88): flags PM_OBJECT_SLIT_X / _Y, p = width_x, width_y; with both, the grid lengths are
 *                     1 / (f[1] - f[0]) of each axis and the bands test the other frequency == 0 exactly
 *   MAP_REAL / MAP_COMPLEX   a user array (ptr, rows ld apart; dtype, or interleaved pairs of it) multiplied in
 * jinc = J1(x) / x from the Chebyshev tables of csrc/fibers_coefs.h (mathops.py:232-259 divides scipy's j1). */
enum { PM_TFP_SINC_X = 0, PM_TFP_SINC_Y = 1, PM_TFP_COS_X = 2, PM_TFP_COS_Y = 3, PM_TFP_GAUSS_R = 4, PM_TFP_JINC_R = 5, PM_TFP_AIRY_FT_R = 6,
       PM_TFP_SLIT_FT = 7, PM_TFP_MAP_REAL = 8, PM_TFP_MAP_COMPLEX = 9, PM_TFP_AIRY_R = 10, PM_TFP_AIRY_EFIELD_R = 11 };
enum { PM_FREQ_GRID = 0, PM_FREQ_VECTORS = 1, PM_FREQ_POINTWISE = 2 };
enum { PM_TF_MAX_RECORDS = 16 };
typedef struct pm_tf_record {
    int32_t kind, flags;
    int64_t ld;
    const void* ptr;
    double p[4];
} pm_tf_record;
/* Where the frequencies of sample (row, col) come from.  GRID: the bin's integer times 1 / (n dx) in double, rounded once to dtype --
 * fttools.forward_ft_unit(dx, n, shift) (fttools.py:128-152), even and odd n.  VECTORS: fx (n values), fy (m values, ldy elements
 * apart).  POINTWISE: m x n arrays fx, fy and / or fr (rows ldx, ldy, ldr apart; fr = hypot(fx, fy) where fr is NULL).
 * shift != 0: the inputs (frequencies and maps) have their origin at the centre, [m / 2, n / 2]; the output never has. */
typedef struct pm_tf_freq {
    int32_t mode, shift;
    double dx;
    const void* fx;
    const void* fy;
    const void* fr;
    int64_t ldx, ldy, ldr;
} pm_tf_freq;

/* out (m x n, rows out_ld apart; complex pairs when out_complex, else dtype) = the product of the records, in their order, with its
 * origin at [0, 0]: out[i, j] = product at input index ((i + m / 2) mod m, (j + n / 2) mod n) when freq->shift, an index rotation
 * in the kernel.  One launch, each sample stored once: what convolution.apply_transfer_functions (convolution.py:34-113) forms map by map. */
int pm_tf_product(int32_t dtype, int64_t m, int64_t n, const pm_tf_freq* freq, const pm_tf_record* records, int64_t nrec, int32_t out_complex,
                  void* out, int64_t out_ld, void* stream);

/* uniform_cart_to_polar (coordinates.py:269-316): out[i, j] = data interpolated bilinearly at (x, y) = rho[j] (cos phi[i], sin phi[i]),
 * data sampled on the ascending regular axes x (nx values) and y (ny values) whose spacings x_step, y_step seed the cell search; 0
 * outside [min, max] of either axis, the boundary inside (scipy's RegularGridInterpolator, linear, fill_value 0).  One gather launch. */
int pm_polar_resample(int32_t dtype, int64_t ny, int64_t nx, const void* x, const void* y, double x_step, double y_step, const void* rho,
                      const void* phi, const void* data, int64_t data_ld, void* out, int64_t out_ld, void* stream);

/* centroid (psf.py:174-203; scipy's center_of_mass): out (DEVICE, 2 doubles) = sum(row d) / sum(d), sum(col d) / sum(d) over an m x n
 * array, summed in double.  Two launches, one partial triple per workgroup in the workspace folded in a fixed order: no atomics, the
 * same bits every run, nothing read on the host. */
size_t pm_centroid_workspace(int64_t m, int64_t n);
int pm_centroid(int32_t dtype, int64_t m, int64_t n, const void* data, int64_t ld, void* out, void* workspace, size_t workspace_bytes,
                void* stream);

/* estimate_size after its resample (psf.py:63-90): the maximum of the polar map (rows x cols), the threshold hm = value * max in dtype
 * (relative != 0) or value, per row -- one wavefront each -- the first (last = 0) or last index where polar > hm changes and the radius
 * r[i] + frac (r[i+1] - r[i]) there, then out (DEVICE, 2 doubles) = the mean over the rows that cross, and their count.  Four launches
 * (maximum partials, its fold, crossings, mean), deterministic as above.  pm_psf_size_groups: the workgroups of the crossing launch,
 * four rows each per trip. */
size_t pm_psf_size_workspace(int64_t rows);
int64_t pm_psf_size_groups(int64_t rows);
int pm_psf_size(int32_t dtype, int64_t rows, int64_t cols, const void* polar, int64_t ld, const void* r, int32_t relative, double value,
                int32_t last, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* The wavefront sensors (csrc/sensors.hip): prysm/x/psi.py, prysm/x/shack_hartmann.py, prysm/x/pdi.py and prysm/x/sri.py.  Every array
 * is on the DEVICE, the small records are HOST structs read at call time.  No atomics and no reductions: each output sample is a
 * function of its own inputs, so results are the same bits every run.  The unit is compiled without multiply-add contraction;
 * prysm_amd/x/sensors_plan.py is the same arithmetic in numpy. */
enum { PM_PSI_MAX_FRAMES = 32 };
/* K frames of one shape, each with its own base pointer (separately allocated frames are not stacked; a (K, rows, cols) array gives
 * frame[k] = base + k * rows * ld), and the scheme's weights.  The kernel receives the table by value in its arguments. */
typedef struct pm_psi_frames {
    const void* frame[PM_PSI_MAX_FRAMES];
    double s[PM_PSI_MAX_FRAMES];
    double c[PM_PSI_MAX_FRAMES];
} pm_psi_frames;

/* psi_accumulate and degroot_formalism_psi (psi.py:45-71, 74-109; the two sum_of_2d_modes calls of polynomials/fitting.py:7-37 and the
 * arctan2): num = sum_k s[k] g_k, den = sum_k c[k] g_k, phase = atan2(num, den) over rows x cols samples, the frames' rows ld apart and
 * the outputs' rows out_ld apart.  Any of num, den, phase may be NULL, not all three.  1 <= K <= PM_PSI_MAX_FRAMES.  frame_dtype
 * PM_F32, PM_F64, PM_U8 or PM_U16; the sums run in double over k ascending for every frame dtype and are rounded once to out_dtype
 * (PM_F32 / PM_F64; the frames' own dtype for float frames), atan2 is taken of the rounded pair in out_dtype.  One launch, every frame
 * read once: 16-byte loads when every frame lies at the same offset from a 16-byte boundary and ld is a multiple of 16 bytes (a
 * scalar head and tail per row), element loads otherwise; 16-byte stores under the same rule for the outputs. */
int pm_psi(int32_t frame_dtype, int32_t out_dtype, int64_t K, int64_t rows, int64_t cols, const pm_psi_frames* frames, int64_t ld, void* num,
           void* den, void* phase, int64_t out_ld, void* stream);

enum { PM_LENSLET_RECTANGLE = 0, PM_LENSLET_CIRCLE = 1 };
/* nx x ny lenslets `pitch` apart: centre i along x is T(i - nx / 2) * T(pitch) + T(shift_x), each operation rounded in the working
 * precision T (make_xy_grid(n, dx=pitch, grid=False) and the += pitch / 2 of shift=True, shack_hartmann.py:83-89), likewise along y.
 * RECTANGLE: the sample is inside where |x - xc| - half_width <= 0 and |y - yc| - half_height <= 0 (geometry.rectangle at angle 0);
 * CIRCLE: where rsq - half_width <= 0 with half_width the SQUARED radius (geometry.circle called on r = rsq, shack_hartmann.py:112).
 * The aperture must stay within one pitch of its centre.  k = -2 pi / (wavelength / 1e3). */
typedef struct pm_lenslets {
    int32_t kind, nx, ny, reserved;
    double pitch, shift_x, shift_y, half_width, half_height, efl, k;
} pm_lenslets;

/* shack_hartmann (shack_hartmann.py:11-117), the double loop over lenslets as ONE launch: out (ny x nx complex samples of dtype's
 * precision, rows out_ld apart) = exp(i k total), total = the sum over the lenslets whose aperture holds the sample of
 * ((x - xc)^2 + (y - yc)^2) / (2 efl), every operation in T.  The reference's windows never clip an aperture, so this windowless sum
 * over the 3 x 3 lenslets around the nearest centre, added with the rows of lenslets outermost as the reference adds them, is its
 * result; a sample on the shared edge of two lenslets satisfies <= in both and gets both terms, as there.  coords as
 * pm_object_render: PM_COORDS_GRID (x = (col - nx / 2) dx, y = (row - ny / 2) dx), PM_COORDS_SEPARABLE (x: nx values; y: ny values ldy
 * elements apart) or PM_COORDS_POINTWISE (ny x nx arrays, rows ldx / ldy apart). */
int pm_lenslet_screen(int32_t dtype, int32_t coords, int64_t ny, int64_t nx, const void* x, int64_t ldx, const void* y, int64_t ldy, double dx,
                      const pm_lenslets* lens, void* out, int64_t out_ld, void* stream);

enum { PM_GRATING_SIN_AMP = 0, PM_GRATING_PULSE = 1 };
/* The grating of PSPDI (pdi.py:129-149, 215-222) and rectangle_pulse (pdi.py:11-51) in one pass: g at xs = x + shift (shift == 0: x
 * itself), out = field * g (complex, field rows field_ld apart) or, field NULL, out = g (real).  x through coords as above (only the
 * first coordinate is read).  p: 5 HOST doubles rounded once to dtype --
 *   SIN_AMP   g = 1 - ((sin(p0 xs) + 1) / 2) 0.1, p0 = rulings pi / (epd / 2)
 *   PULSE     xw = mod(xs, p0) with numpy's sign rule; g = p2 where xw < p1, else p3; g = p4 where |xw| < eps of dtype
 *             (p0 = period, p1 = duty period, p2 = offset + amplitude, p3 = offset - amplitude, p4 = offset) */
int pm_grating(int32_t dtype, int32_t kind, int32_t coords, int64_t rows, int64_t cols, const void* x, int64_t ldx, double dx, double shift,
               const double* p, const void* field, int64_t field_ld, void* out, int64_t out_ld, void* stream);

/* The beam combination of the interferometers (pdi.py:235-253, sri.py:171-178): t = ca a + cb b for complex a, b (PM_C64 / PM_C128) and
 * real ca, cb; intensity = |t|^2 (real) and / or total = t, each stored once; one of the two may be NULL. */
int pm_beam_combine(int32_t dtype, int64_t rows, int64_t cols, const void* a, int64_t lda, double ca, const void* b, int64_t ldb, double cb,
                    void* intensity, int64_t intensity_ld, void* total, int64_t total_ld, void* stream);

/* The field a single-mode fibre emits (sri.py:62-72): out = efib sqrt(P eta) (cos_phi + i sin_phi), efib real, P (the power at the
 * facet) and eta (the coupling) DEVICE scalars of dtype read by the kernel -- nothing is read on the host. */
int pm_fiber_scale(int32_t dtype, int64_t rows, int64_t cols, const void* efib, int64_t efib_ld, const void* power, const void* eta, double cos_phi,
                   double sin_phi, void* out, int64_t out_ld, void* stream);

/* Segmented apertures (csrc/segmented.hip): CompositeHexagonalAperture.compose_opd (prysm/segmented.py:178-285) and its adjoint.
 * The grid is rows x cols REAL points (dtype PM_F32 / PM_F64, computed in that precision); x, y are the aperture's DEVICE coordinate
 * arrays.  `plan` is a DEVICE array of nseg 80-byte segment records built by prysm_amd/segmented.py (struct pm::SegDesc: int32 y0, x0,
 * h, w -- the segment's window; int32 gy0, gx0 and 2 pad -- the window of its grid source, whose local coordinates it uses; int64 moff
 * -- its mask in `masks`, h x w values; int64 boff -- the (nmodes, h, w) stored basis of its grid source in `basis`; double cx, cy --
 * the grid source's centre; double nr -- the normalisation radius; double pad).  Z_{s,k} comes from `source`: PM_SEGMENT_ZERNIKE walks
 * the Zernike step `table` (as pm_zernike_sum, Cartesian) at ((x - cx) / nr, (y - cy) / nr) of the grid source, at the same position
 * in its window; PM_SEGMENT_STORED reads basis[boff + k h w + position].  Check a plan with pm_segment_plan_check before it is used. */
enum { PM_SEGMENT_ZERNIKE = 0, PM_SEGMENT_STORED = 1 };

/* Host-side check of a HOST copy of `plan`: every window and grid-source window inside the grid, every mask inside mask_elems and,
 * for basis_elems >= 0, every stored basis of nmodes planes inside basis_elems; nr > 0.  0, or PM_ERR_ARG with pm_last_error(). */
int pm_segment_plan_check(int64_t rows, int64_t cols, int64_t nseg, const void* plan, int64_t mask_elems, int64_t nmodes,
                          int64_t basis_elems);

/* out[b][p] (+)= sum over the segments s of p's cover list of mask_s[p] * sum_k coefs[b][s][k] Z_{s,k}[p] -- compose_opd
 * (segmented.py:261-285) with the segments' windows added in segment order.  cover: ncover DEVICE int16 planes of rows x cols, plane
 * i holding the i-th segment (index into plan) whose window covers the point with a non-zero mask, -1 after the last; points of no
 * segment keep out (accumulate != 0) or get 0.  coefs: DEVICE, batch x nseg x nmodes, read at launch time (a captured graph uses their
 * current values).  One launch per group of up to 8 coefficient stacks. */
int pm_segment_compose(int32_t dtype, int32_t source, int64_t rows, int64_t cols, const void* x, const void* y, int64_t nseg, const void* plan,
                       const void* masks, int64_t ncover, const void* cover, const void* table, int64_t nsteps, int64_t nmodes,
                       const void* basis, int64_t batch, const void* coefs, int32_t accumulate, void* out, void* stream);

/* out[b][s][k] = sum over the window of s of mask_s[p] Z_{s,k}[p] databar[b][p] (databar batch x rows x cols, out batch x nseg x
 * nmodes): the adjoint of pm_segment_compose with respect to the coefficients; the reference has none (prepare_opd_bases /
 * compose_opd, segmented.py:178-285).  window_pts: the largest h * w of the plan.  Two launches: one partial per (workgroup, b, s, k)
 * into the workspace, each workgroup on one segment, then a fixed-order sum -- no atomics, bitwise reproducible. */
size_t pm_segment_project_workspace(int32_t dtype, int64_t window_pts, int64_t nseg, int64_t nmodes, int64_t batch);
int pm_segment_project(int32_t dtype, int32_t source, int64_t rows, int64_t cols, const void* x, const void* y, int64_t nseg, const void* plan,
                       const void* masks, int64_t window_pts, const void* table, int64_t nsteps, int64_t nmodes, const void* basis,
                       int64_t batch, const void* databar, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* P = amp * exp(i * k * opd), k = 2 pi / (wavelength_um * 1e3) for opd in nm.
 * amp may be NULL (unit amplitude: phase_screen).  amp_dtype in {PM_F32, PM_F64, PM_BOOL}.
 * Wavefront.from_amp_and_phase / phase_screen (wavefront.py:58-96), phase_prefix (_kernels.py:40-43). */
int pm_pupil_synth(int32_t dtype, int64_t rows, int64_t cols, const void* amp, int32_t amp_dtype, int64_t amp_ld,
                   const void* opd, int64_t opd_ld, double k, void* out, int64_t out_ld, void* stream);

/* out[i][j] = exp(i * c * (x[i][j]^2 + y[i][j]^2)); Wavefront.thin_lens (wavefront.py:98-144), c = -pi/(w f). */
int pm_quadratic_phase(int32_t dtype, int64_t rows, int64_t cols, const void* x, int64_t x_ld, const void* y,
                       int64_t y_ld, double c, void* out, int64_t out_ld, void* stream);

/* Separable Fresnel transfer-function factors: hy[i] = exp(-i pi wvl_mm z ky[i]^2), ky = fftfreq(rows, dx)
 * rounded to the real dtype first (angular_spectrum.py:105-113).  hx likewise.  Vectors of length rows / cols. */
int pm_as_tf_vectors(int32_t dtype, int64_t rows, int64_t cols, double wvl_um, double dx, double z, void* hy,
                     void* hx, void* stream);

/* out = outer(hy, hx) -- materialises the transfer function for API parity (angular_spectrum.py:114). */
int pm_outer(int32_t dtype, int64_t rows, int64_t cols, const void* hy, const void* hx, void* out, int64_t out_ld,
             void* stream);

/* out window copy: out (orows x ocols) = fill everywhere, then in placed at (off_y, off_x); negative offsets
 * crop.  fttools.pad2d constant mode / crop_center (prysm/fttools.py:43-125).  elem_bytes in {1,4,8,16}. */
int pm_embed(int32_t elem_bytes, int64_t irows, int64_t icols, const void* in, int64_t in_ld, int64_t orows,
             int64_t ocols, int64_t off_y, int64_t off_x, const void* fill_elem_host, void* out, int64_t out_ld,
             void* stream);

/* The index-mapping modes of np.pad that fttools.pad2d(mode=...) forwards to (prysm/fttools.py:96-98): out (orows x ocols) holds
 * in at (off_y, off_x) and, around it, in[map(r)][map(c)] with mode 1 = 'edge', 2 = 'reflect', 3 = 'symmetric', 4 = 'wrap'
 * (any pad width, also wider than the array).  elem_bytes in {1, 4, 8, 16}.  The statistical modes ('mean', 'maximum', 'minimum',
 * 'median') and 'linear_ramp' are not entry points: the mirror package composes them from device tensor reductions (off the hot path). */
int pm_pad_index(int32_t elem_bytes, int32_t mode, int64_t irows, int64_t icols, const void* in, int64_t in_ld, int64_t orows,
                 int64_t ocols, int64_t off_y, int64_t off_x, void* out, int64_t out_ld, void* stream);

/* The chirps of one chirp-Z axis from its scalars, one launch (prysm/fttools.py:364-389 _prepare_czt_basis: arange / exp / zero-pad
 * as a dozen array operations per axis -- the polychromatic recipe builds one executor per wavelength): with e(t) = exp(2 pi i t),
 *   b[j] = e(half n^2), n = j - N/2 (j < N);   a[i] = e(half q^2), q = i - M/2 + shift (i < M);
 *   h[t] = e(-half (d + shift)^2), d = t - M/2 - (N - 1 - N/2) for t < N + M - 1, zero up to K  (its transform is the H of pm_czt_axis);
 * half = sign dx dfx / 2, shift = f[M/2] / dfx. */
int pm_czt_vectors(int32_t dtype, int64_t N, int64_t M, int64_t K, double shift, double half, void* b, void* a, void* h,
                   void* stream);

/* --- matrix DFT --------------------------------------------------------------------------- */

/* E[m][n] = exp(sign * 2 pi i * f[m] * x[n]) (M x N), phases reduced in fp64, rounded once.
 * f and x are real device vectors of the complex dtype's real type.  fttools.MDFT.__init__
 * (prysm/fttools.py:187-191). */
int pm_mdft_basis(int32_t dtype, int64_t M, int64_t N, const void* f, const void* x, int32_t sign, void* E,
                  int64_t E_ld, void* stream);

/* The same basis for the FFT-centred grids of dft.coordinates_for_focus (prysm/propagation/dft.py:58-65), generated inside the
 * kernel instead of read from vectors -- prepare_executor then costs two launches, not a dozen small array operations:
 *     x[n] = (n - N/2) * x_step                      (fftrange(N) * pupil_dx)
 *     f[m] = ((m - M/2) * f_step + f_shift) * f_scale   ((fftrange(M) * focal_dx + focal_shift) / (wavelength * efl))
 * every operation rounded once in the real type of dtype, i.e. bit for bit the vectors numpy builds at config.precision. */
int pm_mdft_basis_grid(int32_t dtype, int64_t M, int64_t N, double f_step, double f_shift, double f_scale, double x_step,
                       int32_t sign, void* E, int64_t E_ld, void* stream);

/* C (M x N) = alpha * opA(A) (M x K) @ opB(B) (K x N), complex, on the MFMA matrix cores.
 *   opA: 0 = A, 1 = conj(A), 2 = A^T, 3 = A^H     (A stored M x K for 0/1, K x M for 2/3)
 *   opB: likewise                                   (B stored K x N for 0/1, N x K for 2/3)
 * The two GEMMs of fttools.MDFT.__call__ / .adjoint (prysm/fttools.py:201-228).
 * Leading dimensions must be below 2^22 elements (PM_ERR_UNSUPPORTED otherwise) and, for an operand or a result of more than one
 * stored row, not below the stored row (PM_ERR_ARG; pm_cgemm_abs2 likewise, after its PM_ERR_UNSUPPORTED). */
int pm_cgemm(int32_t dtype, int32_t opA, int32_t opB, int64_t M, int64_t N, int64_t K, double alpha,
             const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, void* workspace,
             size_t workspace_bytes, void* stream);
/* bytes of split-K workspace pm_cgemm wants for this shape (0 = none; without it the GEMM runs unsplit) */
size_t pm_cgemm_workspace(int32_t dtype, int64_t M, int64_t N, int64_t K);

/* R = (accumulate ? R : 0) + weight * |alpha * opA(A) @ opB(B)|^2, R REAL (float for PM_C64): the second product of a matrix-DFT
 * focus with Wavefront.intensity (prysm/propagation/wavefront.py:146-151) and the weighted sum of the polychromatic recipe
 * (polynomials.sum_of_2d_modes, prysm/polynomials/fitting.py:7-37) in its epilogue -- the complex focal field is never written.
 * Same workspace as pm_cgemm.  Only the shapes the LDS-DMA kernel takes (PM_C64, M and N multiples of 64, K of 16, 16-byte aligned
 * operands, even leading dimensions); PM_ERR_UNSUPPORTED otherwise: compose pm_cgemm and pm_abs2. */
int pm_cgemm_abs2(int32_t dtype, int32_t opA, int32_t opB, int64_t M, int64_t N, int64_t K, double alpha, const void* A,
                  int64_t lda, const void* B, int64_t ldb, void* R, int64_t ldr, double weight, int32_t accumulate, void* workspace,
                  size_t workspace_bytes, void* stream);

/* --- interferogram: measured maps with invalid pixels (csrc/interferogram.hip) ------------- */

/* A map is a rows x cols window of a real array, rows `ld` elements apart; NaN marks an invalid pixel and +-inf is left out of every
 * sum, as np.isfinite does in the reference.  Sums are accumulated in double in two stages without atomics: a call repeated on the
 * same data leaves the same bits.
 *
 * The statistics record: PM_IFG_RECORD DEVICE doubles. */
enum {
    PM_IFG_N = 0,      /* finite values */
    PM_IFG_NNAN = 1,   /* NaN values (inf is in neither count) */
    PM_IFG_SUM = 2,
    PM_IFG_SUMSQ = 3,
    PM_IFG_MIN = 4,    /* of the finite values; NaN when there is none */
    PM_IFG_MAX = 5,
    PM_IFG_ROW0 = 6,   /* bounding box of the finite values, inclusive; -1 when there is none */
    PM_IFG_ROW1 = 7,
    PM_IFG_COL0 = 8,
    PM_IFG_COL1 = 9,
    PM_IFG_MEAN = 10,  /* SUM / N */
    PM_IFG_SAD = 11,   /* sum |z - MEAN| */
    PM_IFG_M2 = 12,    /* sum (z - MEAN)^2 */
    PM_IFG_STD = 13,   /* sqrt(M2 / N) */
    PM_IFG_RMS = 14,   /* sqrt(SUMSQ / N) */
    PM_IFG_SA = 15,    /* SAD / N */
    PM_IFG_RECORD = 16
};
/* the basis of the low-order fit, as a set of bits */
enum { PM_IFG_TERM_PISTON = 1, PM_IFG_TERM_X = 2, PM_IFG_TERM_Y = 4, PM_IFG_TERM_R2 = 8 };
enum { PM_IFG_FILL = 0, PM_IFG_MASK = 1, PM_IFG_CLIP = 2 };
enum { PM_IFG_WIN_WELCH = 0, PM_IFG_WIN_HANN = 1, PM_IFG_WIN_ARRAY = 2 };
enum { PM_IFG_LP = 0, PM_IFG_HP = 1, PM_IFG_BP = 2, PM_IFG_BR = 3 };
enum { PM_IFG_PSD_ABC = 0, PM_IFG_PSD_AB = 1 };
enum { PM_IFG_IIR_HANN = 1, PM_IFG_IIR_LPF = 2 };

/* x and y of pixel (r, c), used as doubles.  PM_COORDS_GRID generates them: x = T(c - ox) * T(dx), y = T(r - oy) * T(dy) in the data's
 * type T (make_xy_grid's elements; prysm/coordinates.py:344-378), or with linspace != 0 x = x0 + c dx, y = y0 + r dy in double
 * (np.linspace; x, y not read).  PM_COORDS_SEPARABLE reads x[c] and y[r * ldy]; PM_COORDS_POINTWISE reads x[r * ldx + c] and
 * y[r * ldy + c]; both of the data's type. */
typedef struct pm_ifg_coords {
    int32_t mode, linspace;
    const void* x;
    const void* y;
    int64_t ldx, ldy;
    int64_t ox, oy;
    double dx, dy, x0, y0;
} pm_ifg_coords;

/* mean, pv, rms, Sa, std of prysm/util.py:7-97 (each an isfinite selection, then one or two numpy reductions), the NaN count of
 * Interferogram.dropout_percentage (prysm/interferogram.py:708-711) and the bounding box Interferogram.crop looks for
 * (interferogram.py:815-822), in one record.  Four launches: the first pair leaves N .. MEAN, the second reads MEAN from the device and
 * leaves SAD .. SA -- a two-pass variance.  A map without a finite value gives counts, NaN statistics and a box of -1; no error.
 * workspace: pm_ifg_stats_workspace() bytes. */
size_t pm_ifg_stats_workspace(int64_t rows, int64_t cols);
int pm_ifg_stats(int32_t dtype, int64_t rows, int64_t cols, const void* data, int64_t ld, void* record, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Least-squares fit of the terms in `terms` over the finite pixels by the normal equations: polynomials.lstsq([x, y], z) of fit_plane
 * (prysm/interferogram.py:35-55, prysm/polynomials/fitting.py:103-126), the np.linalg.lstsq of fit_sphere (interferogram.py:58-82)
 * and the mean of remove_piston (interferogram.py:862-865).  coef: four DEVICE doubles in the order piston, x, y, x^2 + y^2; a term
 * that is not fitted, or whose pivot falls below eps (largest pivot), gets 0.  Two launches, nothing is read back.
 * workspace: pm_ifg_fit_workspace() bytes. */
size_t pm_ifg_fit_workspace(int64_t rows, int64_t cols);
int pm_ifg_fit(int32_t dtype, int32_t terms, int64_t rows, int64_t cols, const void* data, int64_t ld, const pm_ifg_coords* coords,
               void* coef, void* workspace, size_t workspace_bytes, void* stream);

/* data -= sum of the terms in `terms` with the coefficients at coef (four DEVICE doubles, as pm_ifg_fit leaves them), on the finite
 * pixels, in place; the sum is formed in double and the result rounded once (interferogram.py:862-877 remove_piston, remove_tiptilt,
 * remove_power).  One launch. */
int pm_ifg_remove(int32_t dtype, int32_t terms, int64_t rows, int64_t cols, void* data, int64_t ld, const pm_ifg_coords* coords,
                  const void* coef, void* stream);

/* In place.  PM_IFG_FILL: NaN becomes `value` (interferogram.py:797-813 fill; inf stays).  PM_IFG_MASK: NaN where the byte mask (rows
 * mask_ld apart) is 0 (interferogram.py:879-894 mask).  PM_IFG_CLIP: NaN where |z| > value * record[PM_IFG_STD], the record read on
 * the device (interferogram.py:965-981 spike_clip: |z|, not |z - mean|).  One launch. */
int pm_ifg_edit(int32_t dtype, int32_t op, int64_t rows, int64_t cols, void* data, int64_t ld, double value, const void* mask,
                int64_t mask_ld, const void* record, void* stream);

/* np.gradient(data, dx) with its default edges and the hypot of the two (interferogram.py:1067-1075 slope): gx along the columns, gy
 * along the rows, gr = hypot(gx, gy); central differences over T(2 dx) inside, one-sided ones over T(dx) on the border; NaN spreads as
 * in numpy.  Any of gx, gy, gr may be NULL; the outputs' rows are out_ld apart.  At least 2 samples per axis.  One launch. */
int pm_ifg_slope(int32_t dtype, int64_t rows, int64_t cols, const void* data, int64_t ld, double dx, void* gx, void* gy, void* gr,
                 int64_t out_ld, void* stream);

/* out = height x window, or the window itself when height is NULL, and s2[0] = sum window^2 (a DEVICE double) from the same pass:
 * make_window and the first two lines of psd (prysm/interferogram.py:85-145, 175-180).  PM_IFG_WIN_WELCH: 1 - |r / rmax|^alpha with r
 * the radius of make_xy_grid(shape, dx) in the data's type and rmax its sample at (rows - 1, cols / 2) (window_2d_welch,
 * interferogram.py:268-286, _rmax_square_array :26-32); PM_IFG_WIN_HANN: np.hanning(rows) (x) np.hanning(cols);
 * PM_IFG_WIN_ARRAY: the caller's window (rows window_ld apart).  The window is formed in double and the product rounded once.  Two
 * launches.  workspace: pm_ifg_window_workspace() bytes. */
size_t pm_ifg_window_workspace(int64_t rows, int64_t cols);
int pm_ifg_window(int32_t dtype, int32_t kind, int64_t rows, int64_t cols, const void* height, int64_t ld, double dx, double alpha,
                  const void* window, int64_t window_ld, void* out, int64_t out_ld, void* s2, void* workspace, size_t workspace_bytes,
                  void* stream);
/* data /= s2[0] * fs * fs in place, s2 a DEVICE double (interferogram.py:179-182).  One launch. */
int pm_ifg_psd_scale(int32_t dtype, int64_t rows, int64_t cols, void* data, int64_t ld, const void* s2, double fs, void* stream);

/* The integral behind bandlimited_rms (interferogram.py:190-265): out[0] = spacing^2 sum w_r w_c psd[r, c] over flow <= nu <= fhigh,
 * w the trapezoid rule's weights (half on the first and last row and column), out[1] = spacing; the caller takes the square root.
 * coords PM_COORDS_GRID: nu = hypot((c - cols / 2) / (cols dx), (r - rows / 2) / (rows dx)) in double, the radius of psd()'s axes
 * (fttools.forward_ft_unit, prysm/fttools.py:128-152), spacing 1 / (rows dx); PM_COORDS_POINTWISE: nu read (rows nu_ld apart),
 * spacing |nu[rows / 2 - 1][cols / 2] - nu[rows / 2][cols / 2]| read on the device -- two samples along axis 0, used for both axes.
 * ndim = 1: a 1-D spectrum passed as rows x 1, no column weights, one power of the spacing.  out: two DEVICE doubles.  Two launches.
 * workspace: pm_ifg_band_workspace() bytes. */
size_t pm_ifg_band_workspace(int64_t rows, int64_t cols);
int pm_ifg_band(int32_t dtype, int32_t coords, int32_t ndim, int64_t rows, int64_t cols, const void* psd, int64_t ld, const void* nu,
                int64_t nu_ld, double dx, double flow, double fhigh, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* parts = PM_IFG_IIR_HANN | PM_IFG_IIR_LPF: h' = hann2d(rows, cols) x ideal_lpf_iir2d(r, dx, fcn) (interferogram.py:547-565) for
 * fcn_low into h_low and, when h_high is not NULL, for fcn_high into h_high: the windowed impulse responses designfilt2d transforms
 * (interferogram.py:568-632).  PM_IFG_IIR_HANN alone: hann2d into h_low; PM_IFG_IIR_LPF alone: the impulse responses without the
 * window.  r: generated (PM_COORDS_GRID: hypot(T(c - ox) T(r_dx), T(r - oy) T(r_dx))) or read (PM_COORDS_POINTWISE, rows r_ld
 * apart); the jinc is the Chebyshev series of csrc/fibers_coefs.h in double, the product is rounded once.  One launch. */
int pm_ifg_iir(int32_t dtype, int32_t parts, int32_t coords, int64_t rows, int64_t cols, const void* r, int64_t r_ld, int64_t oy,
               int64_t ox, double r_dx, double dx, double fcn_low, double fcn_high, void* h_low, void* h_high, int64_t out_ld,
               void* stream);
/* the transfer function of a filter type from |fft2(h')| (interferogram.py:594-630): PM_IFG_LP Hl, PM_IFG_HP 1 - Hl,
 * PM_IFG_BP 1 - ((1 - Hh) + Hl), PM_IFG_BR (1 - Hh) + Hl; real, or with complex_out complex with a zero imaginary part, the
 * multiplier of pm_fft2_mul_ifft2.  One launch. */
int pm_ifg_combine(int32_t dtype, int32_t typ, int32_t complex_out, int64_t rows, int64_t cols, const void* h_low, int64_t low_ld,
                   const void* h_high, int64_t high_ld, void* out, int64_t out_ld, void* stream);

/* PM_IFG_PSD_ABC: a / (1 + (nu / b)^c); PM_IFG_PSD_AB: a nu^(-b) (interferogram.py:289-330), n values.  One launch. */
int pm_ifg_psd_model(int32_t dtype, int32_t kind, int64_t n, const void* nu, double a, double b, double c, void* out, void* stream);

/* --- surfaces synthesised from a PSD (csrc/psdsynth.hip) ------------------------------------ */
/* The pointwise passes of synthesize_surface_from_psd and render_synthetic_surface (prysm/interferogram.py:333-432) around the two
 * transforms of pm_fft2, on a stack of `batch` (<= 65535) surfaces of rows x cols samples of the real type `dtype` (PM_F32 / PM_F64;
 * spectra and fields are complex of the same precision), rows `ld` and members `bstride` elements apart.  prysm_amd/psdsynth_plan.py
 * is the same arithmetic in numpy. */
enum { PM_PSD_MASK_NONE = 0, PM_PSD_MASK_ARRAY = 1, PM_PSD_MASK_CIRCLE = 2 };

/* a PSD evaluated inside pm_psd_signal: kind PM_IFG_PSD_ABC a / (1 + (nu / b)^c) or PM_IFG_PSD_AB a nu^(-b) at nu = the root sum of
 * squares of element (row, col) of forward_ft_unit(dxg, rows) and forward_ft_unit(dxg, cols), each with its centre sample n / 2
 * replaced by a tenth of the next one (interferogram.py:404-412), in double, rounded once to the data's type */
typedef struct pm_psd_model {
    int32_t kind, reserved;
    double a, b, c, dxg;
} pm_psd_model;

/* np.random.rand (interferogram.py:347) on the device: uniform numbers in [0, 1) from Philox4x32-10 with key = seed and counter =
 * (pixel low word, pixel high word, surface0 + member, 0), pixel = row * cols + col.  PM_F32: (word 0 >> 8) 2^-24; PM_F64:
 * ((word 0 >> 5) 2^26 + (word 1 >> 6)) 2^-53; every step exact.  One launch. */
int pm_psd_uniform(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, int64_t seed, int64_t surface0, void* out, int64_t ld,
                   int64_t bstride, void* stream);
/* exp(i angle(X)) sqrt(A psd) (interferogram.py:349, 363) in place on the complex spectrum X: (X / |X|, or 1 where X == 0) times
 * sqrt(area psd) in the data's type; a negative psd gives NaN.  Exactly one of `psd` (a real rows x cols array shared by the stack,
 * rows psd_ld apart) and `model` is given.  One launch. */
int pm_psd_signal(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, void* spectrum, int64_t ld, int64_t bstride, const void* psd,
                  int64_t psd_ld, const pm_psd_model* model, double area, void* stream);
/* out = real(field) (interferogram.py:367), NaN where the mask fails (interferogram.py:418-424): PM_PSD_MASK_ARRAY a rows x cols array
 * of bytes shared by the stack (0: outside), PM_PSD_MASK_CIRCLE hypot(x, y) <= radius on make_xy_grid's x = T(col - cols / 2) T(step),
 * y = T(row - rows / 2) T(step); and sums[2 b], sums[2 b + 1] = the count and the sum of squares of the finite pixels of member b,
 * as doubles, the same bits every run.  Two launches. */
size_t pm_psd_finish_workspace(int64_t batch, int64_t rows, int64_t cols);
int pm_psd_finish(int32_t dtype, int32_t mask_kind, int64_t batch, int64_t rows, int64_t cols, const void* field, int64_t ld, int64_t bstride,
                  const void* mask, int64_t mask_ld, double radius, double step, void* out, int64_t out_ld, int64_t out_bstride, void* sums,
                  void* workspace, size_t workspace_bytes, void* stream);
/* z *= rms / sqrt(sum / count) (interferogram.py:427-430) with the sums of pm_psd_finish read on the device; a member with count 0 or
 * sum 0 is left as it is.  One launch. */
int pm_psd_scale(int32_t dtype, int64_t batch, int64_t rows, int64_t cols, void* z, int64_t ld, int64_t bstride, const void* sums, double rms,
                 void* stream);

/* --- Jones and Mueller calculus (csrc/jones.hip) -------------------------------------------- */
/* prysm/x/polarization.py:45-475 and 555-578 per pixel of a rows x cols grid, `dtype` PM_C64 or PM_C128, arithmetic in its real type.
 * A Jones field has four complex components per pixel in the order (0,0), (0,1), (1,0), (1,1), a Jones vector two, (0,0), (1,0).
 * PM_JONES_AOS: the reference's (..., 2, 2) / (..., 2, 1), pixel (r, c) at (r ld + c) ncomp elements.  PM_JONES_PLANES: (ncomp, rows,
 * cols), component k of pixel (r, c) at k pstride + r ld + c elements (pstride >= rows ld; ignored for aos).  ld counts pixels and is
 * at least cols.  Every entry point is one launch, reads each input once and stores each output once; an empty shape returns 0.
 * prysm_amd/x/polarization_plan.py is the same arithmetic in numpy. */
enum { PM_JONES_AOS = 0, PM_JONES_PLANES = 1 };
enum { PM_JONES_ROTATION = 0, PM_JONES_RETARDER = 1, PM_JONES_DIATTENUATOR = 2, PM_JONES_VORTEX = 3, PM_JONES_LINPOL_VECTOR = 4 };
enum { PM_JONES_FIELD_NONE = 0, PM_JONES_FIELD_REAL = 1, PM_JONES_FIELD_COMPLEX = 2 };
#define PM_JONES_LEAKAGE_IDENTITY 1
#define PM_JONES_MAX_CHAIN 6

/* a real parameter: `map` (rows x cols of the dtype's real type, rows ld apart) where it is not NULL, else the host's `value` */
typedef struct pm_jones_param {
    double value;
    const void* map;
    int64_t ld;
} pm_jones_param;

/* kind and parameters of a generated optic, angles in radians:
 *   PM_JONES_ROTATION       p[0] = theta                         jones_rotation_matrix (polarization.py:133-160)
 *   PM_JONES_RETARDER       p[0] = retardance, p[1] = theta      linear_retarder, the wave plates (:163-196, 234-272)
 *   PM_JONES_DIATTENUATOR   p[0] = alpha, p[1] = theta           linear_diattenuator, linear_polarizer (:199-231, 275-293)
 *   PM_JONES_VORTEX         p[0] = theta, p[1] = retardance, p[2] = rotate, charge; flags PM_JONES_LEAKAGE_IDENTITY puts the
 *                           -i cos(retardance / 2) term on both diagonal elements (Mawet 2009 eq. 7), 0 on element (0,0) only as the
 *                           reference does (:296-346).  charge x theta is formed in the map's precision before the cosine and sine
 *   PM_JONES_LINPOL_VECTOR  p[0] = angle, multiplied by `charge` (1 for radians, pi / 180 for degrees) in the map's precision;
 *                           the output is a vector                linear_pol_vector (:45-77) */
typedef struct pm_jones_optic_desc {
    int32_t kind, flags;
    double charge;
    pm_jones_param p[3];
} pm_jones_optic_desc;

/* one operand of pm_jones_chain: `map` in the chain's layout where it is not NULL, else the constant c = (re, im) of the four
 * components (of the two of a vector in c[0..3]) */
typedef struct pm_jones_operand {
    const void* map;
    int64_t ld, pstride;
    double c[8];
} pm_jones_operand;

/* The optic of `optic` at every pixel, times the complex map `field` (rows field_ld apart) where it is not NULL: the generators
 * followed by apply_polarization_optic (polarization.py:555-578) without the unit-amplitude optic in memory. */
int pm_jones_optic(int32_t dtype, const pm_jones_optic_desc* optic, int64_t rows, int64_t cols, const void* field, int64_t field_ld, void* out,
                   int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream);
/* out = A_1 @ A_2 @ ... @ A_count, 1 <= count <= PM_JONES_MAX_CHAIN, evaluated from the left as derot @ jones @ rot is
 * (polarization.py:193-195, 228-230, 344).  vector_tail != 0: the last operand, and then the output, is a vector.  No temporary. */
int pm_jones_chain(int32_t dtype, int32_t count, const pm_jones_operand* operands, int32_t layout, int32_t vector_tail, int64_t rows, int64_t cols,
                   void* out, int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream);
/* out = field x in (polarization.py:573-576) for matrices (ncomp 4) or vectors (ncomp 2); field_kind PM_JONES_FIELD_COMPLEX a complex
 * map, PM_JONES_FIELD_REAL a map of the real type, PM_JONES_FIELD_NONE the relayout alone (aos <-> planes, bit-exact).  out may be in
 * when layouts and strides are equal; in == out with anything else is refused.  Arrays that overlap in part are NOT detected and
 * give undefined results: the caller keeps in and out either identical or disjoint. */
int pm_jones_scale(int32_t dtype, int32_t ncomp, int64_t rows, int64_t cols, const void* in, int32_t layout, int64_t ld, int64_t pstride,
                   int32_t field_kind, const void* field, int64_t field_ld, void* out, int32_t out_layout, int64_t out_ld, int64_t out_pstride,
                   void* stream);
/* jones_to_mueller (polarization.py:349-407): the sixteen real elements of Re(U (J* (x) J) U^H) per pixel, row-major, as closed forms
 * in the four components.  out holds the real type: aos 16 values per pixel, planes 16 planes. */
int pm_jones_to_mueller(int32_t dtype, int64_t rows, int64_t cols, const void* jones, int32_t layout, int64_t ld, int64_t pstride, void* out,
                        int32_t out_layout, int64_t out_ld, int64_t out_pstride, void* stream);
/* pauli_coefficients (polarization.py:455-475): the four complex planes c0 ... c3 of out, out_pstride apart. */
int pm_pauli_coefficients(int32_t dtype, int64_t rows, int64_t cols, const void* jones, int32_t layout, int64_t ld, int64_t pstride, void* out,
                          int64_t out_ld, int64_t out_pstride, void* stream);

/* --- masked modal fitting (csrc/modalfit.hip) ---------------------------------------------- */
/* lstsq, normalize_modes and orthogonalize_modes of prysm/polynomials/fitting.py:103-187 over a stored basis: K real planes
 * modes[k * mode_stride + p], p < npts, PM_F32 or PM_F64, K <= PM_MODES_FIT_MAX (more: PM_ERR_UNSUPPORTED).  A point is valid when
 * (mask == NULL || mask[p] != 0) && (!finite_from_data || isfinite(data[0][p])); mask is bytes.  Validity is a select: a NaN at an
 * invalid point leaves no trace in any sum, a non-finite value at a valid point propagates.
 *
 * The record: pm_modes_record_doubles(K, nrhs) DEVICE doubles,
 *   [COUNT | RANK | G (K x K, both triangles) | L (K x K, lower) | dropped (K, 1.0 = dropped) | T (K x K) | b (nrhs x K) | coef (nrhs x K)]
 * so that everything before b depends on K alone. */
#define PM_MODES_FIT_MAX 128
#define PM_MODES_REC_COUNT 0
#define PM_MODES_REC_RANK 1
#define PM_MODES_REC_G 2
#define PM_MODES_GRAM 1
#define PM_MODES_RHS 2
#define PM_MODES_FACTOR 0
#define PM_MODES_SOLVE 1
#define PM_MODES_INVERT 2
#define PM_MODES_NORMS_STD 3
#define PM_MODES_NORMS_PTP 4
#define PM_MODES_LOWER 0
#define PM_MODES_DIAGONAL 1
#define PM_MODES_STAT_N 0
#define PM_MODES_STAT_SUM 1
#define PM_MODES_STAT_MIN 2
#define PM_MODES_STAT_MAX 3
#define PM_MODES_STAT_MEAN 4
#define PM_MODES_STAT_M2 5
#define PM_MODES_STAT_STD 6
#define PM_MODES_STAT_RECORD 7
size_t pm_modes_record_doubles(int64_t K, int64_t nrhs);

/* COUNT, G = sum_valid m_i m_j (with PM_MODES_GRAM) and b[r][i] = sum_valid m_i data[r] for nrhs >= 0 vectors data[r * data_stride + p]
 * (with PM_MODES_RHS; COUNT and G are then left as they are, so a prepared fit pays for b only).  Every product and sum in double on
 * v_mfma_f64_16x16x4_f64 over 16-blocks of modes; two stages in a fixed order, no atomics: a repeated call returns the same bits.
 * Each stored plane is read once per 16 data vectors.  16-byte loads when npts is a multiple of 4 and every plane starts on a
 * 16-byte boundary, element-wise otherwise.  workspace: pm_modes_gram_workspace() bytes; it grows with the workgroup count
 * (one per 1024 points) up to the cap. */
size_t pm_modes_gram_workspace(int32_t dtype, int64_t K, int64_t npts, int64_t nrhs);
int pm_modes_gram(int32_t dtype, int32_t parts, int64_t K, int64_t npts, const void* modes, int64_t mode_stride, int64_t nrhs,
                  const void* data, int64_t data_stride, const void* mask, int32_t finite_from_data, void* record, void* workspace,
                  size_t workspace_bytes, void* stream);

/* One single-workgroup launch on the record.  PM_MODES_FACTOR: the unpivoted Cholesky G = L L^T in mode order, in double; a mode whose
 * pivot is not above K eps64 (largest pivot so far) is dropped: its row and column are zero, it is flagged and RANK counts the rest.
 * PM_MODES_SOLVE: coef[r] = G^-1 b[r] by the two substitutions for the nrhs vectors, dropped modes 0; stored as doubles in the record
 * and in `dtype` at coef (nrhs x K).  PM_MODES_INVERT: T = L^-1, lower triangular, dropped rows and columns zero.  PM_MODES_NORMS_STD /
 * _PTP: T = diag(1 / norm) from the pm_modes_stats record at `stats`, norm < 1e-9 -> 1 (normalize_modes' loophole for piston). */
int pm_modes_small(int32_t dtype, int32_t op, int64_t K, int64_t nrhs, void* record, const void* stats, void* coef, void* stream);

/* out[k][p] = sum_{j <= k} T[k][j] modes[j][p] (PM_MODES_LOWER) or T[k][k] modes[k][p] (PM_MODES_DIAGONAL) with T read from the
 * record on the device; sums in double, each output rounded once.  zero_outside: points with mask[p] == 0 store 0 (orthogonalize);
 * otherwise every point is transformed (normalize).  All K values of a point are read before any is stored: out may be modes. */
int pm_modes_transform(int32_t dtype, int32_t form, int32_t zero_outside, int64_t K, int64_t npts, const void* modes, int64_t mode_stride,
                       const void* record, const void* mask, void* out, int64_t out_stride, void* stream);

/* Per mode over the points with mask[p] != 0 (all with mask NULL): N, SUM, MIN, MAX, MEAN, then M2 = sum (m - MEAN)^2 in a second
 * pass that reads MEAN on the device, and STD = sqrt(M2 / N), numpy's population std.  stats: K x PM_MODES_STAT_RECORD DEVICE doubles.
 * Four launches.  workspace: pm_modes_stats_workspace() bytes. */
size_t pm_modes_stats_workspace(int64_t K, int64_t npts);
int pm_modes_stats(int32_t dtype, int64_t K, int64_t npts, const void* modes, int64_t mode_stride, const void* mask, void* stats,
                   void* workspace, size_t workspace_bytes, void* stream);

/* --- housekeeping ------------------------------------------------------------------------- */
/* Real-input 2-D spectrum on ANY even width (round 5; prysm/otf.py:28-33 transform_psf, :62-135 the centre-normalised MTF / PTF / OTF
 * take any size through scipy): the real M x N array IS an M x N/2 complex array z[r][j] = x[r][2j] + i x[r][2j+1]; transform that
 * with pm_fft2 (forward, no rotations -- half the work, on whatever route its lengths take) and hand the result `zf` to this sweep,
 * which untangles F = fft2(x) from it, applies the rotation of the INPUT by (in_shift_y, in_shift_x) samples as a phase, divides by
 * F[0][0] (norm_dc; real: the sum of the samples), multiplies by `scale`, takes the epilogue (PM_EPI_NONE complex out, PM_EPI_ABS,
 * PM_EPI_ABS2, PM_EPI_ARG real out) and writes all M x N bins rotated by (out_shift_y, out_shift_x).  Lengths the library's own
 * Hermitian path takes (powers of two, PM_FLAG_REAL_INPUT in pm_fft2) do not need it. */
int pm_r2c_untangle(int32_t dtype, int64_t M, int64_t N, const void* zf, int64_t zf_ld, int64_t in_shift_y, int64_t in_shift_x,
                    int64_t out_shift_y, int64_t out_shift_x, int32_t epilogue, int32_t norm_dc, double scale, void* out, int64_t out_ld,
                    void* stream);

int pm_version(void);
const char* pm_last_error(void);   /* thread-local message for the last negative return */
int pm_plan_prepare(int32_t dtype, int64_t n);   /* build + cache the tables of a transform length now (twiddles; for a length on the
                                                  * Bluestein path its chirp tables and the twiddles of the convolution length): the first
                                                  * transform of a length otherwise does it, with a blocking upload that a hipGraph capture
                                                  * cannot record */
void pm_shutdown(void);            /* free cached tables */
/* performance knobs (they choose among equivalent routes and tilings; results agree to rounding): "col_var" picks the column
 * pass's tiling, "nt_in" / "nt_out" in {0,1} make the input loads / output stores non-temporal, "fold", "log_k", "batch_ws_mib",
 * "gemm_min_wgs" tune the engine and the GEMM; routing of awkward lengths: "blue_min" (shortest length on the Bluestein
 * path, 0 = off), "blue_2d" / "blue_fuse" (both-axes form; chirp multiplies inside the chain), "big_native_log" (log2 of the longest
 * length given to the engine as it is; the GPU tests lower it to run the 16384-point path on small arrays); real inputs: "r2c"
 * (Hermitian path: 0 never, 1 where it pays, 2 wherever legal), "herm_t" (its transposed form, real-input column transforms first:
 * -1 where it measured faster, 0 never, 1 wherever legal) with "herm_t_fold" (its column pass as planes of half-height tiles).  The full list with
 * defaults and measurements: struct Tuning in prysm_amd/csrc/pm_internal.h.  Also read once from the environment:
 * PM_TUNE="nt_in=1,fold=0".  Knobs whose variants left the library keep their names: the one value each still accepts returns 0,
 * any other PM_ERR_UNSUPPORTED (a PM_TUNE entry of that kind is skipped). */
int pm_set_tuning(const char* key, int32_t value);
/* the same knob for the CALLING host thread only: its first call gives the thread a private copy of the process-wide values, which
 * every later library call on that thread reads; pm_reset_tuning_local() returns the thread to the shared values.  This is the form
 * to use when several host threads drive the library at once -- prysm's own advice for several pipelines / devices is one thread
 * each (docs/source/how-tos/GPU and Exascale Computing.ipynb, file line 66) -- pm_set_tuning changes what every thread without a
 * private copy sees. */
int pm_set_tuning_local(const char* key, int32_t value);
void pm_reset_tuning_local(void);
/* Which route does this descriptor take?  Writes ONE line into buf (n >= 64 bytes; longer lines are cut) that names the planner's
 * decisions for op = 0 (pm_fft2) or op = 1 (pm_fft2_mul_ifft2) under the calling thread's knobs: the route ("engine", "engine-fold",
 * "hermitian[-fold]", "hermitian-transposed", "natural-mixed", "natural", "radix-step", "bluestein-2d[-big]"; "fused", "fused-composite", "hermitian-chain",
 * "composed"), the kernel class of each axis ("stockham", "mixed-radix", "bluestein", "direct"), tile width, layout and workspace
 * bytes.  Host logic only -- no device is touched, so a table of shapes can be pinned to its routes on a machine without a GPU
 * (the reference reaches every size through one scipy call, prysm/fttools.py:23-31; here a shape that slips to a slow route
 * should fail a test, not a benchmark).  Returns 0, or the error pm_fft2 would return for an invalid descriptor. */
int pm_plan_explain(const pm_fft2_desc* d, int32_t op, char* buf, size_t n);
/* time `reps` launches of each pass of the transform with hipEvents on `stream`; ms[0] = row pass,
 * ms[1] = column pass (average per launch).  Used by bench.py for the roofline object. */
int pm_fft2_time_passes(const pm_fft2_desc* d, const void* in, void* out, void* workspace,
                        size_t workspace_bytes, int reps, double* ms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRYSM_AMD_H */
