/*
 * dsc_mi355x.h — C ABI of the MI355X (gfx950) backend for DSC's FFT hot path.
 *
 * Drop-in seam: the `extern "C"` block of the reference's dsc/include/dsc.h:85-428.
 * Every function in section A keeps the reference's name, argument order, argument
 * meaning and error behaviour (invalid arguments / out of memory print to stderr and
 * exit(EXIT_FAILURE), dsc.h:14-28), so the reference's own bindings
 * (python/dsc/_bindings.py, dsc/api/dsc_api.h) load this library unchanged for that
 * subset.  What differs, and why:
 *
 *   - `dsc_tensor.data` is a DEVICE pointer into an HBM arena.  Host code must not
 *     dereference it; section B adds the explicit copy entry points the reference
 *     never needed (python/dsc/tensor.py:305-323, 371-377 memmove / view the pointer).
 *   - `dsc_tensor.backend` is DSC_BACKEND_MI355X (1); the reference only has CPU = 0
 *     (dsc/include/dsc_backend.h:11-13).
 *   - tensor headers, buffer refcounts, allocator nodes and FFT plans live in host
 *     memory next to the context instead of inside the arena
 *     (reference: dsc/src/dsc_allocator.cpp:34-49, dsc/src/dsc.cpp:255-256, 356-361).
 *   - operators are enqueued on the context's HIP stream and return immediately;
 *     every host-visible read (dsc_copy_to_host, dsc_synchronize) waits for them.
 *     Since `data` is not host-readable, this is indistinguishable from the
 *     reference's blocking calls.
 *
 * Plain C: pointers, sizes and PODs only.  No torch / HIP types in any signature.
 * Citations are file:line under the reference tree.
 */
#ifndef DSC_MI355X_H
#define DSC_MI355X_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSC_MAX_DIMS 4                         /* dsc.h:72-76 */

/* dsc_dtype.h:51-56 — `enum dsc_dtype : u8`; values are ABI (python/dsc/dtype.py:15-19) */
typedef uint8_t dsc_dtype;
enum { DSC_F32 = 0, DSC_F64 = 1, DSC_C32 = 2, DSC_C64 = 3 };

/* dsc_fft.h:13-16 — `enum dsc_fft_type : u8` */
typedef uint8_t dsc_fft_type;
enum { DSC_FFT_REAL = 0, DSC_FFT_COMPLEX = 1 };

/* dsc_backend.h:11-13 — `enum dsc_backend_type : u8 { CPU = 0 }`; MI355X is new */
typedef uint8_t dsc_backend_type;
enum { DSC_BACKEND_CPU = 0, DSC_BACKEND_MI355X = 1 };

/* dsc_dtype.h:36-49 — interleaved (real, imag) */
typedef struct { float  real, imag; } dsc_c32;
typedef struct { double real, imag; } dsc_c64;

typedef struct dsc_ctx dsc_ctx;                 /* dsc.cpp:140-145 (opaque) */
typedef struct dsc_fft_plan dsc_fft_plan;       /* dsc_fft.h:18-27 (opaque here) */

/* dsc.cpp:136-138 — `refs` first, as python/dsc/_bindings.py:38-41 mirrors it. */
typedef struct dsc_tensor_buffer {
    int refs;
} dsc_tensor_buffer;

/* dsc.h:96-108 — 64-byte POD; shape right-aligned and padded with 1; stride in
 * ELEMENTS, row-major contiguous (dsc.cpp:373-384); mirrored by _bindings.py:44-54. */
typedef struct dsc_tensor {
    int shape[DSC_MAX_DIMS];
    int stride[DSC_MAX_DIMS];
    dsc_tensor_buffer *buffer;
    void *data;                 /* DEVICE pointer (HBM arena), 256-B aligned */
    int ne;
    int n_dim;
    dsc_dtype dtype;
    dsc_backend_type backend;
} dsc_tensor;

/* ===================================================================== A. reference surface */

/* dsc.h:137, dsc.cpp:150-180.  Allocates the main arena (best-fit free list, as
 * dsc_allocator.cpp:51-221) and the scratch arena (bump allocator, :226-304) in HBM on
 * the current HIP device (see dsc_set_device) and creates the context's stream. */
dsc_ctx *dsc_ctx_init(size_t main_mem, size_t scratch_mem);

/* dsc.h:139-141, dsc.cpp:218-267: 16-slot plan cache keyed on (pow2ceil(n), fft_type,
 * twiddle precision), LRU eviction.  A plan here is the device twiddle tables. */
dsc_fft_plan *dsc_plan_fft(dsc_ctx *ctx, int n, dsc_fft_type fft_type, dsc_dtype dtype);

void   dsc_ctx_free(dsc_ctx *ctx);                          /* dsc.h:146, dsc.cpp:272-285 */
void   dsc_ctx_clear(dsc_ctx *ctx);                         /* dsc.h:148, dsc.cpp:287-291 */
void   dsc_tensor_free(dsc_ctx *ctx, dsc_tensor *x);        /* dsc.h:150, dsc.cpp:293-303; NULL and repeated frees are ignored */
size_t dsc_used_mem(dsc_ctx *ctx);                          /* dsc.h:155, dsc.cpp:310-312 */
void   dsc_print_mem_usage(dsc_ctx *ctx);                   /* dsc.h:157, dsc.cpp:314-322 */

/* dsc.h:159-168, dsc_tracing.h — operator tracing.  While recording, every operator call logs its
 * host-side begin / end AND the span its kernels took on the context's HIP stream (a pair of events); dsc_dump_traces
 * writes a Perfetto / chrome://tracing JSON array with the reference's fields ("name", "cat", "ph", "ts", "pid", "tid",
 * "args") on two tracks: tid 0 = API calls ("B" / "E"), tid 1 = device execution ("X" with "dur").  Always compiled in
 * (the reference needs DSC_ENABLE_TRACING); not recording costs one branch per call. */
void dsc_traces_record(dsc_ctx *ctx, bool record);
void dsc_dump_traces(dsc_ctx *ctx, const char *filename);
void dsc_clear_traces(dsc_ctx *ctx);

/* dsc.h:173-198, dsc.cpp:342-428.  buffer == NULL allocates; otherwise the new tensor
 * shares (and references) `buffer`. */
dsc_tensor *dsc_new_tensor(dsc_ctx *ctx, int n_dim, const int *shape, dsc_dtype dtype, dsc_tensor_buffer *buffer);
dsc_tensor *dsc_view(dsc_ctx *ctx, const dsc_tensor *x);
dsc_tensor *dsc_tensor_1d(dsc_ctx *ctx, dsc_dtype dtype, int dim1);
dsc_tensor *dsc_tensor_2d(dsc_ctx *ctx, dsc_dtype dtype, int dim1, int dim2);
dsc_tensor *dsc_tensor_3d(dsc_ctx *ctx, dsc_dtype dtype, int dim1, int dim2, int dim3);
dsc_tensor *dsc_tensor_4d(dsc_ctx *ctx, dsc_dtype dtype, int dim1, int dim2, int dim3, int dim4);

/* dsc.h:200-210, dsc.cpp:430-470: one-element 1-D tensors holding a scalar. */
dsc_tensor *dsc_wrap_f32(dsc_ctx *ctx, float val);
dsc_tensor *dsc_wrap_f64(dsc_ctx *ctx, double val);
dsc_tensor *dsc_wrap_c32(dsc_ctx *ctx, dsc_c32 val);
dsc_tensor *dsc_wrap_c64(dsc_ctx *ctx, dsc_c64 val);

/* dsc.h:221-223, dsc.cpp:587-597: returns x itself when the dtype already matches. */
dsc_tensor *dsc_cast(dsc_ctx *ctx, dsc_tensor *x, dsc_dtype new_dtype);

/* dsc.h:212-219, dsc.cpp:477-534 — creation.  dsc_arange: [0, 1, .., n-1] as the reference's running sum in the dtype
 * (f32 / c32 saturate at 2^24), made on the device.  dsc_randn: f32 / f64 only; every call returns the same fixed sequence,
 * the reference's default-seeded std::mt19937 + std::normal_distribution, generated on the host and copied to HBM. */
dsc_tensor *dsc_arange(dsc_ctx *ctx, int n, dsc_dtype dtype);
dsc_tensor *dsc_randn(dsc_ctx *ctx, int n_dim, const int *shape, dsc_dtype dtype);

/* dsc.h:225-232, dsc.cpp:599-740.  dsc_reshape: a view sharing x's buffer (and its refcount, as dsc_view); `dimensions` ints
 * follow, at most one of them negative (inferred); a mismatched element count is fatal.  dsc_concat: `tensors` dsc_tensor*
 * follow (same dtype and n_dim, equal extents off the axis); axis == DSC_VALUE_NONE flattens into a 1-D tensor. */
dsc_tensor *dsc_reshape(dsc_ctx *ctx, const dsc_tensor *x, int dimensions, ...);
dsc_tensor *dsc_concat(dsc_ctx *ctx, int axis, int tensors, ...);

/* dsc.h:275-278, dsc.cpp:1273-1284 (+ :44-69, :1174-1245; dsc_ops.h:68-78).
 * NumPy-style broadcasting over the 4 right-aligned dims, result dtype from the
 * promotion table dsc_dtype.h:73-78 (F64 x C32 -> C32).  out may be NULL. */
dsc_tensor *dsc_mul(dsc_ctx *ctx, dsc_tensor *xa, dsc_tensor *xb, dsc_tensor *out);
/* dsc.h:265-283, dsc.cpp:1247-1297 — same skeleton with add_op / sub_op / div_op (dsc_ops.h:46-90);
 * SURVEY 8f "next" row 2. */
dsc_tensor *dsc_add(dsc_ctx *ctx, dsc_tensor *xa, dsc_tensor *xb, dsc_tensor *out);
dsc_tensor *dsc_sub(dsc_ctx *ctx, dsc_tensor *xa, dsc_tensor *xb, dsc_tensor *out);
dsc_tensor *dsc_div(dsc_ctx *ctx, dsc_tensor *xa, dsc_tensor *xb, dsc_tensor *out);
/* dsc.h:285-288, dsc.cpp:1299-1310 — pow_op (dsc_ops.h:305-316): pow on reals, exp(b log a) on complex values; the same
 * broadcasting, promotion and result shape as dsc_add. */
dsc_tensor *dsc_pow(dsc_ctx *ctx, dsc_tensor *xa, dsc_tensor *xb, dsc_tensor *out);

/* dsc.h:293-323, dsc.cpp:1348-1443 (functors dsc_ops.h:92-229) — element-wise transcendental functions; the result has x's
 * dtype (out may be NULL; if given it must match x's dtype and shape).  Complex values follow the reference's formulas. */
dsc_tensor *dsc_cos(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_sin(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_sinc(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_logn(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_log2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_log10(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_exp(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_sqrt(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);

/* dsc.h:342-353, dsc.cpp:1625-1770.  dsc_i0: modified Bessel function I0 of f32 / f64 tensors (Abramowitz & Stegun 9.8.1 /
 * 9.8.2).  dsc_clip: min(max(x, x_min), x_max) with the reference's comparisons (NaN -> x_min; complex values compare by
 * their real part and a bound comes back as (bound, 0)); pass -INFINITY / INFINITY for "no bound". */
dsc_tensor *dsc_i0(dsc_ctx *ctx, const dsc_tensor *x);
dsc_tensor *dsc_clip(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, double x_min, double x_max);

/* dsc.h:325-340, dsc.cpp:1480-1622 (functors dsc_ops.h:242-303) — magnitude / phase / parts of a spectrum
 * (SURVEY 8f "next" row 2).  abs, angle, imag (and real of a complex tensor) return the REAL dtype of x;
 * dsc_conj / dsc_real of a real tensor return x itself, as the reference does. */
dsc_tensor *dsc_abs(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out);
dsc_tensor *dsc_angle(dsc_ctx *ctx, const dsc_tensor *x);
dsc_tensor *dsc_conj(dsc_ctx *ctx, dsc_tensor *x);
dsc_tensor *dsc_real(dsc_ctx *ctx, dsc_tensor *x);
dsc_tensor *dsc_imag(dsc_ctx *ctx, const dsc_tensor *x);

/* dsc.h:110-117 — one slice per leading dimension; DSC_VALUE_NONE (dsc.h:78) in a field selects NumPy's
 * default for it; start == stop == step != NONE means "this single index" and collapses the dimension
 * (how the wrapper spells x[:, 1], tensor.py:106-118). */
#define DSC_VALUE_NONE INT32_MAX
typedef struct dsc_slice {
    int start, stop, step;
} dsc_slice;

/* dsc.h:236-260, dsc.cpp:829-1169 — indexing and slicing ON THE DEVICE (SURVEY 8f "next" row 1): the
 * `[:output_length]` crop after dsc_irfft and the placement of a block into a zero-padded buffer no longer
 * round-trip through the host.  Variadic exactly as the reference: `indexes` ints, or `slices` dsc_slice
 * structs BY VALUE.  get_* return a new contiguous tensor (a fully indexed element is a 1-element 1-D tensor);
 * set_* write xb (same dtype; a 1-element tensor is broadcast, anything else is consumed cyclically in
 * row-major order, dsc.cpp:1010-1041) into the selected region of xa.  Negative indexes / starts / stops count
 * from the end, negative steps walk backwards; out-of-range arguments abort as the reference's asserts do. */
dsc_tensor *dsc_tensor_get_idx(dsc_ctx *ctx, const dsc_tensor *x, int indexes, ...);
dsc_tensor *dsc_tensor_get_slice(dsc_ctx *ctx, const dsc_tensor *x, int slices, ...);
void dsc_tensor_set_idx(dsc_ctx *ctx, dsc_tensor *xa, const dsc_tensor *xb, int indexes, ...);
void dsc_tensor_set_slice(dsc_ctx *ctx, dsc_tensor *xa, const dsc_tensor *xb, int slices, ...);

/* dsc.h:233-235, dsc.cpp:764-827 — permutation of the axes into a new contiguous tensor;
 * `axes` = 0 reverses them, otherwise `axes` == n_dim ints follow.  A 1-D tensor returns a view, as the reference. */
dsc_tensor *dsc_transpose(dsc_ctx *ctx, const dsc_tensor *x, int axes, ...);

/* dsc.h:416-424, dsc.cpp:2262-2340 — bin centre frequencies; dtype must be real.  Computed in
 * the output precision exactly as the reference does, then placed in HBM. */
dsc_tensor *dsc_fftfreq(dsc_ctx *ctx, int n, double d, dsc_dtype dtype);
dsc_tensor *dsc_rfftfreq(dsc_ctx *ctx, int n, double d, dsc_dtype dtype);

/* dsc.h:358-380, dsc.cpp:1771-1953.  Sequential left-to-right accumulation order per
 * output element is NOT reproduced on the GPU (tree order); max/min are exact
 * including the reference's tie rules on the real part (dsc_ops.h:318-339). */
dsc_tensor *dsc_sum (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_mean(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_max (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_min (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);

/* dsc.h:392-414, dsc.cpp:1958-2260.  Out-of-place, any axis, every length rounded up
 * to a power of two; n <= 0 means "length of the axis"; irfft's n counts BINS
 * (dsc.cpp:2199-2200).  out may be NULL; if given it must match dtype/n_dim/shape. */
dsc_tensor *dsc_fft  (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n, int axis);
dsc_tensor *dsc_ifft (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n, int axis);
dsc_tensor *dsc_rfft (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n, int axis);
dsc_tensor *dsc_irfft(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n, int axis);

/* ===================================================================== B. device seam (new) */

/* Select the HIP device used by the next dsc_ctx_init (one process per GPU: call with
 * LOCAL_RANK).  Returns the number of visible devices. */
int dsc_set_device(int device);

/* Replaces the host memmove in python/dsc/tensor.py:371-377 (from_numpy) and the
 * zero-copy view in :305-323 (numpy()).  nbytes must be <= ne * sizeof(dtype).
 * Both are stream-ordered; dsc_copy_to_host returns after the bytes have landed. */
void dsc_copy_from_host(dsc_ctx *ctx, dsc_tensor *dst, const void *src, size_t nbytes);
void dsc_copy_to_host(dsc_ctx *ctx, const dsc_tensor *src, void *dst, size_t nbytes);

/* Wait for everything enqueued on the context's stream. */
void dsc_synchronize(dsc_ctx *ctx);

/* The context's hipStream_t as an opaque pointer (interop / profiling). */
void *dsc_stream(dsc_ctx *ctx);

/* HIP-event stopwatch on the context's stream: start records an event, stop records a
 * second one, waits for it and returns the elapsed milliseconds between the two. */
void  dsc_timer_start(dsc_ctx *ctx);
float dsc_timer_stop(dsc_ctx *ctx);

/* Fused README filterFFT (README.md:113-135): out = irfft(rfft(s, n) * H) along the last
 * axis, one launch per batch of rows, the spectrum never written to HBM.
 *   s   real [.., ls]   (f32 or f64), zero-padded / cropped to n = 2*(H_bins-1) like dsc_rfft
 *   H   complex [H_bins] (c32 or c64) filter spectrum, H_bins = n/2 + 1, broadcast over rows;
 *       the imaginary parts of bins 0 and n/2 are ignored, as irfft ignores them
 *   out real [.., n] or NULL
 * Equals dsc_irfft(dsc_mul(dsc_rfft(s, n), H)) within float rounding.  Fused for f32 + c32
 * at n = 512 .. 65536 and f64 + c64 at n = 512 .. 32768 ("filter_mid_regs",
 * "filter_64k_regs").  Everything else runs exactly that three-op composition
 * ("filter_composed"): n <= 256, f64 at n = 65536, n >= 131072, rows with ls * 512 >= 2^30
 * at n <= 32768, and mixed precisions (f32 + c64, f64 + c32), whose output dsc_mul
 * promotes to f64. */
dsc_tensor *dsc_filter_fft(dsc_ctx *ctx, const dsc_tensor *s, const dsc_tensor *H, dsc_tensor *out);

/* Name of the kernel path the last FFT-family call took ("r2c_64k_regs", "generic_lds",
 * "generic_4step", ...): lets tests assert that the hand-written path really ran. */
const char *dsc_last_fft_path(dsc_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Section D — short-time transforms (no reference counterpart).
 *
 * torch.stft / torch.istft with onesided=True, normalized=False and win_length == n_fft, except for the layout: the
 * spectrum is FRAMES-MAJOR, [.., n_frames, n_fft/2 + 1] — torch.stft(...).transpose(-2, -1) — each frame's bins contiguous
 * like a batched dsc_rfft.  n_fft is a power of two, 4 <= n_fft <= 2^20, never rounded; hop >= 1 (larger than n_fft too).
 * window: real [n_fft] of the transform's precision, or NULL = ones.  Argument errors print and exit like every operator.
 * dsc_last_fft_path: "stft_regs" (one pass, framing and window in the load of the register kernels: n_fft 64 .. 32768),
 * "stft_composed" (windowed frames gathered into scratch, then the rfft routes; DSC_NO_STFT_FUSED=1 forces it, and so does a
 * row too long for the fused kernels' 31-bit buffer offsets: T * element size + n_fft * element size near 2 GB), "istft_ola".
 */
/* pad_mode: 0 = reflect (torch default), 1 = constant zeros.  window: real [n_fft] of x's precision, or NULL = ones.
 * x real [.., T] (f32 -> c32, f64 -> c64, at most 3 dims); out [.., n_frames, n_fft/2+1] or NULL.
 * n_frames = 1 + T / hop (center), 1 + (T - n_fft) / hop (not center).  center with reflect padding needs T > n_fft/2,
 * no center T >= n_fft. */
dsc_tensor *dsc_stft(dsc_ctx *ctx, const dsc_tensor *x, int n_fft, int hop, const dsc_tensor *window,
                     bool center, int pad_mode, dsc_tensor *out);
/* X complex [.., n_frames, n_fft/2+1]; length <= 0 = the natural length (hop (n_frames - 1), plus n_fft without center);
 * out real [.., length] or NULL.  Samples past the last frame are zero.  NOLA: the squared-window envelope must be >= 1e-11
 * wherever the output is read; the check copies the window (n_fft elements) to the host, which SYNCHRONISES the stream. */
dsc_tensor *dsc_istft(dsc_ctx *ctx, const dsc_tensor *X, int n_fft, int hop, const dsc_tensor *window,
                      bool center, int length, dsc_tensor *out);

/* ---------------------------------------------------------------------------------------------
 * Section E — linear convolution (no reference counterpart).
 *
 * Row r of out = np.convolve(x[r], h, 'full')[n0 : n0 + T_out]: scipy.signal.fftconvolve(x, h[None], mode, axes=-1), which is
 * np.convolve(x[r], h, mode) whenever M <= T.  Overlap-save in blocks of a power-of-two n points, D = M - 1 rounded up to even
 * of each block discarded.  Argument errors print and exit like every operator.
 * dsc_last_fft_path: "conv_regs" (one pass: blocks loaded from x, filtered and cropped in the fused filter kernel; D <= 16384),
 * "conv_composed" (blocks gathered into scratch, dsc_filter_fft, a crop-scatter kernel; D > 16384, rows too long for 31-bit
 * buffer offsets, or DSC_NO_CONV_FUSED=1).
 */
/* x real [.., T] (f32 or f64, at most 3 dims), h real [M] of the same dtype, broadcast over the rows of x.
 * mode 0 = full (T + M - 1 samples), 1 = same (T samples, start (M - 1) / 2), 2 = valid (T - M + 1 samples, needs M <= T).
 * out real [.., T_out] or NULL; it must not share memory with x.  dsc_last_fft_path: "conv_regs" | "conv_composed". */
dsc_tensor *dsc_convolve(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, int mode, dsc_tensor *out);
/* numpy.correlate for real inputs: dsc_convolve with h reversed. */
dsc_tensor *dsc_correlate(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, int mode, dsc_tensor *out);

/* ---------------------------------------------------------------------------------------------
 * Section F — 2-D transforms (no reference counterpart).
 *
 * numpy.fft.fft2 / ifft2 / rfft2 / irfft2 over the LAST TWO axes (n0 belongs to axis -2, n1 to axis -1); leading axes are batch;
 * 2 <= n_dim <= 4.  Each call is DEFINED as a composition of the 1-D operators, so their shape rules (rounding to a power of
 * two, zero padding / cropping, n <= 0 = the axis length, irfft's bin rule) carry over unchanged:
 *   dsc_fft2  (x, n0, n1) = dsc_fft  (dsc_fft  (x, n1, -1), n0, -2)   complex [.., N0, N1]; real input widened as dsc_fft does
 *   dsc_ifft2 (x, n0, n1) = dsc_ifft (dsc_ifft (x, n1, -1), n0, -2)   the same, scaled 1 / (N0 N1)
 *   dsc_rfft2 (x, n0, n1) = dsc_fft  (dsc_rfft (x, n1, -1), n0, -2)   x real; complex [.., N0, N1/2 + 1]
 *   dsc_irfft2(X, n0, n1) = dsc_irfft(dsc_ifft (X, n0, -2), n1, -1)   X complex [.., h, b]; real [.., N0, 2 order],
 *                           order = pow2((n1 > 0 ? n1 : b) - 1); the imaginary parts of columns 0 and `order` of the
 *                           intermediate are dropped, as dsc_irfft drops them
 * with N0 = pow2(n0 > 0 ? n0 : h), N1 = pow2(n1 > 0 ? n1 : w).  On power-of-two shapes these equal numpy's with s = (N0, N1).
 * out: NULL or a tensor of the result's shape and dtype; for dsc_fft2 / dsc_ifft2 of complex input with h == N0 and w == N1, out
 * may be x itself (in place), on every route.  Argument errors print and exit like every operator.
 * dsc_last_fft_path: "fft2_regs" / "rfft2_regs" — ONE pass, the image resident in registers (fft_2d.hip): fft2 / ifft2 with
 * N0, N1 in {32, 64, 128}, rfft2 with N0 in {32, 64, 128} and N1 in {64, 128, 256}; needs no intermediate — or "fft2_composed" /
 * "rfft2_composed" / "irfft2_composed": the two 1-D operators in turn with an arena intermediate that is freed before returning
 * (every other size, DSC_NO_FFT2_FUSED=1, images too large for the fused kernel's 31-bit buffer offsets).  dsc_irfft2 is NOT
 * fused: it always runs composed.
 */
dsc_tensor *dsc_fft2  (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1);
dsc_tensor *dsc_ifft2 (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1);
dsc_tensor *dsc_rfft2 (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1);
dsc_tensor *dsc_irfft2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1);

/* ---------------------------------------------------------------------------------------------
 * Section G — analytic signal (no reference counterpart).
 *
 * Along the LAST axis of x real [.., T] (f32 or f64, at most 4 dims); other axes: transpose first.  N = pow2(n > 0 ? n : T), the
 * length rule of dsc_fft; N >= 2.  Each row is cropped or zero padded to N samples (x_used), and with H[0] = H[N/2] = 0 and
 * H[k] = -i for 0 < k < N/2
 *   y = dsc_irfft(dsc_rfft(x_used, N) * H, N)
 *   dsc_hilbert (x, n) = x_used + i y            complex [.., N] (c32 / c64); the real part is a bit-for-bit copy of x_used
 *   dsc_envelope(x, n) = sqrt(x_used^2 + y^2)    real [.., N] of x's dtype, the formula of dsc_abs
 * On power-of-two rows dsc_hilbert is scipy.signal.hilbert(x, N) and dsc_envelope its absolute value.
 * out: NULL or a tensor of the result's shape and dtype; it must not share memory with x.  Argument errors (complex input, N < 2,
 * a wrong out) print and exit like every operator.
 * dsc_last_fft_path: "hilbert_regs" / "envelope_regs" — ONE pass for N = 512 .. 32768: the fused filter kernel with the constant H
 * (nothing loaded for it) stores the complex pairs or their moduli; needs no scratch — or "hilbert_composed" /
 * "envelope_composed": H written into scratch, rows in chunks through dsc_filter_fft into a scratch chunk, then zipped with x into
 * out (every other N, rows too long for the fused kernel's 31-bit buffer offsets, DSC_NO_HILBERT_FUSED=1; the switch is read at
 * every call).  On that route f32 rows of N >= 131072 are widened to f64 for the filter and y is rounded to f32 once: an f32
 * transform of that length cannot hold the operator's error bound on rows whose energy sits in a few samples.
 */
dsc_tensor *dsc_hilbert (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n);
dsc_tensor *dsc_envelope(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n);

/* ---------------------------------------------------------------------------------------------
 * Section H — polyphase FIR resampling (no reference counterpart).
 *
 * Along the LAST axis of x real [.., T] (f32 or f64, at most 4 dims); h real [M] of x's dtype, broadcast over the rows.  Nothing is
 * rounded to a power of two.  All three operators are one primitive P(x, h, gain, up, down, t0, T_out):
 *   y[r][m] = sum_i (h[t - i up] gain) x[r][i],   t = m down + t0 (64-bit),   over every i with 0 <= i < T and 0 <= t - i up < M,
 *   for 0 <= m < T_out.  The taps are multiplied by gain once, in x's dtype (one rounding: scipy's h * up); accumulation is in x's
 *   dtype; no atomics, every output written once: results are deterministic.
 *   dsc_upfirdn(h, x, up, down)          gain 1, t0 0, T_out = ceil(((T - 1) up + M) / down): scipy.signal.upfirdn(h, x, up, down, axis=-1)
 *   dsc_resample_poly(x, up, down, taps) up and down are first divided by their gcd.  1 / 1 is a copy of x (scipy's early return).
 *                                        Otherwise T_out = ceil(T up / down), gain up, t0 = half_len; taps NULL: half_len =
 *                                        10 max(up, down), h = dsc_firwin(2 half_len + 1, 1 / max(up, down), kaiser, beta 5) in x's
 *                                        dtype; taps [M] (scipy's window=array): half_len = (M - 1) / 2.
 *                                        scipy.signal.resample_poly(x, up, down, axis=-1[, window=taps]).
 *   dsc_decimate(x, q, n)                dsc_resample_poly(x, 1, q, dsc_firwin(n + 1, 1 / q, hamming)), n = 20 q when n <= 0; q >= 2:
 *                                        scipy.signal.decimate(x, q, n, ftype='fir', zero_phase=True)
 *   dsc_firwin(numtaps, cutoff, window, beta, dtype)   the low-pass design scipy.signal.firwin(numtaps, cutoff, window=..,
 *                                        pass_zero=True, scale=True) with fs = 2: h[k] = cutoff sinc(cutoff (k - alpha)) w[k],
 *                                        alpha = (numtaps - 1) / 2, divided by sum h; window 0 = symmetric Hamming
 *                                        0.54 - 0.46 cos(2 pi k / (numtaps - 1)), 1 = symmetric Kaiser
 *                                        I0(beta sqrt(1 - ((k - alpha) / alpha)^2)) / I0(beta); 0 < cutoff < 1.  Designed on the host in
 *                                        long double, rounded once to dtype (f32 / f64), uploaded on the context's stream (it
 *                                        synchronises, as dsc_randn does).  Designs are not cached: pass `taps` to reuse one.
 * out: NULL or a tensor of the result's shape and dtype; it must not share memory with x.  Argument errors (complex input, up or
 * down < 1, M < 1, a dtype mismatch, a wrong out, out overlapping x, a result of more than 2^31 - 1 elements, q < 2, a cutoff outside
 * (0, 1)) print and exit like every operator.
 * dsc_last_fft_path: "polyphase_direct" — ONE pass of the direct kernel (polyphase.hip): a workgroup stages the taps (phase-major, times
 * gain) and the samples of a tile of consecutive outputs in LDS and forms K = ceil(M / up) products per output; no scratch.  The host
 * sizes the tile to the LDS; when the taps and the samples of even a 64-output tile exceed 160 KiB (about down (64 + M / up) + M + 4 up
 * elements) the call is an argument error.  Guaranteed to run in both dtypes: every reduced (up, down) with max(up, down) <= 160 with the
 * designed filters, and any M <= 4096 with up, down <= 16.  "polyphase_copy": dsc_resample_poly whose reduced rates are 1 / 1.
 */
dsc_tensor *dsc_upfirdn      (dsc_ctx *ctx, const dsc_tensor *h, const dsc_tensor *x, int up, int down, dsc_tensor *out);
dsc_tensor *dsc_resample_poly(dsc_ctx *ctx, const dsc_tensor *x, int up, int down, const dsc_tensor *taps, dsc_tensor *out);
dsc_tensor *dsc_decimate     (dsc_ctx *ctx, const dsc_tensor *x, int q, int n, dsc_tensor *out);
dsc_tensor *dsc_firwin       (dsc_ctx *ctx, int numtaps, double cutoff, int window, double beta, dsc_dtype dtype);
/* host only, needs no device: the design dsc_firwin uploads, in double before the rounding to dtype */
void        dsc_firwin_host  (double *taps, int numtaps, double cutoff, int window, double beta);

/* ---------------------------------------------------------------------------------------------
 * Section I — prefix scans along one axis (no reference counterpart).
 *
 * Along `axis` of x (any axis, negative counts from the end; at most 4 dims), the tensor viewed as [outer][n][inner] like the
 * reductions.
 *   dsc_cumsum(x, axis)   numpy.cumsum(x, axis): f32 / f64 / c32 / c64 (complex component-wise), shape and dtype unchanged.  Accumulated
 *                         in x's dtype; no atomics, every output written once: bit-identical from run to run for a given shape and
 *                         route.  Element 0 along the axis is a bit-for-bit copy.
 *   dsc_diff(x, axis)     numpy.diff(x, 1, axis): out[j] = x[j + 1] - x[j], the four dtypes, the axis one shorter (n >= 2); one
 *                         subtraction per component, equal to numpy bit for bit.
 *   dsc_unwrap(x, axis)   numpy.unwrap(x, axis=axis), period 2 pi, default discontinuity, f32 / f64 — defined so that the result does
 *                         not depend on the order of the scan.  With TWO_PI = 6.283185307179586 and PI = 3.141592653589793 as doubles:
 *                           d[j] = (double) x[j] - (double) x[j - 1]                               j >= 1
 *                           m[j] = 0 when |d[j]| <= PI or d[j] is not finite, else the integer nearest to d[j] / TWO_PI, ties toward zero
 *                           K[j] = m[1] + .. + m[j], exact int32 arithmetic, K[0] = 0
 *                           out[j] = x[j] - K[j] TWO_PI, formed in double (one FMA) and rounded once to x's dtype; K[j] = 0: a copy
 *                         Every route gives the same bits; out[0] is a copy; rows without a jump come back unchanged.  Limits: |K| must
 *                         stay below 2^31; a sample that is not finite does not spread to the samples after it (numpy's float cumsum of
 *                         corrections would make them all NaN).  The definition agrees with numpy.unwrap in double to 6e-11 on rows of
 *                         70001 samples with |K| up to 620 (numpy's own accumulated rounding; tests/test_scan_abi.py).
 *   dsc_phase(z, axis)    dsc_unwrap(dsc_angle(z), axis) for z c32 / c64 in one pass, real result of the matching precision, bit-identical
 *                         to the composition: the atan2 of dsc_angle in the load, the integer scan, one store.
 * out: NULL or a tensor of the result's shape and dtype; it must not share memory with the input.  Argument errors (a wrong dtype, a
 * wrong out, an overlap, an axis out of range, n < 2 for dsc_diff) print and exit like every operator.
 * dsc_last_fft_path:
 *   "scan_rows"   inner == 1, 128 rows or more (or rows of at most one tile of 2048 - 8192 elements): one workgroup walks a row in chunks and carries the running
 *                 value in a register; persistent grid over the rows; one HBM round trip.
 *   "scan_tiles"  inner == 1, fewer than 128 rows longer than a tile: three plain launches — per-tile totals into scratch, a scan of the totals per row, the tile
 *                 scan with its carry-in.  x is read twice (ceiling: 2/3 of the roofline); no workgroup ever waits on another.
 *   "scan_cols"   inner > 1: one thread per (outer, inner) element walks the axis sequentially, neighbouring threads on neighbouring
 *                 addresses; dsc_cumsum is numpy's own left-to-right order here (bit-identical to numpy.cumsum).  The axis is not
 *                 segmented: a few columns with a long axis are slow.
 *   "scan_diff"   dsc_diff: element-wise.
 * DSC_SCAN_ROUTE=rows|tiles (read at every call) forces either route on any inner == 1 shape.
 */
dsc_tensor *dsc_cumsum(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis);
dsc_tensor *dsc_diff  (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis);
dsc_tensor *dsc_unwrap(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis);
dsc_tensor *dsc_phase (dsc_ctx *ctx, const dsc_tensor *z, dsc_tensor *out, int axis);

/* ---------------------------------------------------------------------------------------------
 * Section J — index maps along axes (no reference counterpart).
 *
 * out[j0, j1, j2, j3] = x[m0(j0), m1(j1), m2(j2), m3(j3)] or a constant, each m a piecewise-affine map of one axis: one plan, one
 * kernel family and ONE pass over memory, whatever the number of axes.  The four dtypes, 1 to 4 dims; elements move as opaque 4-, 8-
 * and 16-byte words, so every result is bit-identical to numpy's (NaN payloads and -0 included).  Negative axes count from the end.
 *   dsc_roll(x, shifts, axes)   numpy.roll(x, shifts, axes): n_axes shifts and axes; shifts of any sign and magnitude, reduced mod the
 *                               extent in 64 bits; a repeated axis adds its shifts.  n_axes == 0: shifts[0] rolls the flattened tensor
 *                               (numpy's axis=None), the result keeps x's shape.
 *   dsc_flip(x, axes)           numpy.flip(x, axes); n_axes == 0: every axis.  A repeated axis is an argument error, as numpy raises.
 *   dsc_fftshift(x, axes)       numpy.fft.fftshift(x, axes): a roll by n / 2 (rounded down) of every listed axis; n_axes == 0: every axis.
 *   dsc_ifftshift(x, axes)      numpy.fft.ifftshift(x, axes): a roll by -(n / 2); its inverse, and different from it on an axis of odd n.
 *   dsc_pad(x, pad_width, mode) numpy.pad(x, pad_width, mode).  pad_width [2 * x->n_dim]: (before, after) per axis of x in order, all >= 0,
 *                               of any width, wider than the axis included (cropping is dsc_tensor_get_slice's).  mode 0 constant
 *                               (value_re for real dtypes, value_re + i value_im for complex, rounded once to the dtype), 1 edge,
 *                               2 reflect, 3 symmetric, 4 wrap.  With n the extent and t = j - before the source index is
 *                                 wrap       t mod n                          edge       t clamped to [0, n - 1]
 *                                 reflect    u = t mod 2 (n - 1); u if u < n, else 2 (n - 1) - u; 0 when n == 1
 *                                 symmetric  u = t mod 2 n; u if u < n, else 2 n - 1 - u
 *                               (mod with a result >= 0): numpy's iterated padding in closed form (tests/test_remap_abi.py).
 * out: NULL or a tensor of the result's exact shape and x's dtype; it must not share memory with x (no in-place form).  Argument
 * errors (an axis out of range, a repeated dsc_flip axis, a negative pad width, an unknown mode, a wrong out, an overlap, a padded
 * result of more than 2^31 - 1 elements — the message names the shape) print and exit like every operator.
 * dsc_last_fft_path, after neighbouring axes that are not mapped have been merged ([4096, 64, 256] rolled on axis 0 is 4096 rows):
 *   "remap_rows"   the last axis is not mapped, its rows are whole 16-byte packs (at least 16 of them) and both tensors start on
 *                  16-byte boundaries: a workgroup resolves the outer source indices once and copies aligned packs.
 *   "remap_packs"  the last axis is mapped, 4- or 8-byte elements, OUTPUT rows of whole packs, aligned bases: every thread stores one
 *                  aligned pack whose sources are consecutive words in either direction (one load of element alignment, swapped in
 *                  registers when reversed) unless the pack straddles a seam of the map, where it gathers per element.
 *   "remap_elems"  everything else (odd row bytes, unaligned bases, 16-byte elements with a mapped last axis, short rows): one element
 *                  per thread.  DSC_REMAP_ROUTE=elems (read at every call) forces it on any shape.
 */
dsc_tensor *dsc_roll     (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *shifts, const int *axes);
dsc_tensor *dsc_flip     (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);
dsc_tensor *dsc_fftshift (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);
dsc_tensor *dsc_ifftshift(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes);
dsc_tensor *dsc_pad      (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, const int *pad_width, int mode, double value_re, double value_im);

/* ---------------------------------------------------------------------------------------------
 * Section K — moments along one axis (no reference counterpart).
 *
 * Along `axis` of x (any axis, negative counts from the end; at most 4 dims), the tensor viewed as [outer][n][inner] like the
 * reductions; f32 / f64 / c32 / c64.  Every sum is accumulated in double, for f32 / c32 data too (the product of two floats is exact
 * there), and every result is rounded once to its dtype.  With m = (sum x[j]) / n:
 *   dsc_sumsq(x)          sum |x[j]|^2: one read of x, no complex intermediate.  A complex x gives its real dtype, as dsc_abs does.
 *   dsc_rms(x)            sqrt(sumsq / n).
 *   dsc_var(x, ddof)      numpy.var(x, axis, ddof) = sum |x[j] - m|^2 / (n - ddof), centred on the computed mean: the two-pass
 *                         definition, which keeps its digits on data with an offset (neither sum |x|^2 - n |m|^2 nor merged
 *                         (count, mean, M2) triples do).  Real dtype of x.  ddof < 0 or ddof >= n is an argument error.
 *   dsc_std(x, ddof)      sqrt of it.
 *   dsc_vdot(a, b)        sum conj(a[j]) b[j]: a and b of one shape and dtype (no broadcasting), the result of that dtype.
 *   dsc_detrend(x, type)  scipy.signal.detrend(x, axis, type): with t[j] = j - (n - 1) / 2 and b = sum t[j] x[j] / (n (n^2 - 1) / 12),
 *                         out[j] = x[j] - m - b t[j] (DSC_DETREND_LINEAR, the least-squares line; n == 1 subtracts the mean only) or
 *                         out[j] = x[j] - m (DSC_DETREND_CONSTANT), per component of complex data.  x's shape and dtype.
 * keep_dims and the shape of a reduction's result are dsc_sum's.  out: NULL or a tensor of the result's shape and dtype; it must not
 * share memory with an input.  No floating-point atomics: partial sums are combined in index order, two identical calls give
 * identical bits.  Argument errors (a wrong out, an overlap, an axis out of range, a bad ddof, operands of dsc_vdot that differ in
 * shape or dtype, an unknown type) print and exit like every operator.
 * dsc_last_fft_path (detrend_rows / detrend_tiles / detrend_cols for dsc_detrend):
 *   "moment_rows"   inner == 1, 1024 rows or more (or rows of at most one tile): a workgroup per row — a wave per row for 1024
 *                   rows or more of at most a quarter of a tile — in 16-byte packs.  A row of at most one tile (32 KiB: 8192 f32, 4096 f64 / c32,
 *                   2048 c64; a quarter of that per wave; 2048 / 512 elements where the length or the address rules packs out) stays in
 *                   registers between the mean and the centred pass of var and detrend: one HBM read, plus one write for detrend.  A
 *                   longer row is read a second time by the same workgroup.
 *   "moment_tiles"  inner == 1, fewer than 1024 rows longer than a tile: per-tile sums to scratch, the statistic per row, the centred
 *                   pass per tile, its sums per row in tile order: two (sumsq, vdot), three (detrend) or four (var) plain launches.
 *   "moment_cols"   inner > 1: one thread per (outer, inner) element walks the axis, neighbouring threads on neighbouring addresses;
 *                   with fewer than 65536 outputs and an axis of at least 128 the axis is cut into segments combined in order.
 * DSC_MOMENT_ROUTE=rows|tiles (read at every call) forces either route on any inner == 1 shape.
 */
typedef enum { DSC_DETREND_CONSTANT = 0, DSC_DETREND_LINEAR = 1 } dsc_detrend_type;
dsc_tensor *dsc_sumsq  (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_rms    (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_var    (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, int ddof, bool keep_dims);
dsc_tensor *dsc_std    (dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, int ddof, bool keep_dims);
dsc_tensor *dsc_vdot   (dsc_ctx *ctx, const dsc_tensor *a, const dsc_tensor *b, dsc_tensor *out, int axis, bool keep_dims);
dsc_tensor *dsc_detrend(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, dsc_detrend_type type);

/* ---------------------------------------------------------------------------------------------
 * Section C — multi-GPU reassembly of batch-sharded outputs.
 *
 * No reference counterpart: the reference has one backend (CPU, dsc/include/dsc_backend.h:11-13) and no communication
 * layer.  Rows of a batched transform are independent, so rank r (one process per GPU) transforms rows
 * [r*B/P, (r+1)*B/P) with no exchange on the data path; these entry points exist to put the P shards next to each
 * other afterwards.  The gathered output of config 4 (65536 x 32769 c32) exceeds `int ne` (dsc.h:104) and therefore is
 * a RAW device buffer, not a dsc_tensor.  dsc_amd/shard.py drives them (and the RCCL variants); plain C here.
 */

/* hipIpcMemHandle_t as bytes, so that no HIP type appears in a signature. */
typedef struct dsc_ipc_handle { unsigned char bytes[64]; } dsc_ipc_handle;

/* A device buffer of its own (hipMalloc on the context's device), outside both arenas: the gather destination
 * [P x shard].  NULL on failure (this one reports instead of exiting: the caller sizes it from the world size). */
void *dsc_device_alloc(dsc_ctx *ctx, size_t nbytes);
void  dsc_device_free(dsc_ctx *ctx, void *ptr);

/* A dsc_tensor header over `nbytes` of caller-owned device memory (e.g. this rank's slot of the gather destination, so
 * that dsc_rfft writes its shard in place — no local copy).  The tensor does not own the bytes: dsc_tensor_free
 * releases the header only, and the memory must outlive it. */
dsc_tensor *dsc_tensor_from_device_ptr(dsc_ctx *ctx, void *ptr, size_t nbytes, int n_dim, const int *shape, dsc_dtype dtype);

/* Export `ptr` (a dsc_device_alloc result) to the other ranks' processes / open another rank's export.  The mapped
 * pointer addresses the PEER GPU's memory over xGMI (or the same GPU when ranks share one).  0 on success. */
int   dsc_ipc_export(dsc_ctx *ctx, void *ptr, dsc_ipc_handle *out);
void *dsc_ipc_open(dsc_ctx *ctx, const dsc_ipc_handle *handle);
int   dsc_ipc_close(dsc_ctx *ctx, void *mapped);

/* Direct push: copy `nbytes` from `src` (local) to `dst` (local or a dsc_ipc_open mapping) on copy lane `lane`
 * (0 <= lane < dsc_peer_lanes(): one HIP stream per lane, i.e. one per xGMI link when lane = peer), ordered AFTER
 * everything enqueued so far on the context's stream — the transform that produced `src` — and asynchronous to what
 * is enqueued afterwards: the gather of chunk i overlaps the transform of chunk i+1.  0 on success. */
int   dsc_peer_lanes(void);
int   dsc_peer_push(dsc_ctx *ctx, void *dst, const void *src, size_t nbytes, int lane);
/* Host waits until every push on every lane has landed (then exchange a barrier before peers read). */
int   dsc_peer_wait(dsc_ctx *ctx);

/* The collective north_star names: an RCCL communicator (one rank per process and GPU) and the all-gather that reassembles
 * the output, callable from a C / C++ host (the reference's C++ users, dsc/api/dsc_api.h:24-34) — no Python required.
 * RCCL is loaded on first use (dlopen); a process that never calls these never maps it.  All calls report failures
 * (-1 / NULL + a message on stderr) instead of exiting: the caller decides what a missing peer means.
 *   bootstrap: rank 0 calls dsc_comm_unique_id, the host ships the 128 bytes to the other ranks by its own means, every rank
 *   calls dsc_comm_init_rank (collective: returns once all n_ranks have called it). */
typedef struct dsc_comm dsc_comm;
typedef struct dsc_comm_id { unsigned char bytes[128]; } dsc_comm_id;      /* ncclUniqueId as bytes */
int       dsc_comm_unique_id(dsc_comm_id *out);
dsc_comm *dsc_comm_init_rank(dsc_ctx *ctx, const dsc_comm_id *id, int n_ranks, int rank);
int       dsc_comm_n_ranks(const dsc_comm *comm);
int       dsc_comm_rank(const dsc_comm *comm);
void      dsc_comm_free(dsc_comm *comm);
/* ONE in-place ncclAllGather on the persistent destination dest[n_ranks][rows][row_bytes]: this rank's shard already lies in
 * slot dest[rank] (its transform wrote it there through dsc_tensor_from_device_ptr views).  Enqueued on the context's stream,
 * i.e. ordered after the transforms enqueued so far; dsc_synchronize waits for it.  Every rank passes the same rows / row_bytes. */
int       dsc_shard_allgather(dsc_ctx *ctx, dsc_comm *comm, void *dest, size_t rows, size_t row_bytes);
/* Rows [row0, row0 + n_rows) of every slot in one group of P-1 ncclSend + P-1 ncclRecv (every GPU talks to all peers at once,
 * one xGMI link per peer): the chunk-wise form, so that chunk i travels while chunk i+1 is transformed.  Same ordering rules. */
int       dsc_shard_exchange_rows(dsc_ctx *ctx, dsc_comm *comm, void *dest, size_t rows, size_t row_bytes, size_t row0, size_t n_rows);

#ifdef __cplusplus
}
#endif
#endif /* DSC_MI355X_H */
