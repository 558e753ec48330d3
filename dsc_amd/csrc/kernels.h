// kernels.h — host-callable launchers of the HIP kernels (gfx950).  Everything is enqueued
// on the given stream; nothing here synchronises or allocates.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

// Error convention of the reference (dsc/include/dsc.h:14-28): message on stderr, exit.  Every kernel launch and every
// attribute call goes through these: a refused launch (grid too large, LDS not granted, ...) must never return an
// uninitialised tensor silently.
#define DSC_KERNEL_CHECK(call)                                                                                   \
    do {                                                                                                         \
        hipError_t kerr_ = (call);                                                                               \
        if (kerr_ != hipSuccess) {                                                                               \
            fprintf(stderr, "HIP error %s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(kerr_)); \
            exit(EXIT_FAILURE);                                                                                  \
        }                                                                                                        \
    } while (0)
#define DSC_LAUNCH(...)                        \
    do {                                       \
        hipLaunchKernelGGL(__VA_ARGS__);       \
        DSC_KERNEL_CHECK(hipGetLastError());   \
    } while (0)

// Dynamic-LDS opt-ins are per device: true the first time a call site runs on the calling thread's current device
// (one process per GPU is the design, but a host that drives several devices from one process stays correct).
static inline bool dsc_first_use_on_device(unsigned long long &seen) {
    int dev = 0;
    DSC_KERNEL_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (seen & bit) return false;
    seen |= bit;
    return true;
}

// A batch of 1-D lines inside a tensor.  Line q (0 <= q < n_lines) starts at element
//   (q / inner) * outer_stride + (q % inner) * inner_stride
// and advances by elem_stride per sample.  Strides are in elements of the array's own
// element type (real or complex).  For a contiguous DSC tensor transformed along `axis`:
// inner = prod(shape[axis+1:]), inner_stride = 1, elem_stride = inner,
// outer_stride = shape[axis] * inner  — the lines dsc_axis_iterator walks
// (reference: dsc/include/dsc_iter.h:11-65).
struct dsc_line_layout {
    long long outer_stride;
    long long inner_stride;
    long long elem_stride;
};

enum dsc_fft_mode {
    DSC_MODE_C2C = 0,        // complex in  -> complex out          (dsc_fft / dsc_ifft)
    DSC_MODE_R2C_CAST = 1,   // real in, cast to complex -> complex (dsc_fft on f32/f64, dsc.cpp:1984-1988)
    DSC_MODE_R2C_PACKED = 2, // 2L reals -> L+1 bins                (dsc_rfft,  dsc_fft.h:178-225)
    DSC_MODE_C2R_PACKED = 3, // L+1 bins -> 2L reals                (dsc_irfft, dsc_fft.h:194-236)
};

struct dsc_fft_lines_args {
    const void *in;
    void *out;
    long long n_lines;
    long long inner;
    dsc_line_layout lin, lout;
    int L;                 // complex transform length (power of two, <= dsc_fft_lds_max_len)
    int in_len;            // valid input samples along the axis (reals for R2C_PACKED, bins for C2R); the rest reads as zero
    int inverse;           // conjugate twiddles
    double scale;          // multiplied into every output
    const void *tw;        // W_L^k, k in [0, L)       interleaved (cos, sin), precision of the transform
    const void *tw_real;   // W_{2L}^k, k in [0, L]    (packed modes only)
    long long tw4_len;     // four-step: also multiply output k of line q by W_{tw4_len}^{(q % inner) * k}; 0 = off
    const void *tw4;       // table W_{tw4_len}^m, m in [0, tw4_len) (gathered, L2 resident); NULL = sincospi in double
};

// Largest complex length the LDS line kernel handles for the given precision.
int dsc_fft_lds_max_len(bool single_precision);

// One pass over HBM: gather -> Stockham radix-4/2 in LDS -> (real post-pass) -> scatter.
void dsc_launch_fft_lines(const dsc_fft_lines_args &a, dsc_fft_mode mode, bool single_precision, hipStream_t stream);

// Helpers of the multi-pass (four-step) path: contiguous [n_lines][L] complex work buffers holding
// tensor lines q_first .. q_first + n_lines - 1.
//   pack     tensor lines -> work (zero-pad / crop / cast / pair-up reals), per `mode`
//   prepass  C2R: bins in work-like layout -> Z = h1 + conj(w) h2           (dsc_fft.h:194-228)
//   postpass R2C: Z (work) -> L+1 bins scattered to the tensor               (dsc_fft.h:199-225)
//   unpack   work -> tensor lines (complex, or 2L reals for C2R) times scale
void dsc_launch_fft_pack(const void *in, void *work, long long q_first, long long n_lines, long long inner, dsc_line_layout lin,
                         int L, int in_len, dsc_fft_mode mode, bool single_precision, hipStream_t stream);
void dsc_launch_fft_c2r_prepass(const void *in, void *work, long long q_first, long long n_lines, long long inner, dsc_line_layout lin,
                                int L, int in_len, const void *tw_real, bool single_precision, hipStream_t stream);
void dsc_launch_fft_r2c_postpass(const void *work, void *out, long long q_first, long long n_lines, long long inner, dsc_line_layout lout,
                                 int L, const void *tw_real, bool single_precision, hipStream_t stream);
void dsc_launch_fft_unpack(const void *work, void *out, long long q_first, long long n_lines, long long inner, dsc_line_layout lout,
                           int L, double scale, dsc_fft_mode mode, bool single_precision, hipStream_t stream);

// ---- register-resident 65536-point real transforms (f32), one HBM round trip ------------
// x: [batch][65536] f32 contiguous rows; X: [batch][32769] c32 contiguous rows.
// aux: tables built by dsc_r2c64k_build_tables (device pointer).
size_t dsc_r2c64k_table_bytes();
void   dsc_r2c64k_build_tables(void *host_dst);          // fills a host staging buffer of table_bytes
// in_pitch: floats between input rows; in_len <= 65536 valid samples per row, the rest reads as zero (zero padding / crop)
void   dsc_launch_rfft64k(const float *x, void *X, int batch, int in_pitch, int in_len, const void *aux, int n_cu, hipStream_t stream);
void   dsc_launch_irfft64k(const void *X, float *x, int batch, int in_pitch, int in_len, const void *aux, int n_cu, hipStream_t stream);   // pitch / valid length in bins
// complex 32768-point transform of c32 rows in the same design (z: [batch][in_pitch], in_len <= 32768 samples used)
void   dsc_launch_fft32k_c32(const void *z, void *Z, int batch, int in_pitch, int in_len, bool inverse, bool cast, const void *aux, int n_cu,
                             hipStream_t stream);
// y = irfft(rfft(s) * H) fused; H: [32769] c32
void   dsc_launch_filter64k(const float *s, const void *H, float *y, int batch, int in_pitch, int in_len, const void *aux, int n_cu,
                            hipStream_t stream);

// ---- transforms along a non-last axis, lanes = neighbouring lines (fft_regs_cols.hip): complex length 32 .. 2048 (c32 data: 4096)
bool   dsc_fft_regs_cols_supports(int L, dsc_fft_mode mode, bool single_precision);
void   dsc_launch_fft_regs_cols(const void *in, void *out, long long slices, int inner, int L, dsc_fft_mode mode, bool inverse, bool single_precision,
                                const void *tw_full, const void *tw_real, double scale, int in_axis, int in_len, int out_axis, hipStream_t stream);
// complex transform of n = n1 n2 points along the middle axis of [slices][n][inner] in two passes of the column kernel (four-step)
bool   dsc_fft_cols_4step_split(int n, bool single_precision, int cols, int *n1, int *n2);
// real transforms of n = n1 n2 points along the middle axis of [slices][n][2 cc_n] reals: two neighbouring columns as one complex column
void   dsc_launch_rfft_cols_4step(const void *in, void *work, void *out, long long slices, int cc_n, int n1, int n2, bool single_precision,
                                  const void *tw1, const void *tw2, const void *twn, hipStream_t stream);
void   dsc_launch_irfft_cols_4step(const void *in, void *work, void *out, long long slices, int cc_n, int n1, int n2, bool single_precision,
                                   const void *tw1, const void *tw2, const void *twn, double scale, hipStream_t stream);
void   dsc_launch_fft_cols_4step(const void *in, void *work, void *out, long long slices, int inner, int n1, int n2, dsc_fft_mode mode, bool inverse,
                                 bool single_precision, const void *tw1, const void *tw2, const void *twn, double scale, hipStream_t stream);

// ---- long real transforms in two passes over HBM (fft_r2c_2pass.hip): packed complex length L = 32768 (f64 only),
// 65536 ... 1048576; f32 and f64.  forward: reals -> out = [rows][L + 1] bins; inverse: bins -> [rows][2L] reals.
// work: rows * L complex of scratch; tw_full: W_L^k, k < L; tw_real: W_{2L}^k, k <= L (the REAL plan's own tables).
bool   dsc_fft_two_pass_supports(int L, bool single_precision);
// the same lengths for complex data (dsc_fft / dsc_ifft of complex tensors): in = complex rows, out = [rows][L]
void   dsc_launch_fft_two_pass(const void *in, void *out, long long rows, int L, bool inverse, bool cast, bool single_precision, void *work,
                               const void *tw_full, long long in_pitch, int in_len, hipStream_t stream);
// in_pitch / in_len: pitch and valid length of the input rows in input elements (reals forward, bins inverse): shorter rows are zero
// padded, longer ones cropped.
void   dsc_launch_rfft_two_pass(const void *in, void *out, long long rows, int L, bool inverse, bool single_precision, void *work,
                                const void *tw_full, const void *tw_real, long long in_pitch, int in_len, hipStream_t stream);

// ---- complex rows of 65536 and 131072 points (f32, f64; the f64 131072 = config 5) and 32768 points (f64) in one launch with the four-step intermediate in the XCD-local L2
// (fft_xcd_fused.hip).  Arguments as the two-pass launchers; `scratch`: dsc_fft_fused_l2_scratch_bytes() bytes, of which the
// first dsc_fft_fused_l2_ctl_bytes() are the control block; host_error: a pinned, device-visible word that receives a non-zero
// code if a barrier of the launch did not complete.  Returns false when the launch cannot be made fully resident on this device.
bool   dsc_fft_fused_l2_supports(int L, bool single_precision, bool real, bool inverse);
size_t dsc_fft_fused_l2_ctl_bytes();
size_t dsc_fft_fused_l2_scratch_bytes(int L, bool single_precision);
bool   dsc_launch_fft_fused_l2(const void *in, void *out, long long rows, int L, bool real, bool inverse, bool cast, bool single_precision, void *scratch,
                               unsigned *host_error, const void *tw_full, const void *tw_real, long long in_pitch, int in_len, hipStream_t stream);

// ---- complex lengths 2 .. 16 (real 4 .. 32), contiguous lines, one thread per line (fft_tiny.hip).  in_pitch / in_len in input
// elements (reals for R2C_PACKED / R2C_CAST), in_pitch < 0 = full lines; scale multiplies the results.
bool dsc_fft_tiny_supports(int L);
// ... and along a non-last axis of [slices][axis][inner] (lane = column, no staging)
void dsc_launch_fft_tiny_cols(const void *in, void *out, long long slices, int inner, int L, dsc_fft_mode mode, bool inverse, bool single_precision,
                              double scale, int in_axis, int in_len, int out_axis, hipStream_t stream);
void dsc_launch_fft_tiny(const void *in, void *out, long long n_lines, int L, dsc_fft_mode mode, bool inverse, bool single_precision, double scale,
                         long long in_pitch, int in_len, hipStream_t stream);

// ---- register-resident transforms of contiguous full lines, complex length 256 .. 16384 (f32, f64; f32 C2C also 32768)
// (fft_regs_mid.hip).  in / out: [n_lines][L] complex (C2C), [n_lines][2L] reals -> [n_lines][L+1] bins
// (R2C_PACKED) or the converse (C2R_PACKED).  tw_full: W_L^k, k < L; tw_real: W_{2L}^k, k <= L.
bool dsc_fft_regs_mid_supports(int L, dsc_fft_mode mode, bool single_precision);
bool dsc_fft_regs_small_supports(int L);        // 32 .. 256: same launcher, full contiguous lines only (in_pitch < 0)
// in_pitch / in_len: input line pitch and valid length in input elements (reals for R2C_PACKED / R2C_CAST, complex otherwise):
// shorter lines are zero padded, longer ones cropped; in_pitch < 0 = full contiguous lines (the fast instantiation).
void dsc_launch_fft_regs_mid(const void *in, void *out, long long n_lines, int L, dsc_fft_mode mode, bool inverse, bool single_precision,
                             const void *tw_full, const void *tw_real, double scale, long long in_pitch, int in_len, hipStream_t stream);

// fused y = irfft(rfft(s, 2L) * H) at the same lengths (README filterFFT): s = [n_lines][in_pitch] reals of which in_len <= 2L are
// used, H = [L + 1] bins shared by all rows, y = [n_lines][2L] reals
void dsc_launch_filter_regs_mid(const void *s, const void *H, void *y, long long n_lines, int L, bool single_precision, const void *tw_full,
                                const void *tw_real, long long in_pitch, int in_len, hipStream_t stream);

// ---- short-time transforms (dsc_stft / dsc_istft, stft.cpp) -----------------------------------
// Fused forward route (fft_regs_mid.hip), n_fft = 64 .. 32768: frames of x [rows][T] (rows = n_lines / n_frames) starting at
// f * hop - pad, reflected (reflect) or zero outside [0, T), times w [n_fft] (NULL = ones), through the packed-real register
// transform into out [n_lines][n_fft/2 + 1].  Tables of the n_fft/2-point REAL plan; x_bytes >= rows T elem, and
// (rows + 1) T elem + n_fft elem < 2^31.
bool dsc_stft_regs_supports(int n_fft);
void dsc_launch_stft_regs(const void *x, const void *w, void *out, long long n_lines, int n_fft, int T, int n_frames, int hop, int pad,
                          bool reflect, bool single_precision, int x_bytes, const void *tw_full, const void *tw_real, hipStream_t stream);
// Frame-and-window gather (fft_stft.hip): frames [n_lines][n_fft] reals <- frames q0 .. q0 + n_lines - 1 (flattened (row, frame)) of x,
// same mapping as above
void dsc_launch_stft_frames(const void *x, const void *w, void *frames, long long q0, long long n_lines, int n_fft, long long T, int n_frames,
                            int hop, int pad, bool reflect, bool single_precision, hipStream_t stream);
// Overlap-add gather (fft_stft.hip).  frames [rows][fpr][n_fft] reals hold frames fa .. fa + fpr - 1 of `rows` consecutive rows starting
// at row r0; writes y[r][p - pad] for padded positions p in [p0, p1) with 0 <= p - pad < length: the sum over the frames f in
// [fa, fa + fpr) ∩ [0, n_frames) covering p (f hop <= p < f hop + n_fft), in increasing f, of frame[p - f hop] w[p - f hop], divided by
// the sum of w^2 over the same frames (0 where no frame covers p).  y: [.., length] reals; no atomics.
void dsc_launch_istft_ola(const void *frames, const void *w, void *y, long long r0, long long rows, int fa, int fpr, int n_fft, int hop,
                          int n_frames, int pad, long long p0, long long p1, int length, bool single_precision, hipStream_t stream);

// ---- linear convolution (dsc_convolve / dsc_correlate, conv.cpp) -------------------------------
// Fused overlap-save route (fft_regs_mid.hip), n = 512 .. 32768: line q = (row, block b), rows = n_lines / n_blocks, is the frame of
// x [rows][T] starting at b hop - pad (zero outside [0, T)) through irfft(rfft(frame, n) * H), H [n/2 + 1] bins; its samples
// [D, n) go to y[row][b hop + j - D] where that is < T_out.  D even, hop = n - D.  Tables of the n/2-point REAL plan;
// x_bytes = rows T elem with (rows + 1) T elem + n elem < 2^31, y_bytes = rows T_out elem < 2^31.
bool dsc_conv_regs_supports(int n);
void dsc_launch_conv_regs(const void *x, const void *H, void *y, long long n_lines, int n, int T, int n_blocks, int hop, int pad, int D, int T_out,
                          bool single_precision, int x_bytes, int y_bytes, const void *tw_full, const void *tw_real, hipStream_t stream);
// Composed route's crop-scatter (fft_conv.hip): frames [n_lines][n] reals are the filtered blocks q0 .. q0 + n_lines - 1 (flattened
// (row, b)); the same mapping to y [..][T_out] as above, hop = n - D
void dsc_launch_conv_crop(const void *frames, void *y, long long q0, long long n_lines, int n, int D, int n_blocks, long long T_out,
                          bool single_precision, hipStream_t stream);
// out[i] = in[n - 1 - i] (fft_conv.hip)
void dsc_launch_reverse(const void *in, void *out, int n, bool single_precision, hipStream_t stream);

// ---- analytic signal (dsc_hilbert / dsc_envelope, hilbert.cpp) ----------------------------------
// Fused route (fft_regs_mid.hip), n = 512 .. 32768: row q of x = [n_lines][in_pitch] reals, of which in_len <= n are used and the rest
// reads as zero, through y = irfft(rfft(row, n) * H) with the constant H[0] = H[n/2] = 0, H[k] = -i otherwise; out = [n_lines][n] complex
// (row, y), or with `envelope` [n_lines][n] reals sqrt(row^2 + y^2).  Tables of the n/2-point REAL plan.  A workgroup addresses its rows
// of x with 31-bit byte offsets: 64 in_pitch elem < 2^30 is the caller's to check.  out must not overlap x (x is read twice).
bool dsc_hilbert_regs_supports(int n);
void dsc_launch_hilbert_regs(const void *x, void *out, long long n_lines, int n, bool envelope, bool single_precision, const void *tw_full,
                             const void *tw_real, long long in_pitch, int in_len, hipStream_t stream);
// The composed route's small kernels (fft_hilbert.hip).  H [n/2 + 1] complex <- the constant response above.
void dsc_launch_hilbert_response(void *H, int n, bool single_precision, hipStream_t stream);
// out rows q0 .. q0 + n_lines - 1 <- rows q0 .. of x [..][in_pitch] (in_len used, zero padded to n) zipped with y [n_lines][n] reals:
// complex pairs (x, y) of out [..][n] complex, or with `envelope` sqrt(x^2 + y^2) of out [..][n] reals.  y_double (f32 x and out only):
// y is f64, the modulus is taken in f64, and the result is rounded once
void dsc_launch_hilbert_zip(const void *x, const void *y, void *out, long long q0, long long n_lines, int n, long long in_pitch, int in_len,
                            bool envelope, bool single_precision, bool y_double, hipStream_t stream);
// xw [n_lines][wpitch] f64 <- samples j < in_len of rows q0 .. of x [..][in_pitch] f32, zero from in_len on; wpitch even, >= in_len
void dsc_launch_hilbert_widen(const void *x, void *xw, long long q0, long long n_lines, long long in_pitch, int in_len, int wpitch,
                              hipStream_t stream);

// ---- polyphase FIR resampling (dsc_upfirdn / dsc_resample_poly / dsc_decimate, resample.cpp) -----
// Direct kernel (polyphase.hip): y[r][m] = sum_i (h[t - i up] gain) x[r][i], t = m down + t0, over 0 <= i < T and 0 <= t - i up < M, for
// 0 <= m < T_out; x [rows][T], h [M], y [rows][T_out] reals of one precision; up, down, M >= 1, t0 >= 0, rows T_out < 2^31.  The taps are
// multiplied by gain once, in the data's precision.  Returns false, with nothing launched, when the taps and the samples of even a
// 64-output tile do not fit dsc_polyphase_lds_limit() bytes of LDS.  y must not overlap x.
size_t dsc_polyphase_lds_limit();
bool dsc_launch_polyphase(const void *x, const void *h, void *y, long long rows, long long T, long long T_out, int M, int up, int down, long long t0,
                          double gain, bool single_precision, hipStream_t stream);

// ---- 2-D transforms of small images (dsc_fft2 / dsc_ifft2 / dsc_rfft2, fft2.cpp) -----------------
// One pass (fft_2d.hip): in [n_img][h][w] (complex for C2C, reals for R2C_CAST and R2C_PACKED), zero padded / cropped to N0 x N1,
// out [n_img][N0][N1] complex (R2C_PACKED: [n_img][N0][N1/2 + 1]).  N0, N1 in {32, 64, 128} (R2C_PACKED: N1 in {64, 128, 256}).
// A workgroup owns dsc_fft2_regs_group() images and addresses them with 31-bit byte offsets: group * h * w * element size < 0x7f000000
// is the caller's to check.  in == out is allowed for C2C with h == N0 and w == N1.
bool dsc_fft2_regs_supports(int N0, int N1, dsc_fft_mode mode);
int dsc_fft2_regs_group(int N0, int N1, dsc_fft_mode mode, bool single_precision);
void dsc_launch_fft2_regs(const void *in, void *out, long long n_img, int N0, int N1, int h, int w, dsc_fft_mode mode, bool inverse,
                          bool single_precision, double scale, hipStream_t stream);

// ---- element-wise ------------------------------------------------------------------------
// dtype codes are dsc_dtype values (0 f32, 1 f64, 2 c32, 3 c64)
void dsc_launch_cast(const void *in, int in_dtype, void *out, int out_dtype, long long ne, hipStream_t stream);

// op: 0 abs, 1 angle, 2 conj, 3 real, 4 imag (output real dtype of the input; conj keeps the dtype);
// 5 cos, 6 sin, 7 sinc, 8 logn, 9 log2, 10 log10, 11 exp, 12 sqrt, 13 i0 (f32 / f64 only), 14 clip to [lo, hi] (output dtype = input's)
void dsc_launch_unary(const void *in, int in_dtype, void *out, int op, long long ne, hipStream_t stream, double lo = 0, double hi = 0);
// out[i] = i in the dtype, saturating at 2^24 in f32 / c32 as the reference's running sum does
void dsc_launch_arange(void *out, int dtype, long long n, hipStream_t stream);

struct dsc_bcast_args {
    int out_shape[4];
    int a_stride[4];       // element strides, 0 on broadcast dims (dsc_iter.h:67-95)
    int b_stride[4];
    long long ne;
    int a_scalar, b_scalar;   // reference's scalar fast paths (dsc.cpp:1194-1212)
    // index fast paths (no per-element divisions): 0 general, 1 both operands have the output's shape,
    // 2 a full / b = the trailing dims of the output (row broadcast: ib = i % b_ne), 3 the converse,
    // 4 a full / b = the leading dims of the output, ones behind (column broadcast: ib = i / small_ne), 5 the converse
    int fast;
    int small_ne;             // fast = 2, 3: element count of the broadcast operand; fast = 4, 5: output elements per element of it
};
// op: 0 add, 1 sub, 2 mul, 3 div, 4 pow
void dsc_launch_binary(const void *a, const void *b, void *out, int dtype, int op, const dsc_bcast_args &g, hipStream_t stream);
// operands of different dtypes, equal shapes, contiguous: casts to the promoted dtype in registers.  false = not taken
// (odd element count or unaligned views): the caller casts into scratch tensors and calls dsc_launch_binary.
bool dsc_launch_binary_mixed(const void *a, int a_dtype, const void *b, int b_dtype, void *out, int op, long long ne, hipStream_t stream);

// ---- reductions along one axis -----------------------------------------------------------
// x viewed as [outer][axis_n][inner] contiguous; out as [outer][inner].
// op: 0 sum, 1 mean, 2 max, 3 min
// workspace: scratch for the segmented path (may be NULL)
void dsc_launch_reduce(const void *x, void *out, int dtype, int op, long long outer, int axis_n, long long inner,
                       void *workspace, size_t workspace_bytes, hipStream_t stream);

// ---- prefix scans along one axis (dsc_cumsum / dsc_diff / dsc_unwrap / dsc_phase, scan.cpp) ------
// x viewed as [outer][n][inner] contiguous (scan.hip).  op: 0 cumsum (dtype f32 / f64 / c32 / c64, out of the same dtype), 1 unwrap
// (f32 / f64, out of the same dtype), 2 phase (c32 / c64 in, f32 / f64 out); dtype is x's.  out has x's shape and must not overlap x.
// rows / tiles: inner == 1, x = [rows][n].  rows: one launch, a workgroup per row.  tiles: three launches (tile totals, their scan per
// row, the tiles with their carry-in) and dsc_scan_tiles_scratch_bytes() bytes of scratch, 256-byte aligned; a tile is
// dsc_scan_tile_len() elements.  cols: any inner, one thread per (outer, inner) element.
int    dsc_scan_tile_len(int op, int dtype);
size_t dsc_scan_tiles_scratch_bytes(int op, int dtype, long long rows, int n);
void   dsc_launch_scan_rows(const void *x, void *out, int op, int dtype, long long rows, int n, hipStream_t stream);
void   dsc_launch_scan_tiles(const void *x, void *out, int op, int dtype, long long rows, int n, void *scratch, hipStream_t stream);
void   dsc_launch_scan_cols(const void *x, void *out, int op, int dtype, long long outer, int n, long long inner, hipStream_t stream);
// out [outer][n - 1][inner] = x[.][j + 1][.] - x[.][j][.], n >= 2, fewer than 2^31 output elements
void   dsc_launch_scan_diff(const void *x, void *out, int dtype, long long outer, int n, long long inner, hipStream_t stream);

// ---- centred moments along one axis (dsc_sumsq / dsc_rms / dsc_var / dsc_std / dsc_vdot / dsc_detrend, moments.cpp) ------
// x (and y, vdot only: the same shape and dtype, else NULL) viewed as [outer][n][inner] contiguous (moments.hip).  op: 0 sumsq / rms
// (root), 1 vdot = sum conj(x) y, 2 var / std (root), 3 detrend constant, 4 detrend linear; dtype is x's, every sum a double.  out: one
// element per (outer, inner) of x's real dtype (op 0, 2) or of x's dtype (op 1); detrend: x's shape and dtype, not overlapping x.
// rows / tiles: inner == 1, x = [rows][n].  rows: one launch, a wave or workgroup per row.  tiles: two to four launches (tile sums, the
// statistic per row, the centred pass per tile, its sums per row) and dsc_moment_scratch_bytes(rows, tiles per row) bytes of scratch,
// 256-byte aligned; a tile is dsc_moment_tile_len() elements, which is also the longest row that stays in registers between the two
// passes of the rows route.  cols: any inner; n_seg from dsc_moment_cols_segments() (1: one thread walks the whole axis, no scratch),
// which never asks for more than scratch_bytes = dsc_moment_scratch_bytes(outer inner, n_seg).
int    dsc_moment_tile_len(int dtype);
size_t dsc_moment_scratch_bytes(long long n_out, long long n_seg);
void   dsc_launch_moment_rows(const void *x, const void *y, void *out, int op, int dtype, long long rows, int n, int ddof, bool root,
                              hipStream_t stream);
void   dsc_launch_moment_tiles(const void *x, const void *y, void *out, int op, int dtype, long long rows, int n, int ddof, bool root,
                               void *scratch, hipStream_t stream);
int    dsc_moment_cols_segments(long long n_out, int n, size_t scratch_bytes);
void   dsc_launch_moment_cols(const void *x, const void *y, void *out, int op, int dtype, long long outer, int n, long long inner, int ddof,
                              bool root, int n_seg, void *scratch, hipStream_t stream);

// ---- strided gather / scatter of a slice region (indexing.cpp) -----------------------------
// Region of a tensor: element (i0, i1, i2, i3), i_d < count[d], sits at base + sum_d i_d * stride[d]
// (elements; strides may be negative).  Row-major order over the region = flat index of the dense side.
struct dsc_region {
    int count[4];
    long long stride[4];
    long long base;
    long long ne;             // product of count
};
// gather: dense[i] = strided[region(i)];  scatter: strided[region(i)] = dense[i % dense_ne]
void dsc_launch_region_copy(const void *src, void *dst, int elem_bytes, const dsc_region &r, bool scatter, long long dense_ne,
                            hipStream_t stream);

// ---- index maps along axes (dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad, remap.cpp) ------
// dsc_axis_map and dsc_remap, the plan: out[j0, j1, j2, j3] = x[m0(j0), m1(j1), m2(j2), m3(j3)] or the plan's constant.  Declared in a
// header of their own with the integer arithmetic on them (dsc_map_index, dsc_remap_merge, dsc_remap_route), which a stand-alone host
// program can include.
#include "remap_plan.h"
// One pass of a MERGED plan (remap.hip) on the given route, which the caller took from dsc_remap_route or weakened to DSC_REMAP_ELEMS;
// the plan travels as a kernel argument.  x and out dense, of elem_bytes-byte elements, not overlapping.
void dsc_launch_remap(const void *x, void *out, int elem_bytes, const dsc_remap &plan, int route, hipStream_t stream);

// out[b][c][r] = in[b][r][c] for `batch` matrices of rows x cols elements (32 x 32 tiles through LDS: both sides coalesced)
void dsc_launch_transpose_last2(const void *in, void *out, int elem_bytes, long long batch, int rows, int cols, hipStream_t stream);
// any permutation that moves the last axis (n_dim <= 4, dense input): tiled through LDS, coalesced on both sides
bool dsc_launch_transpose_moving_last(const void *in, void *out, int elem_bytes, int n_dim, const int *shape, const int *in_stride, const int *perm,
                                      hipStream_t stream);
