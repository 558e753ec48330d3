// conv.cpp — dsc_convolve / dsc_correlate (include/dsc_mi355x.h, Section E): linear convolution of every row of x [.., T] with one
// real filter h [M] by overlap-save, in modes full / same / valid (numpy.convolve's, scipy.signal.fftconvolve's along the last axis).
//
// Block plan.  D = M - 1 rounded up to even, blocks of n = 2^k points, hop = n - D; block b of a row is the frame x[n0 + b hop - D + i],
// i < n (zero outside [0, T)); irfft(rfft(frame) * H), H = rfft(h, n), is linear at samples [D, n), which are out[b hop + j - D].
// n_blocks = ceil(T_out / hop).  n minimises c(n) n / (n - D), the time per output sample, over n in [max(512, 2 D), 32768] (the smallest
// n on ties); c(n) is the fused kernel's measured time per block sample, per dtype (kSampleCost).  f64 stays at n <= 8192, where its
// kernels do not spill, whenever D <= 4096.  When one block of the chosen size covers the row, the smallest n >= T_out + D instead.
// Past 32768 (D > 16384, composed route) c(n) = log2 n: transform work.
//
// Routes (dsc_last_fft_path):
//   conv_regs      D <= 16384: ONE pass.  The fused filter kernel (fft_regs_mid.hip) loads the blocks straight from x through the
//                  stft frame path and stores only the kept samples of each block into out.
//   conv_composed  D > 16384, rows too long for the fused kernel's 31-bit buffer offsets, and DSC_NO_CONV_FUSED=1: blocks are
//                  gathered into a pinned scratch chunk (fft_stft.hip), filtered by dsc_filter_fft into a second one, and the kept
//                  samples scattered to out (fft_conv.hip).
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

namespace {

constexpr int kFusedMaxN = 32768;

int ilog2(long long n) {
    int l = 0;
    while ((1LL << l) < n) ++l;
    return l;
}

// c(n), n = 512 .. 32768: time per block sample of conv_regs, in ps, f32 and f64 ([64, 2^20], M = 63, where hop ~ n: ms / (n / hop) /
// 2^26 samples; tools/bench_conv.py --sweep, profiles/conv_sweep.txt and conv_sweep_f64.txt).  Not n log2 n: below 2048 points the short
// lines cost more per sample than their transform work says, and 16384 runs slower than 32768.
constexpr double kSampleCost[2][7] = {{3.71, 2.97, 2.24, 2.19, 2.43, 2.94, 2.66}, {6.12, 4.61, 4.00, 4.42, 4.84, 6.80, 6.16}};
// f64 blocks of 16384 and 32768 points spill (28 and 2 VGPRs, like the plain f64 filter kernel at those sizes): f64 takes them only when
// no block of at most 8192 points can hold the discard (D > 4096)
constexpr int kF64NoSpillMaxN = 8192;

// The block rule of the file header.  n_max bounds the search (the fused kernels stop at 32768; the composed route searches up to
// 2^20, or 2 D where that is more).  DSC_CONV_N (a power of two in [max(512, 2 D), n_max]) overrides it: tools/bench_conv.py --sweep.
int block_n(int D, long long T_out, int n_max, bool f64) {
    int n_min = 512;
    while (n_min < 2 * D) n_min *= 2;
    if (n_max < n_min) n_max = n_min;
    if (const char *e = getenv("DSC_CONV_N")) {
        const int n = atoi(e);
        if (n < n_min || n > n_max || (n & (n - 1)) != 0)
            DSC_LOG_FATAL("DSC_CONV_N = %s: the block size must be a power of two in [%d, %d] here", e, n_min, n_max);
        return n;
    }
    if (f64 && n_min <= kF64NoSpillMaxN && n_max > kF64NoSpillMaxN) n_max = kF64NoSpillMaxN;
    int best = n_min;
    double best_cost = 0;
    for (int n = n_min; n <= n_max; n *= 2) {
        const double c = n <= kFusedMaxN ? kSampleCost[f64][ilog2(n) - 9] : (double) ilog2(n);
        const double cost = c * n / (double) (n - D);
        if (n == n_min || cost < best_cost) { best = n; best_cost = cost; }
    }
    if (T_out + D <= best) {                                       // one block per row: no larger than the row needs
        int n = n_min;
        while (n < T_out + D) n *= 2;
        best = n;
    }
    return best;
}

dsc_tensor *conv_impl(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, int mode, dsc_tensor *out, bool reverse) {
    DSC_ASSERT(x != nullptr && h != nullptr);
    if (x->dtype != DSC_F32 && x->dtype != DSC_F64) DSC_LOG_FATAL("convolution input must be real (f32 / f64)");
    if (h->dtype != x->dtype) DSC_LOG_FATAL("filter dtype must match the input dtype");
    if (x->n_dim > 3) DSC_LOG_FATAL("convolution input has at most 3 dimensions, got %d", x->n_dim);
    if (h->n_dim != 1) DSC_LOG_FATAL("filter must be 1-D, got %d dimensions", h->n_dim);
    if (mode < 0 || mode > 2) DSC_LOG_FATAL("mode must be 0 (full), 1 (same) or 2 (valid), got %d", mode);
    const int T = x->shape[DSC_MAX_DIMS - 1], M = h->ne;
    if (M < 1) DSC_LOG_FATAL("filter must have at least one tap");
    if (mode == 2 && M > T) DSC_LOG_FATAL("valid mode needs M <= T (M = %d, T = %d)", M, T);
    const long long n0 = mode == 0 ? 0 : mode == 1 ? (M - 1) / 2 : M - 1;
    const long long T_out = mode == 0 ? (long long) T + M - 1 : mode == 1 ? T : (long long) T - M + 1;
    const long long rows = x->ne / T;
    if (T_out > 0x7fffffffLL || rows * T_out > 0x7fffffffLL) DSC_LOG_FATAL("convolution output exceeds the tensor size limit");

    const bool sp = x->dtype == DSC_F32;
    const dsc_dtype cdt = sp ? DSC_C32 : DSC_C64;
    const size_t rb = sp ? 4 : 8, csz = 2 * rb;
    int out_shape[DSC_MAX_DIMS];
    memcpy(out_shape, x->shape, sizeof(out_shape));
    out_shape[DSC_MAX_DIMS - 1] = (int) T_out;
    DSC_RESULT(out, ctx, x->n_dim, out_shape, x->dtype, "the input's dtype and shape [.., %lld]", T_out);
    DSC_NO_OVERLAP(out, x, "x");
    if (rows == 0) return out;

    const int D = (M - 1) + ((M - 1) & 1);
    const int pad = D - (int) n0;                                  // block b starts at b hop - pad
    // fused: rows per launch such that every byte offset into x (one spare row, plus a block past its end) and into out fits 31 bits
    const long long rows_per = dsc_fused_rows_per_launch(0x7f000000LL - (long long) kFusedMaxN * (long long) rb, (long long) T * (long long) rb,
                                                         T_out * (long long) rb, rows, (T | T_out) & 1);
    const bool fused = !dsc_env_set("DSC_NO_CONV_FUSED") && D <= kFusedMaxN / 2 && rows_per > 0;
    const int n = block_n(D, T_out, D <= kFusedMaxN / 2 ? kFusedMaxN : 1 << 20, !sp);
    const int hop = n - D;
    const long long n_blocks = (T_out + hop - 1) / hop;
    const int bins = n / 2 + 1;

    // H = rfft(h, n) (h reversed for correlate) in a pinned scratch block, with the composed route's two chunks next to it
    dsc_scratch_pin held(ctx);
    const size_t capacity = ctx->scratch.capacity();
    char *Hb = held.alloc((size_t) bins * csz);
    char *hr = reverse ? held.alloc((size_t) M * rb) : nullptr;
    const size_t frame_b = (size_t) n * rb;
    long long chunk = 0;
    char *frames = nullptr, *filtered = nullptr;
    const long long n_lines = rows * n_blocks;
    if (!fused) {
        // two blocks per chunk line (frames, filtered frames) next to H and the reversed taps; the inner routes keep two more frames
        const size_t fixed = (size_t) bins * csz + (reverse ? (size_t) M * rb : 0) + 2 * DSC_DEVICE_ALIGN;
        const size_t reserve = 2 * frame_b + 4 * DSC_DEVICE_ALIGN;
        chunk = dsc_chunk_lines(capacity, fixed, 2 * frame_b, reserve, n_lines);
        // dsc_convolve is charged the reversed taps here too, though it allocates none: the threshold it has always had
        if (chunk == 0 || capacity < fixed + (reverse ? 0 : (size_t) M * rb) + 2 * frame_b + reserve)
            DSC_LOG_FATAL("scratch arena too small: a convolution in %d-point blocks needs %.2f MB of scratch", n,
                          (double) ((size_t) bins * csz + (size_t) M * rb + 4 * frame_b) / 1048576.);
        frames = held.alloc((size_t) chunk * frame_b);
        filtered = held.alloc((size_t) chunk * frame_b);
    }
    held.pin();
    dsc_scoped_view Ht(ctx, Hb, 1, &bins, cdt);
    if (reverse) {
        dsc_launch_reverse(h->data, hr, M, sp, ctx->stream);
        dsc_scoped_view hrt(ctx, hr, 1, &M, x->dtype);
        dsc_rfft(ctx, hrt, Ht, n, -1);
    } else {
        dsc_rfft(ctx, h, Ht, n, -1);
    }

    if (fused) {
        DSC_ASSERT(dsc_conv_regs_supports(n));
        const dsc_fft_plan *plan = dsc_plan_fft(ctx, n / 2, DSC_FFT_REAL, x->dtype);
        for (long long r = 0; r < rows; r += rows_per) {
            const long long nr = rows - r < rows_per ? rows - r : rows_per;
            dsc_launch_conv_regs((const char *) x->data + (size_t) r * T * rb, Hb, (char *) out->data + (size_t) (r * T_out) * rb, nr * n_blocks, n, T,
                                 (int) n_blocks, hop, pad, D, (int) T_out, sp, (int) (nr * T * (long long) rb), (int) (nr * T_out * (long long) rb),
                                 plan->tw_full, plan->tw_real, ctx->stream);
        }
        ctx->last_fft_path = "conv_regs";
        return out;
    }

    for (long long q = 0; q < n_lines; q += chunk) {
        const int nl = (int) (n_lines - q < chunk ? n_lines - q : chunk);
        dsc_launch_stft_frames(x->data, nullptr, frames, q, nl, n, T, (int) n_blocks, hop, pad, false, sp, ctx->stream);
        const int fshape[2] = {nl, n};
        dsc_scoped_view ft(ctx, frames, 2, fshape, x->dtype), yt(ctx, filtered, 2, fshape, x->dtype);
        dsc_filter_fft(ctx, ft, Ht, yt);
        dsc_launch_conv_crop(filtered, out->data, q, nl, n, D, (int) n_blocks, T_out, sp, ctx->stream);
    }
    ctx->last_fft_path = "conv_composed";
    return out;
}

}  // namespace

extern "C" dsc_tensor *dsc_convolve(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, int mode, dsc_tensor *out) {
    DSC_TRACE_OP(ctx, "op;fft", x, h, mode, 0);
    return conv_impl(ctx, x, h, mode, out, false);
}

extern "C" dsc_tensor *dsc_correlate(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, int mode, dsc_tensor *out) {
    DSC_TRACE_OP(ctx, "op;fft", x, h, mode, 0);
    return conv_impl(ctx, x, h, mode, out, true);
}
