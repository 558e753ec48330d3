// hilbert.cpp — dsc_hilbert / dsc_envelope (include/dsc_mi355x.h, Section G): the analytic signal of every row of x [.., T] and its
// modulus, along the last axis (scipy.signal.hilbert(x, N) and its absolute value on power-of-two N).
//
// N = pow2(n > 0 ? n : T); x_used = the row cropped or zero padded to N samples; with H[0] = H[N/2] = 0 and H[k] = -i in between,
//   y = irfft(rfft(x_used, N) * H, N),   hilbert = x_used + i y,   envelope = sqrt(x_used^2 + y^2).
// The real part is a copy of x_used on every route.
//
// Routes (dsc_last_fft_path):
//   hilbert_regs / envelope_regs          N = 512 .. 32768: ONE pass.  The fused filter kernel (fft_regs_mid.hip) with the constant H (a swap
//                                         and a sign, nothing loaded) reads its sample pairs a second time after the inverse passes and
//                                         stores the complex pairs, or their moduli.
//   hilbert_composed / envelope_composed  every other N, rows the fused launch cannot address with 31-bit offsets, and
//                                         DSC_NO_HILBERT_FUSED=1: H is written into a pinned scratch block, rows go in chunks through
//                                         dsc_filter_fft into a pinned scratch chunk, and x_used and the chunk are zipped into out
//                                         (fft_hilbert.hip).  f32 rows of 131072 points and more are widened to f64 for the filter.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

#include <climits>

namespace {

constexpr int kF32WideMinN = 131072;                      // f32 rows from this length on are filtered in f64

dsc_tensor *hilbert_impl(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n, bool envelope) {
    DSC_ASSERT(x != nullptr);
    if (x->dtype != DSC_F32 && x->dtype != DSC_F64) DSC_LOG_FATAL("input must be real (f32 / f64)");
    const int T = x->shape[DSC_MAX_DIMS - 1];
    if ((n > 0 ? n : T) < 2) DSC_LOG_FATAL("the transform length must be at least 2, got %d", n > 0 ? n : T);
    const int N = dsc_pow2_n(n > 0 ? n : T);
    const long long rows = x->ne / T;
    if (rows * N > 0x7fffffffLL) DSC_LOG_FATAL("output exceeds the tensor size limit");

    const bool sp = x->dtype == DSC_F32;
    const dsc_dtype cdt = sp ? DSC_C32 : DSC_C64, odt = envelope ? x->dtype : cdt;
    const size_t rb = sp ? 4 : 8;
    // f32 rows of 131072 points and more — longer than any fused f32 filter kernel — are filtered in f64: an f32 transform of that length
    // leaves more than tau 8 ||x|| / sqrt(N) on the weak samples of a row whose energy sits in a few strong ones (a single impulse:
    // 1.34 of the envelope's bound at N = 131072, on this route and on the hand composition ifft(fft(x) * h) alike).  The real part
    // and the moduli still take x itself; y is rounded to f32 once, at the store.
    const bool wide = sp && N >= kF32WideMinN;
    // the plan first: its tables come from the main arena, and a context too tight for them must say so here, before anything is probed
    const dsc_fft_plan *plan = dsc_plan_fft(ctx, N / 2, DSC_FFT_REAL, wide ? DSC_F64 : x->dtype);
    int out_shape[DSC_MAX_DIMS];
    memcpy(out_shape, x->shape, sizeof(out_shape));
    out_shape[DSC_MAX_DIMS - 1] = N;
    DSC_RESULT(out, ctx, x->n_dim, out_shape, odt, "the %s dtype and shape [.., %d]", envelope ? "input's" : "input's complex", N);
    DSC_NO_OVERLAP(out, x, "x");
    if (rows == 0) return out;
    const int in_len = T < N ? T : N;

    // fused: a workgroup holds up to 64 rows and addresses their samples with 31-bit byte offsets from its first row — 64 T elem < 2^30,
    // the condition of dsc_filter_fft.  Its rows of out are 2 N elem each and a group's transform lengths add up to at most 2^15
    // points: 1 MiB of output per group, always addressable.
    if (!dsc_env_set("DSC_NO_HILBERT_FUSED") && dsc_hilbert_regs_supports(N) && (long long) T * 8 * 64 < (1LL << 30)) {
        dsc_launch_hilbert_regs(x->data, out->data, rows, N, envelope, sp, plan->tw_full, plan->tw_real, T, in_len, ctx->stream);
        ctx->last_fft_path = envelope ? "envelope_regs" : "hilbert_regs";
        return out;
    }

    // composed: H and a chunk of filtered rows in pinned scratch; the inner routes keep room for two more rows.  wide: the chunk's rows
    // are widened to f64 (in_len samples, the pitch rounded up to even: the spare sample is a zero of the padding) next to it, and H
    // and the filtered rows are f64 / c64.
    const dsc_dtype fdt = wide ? DSC_F64 : x->dtype, fcdt = wide ? DSC_C64 : cdt;
    const size_t frb = wide ? 8 : rb;
    const int bins = N / 2 + 1, wpitch = in_len + (in_len & 1);
    const size_t y_b = (size_t) N * frb, w_b = wide ? (size_t) wpitch * frb : 0, frame_b = y_b + w_b, h_b = (size_t) bins * 2 * frb;
    const size_t reserve = 2 * y_b + 4 * DSC_DEVICE_ALIGN;
    dsc_scratch_pin held(ctx);
    // rounded before it is bounded by the rows, hence no bound in the call
    long long chunk = dsc_chunk_lines(ctx->scratch.capacity(), h_b + 3 * DSC_DEVICE_ALIGN, frame_b, reserve, LLONG_MAX);
    if (chunk == 0)
        DSC_LOG_FATAL("scratch arena too small: an analytic signal of %d points needs %.2f MB of scratch", N,
                      (double) (h_b + frame_b + 2 * y_b) / 1048576.);
    if (chunk > 4) chunk &= ~3LL;                                  // chunks start on whole 16-byte packs of out whatever N
    if (chunk > rows) chunk = rows;
    char *Hb = held.alloc(h_b);
    char *filtered = held.alloc((size_t) chunk * y_b);
    char *widened = wide ? held.alloc((size_t) chunk * w_b) : nullptr;
    held.pin();
    dsc_launch_hilbert_response(Hb, N, !wide && sp, ctx->stream);
    dsc_scoped_view Ht(ctx, Hb, 1, &bins, fcdt);
    for (long long q = 0; q < rows; q += chunk) {
        const int nl = (int) (rows - q < chunk ? rows - q : chunk);
        const int xshape[2] = {nl, wide ? wpitch : T}, yshape[2] = {nl, N};
        if (wide) dsc_launch_hilbert_widen(x->data, widened, q, nl, T, in_len, wpitch, ctx->stream);
        dsc_scoped_view xt(ctx, wide ? widened : (char *) x->data + (size_t) q * T * rb, 2, xshape, fdt), yt(ctx, filtered, 2, yshape, fdt);
        dsc_filter_fft(ctx, xt, Ht, yt);
        dsc_launch_hilbert_zip(x->data, filtered, out->data, q, nl, N, T, in_len, envelope, sp, wide, ctx->stream);
    }
    ctx->last_fft_path = envelope ? "envelope_composed" : "hilbert_composed";
    return out;
}

}  // namespace

extern "C" dsc_tensor *dsc_hilbert(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n, 0);
    return hilbert_impl(ctx, x, out, n, false);
}

extern "C" dsc_tensor *dsc_envelope(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n, 0);
    return hilbert_impl(ctx, x, out, n, true);
}
