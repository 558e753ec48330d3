// stft.cpp — dsc_stft / dsc_istft (include/dsc_mi355x.h, Section D): the short-time Fourier transform and its inverse, with
// torch.stft / torch.istft semantics (onesided, normalized=False, win_length == n_fft) and a frames-major layout
// [.., n_frames, n_fft/2 + 1] (= torch.stft(...).transpose(-2, -1)).  Routes (dsc_last_fft_path):
//
//   stft_regs      n_fft = 64 .. 32768: ONE pass — framing, reflect / zero padding and the window are done in the load of the
//                  packed-real register kernels (fft_regs_mid.hip), bins stored frame by frame
//   stft_composed  any other power of two, and DSC_NO_STFT_FUSED=1: a gather kernel writes [chunk][n_fft] windowed frames into
//                  the scratch arena (fft_stft.hip), the internal rfft routes transform them into the output rows
//   istft_ola      the internal irfft routes write chunks of frames into scratch, an overlap-add GATHER kernel (fft_stft.hip)
//                  writes every output sample once: window-weighted sum over the covering frames in frame order, divided by the
//                  squared-window envelope over the same frames, crop of n_fft/2 (center) and trim / zero fill to `length`
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

#include <cmath>
#include <vector>

namespace {

void check_common(int n_fft, int hop, const dsc_tensor *window, dsc_dtype real_dtype) {
    if (n_fft < 4 || n_fft > (1 << 20) || (n_fft & (n_fft - 1)) != 0)
        DSC_LOG_FATAL("n_fft must be a power of two in [4, 2^20], got %d", n_fft);
    if (hop < 1) DSC_LOG_FATAL("hop must be >= 1, got %d", hop);
    if (window != nullptr) {
        if (window->ne != n_fft) DSC_LOG_FATAL("window must have n_fft = %d elements, got %d", n_fft, window->ne);
        if (window->dtype != real_dtype) DSC_LOG_FATAL("window dtype must match the real dtype of the transform");
    }
}

// frames of the scratch chunk (nothing else pinned), leaving the inner transform routes room for two frames
long long chunk_frames(dsc_ctx *ctx, size_t frame_b, long long n_lines) {
    const size_t reserve = 2 * frame_b + 4 * DSC_DEVICE_ALIGN;
    const long long chunk = dsc_chunk_lines(ctx->scratch.capacity(), 0, frame_b, reserve, n_lines);
    if (chunk == 0)
        DSC_LOG_FATAL("scratch arena too small: a short-time transform of %zu-byte frames needs %.2f MB of scratch", frame_b,
                      (double) (frame_b + reserve) / 1048576.);
    return chunk;
}

// Smallest squared-window envelope env(p) = sum over frames f in [0, n_frames) with 0 <= p - f hop < n_fft of w2[p - f hop], over the
// padded positions p in [start, end) (end clipped to the last frame's end); +inf for an empty range, *at = where it is.  With
// W[k][r] = w2[r + k hop] (zero past n_fft), k < K = ceil(n_fft / hop), env(p) for q = p / hop, r = p % hop sums W[k][r] over
// k in [max(0, q - n_frames + 1), min(K - 1, q)]: a difference of prefix sums down column r (suffix sums where the range reaches the
// last row, plain prefix sums where it starts at 0, so that small tails lose nothing to cancellation).  Positions more than (K + 1) hop
// from both ends see every k, i.e. the periodic value W-column sum: one period of them stands for all.  dsc_amd/tensor.py
// (_nola_min) computes the same numbers in the same order.
double nola_min(const std::vector<double> &w2, int n_fft, int hop, long long n_frames, long long start, long long end, long long *at) {
    const long long expected = (long long) n_fft + (long long) hop * (n_frames - 1);
    if (end > expected) end = expected;
    double best = HUGE_VAL;
    *at = start;
    if (end <= start) return best;
    const long long K = (n_fft + (long long) hop - 1) / hop;
    std::vector<double> pre((size_t) (K + 1) * hop, 0.0), suf((size_t) (K + 1) * hop, 0.0);     // [k][r]
    auto W = [&](long long k, long long r) { const long long j = r + k * hop; return j < n_fft ? w2[(size_t) j] : 0.0; };
    for (long long r = 0; r < hop; ++r) {
        for (long long k = 0; k < K; ++k) pre[(size_t) ((k + 1) * hop + r)] = pre[(size_t) (k * hop + r)] + W(k, r);
        for (long long k = K - 1; k >= 0; --k) suf[(size_t) (k * hop + r)] = suf[(size_t) ((k + 1) * hop + r)] + W(k, r);
    }
    auto env = [&](long long p) {
        const long long q = p / hop, r = p % hop;
        const long long lo = q - n_frames + 1 > 0 ? q - n_frames + 1 : 0, hi = q < K - 1 ? q : K - 1;
        if (hi < lo) return 0.0;
        if (lo == 0) return pre[(size_t) ((hi + 1) * hop + r)];
        if (hi == K - 1) return suf[(size_t) (lo * hop + r)];
        return pre[(size_t) ((hi + 1) * hop + r)] - pre[(size_t) (lo * hop + r)];
    };
    auto visit = [&](long long p, double e) { if (e < best) { best = e; *at = p; } };
    const long long span = (K + 1) * hop;
    const long long h_end = end < start + span ? end : start + span;
    const long long t_start = end - span > h_end ? end - span : h_end;
    for (long long p = start; p < h_end; ++p) visit(p, env(p));
    for (long long p = t_start; p < end; ++p) visit(p, env(p));
    for (long long p = h_end; p < t_start && p < h_end + hop; ++p) visit(p, suf[(size_t) (p % hop)]);
    return best;
}

}  // namespace

extern "C" dsc_tensor *dsc_stft(dsc_ctx *ctx, const dsc_tensor *x, int n_fft, int hop, const dsc_tensor *window, bool center, int pad_mode,
                                dsc_tensor *out) {
    DSC_ASSERT(x != nullptr);
    dsc_trace_scope trace__(ctx, "dsc_stft", "op;fft", x, window, n_fft, hop);
    if (x->dtype != DSC_F32 && x->dtype != DSC_F64) DSC_LOG_FATAL("STFT input must be real");
    if (x->n_dim > 3) DSC_LOG_FATAL("STFT input has at most 3 dimensions, got %d", x->n_dim);
    check_common(n_fft, hop, window, x->dtype);
    if (pad_mode != 0 && pad_mode != 1) DSC_LOG_FATAL("pad_mode must be 0 (reflect) or 1 (constant), got %d", pad_mode);
    const int T = x->shape[DSC_MAX_DIMS - 1];
    const bool reflect = center && pad_mode == 0;
    if (reflect && T <= n_fft / 2) DSC_LOG_FATAL("reflect padding needs T > n_fft/2 (T = %d, n_fft = %d)", T, n_fft);
    if (!center && T < n_fft) DSC_LOG_FATAL("without center the input needs T >= n_fft (T = %d, n_fft = %d)", T, n_fft);
    const int pad = center ? n_fft / 2 : 0;
    const long long n_frames = 1 + ((long long) T + 2 * pad - n_fft) / hop;
    const int bins = n_fft / 2 + 1;
    const long long rows = x->ne / T;
    const long long n_lines = rows * n_frames;
    if (n_lines * bins > 0x7fffffffLL) DSC_LOG_FATAL("STFT output of %lld x %d bins exceeds the tensor size limit", n_lines, bins);

    const bool sp = x->dtype == DSC_F32;
    const dsc_dtype cdt = sp ? DSC_C32 : DSC_C64;
    int out_shape[DSC_MAX_DIMS];
    for (int i = 0; i < DSC_MAX_DIMS - 1; ++i) out_shape[i] = x->shape[i + 1];
    out_shape[DSC_MAX_DIMS - 2] = (int) n_frames;
    out_shape[DSC_MAX_DIMS - 1] = bins;
    DSC_RESULT(out, ctx, x->n_dim + 1, out_shape, cdt, "the input's complex dtype and shape [.., %lld, %d]", n_frames, bins);
    const size_t rb = sp ? 4 : 8, csz = 2 * rb;
    const void *w = window != nullptr ? window->data : nullptr;

    // fused: rows per launch such that every offset of the buffer descriptor over x (plus a frame past its end) fits 31 bits.  A row
    // too long for that takes the composed route below (64-bit gather indices) at any n_fft.
    const long long rows_per = dsc_fused_rows_per_launch(0x7f000000LL - (long long) n_fft * (long long) rb, (long long) T * (long long) rb, 0, rows, T & 1);
    if (!dsc_env_set("DSC_NO_STFT_FUSED") && dsc_stft_regs_supports(n_fft) && rows_per > 0) {
        const dsc_fft_plan *plan = dsc_plan_fft(ctx, n_fft / 2, DSC_FFT_REAL, cdt);
        for (long long r = 0; r < rows; r += rows_per) {
            const long long nr = rows - r < rows_per ? rows - r : rows_per;
            dsc_launch_stft_regs((const char *) x->data + (size_t) r * T * rb, w, (char *) out->data + (size_t) (r * n_frames) * bins * csz,
                                 nr * n_frames, n_fft, T, (int) n_frames, hop, pad, reflect, sp, (int) (nr * T * (long long) rb), plan->tw_full,
                                 plan->tw_real, ctx->stream);
        }
        ctx->last_fft_path = "stft_regs";
        return out;
    }

    // composed: frames of one chunk in a pinned scratch block, the rfft routes below it
    const size_t frame_b = (size_t) n_fft * rb;
    dsc_scratch_pin held(ctx);
    const long long chunk = chunk_frames(ctx, frame_b, n_lines);
    char *frames = held.alloc((size_t) chunk * frame_b);
    held.pin();
    for (long long q = 0; q < n_lines; q += chunk) {
        const int nl = (int) (n_lines - q < chunk ? n_lines - q : chunk);
        dsc_launch_stft_frames(x->data, w, frames, q, nl, n_fft, T, (int) n_frames, hop, pad, reflect, sp, ctx->stream);
        const int fshape[2] = {nl, n_fft}, bshape[2] = {nl, bins};
        dsc_scoped_view ft(ctx, frames, 2, fshape, x->dtype), bt(ctx, (char *) out->data + (size_t) q * bins * csz, 2, bshape, cdt);
        dsc_rfft(ctx, ft, bt, n_fft, -1);
    }
    ctx->last_fft_path = "stft_composed";
    return out;
}

extern "C" dsc_tensor *dsc_istft(dsc_ctx *ctx, const dsc_tensor *X, int n_fft, int hop, const dsc_tensor *window, bool center, int length,
                                 dsc_tensor *out) {
    DSC_ASSERT(X != nullptr);
    dsc_trace_scope trace__(ctx, "dsc_istft", "op;fft", X, window, n_fft, hop);
    if (X->dtype != DSC_C32 && X->dtype != DSC_C64) DSC_LOG_FATAL("ISTFT input must be complex");
    if (X->n_dim < 2) DSC_LOG_FATAL("ISTFT input must be [.., n_frames, n_fft/2 + 1]");
    const bool sp = X->dtype == DSC_C32;
    const dsc_dtype rdt = sp ? DSC_F32 : DSC_F64;
    check_common(n_fft, hop, window, rdt);
    const int bins = X->shape[DSC_MAX_DIMS - 1], n_frames = X->shape[DSC_MAX_DIMS - 2];
    if (bins != n_fft / 2 + 1) DSC_LOG_FATAL("ISTFT input has %d bins, n_fft = %d needs %d", bins, n_fft, n_fft / 2 + 1);
    const int pad = center ? n_fft / 2 : 0;
    const long long expected = (long long) n_fft + (long long) hop * (n_frames - 1);
    const long long natural = center ? expected - n_fft : expected;
    const long long len = length > 0 ? length : natural;
    if (len < 1 || len > 0x7fffffffLL) DSC_LOG_FATAL("ISTFT output length %lld out of range", len);
    const long long rows = X->ne / ((long long) n_frames * bins);
    if (rows * len > 0x7fffffffLL) DSC_LOG_FATAL("ISTFT output exceeds the tensor size limit");
    const size_t rb = sp ? 4 : 8, csz = 2 * rb;

    // NOLA: the squared-window envelope must not vanish where the output is read ([pad, pad + len), as far as frames reach).  One
    // SYNCHRONOUS n_fft-element copy of the window, then nola_min: O(n_fft + hop), not O(output length x frames per sample).
    {
        std::vector<double> w2(n_fft, 1.0);
        if (window != nullptr) {
            std::vector<char> host((size_t) n_fft * rb);
            HIP_CHECK(hipMemcpyAsync(host.data(), window->data, host.size(), hipMemcpyDeviceToHost, ctx->stream));
            dsc_stream_sync(ctx);
            for (int j = 0; j < n_fft; ++j) {
                const double v = sp ? (double) ((const float *) host.data())[j] : ((const double *) host.data())[j];
                w2[j] = v * v;
            }
        }
        long long at = 0;
        const double env = nola_min(w2, n_fft, hop, n_frames, pad, (long long) pad + len, &at);
        if (!(env >= 1e-11)) DSC_LOG_FATAL("window overlap-add envelope %.3g < 1e-11 at sample %lld: NOLA does not hold", env, at - pad);
    }

    int out_shape[DSC_MAX_DIMS];
    for (int i = 0; i < DSC_MAX_DIMS; ++i) out_shape[i] = i == 0 ? 1 : X->shape[i - 1];
    out_shape[DSC_MAX_DIMS - 1] = (int) len;
    DSC_RESULT(out, ctx, X->n_dim - 1, out_shape, rdt, "the input's real dtype and shape [.., %lld]", len);
    const void *w = window != nullptr ? window->data : nullptr;

    const size_t frame_b = (size_t) n_fft * rb;
    const long long n_lines = rows * n_frames;
    dsc_scratch_pin held(ctx);
    const long long chunk = chunk_frames(ctx, frame_b, n_lines);
    char *frames = held.alloc((size_t) chunk * frame_b);
    held.pin();
    // frames [first, first + n) of the flattened (row, frame) list -> the pinned block
    auto irfft_frames = [&](long long first, int n) {
        const int bshape[2] = {n, bins}, fshape[2] = {n, n_fft};
        dsc_scoped_view bt(ctx, (char *) X->data + (size_t) first * bins * csz, 2, bshape, X->dtype), ft(ctx, frames, 2, fshape, rdt);
        dsc_irfft(ctx, bt, ft, -1, -1);
    };
    const long long p_end = (long long) pad + len;
    if (n_frames <= chunk) {                                   // whole rows per chunk
        const long long rows_per = chunk / n_frames;
        for (long long r = 0; r < rows; r += rows_per) {
            const long long nr = rows - r < rows_per ? rows - r : rows_per;
            irfft_frames(r * n_frames, (int) (nr * n_frames));
            dsc_launch_istft_ola(frames, w, out->data, r, nr, 0, n_frames, n_fft, hop, n_frames, pad, 0, p_end, (int) len, sp, ctx->stream);
        }
    } else {                                                   // windows of frames within a row; each sees every frame covering its span
        const long long cover = (n_fft + hop - 1) / hop;
        if (chunk <= cover) DSC_LOG_FATAL("scratch arena too small: an ISTFT chunk must hold more than %lld frames", cover);
        for (long long r = 0; r < rows; ++r) {
            long long p = 0;
            while (p < p_end) {
                const long long fa = p < n_fft ? 0 : (p - n_fft) / hop + 1;   // first frame that covers p
                if (fa >= n_frames) {                                          // past the last frame: zeros
                    dsc_launch_istft_ola(frames, w, out->data, r, 1, n_frames, 0, n_fft, hop, n_frames, pad, p, p_end, (int) len, sp, ctx->stream);
                    break;
                }
                const long long fb = fa + chunk < n_frames ? fa + chunk : n_frames;
                const long long p1 = fb == n_frames ? p_end : fb * hop;       // frames >= fb start at or after fb hop
                irfft_frames(r * n_frames + fa, (int) (fb - fa));
                dsc_launch_istft_ola(frames, w, out->data, r, 1, (int) fa, (int) (fb - fa), n_fft, hop, n_frames, pad, p, p1, (int) len, sp,
                                     ctx->stream);
                p = p1;
            }
        }
    }
    ctx->last_fft_path = "istft_ola";
    return out;
}
