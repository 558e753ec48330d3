// resample.cpp — dsc_upfirdn / dsc_resample_poly / dsc_decimate / dsc_firwin (include/dsc_mi355x.h, Section H): polyphase FIR
// resampling along the last axis of real x [.., T] with one real filter h [M] (scipy.signal.upfirdn, resample_poly, decimate with
// ftype='fir', and the low-pass firwin they are built on).
//
// All three operators are one primitive P(x, h, gain, up, down, t0, T_out):
//   y[r][m] = sum_i (h[t - i up] gain) x[r][i],   t = m down + t0 (64-bit),   over 0 <= i < T and 0 <= t - i up < M;   0 <= m < T_out
//   upfirdn(h, x, up, down)         gain 1,  t0 0,         T_out = ceil(((T - 1) up + M) / down)
//   resample_poly(x, up, down, h)   gain up, t0 half_len,  T_out = ceil(T up / down), after up and down are divided by their gcd;
//                                   h = firwin(2 half_len + 1, 1 / max(up, down), kaiser 5), half_len = 10 max(up, down), or the caller's
//                                   taps with half_len = (M - 1) / 2.  scipy pads h in front and drops the first outputs, which is t0.
//   decimate(x, q, n)               resample_poly(x, 1, q, firwin(n + 1, 1 / q, hamming)), n = 20 q when n <= 0
//
// One route (dsc_last_fft_path "polyphase_direct"): the direct kernel of polyphase.hip, one HBM round trip, nothing rounded to a power
// of two, no scratch.  resample_poly whose reduced rate pair is 1 / 1 copies x ("polyphase_copy"), scipy's early return.
//
// The design.  dsc_firwin_host designs in long double — h[k] = cutoff sinc(cutoff (k - alpha)) w[k] / sum, I0 of the Kaiser window from its
// power series — and rounds to double; dsc_firwin rounds once more to the dtype and uploads on the context's stream, as dsc_randn does.
// The designed taps of resample_poly / decimate are NOT cached between calls: they live in the main arena, which dsc_ctx_clear empties
// under any cache, the design is O(M) host work (M <= 3201 for rates up to 160) and the upload a few KB; a caller who resamples many
// buffers at one rate designs once with dsc_firwin and passes `taps`.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

#include <cmath>
#include <vector>

namespace {

long double bessel_i0(long double v) {                        // sum_k ((v / 2)^2)^k / (k!)^2
    const long double q = v * v / 4;
    long double term = 1, sum = 1;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((long double) k * k);
        sum += term;
        if (term < 1e-22L * sum) break;
    }
    return sum;
}

int gcd_of(int a, int b) {
    while (b != 0) { const int t = a % b; a = b; b = t; }
    return a;
}

void check_real(const dsc_tensor *x) {
    if (x->dtype != DSC_F32 && x->dtype != DSC_F64) DSC_LOG_FATAL("input must be real (f32 / f64)");
}

void check_filter(const dsc_tensor *x, const dsc_tensor *h) {
    if (h->dtype != x->dtype) DSC_LOG_FATAL("filter dtype must match the input dtype");
    if (h->n_dim != 1) DSC_LOG_FATAL("filter must be 1-D, got %d dimensions", h->n_dim);
    if (h->ne < 1) DSC_LOG_FATAL("filter must have at least one tap");
}

// out [.., T_out] of x's dtype: allocated, or the caller's checked
dsc_tensor *result_of(dsc_ctx *ctx, const dsc_tensor *x, long long T_out, dsc_tensor *out) {
    const int T = x->shape[DSC_MAX_DIMS - 1];
    const long long rows = x->ne / T;
    if (T_out > 0x7fffffffLL || rows * T_out > 0x7fffffffLL) DSC_LOG_FATAL("output exceeds the tensor size limit of 2^31 - 1 elements");
    int out_shape[DSC_MAX_DIMS];
    memcpy(out_shape, x->shape, sizeof(out_shape));
    out_shape[DSC_MAX_DIMS - 1] = (int) T_out;
    DSC_RESULT(out, ctx, x->n_dim, out_shape, x->dtype, "the input's dtype and shape [.., %lld]", T_out);
    DSC_NO_OVERLAP(out, x, "x");
    return out;
}

// the primitive P of the file header; x, h and the rates are checked by the caller
dsc_tensor *polyphase(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *h, double gain, int up, int down, long long t0, long long T_out,
                      dsc_tensor *out) {
    const int T = x->shape[DSC_MAX_DIMS - 1], M = h->ne;
    out = result_of(ctx, x, T_out, out);
    DSC_NO_OVERLAP(out, h, "the filter");                          // every workgroup reads h while others already write
    const long long rows = x->ne / T;
    if (!dsc_launch_polyphase(x->data, h->data, out->data, rows, T, T_out, M, up, down, t0, gain, x->dtype == DSC_F32, ctx->stream))
        DSC_LOG_FATAL("up = %d, down = %d with %d taps: the taps and the samples of a 64-output tile exceed the %zu KiB of LDS", up, down, M,
                      dsc_polyphase_lds_limit() >> 10);
    ctx->last_fft_path = "polyphase_direct";
    return out;
}

dsc_tensor *resample_impl(dsc_ctx *ctx, const dsc_tensor *x, int up, int down, const dsc_tensor *taps, dsc_tensor *out) {
    const int g = gcd_of(up, down);
    up /= g;
    down /= g;
    const int T = x->shape[DSC_MAX_DIMS - 1];
    if (up == 1 && down == 1) {                                    // scipy's early return: a copy
        out = result_of(ctx, x, T, out);
        HIP_CHECK(hipMemcpyAsync(out->data, x->data, (size_t) x->ne * dsc_dtype_size(x->dtype), hipMemcpyDeviceToDevice, ctx->stream));
        ctx->last_fft_path = "polyphase_copy";
        return out;
    }
    const long long T_out = ((long long) T * up + down - 1) / down;
    if (taps != nullptr) return polyphase(ctx, x, taps, (double) up, up, down, (taps->ne - 1) / 2, T_out, out);
    const int rate = up > down ? up : down;
    if (rate > (0x7fffffff - 1) / 20) DSC_LOG_FATAL("up = %d, down = %d: the designed filter has too many taps", up, down);
    const int half_len = 10 * rate;
    dsc_tensor *h = dsc_firwin(ctx, 2 * half_len + 1, 1.0 / rate, 1, 5.0, x->dtype);
    out = polyphase(ctx, x, h, (double) up, up, down, half_len, T_out, out);
    dsc_tensor_free(ctx, h);                                       // the stream is in order: the block is not reused before the kernel has read it
    return out;
}

}  // namespace

extern "C" void dsc_firwin_host(double *taps, int numtaps, double cutoff, int window, double beta) {
    DSC_ASSERT(taps != nullptr);
    if (numtaps < 1) DSC_LOG_FATAL("numtaps must be at least 1, got %d", numtaps);
    if (!(cutoff > 0 && cutoff < 1)) DSC_LOG_FATAL("cutoff must lie strictly between 0 and 1 (the Nyquist frequency), got %g", cutoff);
    if (window != 0 && window != 1) DSC_LOG_FATAL("window must be 0 (hamming) or 1 (kaiser), got %d", window);
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double alpha = (numtaps - 1) / 2.0L, fc = cutoff;
    const long double i0_beta = window == 1 ? bessel_i0(beta) : 1;
    std::vector<long double> h((size_t) numtaps);
    long double sum = 0;
    for (int k = 0; k < numtaps; ++k) {
        const long double m = k - alpha, arg = pi * fc * m;
        const long double s = arg == 0 ? 1 : sinl(arg) / arg;
        long double w = 1;
        if (numtaps > 1) {
            if (window == 0) {
                w = 0.54L - 0.46L * cosl(2 * pi * k / (numtaps - 1));
            } else {
                const long double r = m / alpha, under = 1 - r * r;
                w = bessel_i0(beta * sqrtl(under > 0 ? under : 0)) / i0_beta;
            }
        }
        h[k] = fc * s * w;
        sum += h[k];
    }
    for (int k = 0; k < numtaps; ++k) taps[k] = (double) (h[k] / sum);
}

extern "C" dsc_tensor *dsc_firwin(dsc_ctx *ctx, int numtaps, double cutoff, int window, double beta, dsc_dtype dtype) {
    DSC_TRACE_OP(ctx, "op;creation", nullptr, nullptr, numtaps, window);
    if (dtype != DSC_F32 && dtype != DSC_F64) DSC_LOG_FATAL("dtype must be real");
    if (numtaps < 1) DSC_LOG_FATAL("numtaps must be at least 1, got %d", numtaps);
    std::vector<double> h((size_t) numtaps);
    dsc_firwin_host(h.data(), numtaps, cutoff, window, beta);
    dsc_tensor *out = dsc_tensor_1d(ctx, dtype, numtaps);
    if (dtype == DSC_F32) {
        std::vector<float> hf(h.begin(), h.end());                  // the one rounding to the dtype
        dsc_copy_from_host(ctx, out, hf.data(), hf.size() * sizeof(float));
    } else {
        dsc_copy_from_host(ctx, out, h.data(), h.size() * sizeof(double));
    }
    return out;
}

extern "C" dsc_tensor *dsc_upfirdn(dsc_ctx *ctx, const dsc_tensor *h, const dsc_tensor *x, int up, int down, dsc_tensor *out) {
    DSC_TRACE_OP(ctx, "op;fft", x, h, up, down);
    DSC_ASSERT(x != nullptr && h != nullptr);
    check_real(x);
    if (up < 1 || down < 1) DSC_LOG_FATAL("up and down must be at least 1, got up = %d, down = %d", up, down);
    check_filter(x, h);
    const long long T = x->shape[DSC_MAX_DIMS - 1];
    const long long T_out = ((T - 1) * up + h->ne + down - 1) / down;
    return polyphase(ctx, x, h, 1.0, up, down, 0, T_out, out);
}

extern "C" dsc_tensor *dsc_resample_poly(dsc_ctx *ctx, const dsc_tensor *x, int up, int down, const dsc_tensor *taps, dsc_tensor *out) {
    DSC_TRACE_OP(ctx, "op;fft", x, taps, up, down);
    DSC_ASSERT(x != nullptr);
    check_real(x);
    if (up < 1 || down < 1) DSC_LOG_FATAL("up and down must be at least 1, got up = %d, down = %d", up, down);
    if (taps != nullptr) check_filter(x, taps);
    return resample_impl(ctx, x, up, down, taps, out);
}

extern "C" dsc_tensor *dsc_decimate(dsc_ctx *ctx, const dsc_tensor *x, int q, int n, dsc_tensor *out) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, q, n);
    DSC_ASSERT(x != nullptr);
    check_real(x);
    if (q < 2) DSC_LOG_FATAL("the decimation factor must be at least 2, got %d", q);
    if (n <= 0) {
        if (q > (0x7fffffff - 1) / 20) DSC_LOG_FATAL("q = %d: the designed filter has too many taps", q);
        n = 20 * q;
    }
    if (n == 0x7fffffff) DSC_LOG_FATAL("n = %d: the filter has too many taps", n);
    dsc_tensor *h = dsc_firwin(ctx, n + 1, 1.0 / q, 0, 0.0, x->dtype);
    out = resample_impl(ctx, x, 1, q, h, out);
    dsc_tensor_free(ctx, h);
    return out;
}
