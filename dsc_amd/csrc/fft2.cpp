// fft2.cpp — dsc_fft2 / dsc_ifft2 / dsc_rfft2 / dsc_irfft2 (include/dsc_mi355x.h, Section F): transforms over the last two axes,
// DEFINED as the composition of the 1-D operators (rows first for the forward real transform, columns first for the inverse one), so
// that every 1-D shape rule carries over.  Routes (dsc_last_fft_path):
//
//   fft2_regs / rfft2_regs        N0, N1 in {32, 64, 128} (rfft2: N1 in {64, 128, 256}): ONE pass, the image register resident
//                                 (fft_2d.hip).  Needs no intermediate: works in a context with room for x and out only.
//   fft2_composed / rfft2_composed / irfft2_composed
//                                 everything else, DSC_NO_FFT2_FUSED=1, and images whose group breaks the kernel's 31-bit buffer
//                                 offsets: the two 1-D operators in turn, the intermediate an arena temporary freed before returning.
//                                 dsc_irfft2 always takes this route.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

namespace {

enum fft2_kind { K_FFT2, K_IFFT2, K_RFFT2, K_IRFFT2 };

dsc_tensor *fft2_impl(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1, fft2_kind kind) {
    DSC_ASSERT(x != nullptr);
    if (x->n_dim < 2) DSC_LOG_FATAL("a 2-D transform needs at least 2 dimensions, got %d", x->n_dim);
    const bool cplx = dsc_is_complex(x->dtype), sp = dsc_is_single(x->dtype);
    if (kind == K_RFFT2 && cplx) DSC_LOG_FATAL("RFFT2 input must be real");
    if (kind == K_IRFFT2 && !cplx) DSC_LOG_FATAL("IRFFT2 input must be complex");
    const int h = x->shape[DSC_MAX_DIMS - 2], w = x->shape[DSC_MAX_DIMS - 1];
    if (h < 1 || w < 1) DSC_LOG_FATAL("a 2-D transform needs a non-empty image, got %d x %d", h, w);
    const int N0 = dsc_pow2_n(n0 > 0 ? n0 : h);
    int N1, out_w;
    if (kind == K_IRFFT2) {
        if ((n1 > 0 ? n1 : w) < 2) DSC_LOG_FATAL("IRFFT2 needs at least 2 bins along the last axis");
        N1 = 2 * dsc_pow2_n((n1 > 0 ? n1 : w) - 1);
        out_w = N1;
    } else {
        N1 = dsc_pow2_n(n1 > 0 ? n1 : w);
        if (kind == K_RFFT2 && N1 < 2) DSC_LOG_FATAL("RFFT2 needs at least 2 points along the last axis");
        out_w = kind == K_RFFT2 ? N1 / 2 + 1 : N1;
    }
    const dsc_dtype out_dtype = kind == K_IRFFT2 ? (sp ? DSC_F32 : DSC_F64) : (sp ? DSC_C32 : DSC_C64);
    int out_shape[DSC_MAX_DIMS];
    memcpy(out_shape, x->shape, sizeof(out_shape));
    out_shape[DSC_MAX_DIMS - 2] = N0;
    out_shape[DSC_MAX_DIMS - 1] = out_w;
    if (out != nullptr) {                                          // allocated late: the composed route leaves it to its second operator
        DSC_RESULT(out, ctx, x->n_dim, out_shape, out_dtype, "the result's dtype and shape [.., %d, %d]", N0, out_w);
        if (out->data == x->data && !((kind == K_FFT2 || kind == K_IFFT2) && cplx && h == N0 && w == N1))
            DSC_LOG_FATAL("in place only for a complex fft2 / ifft2 whose image already has the transform's size");
    }

    const long long n_img = (long long) x->ne / ((long long) h * w);
    const dsc_fft_mode mode = kind == K_RFFT2 ? DSC_MODE_R2C_PACKED : kind == K_IRFFT2 ? DSC_MODE_C2R_PACKED : cplx ? DSC_MODE_C2C : DSC_MODE_R2C_CAST;
    bool fused = !dsc_env_set("DSC_NO_FFT2_FUSED") && dsc_fft2_regs_supports(N0, N1, mode);
    if (fused) {
        // a workgroup addresses its images through one descriptor with 31-bit byte offsets
        const long long group_b = (long long) dsc_fft2_regs_group(N0, N1, mode, sp) * h * w * (long long) dsc_dtype_size(x->dtype);
        fused = group_b < 0x7f000000LL;
    }
    if (fused) {
        if (out == nullptr) out = dsc_new_tensor(ctx, x->n_dim, &out_shape[DSC_MAX_DIMS - x->n_dim], out_dtype, nullptr);
        const double scale = kind == K_IFFT2 ? 1.0 / ((double) N0 * (double) N1) : 1.0;
        dsc_launch_fft2_regs(x->data, out->data, n_img, N0, N1, h, w, mode, kind == K_IFFT2, sp, scale, ctx->stream);
        ctx->last_fft_path = kind == K_RFFT2 ? "rfft2_regs" : "fft2_regs";
        return out;
    }

    // the definition: two 1-D operators, the intermediate from the arena
    dsc_tensor *mid = nullptr;
    switch (kind) {
        case K_FFT2:
            mid = dsc_fft(ctx, x, nullptr, n1, -1);
            out = dsc_fft(ctx, mid, out, n0, -2);
            break;
        case K_IFFT2:
            mid = dsc_ifft(ctx, x, nullptr, n1, -1);
            out = dsc_ifft(ctx, mid, out, n0, -2);
            break;
        case K_RFFT2:
            mid = dsc_rfft(ctx, x, nullptr, n1, -1);
            out = dsc_fft(ctx, mid, out, n0, -2);
            break;
        case K_IRFFT2:
            mid = dsc_ifft(ctx, x, nullptr, n0, -2);
            out = dsc_irfft(ctx, mid, out, n1, -1);
            break;
    }
    dsc_tensor_free(ctx, mid);
    ctx->last_fft_path = kind == K_RFFT2 ? "rfft2_composed" : kind == K_IRFFT2 ? "irfft2_composed" : "fft2_composed";
    return out;
}

}  // namespace

extern "C" dsc_tensor *dsc_fft2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n0, n1);
    return fft2_impl(ctx, x, out, n0, n1, K_FFT2);
}
extern "C" dsc_tensor *dsc_ifft2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n0, n1);
    return fft2_impl(ctx, x, out, n0, n1, K_IFFT2);
}
extern "C" dsc_tensor *dsc_rfft2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n0, n1);
    return fft2_impl(ctx, x, out, n0, n1, K_RFFT2);
}
extern "C" dsc_tensor *dsc_irfft2(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n0, int n1) {
    DSC_TRACE_OP(ctx, "op;fft", x, nullptr, n0, n1);
    return fft2_impl(ctx, x, out, n0, n1, K_IRFFT2);
}
