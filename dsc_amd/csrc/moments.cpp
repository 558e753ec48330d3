// moments.cpp — dsc_sumsq / dsc_rms / dsc_var / dsc_std / dsc_vdot / dsc_detrend (include/dsc_mi355x.h, Section K): centred moments along
// one axis of a tensor viewed as [outer][n][inner].  Every sum is a double; the arithmetic is stated in the header of moments.hip.
//
//   dsc_sumsq    sum |x|^2, f32 / f64 / c32 / c64 -> f32 / f64             dsc_rms   sqrt(sumsq / n)
//   dsc_var      numpy.var(x, axis, ddof), centred on the computed mean    dsc_std   its square root
//   dsc_vdot     sum conj(a) b along the axis, a and b of one shape and dtype -> that dtype
//   dsc_detrend  scipy.signal.detrend(x, axis, type), x's shape and dtype
//
// Routes (dsc_last_fft_path), kernels in moments.hip; detrend_... for dsc_detrend:
//   moment_rows   inner == 1, at least kTilesBelowRows (1024) rows or rows of at most one tile: one launch, a wave or workgroup per row
//   moment_tiles  inner == 1, fewer rows than that: tile sums -> the statistic per row -> the centred pass per tile -> its sums per row,
//                 two to four plain launches on the context's stream and 32 bytes per tile of scratch
//   moment_cols   inner > 1: one thread per (outer, inner) element walks the axis; with few outputs the axis is cut into segments
// DSC_MOMENT_ROUTE=rows|tiles, read at every call, forces either route on any inner == 1 shape.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

namespace {

// inner == 1 with fewer rows than this (and rows longer than a tile) takes moment_tiles: the rows route gives a row to one workgroup, and
// the chip wants four of them per compute unit.  Measured on 2^26 f32 elements (profiles/moments_bench.txt), moment_tiles /
// moment_rows in time for sumsq, var, detrend: 0.51, 0.54, 0.65 at 256 rows, 0.85, 0.92, 0.78 at 512, 1.10, 0.93, 1.01 at 1024 and
// 1.11, 1.21, 1.05 at 2048.
constexpr long long kTilesBelowRows = 1024;

enum { K_SUMSQ = 0, K_VDOT = 1, K_VAR = 2, K_DETREND_C = 3, K_DETREND_L = 4 };      // the codes of moments.hip

// op: a code of moments.hip; y: the second operand of vdot; root: rms / std
dsc_tensor *moment_impl(dsc_ctx *ctx, const dsc_tensor *x, const dsc_tensor *y, dsc_tensor *out, int axis, bool keep_dims, int op,
                        int ddof, bool root) {
    DSC_ASSERT(x != nullptr);
    const dsc_axis_view v = dsc_axis_view_of(x, axis);
    const bool detrend = op >= K_DETREND_C;
    if (op == K_VDOT) {
        DSC_ASSERT(y != nullptr);
        if (y->dtype != x->dtype || y->n_dim != x->n_dim || memcmp(x->shape, y->shape, sizeof(x->shape)) != 0)
            DSC_LOG_FATAL("a and b must have one shape and dtype (no broadcasting)");
    }
    if (op == K_VAR && (ddof < 0 || ddof >= v.n)) DSC_LOG_FATAL("ddof must be in [0, n): got %d with %d elements along the axis", ddof, v.n);

    if (detrend) {
        DSC_RESULT(out, ctx, x->n_dim, x->shape, x->dtype, "the input's shape and dtype");
    } else {
        const dsc_dtype odt = op == K_VDOT ? x->dtype : x->dtype == DSC_C32 ? DSC_F32 : x->dtype == DSC_C64 ? DSC_F64 : x->dtype;
        int out_shape[DSC_MAX_DIMS];
        const int out_ndim = dsc_reduced_shape(x->shape, x->n_dim, v.slot, keep_dims, out_shape);
        DSC_RESULT(out, ctx, out_ndim, out_shape, odt, "the reduced shape (%s the axis) and the result's dtype", keep_dims ? "1 along" : "without");
    }
    DSC_NO_OVERLAP(out, x, "the input");
    if (y != nullptr) DSC_NO_OVERLAP(out, y, "the input");

    const char *const routes[2][3] = {{"moment_rows", "moment_tiles", "moment_cols"}, {"detrend_rows", "detrend_tiles", "detrend_cols"}};
    const void *yd = y != nullptr ? y->data : nullptr;
    if (v.inner > 1) {
        const size_t cap = ctx->scratch.capacity() > DSC_DEVICE_ALIGN ? ctx->scratch.capacity() - DSC_DEVICE_ALIGN : 0;
        const long long n_out = v.outer * v.inner;
        const int n_seg = dsc_moment_cols_segments(n_out, v.n, cap);
        const size_t need = n_seg > 1 ? dsc_moment_scratch_bytes(n_out, n_seg) : 0;
        DSC_SCRATCH_BLOCK(scratch, ctx, need, "the segment sums of %lld columns need %.2f MB", n_out, (double) need / 1048576.);
        dsc_launch_moment_cols(x->data, yd, out->data, op, x->dtype, v.outer, v.n, v.inner, ddof, root, n_seg, scratch.ptr, ctx->stream);
        ctx->last_fft_path = routes[detrend][2];
        return out;
    }
    const int tile_len = dsc_moment_tile_len(x->dtype);
    const int forced = dsc_forced_route("DSC_MOMENT_ROUTE", {"rows", "tiles"});
    if (forced >= 0 ? forced == 1 : v.outer < kTilesBelowRows && v.n > tile_len) {
        const size_t need = dsc_moment_scratch_bytes(v.outer, (v.n + tile_len - 1) / tile_len);
        DSC_SCRATCH_BLOCK(scratch, ctx, need, "the tile sums of %lld rows of %d need %.2f MB", v.outer, v.n, (double) need / 1048576.);
        dsc_launch_moment_tiles(x->data, yd, out->data, op, x->dtype, v.outer, v.n, ddof, root, scratch.ptr, ctx->stream);
        ctx->last_fft_path = routes[detrend][1];
    } else {
        dsc_launch_moment_rows(x->data, yd, out->data, op, x->dtype, v.outer, v.n, ddof, root, ctx->stream);
        ctx->last_fft_path = routes[detrend][0];
    }
    return out;
}

}  // namespace

extern "C" dsc_tensor *dsc_sumsq(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, 0, axis);
    return moment_impl(ctx, x, nullptr, out, axis, keep_dims, K_SUMSQ, 0, false);
}

extern "C" dsc_tensor *dsc_rms(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, 0, axis);
    return moment_impl(ctx, x, nullptr, out, axis, keep_dims, K_SUMSQ, 0, true);
}

extern "C" dsc_tensor *dsc_var(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, int ddof, bool keep_dims) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, ddof, axis);
    return moment_impl(ctx, x, nullptr, out, axis, keep_dims, K_VAR, ddof, false);
}

extern "C" dsc_tensor *dsc_std(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, int ddof, bool keep_dims) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, ddof, axis);
    return moment_impl(ctx, x, nullptr, out, axis, keep_dims, K_VAR, ddof, true);
}

extern "C" dsc_tensor *dsc_vdot(dsc_ctx *ctx, const dsc_tensor *a, const dsc_tensor *b, dsc_tensor *out, int axis, bool keep_dims) {
    DSC_TRACE_OP(ctx, "op;binary", a, b, 0, axis);
    return moment_impl(ctx, a, b, out, axis, keep_dims, K_VDOT, 0, false);
}

extern "C" dsc_tensor *dsc_detrend(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, dsc_detrend_type type) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, (int) type, axis);
    if (type != DSC_DETREND_CONSTANT && type != DSC_DETREND_LINEAR) DSC_LOG_FATAL("type must be DSC_DETREND_CONSTANT or DSC_DETREND_LINEAR, got %d", (int) type);
    return moment_impl(ctx, x, nullptr, out, axis, true, type == DSC_DETREND_LINEAR ? K_DETREND_L : K_DETREND_C, 0, false);
}
