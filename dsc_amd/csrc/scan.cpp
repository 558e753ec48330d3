// scan.cpp — dsc_cumsum / dsc_diff / dsc_unwrap / dsc_phase (include/dsc_mi355x.h, Section I): prefix scans along one axis of a tensor
// viewed as [outer][n][inner], and the first difference that undoes them.
//
//   dsc_cumsum  numpy.cumsum(x, axis), f32 / f64 / c32 / c64, accumulated in x's dtype
//   dsc_diff    numpy.diff(x, 1, axis): out[j] = x[j + 1] - x[j], the axis one shorter
//   dsc_unwrap  numpy.unwrap(x, axis=axis) by integers: m[j] = the whole periods in x[j] - x[j - 1] (0 for |step| <= pi or a step that is
//               not finite; otherwise the integer nearest to step / 2 pi, ties toward zero), K = the exact int32 scan of m, and
//               out[j] = x[j] - K[j] 2 pi in double, rounded once.  f32 / f64
//   dsc_phase   dsc_unwrap(dsc_angle(z)) in one pass: the angle is formed in the load, c32 / c64 -> f32 / f64
//
// Routes (dsc_last_fft_path), kernels in scan.hip:
//   scan_rows   inner == 1, at least kTilesBelowRows (128) rows or rows of at most one tile: one launch, one workgroup per row at a time
//   scan_tiles  inner == 1, fewer rows than that: tile totals -> their scan per row -> the tiles with their carry-in, three plain
//               launches on the context's stream and two words per tile of scratch
//   scan_cols   inner > 1: one thread per (outer, inner) element walks the axis
//   scan_diff   dsc_diff, element-wise
// DSC_SCAN_ROUTE=rows|tiles, read at every call, forces either route on any inner == 1 shape.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

namespace {

// inner == 1 with fewer rows than this (and rows longer than a tile) takes scan_tiles.  Measured on 2^26 elements (profiles/scan_bench.txt,
// DESIGN 4.10): scan_tiles / scan_rows = 0.63 (cumsum f32) and 0.53 (unwrap f32) at 64 rows, 1.07 and 1.01 at 128, 1.46 and 1.50 at 192.
constexpr long long kTilesBelowRows = 128;

// out of dtype odt and x's shape with n_out along the axis: allocated, or the caller's checked
dsc_tensor *result_of(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, dsc_dtype odt, const dsc_axis_view &v, int n_out) {
    int out_shape[DSC_MAX_DIMS];
    memcpy(out_shape, x->shape, sizeof(out_shape));
    out_shape[v.slot] = n_out;
    DSC_RESULT(out, ctx, x->n_dim, out_shape, odt, "the result's dtype and shape (%d along the axis)", n_out);
    DSC_NO_OVERLAP(out, x, "the input");
    return out;
}

// op: 0 cumsum, 1 unwrap, 2 phase (the codes of scan.hip)
dsc_tensor *scan_impl(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, int op) {
    DSC_ASSERT(x != nullptr);
    if (op == 1 && x->dtype != DSC_F32 && x->dtype != DSC_F64) DSC_LOG_FATAL("input must be real (f32 / f64)");
    if (op == 2 && x->dtype != DSC_C32 && x->dtype != DSC_C64) DSC_LOG_FATAL("input must be complex (c32 / c64)");
    const dsc_axis_view v = dsc_axis_view_of(x, axis);
    const dsc_dtype odt = op != 2 ? x->dtype : x->dtype == DSC_C32 ? DSC_F32 : DSC_F64;
    out = result_of(ctx, x, out, odt, v, v.n);

    if (v.inner > 1) {
        dsc_launch_scan_cols(x->data, out->data, op, x->dtype, v.outer, v.n, v.inner, ctx->stream);
        ctx->last_fft_path = "scan_cols";
        return out;
    }
    const int forced = dsc_forced_route("DSC_SCAN_ROUTE", {"rows", "tiles"});
    if (forced >= 0 ? forced == 1 : v.outer < kTilesBelowRows && v.n > dsc_scan_tile_len(op, x->dtype)) {
        const size_t need = dsc_scan_tiles_scratch_bytes(op, x->dtype, v.outer, v.n);
        DSC_SCRATCH_BLOCK(scratch, ctx, need, "the tile totals of %lld rows of %d need %.2f MB", v.outer, v.n, (double) need / 1048576.);
        dsc_launch_scan_tiles(x->data, out->data, op, x->dtype, v.outer, v.n, scratch.ptr, ctx->stream);
        ctx->last_fft_path = "scan_tiles";
    } else {
        dsc_launch_scan_rows(x->data, out->data, op, x->dtype, v.outer, v.n, ctx->stream);
        ctx->last_fft_path = "scan_rows";
    }
    return out;
}

}  // namespace

extern "C" dsc_tensor *dsc_cumsum(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, 0, axis);
    return scan_impl(ctx, x, out, axis, 0);
}

extern "C" dsc_tensor *dsc_unwrap(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, 0, axis);
    return scan_impl(ctx, x, out, axis, 1);
}

extern "C" dsc_tensor *dsc_phase(dsc_ctx *ctx, const dsc_tensor *z, dsc_tensor *out, int axis) {
    DSC_TRACE_OP(ctx, "op;unary", z, nullptr, 0, axis);
    return scan_impl(ctx, z, out, axis, 2);
}

extern "C" dsc_tensor *dsc_diff(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis) {
    DSC_TRACE_OP(ctx, "op;unary", x, nullptr, 0, axis);
    DSC_ASSERT(x != nullptr);
    const dsc_axis_view v = dsc_axis_view_of(x, axis);
    if (v.n < 2) DSC_LOG_FATAL("the axis must have at least 2 elements, got %d", v.n);
    out = result_of(ctx, x, out, x->dtype, v, v.n - 1);
    dsc_launch_scan_diff(x->data, out->data, x->dtype, v.outer, v.n, v.inner, ctx->stream);
    ctx->last_fft_path = "scan_diff";
    return out;
}
