// reduce.cpp — dsc_sum / dsc_mean / dsc_max / dsc_min: reductions along one axis of a tensor viewed as [outer][n][inner], in x's dtype;
// the host-side mirror of dsc/src/dsc.cpp:1793-1953.  The kernels and the choice among them are reduce.hip's; no dsc_last_fft_path.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

// dsc.cpp:83-115 (validate_reduce_params).  For keep_dims=false the reference leaves 0x01010101 in the leading slots of its scratch
// shape (memset with 1, :98), which only a user-supplied `out` can observe; here those slots are 1 and such an `out` is accepted.
static dsc_tensor *reduce_entry(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int axis, bool keep_dims, int op) {
    DSC_ASSERT(x != nullptr);
    static const char *names[] = {"dsc_sum", "dsc_mean", "dsc_max", "dsc_min"};
    dsc_trace_scope trace__(ctx, names[op], "op;unary", x, nullptr, 0, axis);
    // the reference's lenient check: an axis in a leading padding slot reduces over an extent of 1; dropping it (a fifth shape slot) is refused
    const int slot = dsc_axis_slot(x, axis);
    DSC_ASSERT(slot >= 0 && slot < DSC_MAX_DIMS);
    DSC_ASSERT(keep_dims || slot >= DSC_MAX_DIMS - x->n_dim);
    const dsc_axis_view v = dsc_axis_view_at(x->shape, slot);

    int out_shape[DSC_MAX_DIMS];
    const int out_ndim = dsc_reduced_shape(x->shape, x->n_dim, slot, keep_dims, out_shape);
    DSC_RESULT(out, ctx, out_ndim, out_shape, x->dtype, "the reduced shape (%s the axis) and x's dtype", keep_dims ? "1 along" : "without");

    // workspace for the segmented path: whatever the scratch arena has, up to 64 MiB
    ctx->scratch.reset();
    size_t ws_bytes = ctx->scratch.capacity() > (64u << 20) ? (64u << 20) : ctx->scratch.capacity() / 2;
    void *ws = ws_bytes >= 4096 ? ctx->scratch.alloc(ws_bytes) : nullptr;
    dsc_launch_reduce(x->data, out->data, x->dtype, op, v.outer, v.n, v.inner, ws, ws_bytes, ctx->stream);
    return out;
}

extern "C" dsc_tensor *dsc_sum (dsc_ctx *c, const dsc_tensor *x, dsc_tensor *o, int axis, bool keep) { return reduce_entry(c, x, o, axis, keep, 0); }
extern "C" dsc_tensor *dsc_mean(dsc_ctx *c, const dsc_tensor *x, dsc_tensor *o, int axis, bool keep) { return reduce_entry(c, x, o, axis, keep, 1); }
extern "C" dsc_tensor *dsc_max (dsc_ctx *c, const dsc_tensor *x, dsc_tensor *o, int axis, bool keep) { return reduce_entry(c, x, o, axis, keep, 2); }
extern "C" dsc_tensor *dsc_min (dsc_ctx *c, const dsc_tensor *x, dsc_tensor *o, int axis, bool keep) { return reduce_entry(c, x, o, axis, keep, 3); }
