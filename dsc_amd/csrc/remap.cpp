// remap.cpp — dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift / dsc_pad (include/dsc_mi355x.h, Section J): index maps along axes.
// Every operator is out[j0, j1, j2, j3] = x[m0(j0), m1(j1), m2(j2), m3(j3)] or a constant, each m a piecewise-affine map of one axis
// (remap_plan.h).  An entry point reduces its arguments to one dsc_remap, right-aligned in the four shape slots with the identity on
// the axes it does not name; neighbouring identity axes are merged; the plan travels as a kernel argument and the result is written in
// ONE pass, whatever the number of axes.  Elements move as opaque words: every result is bit-identical to numpy's.  No scratch.
//
// Routes (dsc_last_fft_path), kernels in remap.hip, chosen by dsc_remap_route:
//   remap_rows   the merged last axis is the identity, rows of whole 16-byte packs, both bases 16-byte aligned
//   remap_packs  the last axis is mapped, 4- or 8-byte elements, output rows of whole packs, both bases aligned
//   remap_elems  everything else
// DSC_REMAP_ROUTE=elems, read at every call, forces remap_elems on any shape.
#include "dsc_internal.h"
#include "kernels.h"
#include "op_common.h"

#include <climits>

namespace {

const char *const kRouteNames[] = {"remap_rows", "remap_packs", "remap_elems"};

// the identity on every axis of x
dsc_remap plan_of(const dsc_tensor *x) {
    DSC_ASSERT(x != nullptr);
    dsc_check_rank(x);
    dsc_remap p{};
    for (int i = 0; i < DSC_MAX_DIMS; ++i) p.ax[i] = dsc_map_identity(x->shape[i]);
    return p;
}

// the result checked or allocated, the plan merged, one launch.  flat: the plan is one axis of x->ne elements and the result has x's shape
dsc_tensor *run(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, dsc_remap &p, bool flat = false) {
    int out_shape[DSC_MAX_DIMS];
    for (int i = 0; i < DSC_MAX_DIMS; ++i) out_shape[i] = flat ? x->shape[i] : p.ax[i].n_out;
    DSC_RESULT(out, ctx, x->n_dim, out_shape, x->dtype, "x's dtype and the shape [%d, %d, %d, %d] (right-aligned)", out_shape[0], out_shape[1],
               out_shape[2], out_shape[3]);
    DSC_NO_OVERLAP(out, x, "the input");
    dsc_remap_merge(p);
    DSC_ASSERT(p.ne_out == out->ne);
    const int elem_bytes = (int) dsc_dtype_size(x->dtype);
    int route = dsc_remap_route(p, elem_bytes, (((size_t) x->data | (size_t) out->data) & 15) == 0);
    if (dsc_forced_route("DSC_REMAP_ROUTE", {"elems"}) == 0) route = DSC_REMAP_ELEMS;
    dsc_launch_remap(x->data, out->data, elem_bytes, p, route, ctx->stream);
    ctx->last_fft_path = kRouteNames[route];
    return out;
}

// numpy.roll's shifts added up per slot in 64 bits; n_axes == 0: every axis by its own n // 2 (sign +1 fftshift, -1 ifftshift)
dsc_tensor *shift_impl(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes, int sign) {
    dsc_remap p = plan_of(x);
    if (n_axes < 0 || (n_axes > 0 && axes == nullptr)) DSC_LOG_FATAL("n_axes must be >= 0 with that many axes, got %d", n_axes);
    long long shift[DSC_MAX_DIMS] = {0, 0, 0, 0};
    if (n_axes == 0) {
        for (int i = DSC_MAX_DIMS - x->n_dim; i < DSC_MAX_DIMS; ++i) shift[i] = sign * (long long) (x->shape[i] / 2);
    } else {
        for (int k = 0; k < n_axes; ++k) {
            const int slot = dsc_checked_axis_slot(x, axes[k]);
            shift[slot] += sign * (long long) (x->shape[slot] / 2);
        }
    }
    for (int i = 0; i < DSC_MAX_DIMS; ++i) p.ax[i] = dsc_map_roll(x->shape[i], shift[i]);
    return run(ctx, x, out, p);
}

}  // namespace

extern "C" dsc_tensor *dsc_roll(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *shifts, const int *axes) {
    DSC_TRACE_OP(ctx, "op;layout", x, nullptr, n_axes, 0);
    dsc_remap p = plan_of(x);
    if (n_axes < 0 || shifts == nullptr || (n_axes > 0 && axes == nullptr)) DSC_LOG_FATAL("n_axes must be >= 0 with that many shifts and axes, got %d", n_axes);
    if (n_axes == 0) {                                                   // numpy's axis=None: the flattened tensor, in x's shape
        for (int i = 0; i < DSC_MAX_DIMS - 1; ++i) p.ax[i] = dsc_map_identity(1);
        p.ax[DSC_MAX_DIMS - 1] = dsc_map_roll(x->ne, shifts[0]);
        return run(ctx, x, out, p, true);
    }
    long long shift[DSC_MAX_DIMS] = {0, 0, 0, 0};
    for (int k = 0; k < n_axes; ++k) shift[dsc_checked_axis_slot(x, axes[k])] += shifts[k];      // a repeated axis adds its shifts, as numpy does
    for (int i = 0; i < DSC_MAX_DIMS; ++i) p.ax[i] = dsc_map_roll(x->shape[i], shift[i]);
    return run(ctx, x, out, p);
}

extern "C" dsc_tensor *dsc_flip(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes) {
    DSC_TRACE_OP(ctx, "op;layout", x, nullptr, n_axes, 0);
    dsc_remap p = plan_of(x);
    if (n_axes < 0 || (n_axes > 0 && axes == nullptr)) DSC_LOG_FATAL("n_axes must be >= 0 with that many axes, got %d", n_axes);
    bool seen[DSC_MAX_DIMS] = {false, false, false, false};
    for (int k = 0; k < n_axes; ++k) {
        const int slot = dsc_checked_axis_slot(x, axes[k]);
        if (seen[slot]) DSC_LOG_FATAL("repeated axis %d", axes[k]);
        seen[slot] = true;
    }
    for (int i = DSC_MAX_DIMS - x->n_dim; i < DSC_MAX_DIMS; ++i)
        if (n_axes == 0 || seen[i]) p.ax[i] = dsc_map_flip(x->shape[i]);
    return run(ctx, x, out, p);
}

extern "C" dsc_tensor *dsc_fftshift(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes) {
    DSC_TRACE_OP(ctx, "op;layout", x, nullptr, n_axes, 0);
    return shift_impl(ctx, x, out, n_axes, axes, 1);
}

extern "C" dsc_tensor *dsc_ifftshift(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, int n_axes, const int *axes) {
    DSC_TRACE_OP(ctx, "op;layout", x, nullptr, n_axes, 0);
    return shift_impl(ctx, x, out, n_axes, axes, -1);
}

extern "C" dsc_tensor *dsc_pad(dsc_ctx *ctx, const dsc_tensor *x, dsc_tensor *out, const int *pad_width, int mode, double value_re, double value_im) {
    DSC_TRACE_OP(ctx, "op;layout", x, nullptr, mode, 0);
    dsc_remap p = plan_of(x);
    DSC_ASSERT(pad_width != nullptr);
    if (mode < DSC_PAD_CONSTANT || mode > DSC_PAD_WRAP) DSC_LOG_FATAL("unknown mode %d (0 constant, 1 edge, 2 reflect, 3 symmetric, 4 wrap)", mode);
    const int lead = DSC_MAX_DIMS - x->n_dim;
    long long shape[DSC_MAX_DIMS] = {1, 1, 1, 1}, ne = 1;
    for (int d = 0; d < x->n_dim; ++d) {
        const long long before = pad_width[2 * d], after = pad_width[2 * d + 1];
        if (before < 0 || after < 0) DSC_LOG_FATAL("negative pad width (%lld, %lld) on axis %d: cropping is dsc_tensor_get_slice's", before, after, d);
        shape[lead + d] = x->shape[lead + d] + before + after;
    }
    bool fits = true;
    for (int i = 0; i < DSC_MAX_DIMS; ++i) fits = fits && shape[i] <= INT_MAX && (ne *= shape[i]) <= INT_MAX;
    if (!fits) DSC_LOG_FATAL("the padded shape [%lld, %lld, %lld, %lld] has more than 2^31 - 1 elements", shape[0], shape[1], shape[2], shape[3]);
    for (int d = 0; d < x->n_dim; ++d) p.ax[lead + d] = dsc_map_pad(x->shape[lead + d], pad_width[2 * d], pad_width[2 * d + 1], mode);
    switch (x->dtype) {                                                  // the constant, rounded once to the dtype
        case DSC_F32: { const float v = (float) value_re; memcpy(p.value, &v, sizeof(v)); break; }
        case DSC_F64: { memcpy(p.value, &value_re, sizeof(value_re)); break; }
        case DSC_C32: { const float v[2] = {(float) value_re, (float) value_im}; memcpy(p.value, v, sizeof(v)); break; }
        default:      { const double v[2] = {value_re, value_im}; memcpy(p.value, v, sizeof(v)); break; }
    }
    return run(ctx, x, out, p);
}
