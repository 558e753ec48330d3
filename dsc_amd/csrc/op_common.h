// op_common.h — what the operator files (stft, conv, hilbert, fft2, resample, reduce, scan, moments, remap .cpp) share on the host side: DESIGN.md 4.0b.
// One rule per helper.  The first part is arithmetic on integers and needs nothing but <cstddef>: define DSC_OP_COMMON_PURE before
// including it from a stand-alone host program (tests/test_op_common.py).
#pragma once

#include <cstddef>

// Lines of a pinned scratch chunk: half of what the arena has left after the caller's other pinned blocks (`fixed`, with their alignment
// slack), at most 128 MiB, leaving `reserve` bytes to the routes called on the chunk; at least one line, at most n_lines.  0: not even one
// line fits (the caller words its own "scratch arena too small: ..."), which capacity < fixed is a case of.
static inline long long dsc_chunk_lines(size_t capacity, size_t fixed, size_t line_bytes, size_t reserve, long long n_lines) {
    const size_t chunk_cap = (size_t) 128 << 20;
    if (capacity < fixed || capacity - fixed < line_bytes + reserve) return 0;
    const size_t cap = capacity - fixed;
    long long chunk = (long long) ((cap / 2 < chunk_cap ? cap / 2 : chunk_cap) / line_bytes);
    if (chunk < 1) chunk = 1;
    const long long room = (long long) ((cap - reserve) / line_bytes);
    if (chunk > room) chunk = room;
    return chunk < n_lines ? chunk : n_lines;
}

// Rows per launch of a fused kernel that addresses its input rows (and its output rows, row_bytes_out > 0) with 31-bit byte offsets
// from the launch's first row: as many as fit under limit_bytes with one spare row (groups past the last line compute their offsets
// from row `rows`).  An even number, so that every launch's first element is even and pairs the kernel finds aligned relative to its
// base are aligned in memory too; with rows of odd length (odd_rows) and more than one of them, one row per launch is not launchable.
// 0: take the composed route.
static inline long long dsc_fused_rows_per_launch(long long limit_bytes, long long row_bytes_in, long long row_bytes_out, long long rows, bool odd_rows) {
    long long rows_per = limit_bytes / row_bytes_in - 1;
    if (row_bytes_out > 0 && limit_bytes / row_bytes_out - 1 < rows_per) rows_per = limit_bytes / row_bytes_out - 1;
    if (rows_per > 1) rows_per &= ~1LL;
    if (rows_per < 1 || (rows_per == 1 && rows != 1 && odd_rows)) return 0;
    return rows_per;
}

// ---- the axis operators (reduce, scan, moments, remap .cpp): a tensor viewed as [outer][n][inner] around one of its four shape slots
enum { DSC_OP_DIMS = 4 };                        // DSC_MAX_DIMS, which the pure part does not see
struct dsc_axis_view { int slot, n; long long outer, inner; };

// The view around a slot, unchecked: the reductions take a slot among the leading padding slots too, an extent of 1.
static inline dsc_axis_view dsc_axis_view_at(const int *shape, int slot) {
    dsc_axis_view v = {slot, shape[slot], 1, 1};
    for (int i = 0; i < slot; ++i) v.outer *= shape[i];
    for (int i = slot + 1; i < DSC_OP_DIMS; ++i) v.inner *= shape[i];
    return v;
}

// The view along the user's axis of a shape right-aligned in the four slots; slot -1 when n_dim is outside 1..4 or axis is outside
// [-n_dim, n_dim).  The slot is dsc_axis_slot's.
static inline dsc_axis_view dsc_axis_view_on(const int *shape, int n_dim, int axis) {
    if (n_dim < 1 || n_dim > DSC_OP_DIMS || axis < -n_dim || axis >= n_dim) return dsc_axis_view{-1, 0, 0, 0};
    return dsc_axis_view_at(shape, axis < 0 ? DSC_OP_DIMS + axis : DSC_OP_DIMS - n_dim + axis);
}

// The shape of a reduction's result, the reference's rule (validate_reduce_params): the axis kept with extent 1, or dropped with ones
// in the leading slots (filled from the right: the padding slots of `shape` hold 1).  Returns the result's rank.
static inline int dsc_reduced_shape(const int *shape, int n_dim, int slot, bool keep_dims, int *out_shape) {
    int oi = DSC_OP_DIMS - 1;
    for (int xi = DSC_OP_DIMS - 1; xi >= 0; --xi)
        if (keep_dims || xi != slot) out_shape[oi--] = xi == slot ? 1 : shape[xi];
    while (oi >= 0) out_shape[oi--] = 1;
    return keep_dims ? n_dim : n_dim - 1;
}

// The index of `value` among n_names route names, or -1.
static inline int dsc_route_index(const char *value, const char *const *names, int n_names) {
    for (int i = 0; i < n_names; ++i) {
        const char *a = value, *b = names[i];
        while (*a != '\0' && *a == *b) ++a, ++b;
        if (*a == '\0' && *b == '\0') return i;
    }
    return -1;
}

#ifndef DSC_OP_COMMON_PURE
#include "dsc_internal.h"

#include <cstring>
#include <initializer_list>

static_assert(DSC_OP_DIMS == DSC_MAX_DIMS, "op_common.h counts the shape slots of dsc_tensor");

// The result: a new tensor of the expected rank, shape (all DSC_MAX_DIMS slots) and dtype, or the caller's `out` if it is one.  A wrong
// `out` ends the process with "out must have <what>", what being the caller's printf format and arguments.
static inline dsc_tensor *dsc_result_of(dsc_ctx *ctx, int n_dim, const int *shape, dsc_dtype dtype, dsc_tensor *out) {
    if (out == nullptr) return dsc_new_tensor(ctx, n_dim, &shape[DSC_MAX_DIMS - n_dim], dtype, nullptr);
    return out->dtype == dtype && out->n_dim == n_dim && memcmp(shape, out->shape, DSC_MAX_DIMS * sizeof(int)) == 0 ? out : nullptr;
}
#define DSC_RESULT(out, ctx, n_dim, shape, dtype, ...)                                                                              \
    do {                                                                                                                            \
        if (((out) = dsc_result_of((ctx), (n_dim), (shape), (dtype), (out))) == nullptr) DSC_LOG_FATAL("out must have " __VA_ARGS__); \
    } while (0)

// `out` is written while `t` is still read: their byte ranges must not meet.  A freshly allocated `out` passes by construction.
static inline bool dsc_share_memory(const dsc_tensor *out, const dsc_tensor *t) {
    const char *ta = (const char *) t->data, *oa = (const char *) out->data;
    return oa < ta + (size_t) t->ne * dsc_dtype_size(t->dtype) && ta < oa + (size_t) out->ne * dsc_dtype_size(out->dtype);
}
#define DSC_NO_OVERLAP(out, t, what)                                                               \
    do {                                                                                           \
        if (dsc_share_memory((out), (t))) DSC_LOG_FATAL("out must not share memory with " what); \
    } while (0)

// A header over device memory the operator owns or borrows, for the length of a scope: an argument for an inner operator call.
// (hidden, like dsc_scratch_pin: the library exports nothing from this header)
struct __attribute__((visibility("hidden"))) dsc_scoped_view {
    dsc_ctx *ctx;
    dsc_tensor *t;
    dsc_scoped_view(dsc_ctx *c, void *ptr, int n_dim, const int *shape, dsc_dtype dtype) : ctx(c) {
        size_t nbytes = dsc_dtype_size(dtype);
        for (int i = 0; i < n_dim; ++i) nbytes *= (size_t) shape[i];
        t = dsc_new_tensor_over(c, ptr, nbytes, n_dim, shape, dtype);
    }
    ~dsc_scoped_view() { dsc_tensor_free(ctx, t); }
    dsc_scoped_view(const dsc_scoped_view &) = delete;
    dsc_scoped_view &operator=(const dsc_scoped_view &) = delete;
    operator dsc_tensor *() const { return t; }
};

// Scratch blocks an operator holds while it calls others that use the arena: reset() on entry; the caller allocates its blocks and
// calls pin(); the destructor unpins on every way out, so that no return can leave the arena short for the operators after it.
struct __attribute__((visibility("hidden"))) dsc_scratch_pin {
    dsc_scratch_arena &arena;
    explicit dsc_scratch_pin(dsc_ctx *ctx) : arena(ctx->scratch) { arena.reset(); }
    ~dsc_scratch_pin() { arena.unpin(); }
    dsc_scratch_pin(const dsc_scratch_pin &) = delete;
    dsc_scratch_pin &operator=(const dsc_scratch_pin &) = delete;
    char *alloc(size_t nb) { return arena.alloc(nb); }
    void pin() { arena.pin(); }
};

// A scratch block for an operator's own launches, nothing else using the arena meanwhile: reset() on entry, `need` bytes if the arena
// has them with their alignment slack (need == 0: no block), reset() on every way out — the stream is in order, nothing reuses the block
// before the launches have read it.  DSC_SCRATCH_BLOCK declares one; a short arena ends the process with "scratch arena too small: <what>".
struct __attribute__((visibility("hidden"))) dsc_scratch_block {
    dsc_scratch_arena &arena;
    char *ptr = nullptr;
    bool fits;
    dsc_scratch_block(dsc_ctx *ctx, size_t need) : arena(ctx->scratch) {
        arena.reset();
        fits = need == 0 || arena.capacity() >= need + DSC_DEVICE_ALIGN;
        if (fits && need > 0) ptr = arena.alloc(need);
    }
    ~dsc_scratch_block() { arena.reset(); }
    dsc_scratch_block(const dsc_scratch_block &) = delete;
};
#define DSC_SCRATCH_BLOCK(name, ctx, need, ...) \
    dsc_scratch_block name((ctx), (need));      \
    if (!name.fits) DSC_LOG_FATAL("scratch arena too small: " __VA_ARGS__)

// The DSC_NO_..._FUSED switches are read at every call: the tests and tools/bench_*.py switch routes within one process.
static inline bool dsc_env_set(const char *name) { return getenv(name) != nullptr; }

// A route forced by the environment variable `var`, read at every call like the switches above: the index of its value among the
// allowed names, -1 when it is not set.  Any other value ends the process with "<var> must be a or b, got "x"".
static inline int dsc_forced_route(const char *var, std::initializer_list<const char *> names) {
    const char *value = getenv(var);
    if (value == nullptr) return -1;
    const int route = dsc_route_index(value, names.begin(), (int) names.size());
    if (route < 0) {
        char allowed[96] = "";
        for (const char *name : names) snprintf(allowed + strlen(allowed), sizeof(allowed) - strlen(allowed), allowed[0] ? " or %s" : "%s", name);
        DSC_LOG_FATAL("%s must be %s, got \"%s\"", var, allowed, value);
    }
    return route;
}

// x's view along the user's axis, and that axis's slot alone (remap.cpp, which maps several axes in one call); a rank outside
// 1..DSC_MAX_DIMS and an axis outside [-n_dim, n_dim) end the process.
static inline void dsc_check_rank(const dsc_tensor *x) {
    if (x->n_dim < 1 || x->n_dim > DSC_MAX_DIMS) DSC_LOG_FATAL("tensors have 1 to %d dimensions, got %d", DSC_MAX_DIMS, x->n_dim);
}
static inline dsc_axis_view dsc_axis_view_of(const dsc_tensor *x, int axis) {
    dsc_check_rank(x);
    const dsc_axis_view v = dsc_axis_view_on(x->shape, x->n_dim, axis);
    if (v.slot < 0) DSC_LOG_FATAL("axis %d is out of range for a tensor of %d dimensions", axis, x->n_dim);
    return v;
}
static inline int dsc_checked_axis_slot(const dsc_tensor *x, int axis) { return dsc_axis_view_of(x, axis).slot; }
#endif
