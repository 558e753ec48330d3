// op_common.h — what the operator files (stft, conv, hilbert, fft2, resample, scan .cpp) share on the host side: DESIGN.md 4.0b.
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

#ifndef DSC_OP_COMMON_PURE
#include "dsc_internal.h"

#include <cstring>

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

// The DSC_NO_..._FUSED switches are read at every call: the tests and tools/bench_*.py switch routes within one process.
static inline bool dsc_env_set(const char *name) { return getenv(name) != nullptr; }
#endif
