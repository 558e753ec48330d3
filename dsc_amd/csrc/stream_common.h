// stream_common.h — what the streaming kernel files (elementwise.hip, layout.hip, remap.hip, reduce.hip, scan.hip, moments.hip) share:
// the element types behind the four dtype codes, the 16-byte pack, the capped streaming grid, the round-up of a scratch block and the
// dtype and element-size tables of the dispatch.h idiom.
// Everything sits in an anonymous namespace: cx and packed appear in kernel signatures, and each file keeps its own internal kernels.
#pragma once

#include "dispatch.h"

#include <hip/hip_runtime.h>

namespace {

template<typename T> struct alignas(2 * sizeof(T)) cx { T x, y; };

template<typename T> struct elem;   // element type -> complex or not, and its real type
template<> struct elem<float>  { static constexpr bool cplx = false; using real = float; };
template<> struct elem<double> { static constexpr bool cplx = false; using real = double; };
template<> struct elem<cx<float>>  { static constexpr bool cplx = true; using real = float; };
template<> struct elem<cx<double>> { static constexpr bool cplx = true; using real = double; };

// V consecutive elements moved as one access
template<typename T, int V> struct alignas(sizeof(T) * V) packed { T e[V]; };
inline bool aligned_to(const void *p, size_t a) { return ((size_t) p & (a - 1)) == 0; }

inline dim3 stream_grid(long long ne) {
    long long blocks = (ne + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;        // 8 blocks per CU, grid-stride beyond that
    if (blocks < 1) blocks = 1;
    return dim3((unsigned) blocks);
}

// bytes of a scratch block of n elements, rounded up so that the block after it starts 256-byte aligned (scan.hip, moments.hip)
inline size_t scratch_block_bytes(long long n, size_t elem) { return ((size_t) n * elem + 255) & ~(size_t) 255; }

// dtype code (dsc_dtype: F32, F64, C32, C64) -> element type
template<typename F> void with_dtype(int dtype, F f) {
    switch (dtype) {
        case 0: return f(float{});
        case 1: return f(double{});
        case 2: return f(cx<float>{});
        case 3: return f(cx<double>{});
    }
    no_kernel("stream_common.h", "dtype", dtype);
}

// element size in bytes -> an unsigned type of that size: the kernels that move elements without looking at them (layout.hip, remap.hip)
struct alignas(16) b16 { unsigned long long a, b; };
template<typename F> void with_elem_bytes(int elem_bytes, F f) {
    switch (elem_bytes) {
        case 4:  return f((unsigned int) 0);
        case 8:  return f((unsigned long long) 0);
        case 16: return f(b16{});
    }
    no_kernel("stream_common.h", "element size", elem_bytes);
}

}  // namespace
