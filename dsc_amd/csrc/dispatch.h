// dispatch.h — the host-side idiom every kernel file uses to get from run-time arguments to one instantiation and to launch it.
//   with_real / with_bool / with_mode   hand a run-time choice to a generic callable as a compile-time constant; each kernel file adds
//                                        its own with_..._len table next to its supports() gate, and ends it with no_kernel
//   with_index<N>                        the same for a code 0 .. N - 1 (operator codes); with_dtype is in stream_common.h
//   dsc_launch_dyn_lds / dsc_launch_var_lds   the one place that opts a kernel in to its dynamic LDS (once per device) and launches it
//   dsc_grid_for                         grid size of the grid-stride helper kernels
//   dsc_cu_count                         grid size of the persistent kernels
#pragma once

#include "kernels.h"

#include <type_traits>
#include <utility>

template<int V> using int_c = std::integral_constant<int, V>;
template<bool V> using bool_c = std::integral_constant<bool, V>;

// A value no kernel is instantiated for.  The supports() gates keep the routes away from these; a caller that skips its gate must not
// get another length's kernel instead.
[[noreturn]] static inline void no_kernel(const char *file, const char *what, long long value) {
    fprintf(stderr, "%s: no kernel for %s %lld\n", file, what, value);
    exit(EXIT_FAILURE);
}

template<typename F> void with_real(bool single_precision, F f) { if (single_precision) f(float{}); else f(double{}); }
template<typename F> void with_bool(bool b, F f) { if (b) f(bool_c<true>{}); else f(bool_c<false>{}); }

// value in 0 .. N - 1 -> int_c<value>; `file` and `what` name the table for no_kernel
template<typename F, int... K> bool with_index_in(int value, F &f, std::integer_sequence<int, K...>) {
    return ((value == K && (f(int_c<K>{}), true)) || ...);
}
template<int N, typename F> void with_index(const char *file, const char *what, int value, F f) {
    if (!with_index_in(value, f, std::make_integer_sequence<int, N>{})) no_kernel(file, what, value);
}

// (mode, inverse) -> (MODE, INV): the packed-real modes have one direction each
template<typename F> void with_mode(dsc_fft_mode mode, bool inverse, F f) {
    switch (mode) {
        case DSC_MODE_R2C_PACKED: return f(int_c<DSC_MODE_R2C_PACKED>{}, bool_c<false>{});
        case DSC_MODE_C2R_PACKED: return f(int_c<DSC_MODE_C2R_PACKED>{}, bool_c<true>{});
        case DSC_MODE_R2C_CAST:   return with_bool(inverse, [&](auto inv) { f(int_c<DSC_MODE_R2C_CAST>{}, inv); });
        case DSC_MODE_C2C:        return with_bool(inverse, [&](auto inv) { f(int_c<DSC_MODE_C2C>{}, inv); });
    }
    no_kernel("dispatch.h", "transform mode", (int) mode);
}

// Launch of a kernel that takes up to MAX_LDS bytes of dynamic LDS, `lds` of them at this launch: opts the kernel in to MAX_LDS the
// first time it runs on the current device, then launches and checks.  The "seen on this device" state is per kernel.
template<auto Kernel, size_t MAX_LDS, typename... Args>
static inline void dsc_launch_var_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    static unsigned long long seen = 0;
    if (dsc_first_use_on_device(seen))
        DSC_KERNEL_CHECK(hipFuncSetAttribute((const void *) Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) MAX_LDS));
    DSC_LAUNCH(Kernel, grid, block, lds, stream, args...);
}

// ... the same size at every launch: opted in to exactly that
template<auto Kernel, typename... Args>
static inline void dsc_launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    static unsigned long long seen = 0;
    if (dsc_first_use_on_device(seen))
        DSC_KERNEL_CHECK(hipFuncSetAttribute((const void *) Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    DSC_LAUNCH(Kernel, grid, block, lds, stream, args...);
}

// blocks of `threads` for `items` work items of a grid-stride kernel: at least 1, at most 65536
static inline unsigned dsc_grid_for(long long items, int threads) {
    const long long blocks = (items + threads - 1) / threads;
    return (unsigned) (blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

// compute units of the current device (asked once per device): the grid of a persistent kernel
static inline int dsc_cu_count() {
    static int cus[64];
    int dev = 0;
    DSC_KERNEL_CHECK(hipGetDevice(&dev));
    dev &= 63;
    if (cus[dev] == 0) DSC_KERNEL_CHECK(hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev));
    return cus[dev];
}
