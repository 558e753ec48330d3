// fft_conv.hip — the two small kernels of the linear convolution (dsc_convolve / dsc_correlate, conv.cpp) that are no transform:
//
//   conv_crop_kernel     the composed route's store side: block q = (row, b) of the circular filter output [n_lines][n] keeps its
//                        samples [D, n), which go to y[row][b hop + j - D] where that is < T_out.  Every output sample is written once.
//                        (The fused route does the same in the store of the filter kernel, fft_regs_mid.hip.)
//   reverse_kernel       h reversed, for dsc_correlate.
#include "dispatch.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;

template<typename R>
__global__ __launch_bounds__(kThreads) void conv_crop_kernel(const R *__restrict__ frames, R *__restrict__ y, long long q0, long long total, int n,
                                                            int D, int hop, int n_blocks, long long T_out) {
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long) gridDim.x * kThreads) {
        const long long f = i / hop;
        const int j = (int) (i - f * hop);
        const long long line = q0 + f;
        const long long row = line / n_blocks;
        const long long o = (line - row * n_blocks) * hop + j;
        if (o < T_out) y[row * T_out + o] = frames[f * n + D + j];
    }
}

template<typename R>
__global__ __launch_bounds__(kThreads) void reverse_kernel(const R *__restrict__ in, R *__restrict__ out, int n) {
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) out[i] = in[n - 1 - i];
}

}  // namespace

void dsc_launch_conv_crop(const void *frames, void *y, long long q0, long long n_lines, int n, int D, int n_blocks, long long T_out,
                          bool single_precision, hipStream_t stream) {
    const int hop = n - D;
    const long long total = n_lines * hop;
    if (total <= 0) return;
    with_real(single_precision, [&](auto real) {
        using R = decltype(real);
        DSC_LAUNCH(conv_crop_kernel<R>, dim3(dsc_grid_for(total, kThreads)), dim3(kThreads), 0, stream, (const R *) frames, (R *) y, q0, total, n, D, hop,
                   n_blocks, T_out);
    });
}

void dsc_launch_reverse(const void *in, void *out, int n, bool single_precision, hipStream_t stream) {
    if (n <= 0) return;
    with_real(single_precision, [&](auto real) {
        using R = decltype(real);
        DSC_LAUNCH(reverse_kernel<R>, dim3(dsc_grid_for(n, kThreads)), dim3(kThreads), 0, stream, (const R *) in, (R *) out, n);
    });
}
