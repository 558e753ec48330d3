// fft_stft.hip — the two gather kernels of the short-time transforms (dsc_stft / dsc_istft, stft.cpp) that are no transform:
//
//   stft_frames_kernel  the frames of the composed forward route: frame q = (row, f) of x [rows][T] starts at f hop - pad; samples
//                       outside [0, T) are reflected (torch's 'reflect': -i, 2 (T - 1) - i) or zero; times the window.  Writes
//                       [n_lines][n_fft] reals, which the internal rfft routes then transform.  (The fused route does the same
//                       mapping in the load of the register kernels, fft_regs_mid.hip.)
//   istft_ola_kernel    overlap-add as a GATHER: one thread per output sample sums the frames that cover it, in increasing frame
//                       order, each times w[j], and divides by the sum of w[j]^2 over the same frames.  Every sample is written
//                       once, without atomics: the result does not depend on the schedule.
#include "dispatch.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int kThreads = 256;

template<typename R>
__global__ __launch_bounds__(kThreads) void stft_frames_kernel(const R *__restrict__ x, const R *__restrict__ w, R *__restrict__ frames, long long q0,
                                                              long long total, int log2n, long long T, int n_frames, int hop, int pad, bool reflect) {
    const int n = 1 << log2n;
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long) gridDim.x * kThreads) {
        const long long line = q0 + (i >> log2n);
        const int j = (int) (i & (n - 1));
        const long long row = line / n_frames;
        long long s = (line - row * n_frames) * hop - pad + j;
        if (reflect) {
            s = s < 0 ? -s : s;
            s = s >= T ? 2 * (T - 1) - s : s;
        }
        R v = (s >= 0 && s < T) ? x[row * T + s] : (R) 0;
        if (w != nullptr) v *= w[j];
        frames[i] = v;
    }
}

template<typename R>
__global__ __launch_bounds__(kThreads) void istft_ola_kernel(const R *__restrict__ frames, const R *__restrict__ w, R *__restrict__ y, long long r0,
                                                            long long rows, int fa, int fpr, int n_fft, int hop, int n_frames, int pad, long long p0,
                                                            long long span, int length) {
    const long long total = rows * span;
    const int f_end = fa + fpr < n_frames ? fa + fpr : n_frames;
    for (long long i = (long long) blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long) gridDim.x * kThreads) {
        const long long r = i / span;
        const long long p = p0 + (i - r * span);
        long long f_lo = p < n_fft ? 0 : (p - n_fft) / hop + 1;           // first frame with f hop + n_fft > p
        long long f_hi = p / hop + 1;                                      // one past the last frame with f hop <= p
        if (f_lo < fa) f_lo = fa;
        if (f_hi > f_end) f_hi = f_end;
        const R *fr = frames + (size_t) r * fpr * n_fft;
        R acc = (R) 0, env = (R) 0;
        for (long long f = f_lo; f < f_hi; ++f) {
            const int j = (int) (p - f * hop);
            const R wj = w != nullptr ? w[j] : (R) 1;
            acc += fr[(size_t) (f - fa) * n_fft + j] * wj;
            env += wj * wj;
        }
        y[(size_t) (r0 + r) * length + (p - pad)] = env > (R) 0 ? acc / env : (R) 0;
    }
}

}  // namespace

void dsc_launch_stft_frames(const void *x, const void *w, void *frames, long long q0, long long n_lines, int n_fft, long long T, int n_frames,
                            int hop, int pad, bool reflect, bool single_precision, hipStream_t stream) {
    const long long total = n_lines * n_fft;
    if (total <= 0) return;
    int log2n = 0;
    while ((1 << log2n) < n_fft) ++log2n;
    with_real(single_precision, [&](auto real) {
        using R = decltype(real);
        DSC_LAUNCH(stft_frames_kernel<R>, dim3(dsc_grid_for(total, kThreads)), dim3(kThreads), 0, stream, (const R *) x, (const R *) w, (R *) frames, q0,
                   total, log2n, T, n_frames, hop, pad, reflect);
    });
}

void dsc_launch_istft_ola(const void *frames, const void *w, void *y, long long r0, long long rows, int fa, int fpr, int n_fft, int hop,
                          int n_frames, int pad, long long p0, long long p1, int length, bool single_precision, hipStream_t stream) {
    if (p0 < pad) p0 = pad;                                                // the n_fft/2 crop of center=True, and the trim to `length`
    if (p1 > (long long) pad + length) p1 = (long long) pad + length;
    const long long span = p1 - p0;
    if (rows <= 0 || span <= 0) return;
    const long long total = rows * span;
    with_real(single_precision, [&](auto real) {
        using R = decltype(real);
        DSC_LAUNCH(istft_ola_kernel<R>, dim3(dsc_grid_for(total, kThreads)), dim3(kThreads), 0, stream, (const R *) frames, (const R *) w, (R *) y, r0, rows,
                   fa, fpr, n_fft, hop, n_frames, pad, p0, span, length);
    });
}
