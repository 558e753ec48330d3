// fft_hilbert.hip — the three small kernels of the analytic signal's composed route (dsc_hilbert / dsc_envelope, hilbert.cpp) that are no
// transform:
//
//   hilbert_response_kernel   H [n/2 + 1] bins <- H[0] = H[n/2] = 0, H[k] = -i otherwise: y = irfft(rfft(x, n) * H) is the Hilbert
//                             transform of x, the imaginary part of the analytic signal.
//   hilbert_zip_kernel        the store side: rows of x (cropped or zero padded to n samples) and the filtered rows y [n_lines][n]
//                             into out, as complex pairs (x, y) or as their moduli sqrt(x^2 + y^2).  (The fused route does the same in the
//                             store of the filter kernel, fft_regs_mid.hip.)
//   hilbert_widen_kernel      f32 rows -> f64 rows of in_len samples (pitch rounded up to even, the spare sample zero): long f32 rows are
//                             filtered in f64 (hilbert.cpp); the zip then takes y as f64 and rounds once.
//
// They stream in 16-byte packs, like elementwise.hip: a thread takes 4 f32 / 2 f64 samples of y and of x and stores one pack of moduli or
// two packs of complex pairs.  Rows of x whose pitch or base is not 16-byte aligned, and the last incomplete pack, go sample by sample.
#include "dispatch.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kThreads = 256;

template<typename R>
__global__ __launch_bounds__(kThreads) void hilbert_response_kernel(R *__restrict__ H, int bins) {
    typedef R pack __attribute__((ext_vector_type(16 / sizeof(R))));
    constexpr int P = 8 / (int) sizeof(R);                          // bins per pack: 2 (c32) or 1 (c64)
    for (int k = (blockIdx.x * kThreads + threadIdx.x) * P; k < bins; k += gridDim.x * kThreads * P) {
        if (k + P <= bins) {
            pack q;
#pragma unroll
            for (int m = 0; m < P; ++m) {
                q[2 * m] = (R) 0;
                q[2 * m + 1] = (k + m == 0 || k + m == bins - 1) ? (R) 0 : (R) -1;
            }
            *(pack *) (H + 2 * (size_t) k) = q;
        } else {                                                    // c32: the last of an odd number of bins, bin n/2
            H[2 * (size_t) k] = (R) 0;
            H[2 * (size_t) k + 1] = (R) 0;
        }
    }
}

__device__ __forceinline__ float modulus(float re, float im) { return sqrtf((re * re) + (im * im)); }       // dsc_abs of a complex value (elementwise.hip)
__device__ __forceinline__ double modulus(double re, double im) { return sqrt((re * re) + (im * im)); }

// total = n_lines n samples; sample e of the chunk is (row q0 + (e >> logn), j = e & (n - 1)).  VEC: the bases of x and out are 16-byte
// aligned, in_pitch and q0 n are whole packs.
// YR: the type of y (R, or double under f32 rows: the modulus is then taken in double and rounded once).
template<typename R, typename YR, bool ENV, bool VEC>
__global__ __launch_bounds__(kThreads) void hilbert_zip_kernel(const R *__restrict__ x, const YR *__restrict__ y, R *__restrict__ out, long long q0,
                                                              long long total, int logn, long long in_pitch, int in_len) {
    constexpr int P = 16 / (int) sizeof(R);
    typedef R pack __attribute__((ext_vector_type(P)));
    typedef YR ypack __attribute__((ext_vector_type(P)));
    const int n = 1 << logn;
    R *o = out + (ENV ? 1 : 2) * (q0 << logn);
    for (long long e0 = ((long long) blockIdx.x * kThreads + threadIdx.x) * P; e0 < total; e0 += (long long) gridDim.x * kThreads * P) {
        const bool whole = e0 + P <= total;
        R xs[P];
        YR ys[P];
        if (whole) {
            const ypack q = *(const ypack *) (y + e0);
#pragma unroll
            for (int m = 0; m < P; ++m) ys[m] = q[m];
        } else {
#pragma unroll
            for (int m = 0; m < P; ++m) ys[m] = e0 + m < total ? y[e0 + m] : (YR) 0;
        }
        const long long row = e0 >> logn;
        const int j = (int) (e0 & (n - 1));
        if (VEC && whole && n >= P && j + P <= in_len) {
            const pack q = *(const pack *) (x + (q0 + row) * in_pitch + j);
#pragma unroll
            for (int m = 0; m < P; ++m) xs[m] = q[m];
        } else {
#pragma unroll
            for (int m = 0; m < P; ++m) {
                const long long e = e0 + m;
                const int jj = (int) (e & (n - 1));
                xs[m] = (e < total && jj < in_len) ? x[(q0 + (e >> logn)) * in_pitch + jj] : (R) 0;
            }
        }
        if constexpr (ENV) {
            if (VEC && whole) {
                pack q;
#pragma unroll
                for (int m = 0; m < P; ++m) q[m] = (R) modulus((YR) xs[m], ys[m]);
                *(pack *) (o + e0) = q;
            } else {
#pragma unroll
                for (int m = 0; m < P; ++m)
                    if (e0 + m < total) o[e0 + m] = (R) modulus((YR) xs[m], ys[m]);
            }
        } else {
            if (VEC && whole) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    pack q;
#pragma unroll
                    for (int m = 0; m < P / 2; ++m) {
                        q[2 * m] = xs[h * (P / 2) + m];
                        q[2 * m + 1] = (R) ys[h * (P / 2) + m];
                    }
                    *(pack *) (o + 2 * e0 + h * P) = q;
                }
            } else {
#pragma unroll
                for (int m = 0; m < P; ++m)
                    if (e0 + m < total) {
                        o[2 * (e0 + m)] = xs[m];
                        o[2 * (e0 + m) + 1] = (R) ys[m];
                    }
            }
        }
    }
}

// xw [n_lines][wpitch] doubles <- samples j < in_len of rows q0 .. of x [..][in_pitch] floats, zero at j >= in_len; wpitch even: one 16-byte
// pack of two doubles per thread
__global__ __launch_bounds__(kThreads) void hilbert_widen_kernel(const float *__restrict__ x, double *__restrict__ xw, long long q0, long long pairs,
                                                                int half_pitch, long long in_pitch, int in_len) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    for (long long p = (long long) blockIdx.x * kThreads + threadIdx.x; p < pairs; p += (long long) gridDim.x * kThreads) {
        const long long row = p / half_pitch;
        const int j = 2 * (int) (p - row * half_pitch);
        const float *src = x + (q0 + row) * in_pitch;
        d2 q;
        q[0] = j < in_len ? (double) src[j] : 0.0;
        q[1] = j + 1 < in_len ? (double) src[j + 1] : 0.0;
        *(d2 *) (xw + 2 * p) = q;
    }
}

}  // namespace

void dsc_launch_hilbert_response(void *H, int n, bool single_precision, hipStream_t stream) {
    const int bins = n / 2 + 1;
    with_real(single_precision, [&](auto real) {
        using R = decltype(real);
        constexpr int P = 8 / (int) sizeof(R);                          // bins per pack
        DSC_LAUNCH(hilbert_response_kernel<R>, dim3(dsc_grid_for((bins + P - 1) / P, kThreads)), dim3(kThreads), 0, stream, (R *) H, bins);
    });
}

void dsc_launch_hilbert_widen(const void *x, void *xw, long long q0, long long n_lines, long long in_pitch, int in_len, int wpitch,
                              hipStream_t stream) {
    const long long pairs = n_lines * (wpitch / 2);
    if (pairs <= 0) return;
    DSC_LAUNCH(hilbert_widen_kernel, dim3(dsc_grid_for(pairs, kThreads)), dim3(kThreads), 0, stream, (const float *) x, (double *) xw, q0, pairs, wpitch / 2,
               in_pitch, in_len);
}

void dsc_launch_hilbert_zip(const void *x, const void *y, void *out, long long q0, long long n_lines, int n, long long in_pitch, int in_len,
                            bool envelope, bool single_precision, bool y_double, hipStream_t stream) {
    const long long total = n_lines * n;
    if (total <= 0) return;
    int logn = 0;
    while ((1 << logn) < n) ++logn;
    // (R, YR): y is of R's type, or double under f32 rows when y_double is set (never float under f64 rows)
    auto launch = [&](auto real, auto yreal) { with_bool(envelope, [&](auto env) {
        using R = decltype(real);
        using YR = decltype(yreal);
        constexpr int P = 16 / (int) sizeof(R);
        const bool vec = ((uintptr_t) x & 15) == 0 && ((uintptr_t) out & 15) == 0 && in_pitch % P == 0 && (q0 << logn) % P == 0;
        with_bool(vec, [&](auto v) {
            DSC_LAUNCH((hilbert_zip_kernel<R, YR, decltype(env)::value, decltype(v)::value>), dim3(dsc_grid_for((total + P - 1) / P, kThreads)), dim3(kThreads), 0,
                       stream, (const R *) x, (const YR *) y, (R *) out, q0, total, logn, in_pitch, in_len);
        });
    }); };
    with_real(single_precision, [&](auto real) {
        if constexpr (sizeof(real) == 4) { if (y_double) return launch(real, double{}); }
        launch(real, real);
    });
}
