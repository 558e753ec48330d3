// Compile-and-link check of dsc::fft2 / ifft2 / rfft2 / irfft2 (dsc_amd/api/dsc_api.h); with a GPU it transforms two 64 x 64 real
// images, checks rfft2 and fft2 against the direct double sum on the host and both round trips against the input.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p %p\n", (void *) &dsc_fft2, (void *) &dsc_ifft2, (void *) &dsc_rfft2, (void *) &dsc_irfft2);
        return 0;
    }
    dsc::init((size_t) 1 << 30);
    const int B = 2, N = 64, K = N / 2 + 1;
    const double pi = 3.14159265358979323846;
    std::vector<double> hx((size_t) B * N * N);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = std::cos(0.013 * (double) i) + 0.25 * std::sin(0.37 * (double) i) + (i % 7 == 0 ? 1.5 : 0.0);
    dsc::tensor<double> x(hx.data(), {B, N, N});
    auto X = dsc::rfft2(x);
    auto F = dsc::fft2(x);
    auto y = dsc::irfft2(X);
    auto z = dsc::ifft2(F);
    bool ok = X.ndim() == 3 && X.dim(0) == B && X.dim(1) == N && X.dim(2) == K && X.dtype() == DSC_C64;
    ok = ok && F.dim(1) == N && F.dim(2) == N && F.dtype() == DSC_C64 && y.dim(2) == N && y.dtype() == DSC_F64 && z.dtype() == DSC_C64;
    const auto hX = X.to_host<dsc_c64>(), hF = F.to_host<dsc_c64>(), hz = z.to_host<dsc_c64>();
    const auto hy = y.to_host<double>();
    double worst = 0, scale = 0;
    for (int b = 0; b < B; ++b)
        for (int k0 = 0; k0 < N; k0 += 5)
            for (int k1 = 0; k1 < N; k1 += 3) {
                double re = 0, im = 0;
                for (int r = 0; r < N; ++r)
                    for (int c = 0; c < N; ++c) {
                        const double a = -2 * pi * (double) ((r * k0 + c * k1) % N) / N, v = hx[((size_t) b * N + r) * N + c];
                        re += v * std::cos(a);
                        im += v * std::sin(a);
                    }
                const dsc_c64 f = hF[((size_t) b * N + k0) * N + k1];
                double e = std::hypot(f.real - re, f.imag - im);
                if (k1 < K) {
                    const dsc_c64 g = hX[((size_t) b * N + k0) * K + k1];
                    e = std::fmax(e, std::hypot(g.real - re, g.imag - im));
                }
                worst = e > worst ? e : worst;
                scale = std::fmax(scale, std::hypot(re, im));
            }
    double rt = 0;
    for (size_t i = 0; i < hx.size(); ++i) rt = std::fmax(rt, std::fmax(std::fabs(hy[i] - hx[i]), std::hypot(hz[i].real - hx[i], hz[i].imag)));
    ok = ok && worst < 1e-12 * scale && rt < 1e-12;
    std::printf("%s: max bin error %.3e (largest bin %.3e), round trip %.3e\n", ok ? "fft2 templates ok" : "FAILED", worst, scale, rt);
    dsc::synchronize();
    return ok ? 0 : 1;
}
