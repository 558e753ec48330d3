// Compile-and-link check of dsc::convolve / dsc::correlate (dsc_amd/api/dsc_api.h); with a GPU it convolves a two-row signal with a
// 37-tap filter in every mode and checks the result against the direct sum on the host.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p\n", (void *) &dsc_convolve, (void *) &dsc_correlate);
        return 0;
    }
    dsc::init((size_t) 1 << 30);
    const int rows = 2, T = 3001, M = 37;
    std::vector<double> hx((size_t) rows * T), hh(M);
    for (int i = 0; i < rows * T; ++i) hx[i] = std::cos(0.013 * i) + 0.25 * std::sin(0.37 * i);
    for (int k = 0; k < M; ++k) hh[k] = 1.0 / (1 + k) - 0.03 * k;
    dsc::tensor<double> x(hx.data(), {rows, T}), h(hh.data(), M);
    bool ok = true;
    double worst = 0;
    for (int mode = 0; mode < 3; ++mode) {
        for (int corr = 0; corr < 2; ++corr) {
            auto y = corr ? dsc::correlate(x, h, mode) : dsc::convolve(x, h, mode);
            const int n0 = mode == 0 ? 0 : mode == 1 ? (M - 1) / 2 : M - 1;
            const int T_out = mode == 0 ? T + M - 1 : mode == 1 ? T : T - M + 1;
            ok = ok && y.ndim() == 2 && y.dim(0) == rows && y.dim(1) == T_out;
            const auto hy = y.to_host();
            for (int r = 0; r < rows; ++r)
                for (int o = 0; o < T_out; ++o) {
                    double want = 0;
                    for (int k = 0; k < M; ++k) {
                        const int i = o + n0 - k;
                        if (i >= 0 && i < T) want += hx[(size_t) r * T + i] * hh[corr ? M - 1 - k : k];
                    }
                    const double e = std::fabs(hy[(size_t) r * T_out + o] - want);
                    worst = e > worst ? e : worst;
                }
        }
    }
    ok = ok && worst < 1e-11;
    std::printf("%s: max abs error %.3e\n", ok ? "conv templates ok" : "FAILED", worst);
    dsc::synchronize();
    return ok ? 0 : 1;
}
