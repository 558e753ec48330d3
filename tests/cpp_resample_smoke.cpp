// Compile-and-link check of dsc::upfirdn / resample_poly / decimate / firwin (dsc_amd/api/dsc_api.h); with a GPU it resamples three rows
// by 3 / 2 and decimates them by 4 and checks samples of both (the first, the last, a stride through the middle) against the direct sum
// y[m] = sum_i h[m down + t0 - i up] gain x[i] over the host design dsc_firwin_host.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static double direct(const std::vector<double> &h, double gain, const double *x, int T, int up, int down, int t0, int m) {
    const long long t = (long long) m * down + t0;
    double acc = 0;
    for (int i = 0; i < T; ++i) {
        const long long k = t - (long long) i * up;
        if (k >= 0 && k < (long long) h.size()) acc += h[(size_t) k] * gain * x[i];
    }
    return acc;
}

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p %p %p\n", (void *) &dsc_upfirdn, (void *) &dsc_resample_poly, (void *) &dsc_decimate, (void *) &dsc_firwin,
                    (void *) &dsc_firwin_host);
        return 0;
    }
    dsc::init((size_t) 1 << 28);
    const int rows = 3, T = 1001;
    std::vector<double> hx((size_t) rows * T);
    unsigned s = 12345;
    for (auto &v : hx) {
        s = s * 1664525u + 1013904223u;
        v = (double) (s >> 8) / (1 << 24) - 0.5;
    }
    dsc::tensor<double> x(hx.data(), {rows, T});
    bool ok = true;
    double worst = 0;

    {   // resample_poly(x, 3, 2): 61 Kaiser taps, gain 3, t0 30
        std::vector<double> h(61);
        dsc_firwin_host(h.data(), 61, 1.0 / 3, 1, 5.0);
        auto y = dsc::resample_poly(x, 3, 2);
        const int T_out = (T * 3 + 1) / 2;
        ok = ok && y.ndim() == 2 && y.dim(0) == rows && y.dim(1) == T_out && y.dtype() == DSC_F64;
        const auto hy = y.to_host<double>();
        for (int r = 0; r < rows; ++r)
            for (int m = 0; m < T_out; m += (m < 8 || m > T_out - 9) ? 1 : 97)
                worst = std::fmax(worst, std::fabs(hy[(size_t) r * T_out + m] - direct(h, 3.0, &hx[(size_t) r * T], T, 3, 2, 30, m)));
        auto taps = dsc::firwin<double>(61, 1.0 / 3, 1, 5.0);
        auto y2 = dsc::resample_poly(x, 3, 2, taps);
        const auto hy2 = y2.to_host<double>();
        for (size_t i = 0; i < hy.size(); ++i) ok = ok && hy[i] == hy2[i];
    }
    {   // decimate(x, 4): 81 Hamming taps, gain 1, t0 40; the same through upfirdn, whose output starts 40 samples of the filter earlier
        std::vector<double> h(81);
        dsc_firwin_host(h.data(), 81, 0.25, 0, 0.0);
        auto y = dsc::decimate(x, 4);
        const int T_out = (T + 3) / 4;
        ok = ok && y.ndim() == 2 && y.dim(0) == rows && y.dim(1) == T_out && y.dtype() == DSC_F64;
        const auto hy = y.to_host<double>();
        for (int r = 0; r < rows; ++r)
            for (int m = 0; m < T_out; m += (m < 8 || m > T_out - 9) ? 1 : 31)
                worst = std::fmax(worst, std::fabs(hy[(size_t) r * T_out + m] - direct(h, 1.0, &hx[(size_t) r * T], T, 1, 4, 40, m)));
        auto taps = dsc::firwin<double>(81, 0.25);
        auto u = dsc::upfirdn(taps, x, 1, 4);
        const int U = (T - 1 + 81 + 3) / 4;
        ok = ok && u.dim(1) == U;
        const auto hu = u.to_host<double>();
        for (int r = 0; r < rows; ++r)
            for (int m = 0; m < T_out; ++m) ok = ok && hu[(size_t) r * U + m + 10] == hy[(size_t) r * T_out + m];
    }
    ok = ok && worst < 1e-13;
    std::printf("%s: max abs error %.3e\n", ok ? "resample templates ok" : "FAILED", worst);
    dsc::synchronize();
    return ok ? 0 : 1;
}
