// Compile-and-link check of dsc::sumsq / rms / var / std / vdot / detrend (dsc_amd/api/dsc_api.h); with a GPU it takes three rows of
// doubles with an offset and a slope and checks every operator against sums in long double on the host.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p %p %p %p\n", (void *) &dsc_sumsq, (void *) &dsc_rms, (void *) &dsc_var, (void *) &dsc_std,
                    (void *) &dsc_vdot, (void *) &dsc_detrend);
        return 0;
    }
    dsc::init((size_t) 1 << 28);
    const int rows = 3, T = 5001;
    std::vector<double> hx((size_t) rows * T), hy((size_t) rows * T);
    unsigned s = 12345;
    for (size_t i = 0; i < hx.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        hx[i] = (double) (s >> 8) / (1 << 24) - 0.5 + 1000.0 + 0.01 * (double) (i % T);      // noise on an offset and a slope
        s = s * 1664525u + 1013904223u;
        hy[i] = (double) (s >> 8) / (1 << 24) - 0.5;
    }
    dsc::tensor<double> x(hx.data(), {rows, T}), y(hy.data(), {rows, T});
    auto q = dsc::sumsq(x), r = dsc::rms(x), v = dsc::var(x, -1, 1), sd = dsc::std(x, -1, 1, false), d = dsc::vdot(x, y);
    auto lin = dsc::detrend(x), con = dsc::detrend(x, -1, DSC_DETREND_CONSTANT);
    bool ok = q.ndim() == 2 && q.dim(0) == rows && q.dim(1) == 1 && sd.ndim() == 1 && sd.dim(0) == rows && lin.dim(1) == T && con.dim(1) == T;
    const auto hq = q.to_host<double>(), hr = r.to_host<double>(), hv = v.to_host<double>(), hs = sd.to_host<double>(), hd = d.to_host<double>();
    const auto hl = lin.to_host<double>(), hc = con.to_host<double>();
    double worst = 0;
    const auto rel = [&](double got, long double want) { worst = std::fmax(worst, (double) (std::fabs((long double) got - want) / std::fabs(want))); };
    for (int i = 0; i < rows; ++i) {
        const double *a = &hx[(size_t) i * T], *b = &hy[(size_t) i * T];
        long double sq = 0, sum = 0, dot = 0, st = 0, stt = 0;
        for (int j = 0; j < T; ++j) {
            const long double t = j - 0.5L * (T - 1);
            sq += (long double) a[j] * a[j];
            sum += a[j];
            dot += (long double) a[j] * b[j];
            st += t * a[j];
            stt += t * t;
        }
        const long double m = sum / T, slope = st / stt;
        long double S = 0;
        for (int j = 0; j < T; ++j) S += (a[j] - m) * (a[j] - m);
        rel(hq[i], sq);
        rel(hr[i], std::sqrt(sq / T));
        rel(hv[i], S / (T - 1));
        rel(hs[i], std::sqrt(S / (T - 1)));
        worst = std::fmax(worst, (double) std::fabs(hd[i] - dot) / 1e6);                       // |x| ~ 1e3 times T terms
        for (int j = 0; j < T; ++j) {
            const long double t = j - 0.5L * (T - 1);
            worst = std::fmax(worst, (double) std::fabs(hl[(size_t) i * T + j] - (a[j] - m - slope * t)) / 1e3);
            worst = std::fmax(worst, (double) std::fabs(hc[(size_t) i * T + j] - (a[j] - m)) / 1e3);
        }
    }
    ok = ok && worst < 1e-12;
    std::printf("%s: worst relative error %.3e\n", ok ? "moment templates ok" : "FAILED", worst);
    dsc::synchronize();
    return ok ? 0 : 1;
}
