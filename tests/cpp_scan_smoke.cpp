// Compile-and-link check of dsc::cumsum / diff / unwrap / phase (dsc_amd/api/dsc_api.h); with a GPU it scans three rows of doubles and
// checks cumsum against the running sum (to a few units of the last place of the row's absolute sum), diff(cumsum(x)) against x, and
// unwrap of a wrapped ramp, and phase of exp(i ramp), against the ramp.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p %p\n", (void *) &dsc_cumsum, (void *) &dsc_diff, (void *) &dsc_unwrap, (void *) &dsc_phase);
        return 0;
    }
    dsc::init((size_t) 1 << 28);
    const int rows = 3, T = 5001;
    std::vector<double> hx((size_t) rows * T), ramp((size_t) rows * T), wrapped((size_t) rows * T);
    unsigned s = 12345;
    for (auto &v : hx) {
        s = s * 1664525u + 1013904223u;
        v = (double) (s >> 8) / (1 << 24) - 0.5;
    }
    const double two_pi = 6.283185307179586;
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < T; ++j) {
            const double p = 0.3 + (0.7 + 0.4 * r) * j;                     // steps below pi
            ramp[(size_t) r * T + j] = p;
            wrapped[(size_t) r * T + j] = p - two_pi * std::floor((p + 3.0) / two_pi);
        }
    bool ok = true;
    double worst = 0;
    dsc::tensor<double> x(hx.data(), {rows, T});
    auto c = dsc::cumsum(x);
    ok = ok && c.ndim() == 2 && c.dim(0) == rows && c.dim(1) == T && c.dtype() == DSC_F64;
    const auto hc = c.to_host<double>();
    for (int r = 0; r < rows; ++r) {
        long double acc = 0, mag = 0;
        for (int j = 0; j < T; ++j) {
            acc += hx[(size_t) r * T + j];
            mag += std::fabs(hx[(size_t) r * T + j]);
            ok = ok && std::fabs((double) (hc[(size_t) r * T + j] - acc)) <= (j + 1) * 1.2e-16 * (double) mag;
        }
    }
    auto d = dsc::diff(c);
    ok = ok && d.dim(1) == T - 1;
    const auto hd = d.to_host<double>();
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j + 1 < T; ++j) worst = std::fmax(worst, std::fabs(hd[(size_t) r * (T - 1) + j] - hx[(size_t) r * T + j + 1]));
    ok = ok && worst < 1e-12;
    dsc::tensor<double> w(wrapped.data(), {rows, T});
    auto u = dsc::unwrap(w);
    const auto hu = u.to_host<double>();
    double off = 0;
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < T; ++j)
            off = std::fmax(off, std::fabs(hu[(size_t) r * T + j] - hu[(size_t) r * T] - (ramp[(size_t) r * T + j] - ramp[(size_t) r * T])));
    ok = ok && off < 1e-8;
    std::vector<dsc_c64> hz((size_t) rows * T);                            // phase(exp(i ramp)) is the ramp again, from its first angle on
    for (size_t i = 0; i < hz.size(); ++i) hz[i] = dsc_c64{std::cos(ramp[i]), std::sin(ramp[i])};
    dsc::tensor<dsc_c64> z(hz.data(), {rows, T});
    auto ph = dsc::phase(z);
    ok = ok && ph.dtype() == DSC_F64 && ph.dim(1) == T;
    const auto hp = ph.to_host<double>();
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < T; ++j)
            off = std::fmax(off, std::fabs(hp[(size_t) r * T + j] - hp[(size_t) r * T] - (ramp[(size_t) r * T + j] - ramp[(size_t) r * T])));
    ok = ok && off < 1e-8;
    std::printf("%s: diff(cumsum) error %.3e, unwrap error %.3e\n", ok ? "scan templates ok" : "FAILED", worst, off);
    dsc::synchronize();
    return ok ? 0 : 1;
}
