// Compile-and-link check of the math templates of dsc_amd/api/dsc_api.h (dsc::cos .. sqrt, pow, i0, clip, arange, randn,
// reshape, concat); with a GPU it runs them and compares against host arithmetic in double.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static bool close(double got, double want, double rel) { return std::fabs(got - want) <= rel * std::fabs(want) + 1e-30; }

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p\n", (void *) &dsc_pow, (void *) &dsc_reshape, (void *) &dsc_concat);
        return 0;
    }
    dsc::init((size_t) 1 << 30);
    bool ok = true;
    auto expect = [&](bool c, const char *what) { if (!c) { ok = false; std::printf("FAILED: %s\n", what); } };

    // arange -> x / 10 -> the unary templates, against libm in double
    const int n = 37;
    auto x = dsc::arange<double>(n) / 10.0;
    const auto hx = x.to_host();
    const struct { dsc::tensor<double> t; double (*f)(double); const char *name; } un[] = {
        {dsc::cos(x), [](double v) { return std::cos(v); }, "cos"},
        {dsc::sin(x), [](double v) { return std::sin(v); }, "sin"},
        {dsc::exp(x), [](double v) { return std::exp(v); }, "exp"},
        {dsc::sqrt(x), [](double v) { return std::sqrt(v); }, "sqrt"},
        {dsc::log2(x + 1.0), [](double v) { return std::log2(v + 1); }, "log2"},
        {dsc::log10(x + 1.0), [](double v) { return std::log10(v + 1); }, "log10"},
        {dsc::logn(x + 1.0), [](double v) { return std::log(v + 1); }, "logn"},
        {dsc::sinc(x), [](double v) { return v == 0 ? 1.0 : std::sin(M_PI * v) / (M_PI * v); }, "sinc"},
    };
    for (const auto &u : un) {
        const auto h = u.t.to_host();
        bool good = (int) h.size() == n;
        for (int i = 0; i < n && good; ++i) good = close(h[i], u.f(hx[i]), 1e-13);
        expect(good, u.name);
    }
    {
        const auto h = dsc::pow(x, 2.5).to_host();
        bool good = true;
        for (int i = 0; i < n; ++i) good = good && close(h[i], std::pow(hx[i], 2.5), 1e-13);
        expect(good, "pow");
    }
    {
        const auto h = dsc::clip(x - 1.8, -0.5, 0.25).to_host();
        bool good = true;
        for (int i = 0; i < n; ++i) { const double v = hx[i] - 1.8; good = good && h[i] == (v > -0.5 ? (v < 0.25 ? v : 0.25) : -0.5); }
        expect(good, "clip");
    }
    {
        const auto h = dsc::i0(x).to_host();
        expect(close(h[0], 1.0, 0) && close(h[n - 1], 8.0277, 1e-4), "i0");       // I0(0) = 1, I0(3.6) = 8.02768 (A&S: 1e-7 relative)
    }
    {
        auto r = dsc::randn<float>({4, 6});
        auto v = dsc::reshape(r, 3, -1);
        expect(v.ndim() == 2 && v.dim(0) == 3 && v.dim(1) == 8 && v.raw()->data == r.raw()->data, "reshape");
        auto c = dsc::concat(0, v, v);
        const auto hc = c.to_host(), hv = v.to_host();
        bool good = c.dim(0) == 6 && c.dim(1) == 8;
        for (int i = 0; i < 48 && good; ++i) good = hc[i] == hv[i % 24];
        expect(good, "concat");
    }
    dsc::synchronize();
    std::printf("math templates %s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
