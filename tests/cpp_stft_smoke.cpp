// Compile-and-link check of dsc::stft / dsc::istft (dsc_amd/api/dsc_api.h); with a GPU it runs a round trip istft(stft(x)) = x
// with a periodic Hann window at hop n_fft / 4 and checks one bin against its DFT sum on the host.
#include "dsc_api.h"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p\n", (void *) &dsc_stft, (void *) &dsc_istft);
        return 0;
    }
    dsc::init((size_t) 1 << 30);
    const int n_fft = 256, hop = 64, T = 4000;
    std::vector<double> hx(T), hw(n_fft);
    for (int i = 0; i < T; ++i) hx[i] = std::cos(2 * M_PI * 16.0 * i / n_fft) + 0.25 * std::sin(0.37 * i);
    for (int j = 0; j < n_fft; ++j) hw[j] = 0.5 - 0.5 * std::cos(2 * M_PI * j / n_fft);
    dsc::tensor<double> x(hx.data(), T), w(hw.data(), n_fft);
    auto X = dsc::stft(x, n_fft, hop, &w);
    const bool shape_ok = X.ndim() == 2 && X.dim(0) == 1 + T / hop && X.dim(1) == n_fft / 2 + 1;
    auto y = dsc::istft(X, n_fft, hop, &w, true, T);
    const auto hy = y.to_host();
    double err = 0, ref = 0;
    for (int i = 0; i < T; ++i) { err += (hy[i] - hx[i]) * (hy[i] - hx[i]); ref += hx[i] * hx[i]; }
    const double rel = std::sqrt(err / ref);
    const auto hX = X.to_host<std::complex<double>>();
    // interior frame 10 (samples 10 hop - n_fft/2 ..), bin 16, against its DFT sum on the host
    std::complex<double> want = 0;
    for (int j = 0; j < n_fft; ++j) want += hx[10 * hop - n_fft / 2 + j] * hw[j] * std::polar(1.0, -2 * M_PI * 16.0 * j / n_fft);
    const double bin_err = std::abs(hX[(size_t) 10 * (n_fft / 2 + 1) + 16] - want) / std::abs(want);
    const bool ok = shape_ok && rel < 1e-12 && bin_err < 1e-12;
    std::printf("%s: shape %d rel %.3e bin %.3e\n", ok ? "stft templates ok" : "FAILED", (int) shape_ok, rel, bin_err);
    dsc::synchronize();
    return ok ? 0 : 1;
}
