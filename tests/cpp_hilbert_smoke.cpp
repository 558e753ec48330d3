// Compile-and-link check of dsc::hilbert / dsc::envelope (dsc_amd/api/dsc_api.h); with a GPU it takes rows of cos(2 pi m j / N) at a
// fused length (1024) and a composed one (64): the analytic signal is cos + i sin, the envelope 1, the real part the input itself.
#include "dsc_api.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p\n", (void *) &dsc_hilbert, (void *) &dsc_envelope);
        return 0;
    }
    dsc::init((size_t) 1 << 30);
    const double pi = 3.14159265358979323846;
    bool ok = true;
    double worst = 0;
    for (const int N : {1024, 64}) {
        const int rows = 3, tones[rows] = {1, 5, N / 4};
        std::vector<double> hx((size_t) rows * N);
        for (int r = 0; r < rows; ++r)
            for (int j = 0; j < N; ++j) hx[(size_t) r * N + j] = std::cos(2 * pi * (double) ((tones[r] * j) % N) / N);
        dsc::tensor<double> x(hx.data(), {rows, N});
        auto z = dsc::hilbert(x);
        auto e = dsc::envelope(x);
        ok = ok && z.ndim() == 2 && z.dim(0) == rows && z.dim(1) == N && z.dtype() == DSC_C64;
        ok = ok && e.ndim() == 2 && e.dim(0) == rows && e.dim(1) == N && e.dtype() == DSC_F64;
        const auto hz = z.to_host<dsc_c64>();
        const auto he = e.to_host<double>();
        for (int r = 0; r < rows; ++r)
            for (int j = 0; j < N; ++j) {
                const size_t i = (size_t) r * N + j;
                ok = ok && hz[i].real == hx[i];
                const double want = std::sin(2 * pi * (double) ((tones[r] * j) % N) / N);
                worst = std::fmax(worst, std::fmax(std::fabs(hz[i].imag - want), std::fabs(he[i] - 1.0)));
            }
    }
    ok = ok && worst < 1e-13;
    std::printf("%s: max abs error %.3e\n", ok ? "hilbert templates ok" : "FAILED", worst);
    dsc::synchronize();
    return ok ? 0 : 1;
}
