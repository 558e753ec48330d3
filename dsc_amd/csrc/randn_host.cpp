// randn_host.cpp — the f64 sequence of dsc_randn (dsc.cpp:501-534), in a translation unit of its own.
//
// dsc_randn reproduces the reference's values bit for bit: a default-constructed std::mt19937 feeding
// std::normal_distribution<T> (libstdc++'s polar method).  The reference is built with -ffp-contract=fast for an FMA
// target, and there the f64 instantiation's `x * x + y * y` becomes a fused multiply-add, which changes the rounding of
// about one value in seven; its f32 instantiation comes out as plain multiplies and adds.  This file is therefore compiled
// with FMA enabled (Makefile: FLAGS_randn_host) and holds the f64 generator only; the f32 one stays in dsc_capi.cpp, built
// without.  Both were checked value by value against the reference build on 100000 samples.
#include <cstddef>
#include <random>

void dsc_randn_host_f64(double *dst, size_t n) {
    std::mt19937 rng;
    std::normal_distribution<double> dist;
    for (size_t i = 0; i < n; ++i) dst[i] = dist(rng);
}
