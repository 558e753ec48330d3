// Compile-and-link check of dsc::roll / flip / fftshift / ifftshift / pad (dsc_amd/api/dsc_api.h); with a GPU, one call of each on a
// tiny tensor against values written out by hand.
#include "dsc_api.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

template<typename T>
static bool is(const dsc::tensor<T> &t, std::initializer_list<int> shape, std::initializer_list<T> want, const char *what) {
    const std::vector<int> s(shape);
    const std::vector<T> w(want);
    bool ok = t.ndim() == (int) s.size() && t.ne() == (int) w.size();
    for (int i = 0; ok && i < (int) s.size(); ++i) ok = t.dim(i) == s[i];
    if (ok) {
        const std::vector<T> got = t.template to_host<T>();
        for (size_t i = 0; i < w.size(); ++i) ok = ok && got[i] == w[i];
    }
    if (!ok) std::printf("FAILED: %s\n", what);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 2 || std::atoi(argv[1]) == 0) {
        std::printf("linked: %p %p %p %p %p\n", (void *) &dsc_roll, (void *) &dsc_flip, (void *) &dsc_fftshift, (void *) &dsc_ifftshift, (void *) &dsc_pad);
        return 0;
    }
    dsc::init((size_t) 1 << 28);
    const float h[6] = {0, 1, 2, 3, 4, 5};
    const dsc::tensor<float> x(h, {2, 3});                                 // [[0, 1, 2], [3, 4, 5]]
    const float h5[5] = {0, 1, 2, 3, 4};
    const dsc::tensor<float> v(h5, 5);
    bool ok = true;
    ok = is(dsc::roll(x, 1), {2, 3}, {5.f, 0.f, 1.f, 2.f, 3.f, 4.f}, "roll, flattened") && ok;
    ok = is(dsc::roll(x, -1, 1), {2, 3}, {1.f, 2.f, 0.f, 4.f, 5.f, 3.f}, "roll, axis 1") && ok;
    ok = is(dsc::roll(x, {1, 4}, {0, -1}), {2, 3}, {5.f, 3.f, 4.f, 2.f, 0.f, 1.f}, "roll, two axes") && ok;
    ok = is(dsc::flip(x), {2, 3}, {5.f, 4.f, 3.f, 2.f, 1.f, 0.f}, "flip, every axis") && ok;
    ok = is(dsc::flip(x, {1}), {2, 3}, {2.f, 1.f, 0.f, 5.f, 4.f, 3.f}, "flip, axis 1") && ok;
    ok = is(dsc::fftshift(v), {5}, {3.f, 4.f, 0.f, 1.f, 2.f}, "fftshift") && ok;
    ok = is(dsc::ifftshift(v), {5}, {2.f, 3.f, 4.f, 0.f, 1.f}, "ifftshift") && ok;
    ok = is(dsc::fftshift(x, {-1}), {2, 3}, {2.f, 0.f, 1.f, 5.f, 3.f, 4.f}, "fftshift, last axis") && ok;
    ok = is(dsc::pad(v, {2, 3}, 2), {10}, {2.f, 1.f, 0.f, 1.f, 2.f, 3.f, 4.f, 3.f, 2.f, 1.f}, "pad, reflect") && ok;
    ok = is(dsc::pad(v, {2, 1}, 3), {8}, {1.f, 0.f, 0.f, 1.f, 2.f, 3.f, 4.f, 4.f}, "pad, symmetric") && ok;
    ok = is(dsc::pad(v, {1, 2}, 4), {8}, {4.f, 0.f, 1.f, 2.f, 3.f, 4.f, 0.f, 1.f}, "pad, wrap") && ok;
    ok = is(dsc::pad(v, {2, 1}, 1), {8}, {0.f, 0.f, 0.f, 1.f, 2.f, 3.f, 4.f, 4.f}, "pad, edge") && ok;
    ok = is(dsc::pad(x, {1, 0, 0, 1}, 0, 9.0), {3, 4}, {9.f, 9.f, 9.f, 9.f, 0.f, 1.f, 2.f, 9.f, 3.f, 4.f, 5.f, 9.f}, "pad, constant") && ok;
    const dsc_c32 hz[2] = {{1, 2}, {3, 4}};
    const dsc::tensor<dsc_c32> z(hz, 2);
    const std::vector<dsc_c32> pz = dsc::pad(z, {1, 0}, 0, 0.5, -0.25).to_host<dsc_c32>();
    ok = ok && pz.size() == 3 && pz[0].real == 0.5f && pz[0].imag == -0.25f && pz[1].real == 1 && pz[2].imag == 4;
    std::printf("%s\n", ok ? "remap templates ok" : "FAILED");
    dsc::synchronize();
    return ok ? 0 : 1;
}
