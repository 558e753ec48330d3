// Stand-alone host program over dsc_amd/csrc/remap_plan.h, the integer arithmetic of dsc_roll / dsc_flip / dsc_fftshift / dsc_ifftshift /
// dsc_pad: the very functions remap.cpp plans with and remap.hip indexes with, with no device and no library.  tests/test_remap_abi.py
// builds it with -fsanitize=address,undefined, feeds it requests on stdin and compares the answers with numpy.
//   map roll N SHIFT | map flip N | map pad N BEFORE AFTER MODE      -> the source index of every output index (-1: the constant)
//   plan EB ALIGNED AXIS AXIS AXIS AXIS, AXIS = id:N | roll:N:SHIFT | flip:N | pad:N:BEFORE:AFTER:MODE
//                                                                    -> the merged axes (n_in n_out kind a b each), ne_out and the route
#include "remap_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static dsc_axis_map parse_axis(const std::string &spec) {
    std::vector<long long> v;
    const size_t colon = spec.find(':');
    const std::string op = spec.substr(0, colon);
    for (size_t at = colon; at != std::string::npos; at = spec.find(':', at + 1)) v.push_back(std::atoll(spec.c_str() + at + 1));
    if (op == "id" && v.size() == 1) return dsc_map_identity((int) v[0]);
    if (op == "roll" && v.size() == 2) return dsc_map_roll((int) v[0], v[1]);
    if (op == "flip" && v.size() == 1) return dsc_map_flip((int) v[0]);
    if (op == "pad" && v.size() == 4) return dsc_map_pad((int) v[0], v[1], v[2], (int) v[3]);
    std::fprintf(stderr, "bad axis \"%s\"\n", spec.c_str());
    std::exit(2);
}

int main() {
    char line[512];
    while (std::fgets(line, sizeof(line), stdin)) {
        std::vector<std::string> w;
        for (char *t = std::strtok(line, " \n"); t != nullptr; t = std::strtok(nullptr, " \n")) w.push_back(t);
        if (w.empty()) continue;
        if (w[0] == "map" && w.size() >= 3) {
            std::string spec = w[1];
            for (size_t i = 2; i < w.size(); ++i) spec += ":" + w[i];
            const dsc_axis_map m = parse_axis(spec);
            for (int j = 0; j < m.n_out; ++j) std::printf(j ? " %d" : "%d", dsc_map_index(m, j));
            std::printf("\n");
        } else if (w[0] == "plan" && w.size() == 3 + DSC_REMAP_DIMS) {
            dsc_remap p{};
            for (int i = 0; i < DSC_REMAP_DIMS; ++i) p.ax[i] = parse_axis(w[3 + i]);
            dsc_remap_merge(p);
            for (int i = 0; i < DSC_REMAP_DIMS; ++i) std::printf("%d %d %d %lld %lld ", p.ax[i].n_in, p.ax[i].n_out, p.ax[i].kind, p.ax[i].a, p.ax[i].b);
            std::printf("%lld %d\n", p.ne_out, dsc_remap_route(p, std::atoi(w[1].c_str()), std::atoi(w[2].c_str()) != 0));
        } else {
            std::fprintf(stderr, "bad request \"%s\"\n", w[0].c_str());
            return 2;
        }
    }
    return 0;
}
