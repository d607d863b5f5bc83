// label_prior_check.cpp — the HIP-free rules of the per-pixel label prior (csrc/eincm_label_prior.h) and of the
// E-step with a prior image (csrc/eincm_responsibilities.h: rs_spatial_check) as a program of its own: the argument checks in their
// order, the layout of the two outputs, and the per-pixel function the kernel runs.  tests/test_host_label_prior.py builds it with the
// sanitizers and compares its lines with numpy.
//
// One case per input line:
//   check in_flight staged fp64 sharded n_models radius flags B n_events[B] ntiles tilecount[B ntiles]
//         ->  check fault code where_b where_i |
//   layout G K H W   ->  layout | prior_offset[G K] | smoothed_offset[G K]
//   prior K floor_mass S[K]   ->  prior | out[K]        (%.9g: the floats read back exactly)
//   spatial has_images flags prior_staged B npix values[B npix]?   ->  spatial fault code where_b where_p |
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_label_prior.h"
#include "eincm_responsibilities.h"

using namespace eincm;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::vector<std::string> tok;
        for (std::string t; s >> t;) tok.push_back(t);
        if (tok.empty()) return 3;
        size_t k = 1;
        auto num = [&]() { return std::strtod(tok.at(k++).c_str(), nullptr); };      // (strtod reads nan and inf)
        auto u64 = [&]() { return (uint64_t)std::strtoull(tok.at(k++).c_str(), nullptr, 10); };
        if (tok[0] == "check") {
            LpState st{};
            st.in_flight = num() != 0; st.staged = num() != 0; st.fp64 = num() != 0; st.sharded = num() != 0;
            const int n_models = (int)num(), radius = (int)num();
            const unsigned flags = (unsigned)u64();
            const int B = (int)num();
            std::vector<int64_t> ne((size_t)B);                                      // exactly B: the sanitizer sees a read past it
            for (auto& v : ne) v = (int64_t)num();
            const int ntiles = (int)num();
            std::vector<int32_t> tc((size_t)B * ntiles);
            for (auto& v : tc) v = (int32_t)num();
            st.n_windows = B; st.n_events = ne.data(); st.tilecount = tc.data(); st.n_tilecounts = (int64_t)tc.size();
            int wb = 0; int64_t wi = 0;
            const LpFault f = lp_check(st, n_models, radius, flags, &wb, &wi);
            if ((f == LP_OK) != (lp_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d %d %lld |\n", (int)f, lp_code(f), wb, (long long)wi);
        } else if (tok[0] == "layout") {
            const int G = (int)num(), K = (int)num(), H = (int)num(), W = (int)num();
            std::printf("layout |");
            for (int b = 0; b < G * K; ++b) std::printf(" %lld", (long long)lp_prior_offset(b, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)lp_smoothed_offset(g, l, K, H, W));
            std::printf("\n");
        } else if (tok[0] == "prior") {
            const int K = (int)num();
            const uint32_t floor_mass = (uint32_t)u64();
            std::vector<uint64_t> S((size_t)K);
            for (auto& v : S) v = u64();
            std::vector<float> out((size_t)K);
            lp_prior(S.data(), K, floor_mass, out.data());
            std::printf("prior |");
            for (float v : out) std::printf(" %.9g", (double)v);
            std::printf("\n");
        } else if (tok[0] == "spatial") {
            const int has_images = (int)num();
            const uint32_t flags = (uint32_t)u64();
            const bool prior_staged = num() != 0;
            const int B = (int)num();
            const int64_t npix = (int64_t)num();
            std::vector<float> v;
            if (has_images) { v.resize((size_t)B * (size_t)npix); for (auto& x : v) x = (float)num(); }
            int wb = 0; int64_t wp = 0;
            const RsSpatialFault f = rs_spatial_check(has_images ? v.data() : nullptr, flags, prior_staged, B, npix, &wb, &wp);
            if ((f == RSS_OK) != (rs_spatial_why(f)[0] == '\0')) return 5;
            std::printf("spatial %d %d %d %lld |\n", (int)f, rs_spatial_code(f), wb, (long long)wp);
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
