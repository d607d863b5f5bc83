// motion_layers_check.cpp — the HIP-free rules of the composition of a motion segmentation (DESIGN.md section 30;
// csrc/eincm_motion_layers.h) as a program of its own: the argument check in its order, the layout of the four outputs, and the four
// per-pixel functions the kernels run.  tests/test_host_motion_layers.py builds it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   check in_flight has_outputs staged model_set fp64 sharded n_models flags n_coeffs B n_events[B] has_coeffs coeffs[B n_coeffs]?
//         ntiles tilecount[B ntiles]   ->  check fault code where_b where_i |
//   layout G K H W   ->  layout | theta_offset[G] | labels_offset[G] | mass_offset[G K] | total_offset[G K]
//   q n w[n]   ->  q | q(w)[n]                         (w: floats)
//   label K mass[K]   ->  label l |                    dominant K total[K]   ->  dominant d |
//   blend K mass[K] f[K 2]   ->  blend | out[2]        (%.17g: the doubles read back exactly)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_motion_layers.h"

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
            MlState st{};
            st.in_flight = num() != 0; st.has_outputs = num() != 0; st.staged = num() != 0; st.model_set = num() != 0;
            st.fp64 = num() != 0; st.sharded = num() != 0;
            const int n_models = (int)num();
            const unsigned flags = (unsigned)u64();
            st.n_coeffs = (int)num();
            const int B = (int)num();
            std::vector<int64_t> ne((size_t)B);                                      // exactly B: the sanitizer sees a read past it
            for (auto& v : ne) v = (int64_t)num();
            const int has_coeffs = (int)num();
            std::vector<double> co;
            if (has_coeffs) { co.resize((size_t)B * st.n_coeffs); for (auto& v : co) v = num(); }
            const int ntiles = (int)num();
            std::vector<int32_t> tc((size_t)B * ntiles);
            for (auto& v : tc) v = (int32_t)num();
            st.n_windows = B; st.n_events = ne.data(); st.tilecount = tc.data(); st.n_tilecounts = (int64_t)tc.size();
            int wb = 0; int64_t wi = 0;
            const MlFault f = ml_check(st, n_models, has_coeffs ? co.data() : nullptr, flags, &wb, &wi);
            if ((f == ML_OK) != (ml_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d %d %lld |\n", (int)f, ml_code(f), wb, (long long)wi);
        } else if (tok[0] == "layout") {
            const int G = (int)num(), K = (int)num(), H = (int)num(), W = (int)num();
            std::printf("layout |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)ml_theta_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)ml_labels_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)ml_mass_offset(g, l, K, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)ml_total_offset(g, l, K));
            std::printf("\n");
        } else if (tok[0] == "q") {
            const int n = (int)num();
            std::printf("q |");
            for (int i = 0; i < n; ++i) std::printf(" %u", (unsigned)ml_q((float)num()));
            std::printf("\n");
        } else if (tok[0] == "label") {
            const int K = (int)num();
            std::vector<uint32_t> m((size_t)K);
            for (auto& v : m) v = (uint32_t)u64();
            std::printf("label %d |\n", ml_label(m.data(), K));
        } else if (tok[0] == "dominant") {
            const int K = (int)num();
            std::vector<uint64_t> t((size_t)K);
            for (auto& v : t) v = u64();
            std::printf("dominant %d |\n", ml_dominant(t.data(), K));
        } else if (tok[0] == "blend") {
            const int K = (int)num();
            std::vector<uint32_t> m((size_t)K);
            for (auto& v : m) v = (uint32_t)u64();
            std::vector<double> f((size_t)K * 2);
            for (auto& v : f) v = num();
            double out[2];
            ml_soft_blend(m.data(), K, f.data(), out);
            std::printf("blend | %.17g %.17g\n", out[0], out[1]);
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
