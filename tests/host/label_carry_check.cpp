// label_carry_check.cpp — the HIP-free rules of the label prior carried to the next window (DESIGN.md section 33;
// csrc/eincm_label_carry.h) as a program of its own: the two argument checks in their order, the resolve rule the kernel runs, the
// layout of the four outputs and the constants of the overflow proof.  tests/test_host_label_carry.py builds it with the sanitizers
// and compares its lines with numpy.
//
// One case per input line:
//   check in_flight staged fp64 sharded n_models radius flags has_coeffs has_tau model_set n_coeffs model_coeffs B n_events[B] ntiles
//         tilecount[B ntiles] tau[B / n_models, where the check reads them: has_tau and a whole number of groups]
//         ->  check fault code where_b where_i |
//   adopt in_flight staged valid k_models k_windows k_H k_W n_models n_windows H W   ->  adopt fault code |
//   resolve a[n]   ->  resolve | c[n]
//   layout G K H W   ->  layout | prior_offset[G K] | carried_offset[G K] | accum_offset[G K] | dropped_offset[G K]
//   constants   ->  constants | shift full half carried_max events_max staging_events_max q_one | full * q_one * events_max (its high and its low 64 bits)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_label_carry.h"

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
            LcArgs a{};
            a.flags = (unsigned)u64();
            a.has_coeffs = num() != 0; a.has_tau = num() != 0; a.model_set = num() != 0;
            a.n_coeffs = (int)num(); a.model_coeffs = (int)num();
            const int B = (int)num();
            std::vector<int64_t> ne((size_t)B);                                      // exactly B: the sanitizer sees a read past it
            for (auto& v : ne) v = (int64_t)u64();
            const int ntiles = (int)num();
            std::vector<int32_t> tc((size_t)B * ntiles);
            for (auto& v : tc) v = (int32_t)num();
            std::vector<double> tau(tok.size() - k);                                 // exactly what the case hands over
            for (auto& v : tau) v = num();
            a.tau = a.has_tau ? tau.data() : nullptr;
            st.n_windows = B; st.n_events = ne.data(); st.tilecount = tc.data(); st.n_tilecounts = (int64_t)tc.size();
            int wb = 0; int64_t wi = 0;
            const int f = lc_check(st, a, n_models, radius, &wb, &wi);
            if ((f == LC_OK) != (lc_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d %d %lld |\n", f, lc_code(f), wb, (long long)wi);
        } else if (tok[0] == "adopt") {
            const bool in_flight = num() != 0, staged = num() != 0;
            LcCarried c{};
            c.valid = num() != 0; c.n_models = (int)num(); c.n_windows = (int)num(); c.H = (int)num(); c.W = (int)num();
            const int n_models = (int)num(), n_windows = (int)num(), H = (int)num(), W = (int)num();
            const LcAdoptFault f = lc_adopt_check(in_flight, staged, c, n_models, n_windows, H, W);
            if ((f == LCA_OK) != (lc_adopt_why(f)[0] == '\0')) return 5;
            std::printf("adopt %d %d |\n", (int)f, lc_adopt_code(f));
        } else if (tok[0] == "resolve") {
            std::printf("resolve |");
            while (k < tok.size()) std::printf(" %lu", (unsigned long)lc_resolve(u64()));
            std::printf("\n");
        } else if (tok[0] == "layout") {
            const int G = (int)num(), K = (int)num(), H = (int)num(), W = (int)num();
            std::printf("layout |");
            for (int b = 0; b < G * K; ++b) std::printf(" %lld", (long long)lc_prior_offset(b, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)lc_carried_offset(g, l, K, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)lc_accum_offset(g, l, K, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) for (int l = 0; l < K; ++l) std::printf(" %lld", (long long)lc_dropped_offset(g, l, K));
            std::printf("\n");
        } else if (tok[0] == "constants") {
            const unsigned __int128 top = (unsigned __int128)LC_FULL * ML_Q_ONE * (unsigned __int128)LC_EVENTS_MAX;
            std::printf("constants | %d %llu %llu %llu %lld %lld %u | %llu %llu\n", LC_SHIFT, (unsigned long long)LC_FULL, (unsigned long long)LC_HALF,
                        (unsigned long long)LC_CARRIED_MAX, (long long)LC_EVENTS_MAX, (long long)LC_STAGING_EVENTS_MAX, (unsigned)ML_Q_ONE,
                        (unsigned long long)(top >> 64), (unsigned long long)(top & ~0ull));
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
