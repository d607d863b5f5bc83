// responsibilities_check.cpp — the HIP-free rules of the E-step operator (csrc/eincm_responsibilities.h) as a
// program of its own: the argument check in its order and the layout of the weights' and the labels' blocks.
// tests/test_host_responsibilities.py builds it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   check in_flight has_outputs staged have_eval fp64 splat_size sharded has_images masked n_models n_refs has_rw rw[n_refs]?
//         has_prior B n_events[B] prior[B]?   ->  check fault code |
//   layout n_models B n_events[B]   ->  layout weights_total labels_total | weights_offset[B] | labels_offset[G] | group_events[G]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

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
        if (tok[0] == "check") {
            RsState st{};
            st.sc.in_flight = num() != 0; st.sc.has_scores = num() != 0; st.sc.staged = num() != 0; st.sc.have_eval = num() != 0;
            st.sc.fp64 = num() != 0; st.sc.splat_size = (int)num(); st.sc.sharded = num() != 0; st.sc.has_images = num() != 0;
            st.sc.masked = num() != 0;
            const int n_models = (int)num(), n_refs = (int)num(), has_rw = (int)num();
            std::vector<double> rw;
            if (has_rw) { rw.resize((size_t)n_refs); for (auto& v : rw) v = num(); }
            const int has_prior = (int)num(), B = (int)num();
            std::vector<int64_t> ne((size_t)B);                                      // exactly B: the sanitizer sees a read past it
            for (auto& v : ne) v = (int64_t)num();
            std::vector<double> prior;
            if (has_prior) { prior.resize((size_t)B); for (auto& v : prior) v = num(); }
            st.n_windows = B; st.n_events = ne.data();
            const RsFault f = rs_check(st, n_models, has_rw ? rw.data() : nullptr, n_refs, has_prior ? prior.data() : nullptr);
            if ((f == RS_OK) != (rs_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d |\n", (int)f, rs_code(f));
        } else if (tok[0] == "layout") {
            const int K = (int)num(), B = (int)num();
            std::vector<int64_t> ne((size_t)B);
            for (auto& v : ne) v = (int64_t)num();
            const int G = B / K;
            std::printf("layout %lld %lld |", (long long)rs_weights_total(ne.data(), B), (long long)rs_labels_total(ne.data(), B, K));
            for (int b = 0; b < B; ++b) std::printf(" %lld", (long long)rs_weights_offset(ne.data(), b));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)rs_labels_offset(ne.data(), g, K));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)rs_group_events(ne.data(), g, K));
            std::printf("\n");
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
