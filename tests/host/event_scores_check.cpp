// event_scores_check.cpp — the HIP-free rules of the per-event scores (csrc/eincm_event_scores.h) as a program of
// its own: the argument check in its order and the layout of the output blocks in both forms.  tests/test_host_event_scores.py builds
// it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   check in_flight has_scores staged have_eval fp64 splat_size sharded has_images masked n_refs has_rw rw[n_refs]?
//          ->  check fault code |
//   layout n_refs combined B n_events[B]   ->  layout total | offset[B] | length[B]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_event_scores.h"

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
            ScState st{};
            st.in_flight = num() != 0; st.has_scores = num() != 0; st.staged = num() != 0; st.have_eval = num() != 0;
            st.fp64 = num() != 0; st.splat_size = (int)num(); st.sharded = num() != 0; st.has_images = num() != 0; st.masked = num() != 0;
            const int n_refs = (int)num(), has_rw = (int)num();
            std::vector<double> rw;
            if (has_rw) { rw.resize((size_t)n_refs); for (auto& v : rw) v = num(); }
            const ScFault f = sc_check(st, has_rw ? rw.data() : nullptr, n_refs);
            if ((f == SC_OK) != (sc_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d |\n", (int)f, sc_code(f));
        } else if (tok[0] == "layout") {
            const int n_refs = (int)num(), combined = (int)num(), B = (int)num();
            std::vector<int64_t> ne((size_t)B);
            for (auto& v : ne) v = (int64_t)num();
            std::printf("layout %lld |", (long long)sc_total(ne.data(), B, n_refs, combined != 0));
            for (int b = 0; b < B; ++b) std::printf(" %lld", (long long)sc_block_offset(ne.data(), b, n_refs, combined != 0));
            std::printf(" |");
            for (int b = 0; b < B; ++b) std::printf(" %lld", (long long)sc_block_len(ne[(size_t)b], n_refs, combined != 0));
            std::printf("\n");
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
