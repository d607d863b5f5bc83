// contrast_landscape_check.cpp — the HIP-free rules of the contrast landscape (csrc/eincm_contrast_landscape.h) as
// a program of its own: the argument check in its order and the band plan.  tests/test_host_contrast_landscape.py builds it with the
// sanitizers and checks its lines.
//
// One case per input line:
//   check in_flight has_outputs staged model_set sharded B K V cell has_coeffs has_tref coeffs[B V K]? t_ref[B]?
//         ->  check fault code where_b where_i |
//   bands H W cell  ->  bands Hc Wc rows n_row_bands cols n_col_bands table n_bands lds_bytes | covered_min covered_max cells_max |
//         covered_*: over every cell, how many bands hold it; cells_max: the most cells any band holds
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_contrast_landscape.h"

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
            ClState st{};
            st.in_flight = num() != 0; st.has_outputs = num() != 0; st.staged = num() != 0; st.model_set = num() != 0; st.sharded = num() != 0;
            st.n_windows = (int)num(); st.n_coeffs = (int)num();
            const int V = (int)num(), cell = (int)num(), has_coeffs = (int)num(), has_tref = (int)num();
            std::vector<double> coeffs, tref;                                        // exactly sized: the sanitizer sees a read past them
            if (has_coeffs) { coeffs.resize((size_t)st.n_windows * (size_t)std::max(V, 0) * (size_t)st.n_coeffs); for (auto& v : coeffs) v = num(); }
            if (has_tref) { tref.resize((size_t)st.n_windows); for (auto& v : tref) v = num(); }
            int wb = -7; int64_t wi = -7;
            const ClFault f = cl_check(st, V, cell, has_coeffs ? coeffs.data() : nullptr, has_tref ? tref.data() : nullptr, &wb, &wi);
            if ((f == CL_OK) != (cl_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            if ((f == CL_NONFINITE) != (wb != -7)) return 6;                         // only that refusal says where
            std::printf("check %d %d %d %lld |\n", (int)f, cl_code(f), wb, (long long)wi);
        } else if (tok[0] == "bands") {
            const int H = (int)num(), W = (int)num(), cell = (int)num();
            const ClBands p = cl_bands(H, W, cell);
            // how often every cell row and every cell column is covered: a cell's count is the product, the bands being a grid
            std::vector<int> rows((size_t)p.Hc, 0), cols((size_t)p.Wc, 0);
            long long cells_max = 0;
            for (int rb = 0; rb < p.n_row_bands; ++rb) {
                const int r0 = rb * p.rows, nr = std::min(p.rows, p.Hc - r0);
                if (nr < 1) return 7;
                for (int r = r0; r < r0 + nr; ++r) rows.at((size_t)r)++;
                for (int cb = 0; cb < p.n_col_bands; ++cb) {
                    const int c0 = cb * p.cols, nc = std::min(p.cols, p.Wc - c0);
                    if (nc < 1) return 7;
                    if (rb == 0) for (int c = c0; c < c0 + nc; ++c) cols.at((size_t)c)++;
                    cells_max = std::max(cells_max, (long long)nr * nc);
                }
            }
            const int lo = *std::min_element(rows.begin(), rows.end()) * *std::min_element(cols.begin(), cols.end());
            const int hi = *std::max_element(rows.begin(), rows.end()) * *std::max_element(cols.begin(), cols.end());
            std::printf("bands %d %d %d %d %d %d %d %d %d | %d %d %lld |\n", p.Hc, p.Wc, p.rows, p.n_row_bands, p.cols, p.n_col_bands, p.table,
                        p.n_bands(), p.lds_bytes(), lo, hi, cells_max);
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
