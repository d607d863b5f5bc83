// motion_fill_check.cpp — the HIP-free rules of the dense composition of a motion segmentation (DESIGN.md section 31;
// csrc/eincm_motion_fill.h) as a program of its own: the argument check in its order, the layout of the five outputs, the packed column
// record, the key and its order, and the feature transform - the two column sweeps and the row search as the kernels run them - on a
// mask.  tests/test_host_motion_fill.py builds it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   check in_flight has_outputs staged model_set fp64 sharded n_models flags n_coeffs B n_events[B] has_coeffs coeffs[B n_coeffs]?
//         ntiles tilecount[B ntiles] W min_site_mass   ->  check fault code where_b where_i |
//   layout G H W   ->  layout | theta_offset[G] | labels_offset[G] | dist2_offset[G] | nearest_offset[G] | n_sites_offset[G]
//   pack dist y   ->  pack rec dist y |                   (y -1 with dist 65535: the no-site record)
//   key dist y dx xs   ->  key key |                      (dist 65535, y -1: no site)
//   site K min_site_mass mass[K]   ->  site 0|1 |
//   ft H W site[H W]   ->  ft | rec[H W] | nearest[H W] | dist2[H W]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_motion_fill.h"

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
            const int W = (int)num();
            const uint32_t min_site_mass = (uint32_t)u64();
            st.n_windows = B; st.n_events = ne.data(); st.tilecount = tc.data(); st.n_tilecounts = (int64_t)tc.size();
            int wb = 0; int64_t wi = 0;
            const int f = mf_check(st, W, n_models, has_coeffs ? co.data() : nullptr, flags, min_site_mass, &wb, &wi);
            if ((f == MF_OK) != (mf_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d %d %lld |\n", f, mf_code(f), wb, (long long)wi);
        } else if (tok[0] == "layout") {
            const int G = (int)num(), H = (int)num(), W = (int)num();
            std::printf("layout |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)mf_theta_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)mf_labels_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)mf_dist2_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)mf_nearest_offset(g, H, W));
            std::printf(" |");
            for (int g = 0; g < G; ++g) std::printf(" %lld", (long long)mf_nsites_offset(g));
            std::printf("\n");
        } else if (tok[0] == "pack") {
            const int dist = (int)num(), y = (int)num();
            const uint32_t rec = y < 0 ? MF_REC_NONE : mf_pack(dist, y);
            std::printf("pack %u %d %d |\n", (unsigned)rec, mf_rec_dist(rec), rec == MF_REC_NONE ? -1 : mf_rec_y(rec));
        } else if (tok[0] == "key") {
            const int dist = (int)num(), y = (int)num();
            const uint32_t dx = (uint32_t)u64();
            const int xs = (int)num();
            std::printf("key %llu |\n", (unsigned long long)mf_key(y < 0 ? MF_REC_NONE : mf_pack(dist, y), dx, xs));
        } else if (tok[0] == "site") {
            const int K = (int)num();
            const uint32_t min_site_mass = (uint32_t)u64();
            std::vector<uint32_t> m((size_t)K);
            for (auto& v : m) v = (uint32_t)u64();
            std::printf("site %d |\n", mf_is_site(m.data(), K, 1, min_site_mass) ? 1 : 0);
        } else if (tok[0] == "ft") {
            const int H = (int)num(), W = (int)num();
            std::vector<uint8_t> site((size_t)H * W);
            for (auto& v : site) v = (uint8_t)num();
            std::vector<uint32_t> rec((size_t)H * W);                                // exactly H * W: the sanitizer sees a read past a row
            for (int x = 0; x < W; ++x) {                                            // k_mf_cols, one column after the other
                int above = -1, below = -1;
                for (int y = 0; y < H; ++y) rec[(size_t)y * W + x] = mf_col_down(site[(size_t)y * W + x] != 0, y, above);
                for (int y = H - 1; y >= 0; --y) rec[(size_t)y * W + x] = mf_col_up(rec[(size_t)y * W + x], y, below);
            }
            std::printf("ft |");
            for (uint32_t r : rec) std::printf(" %u", (unsigned)r);
            std::vector<uint64_t> key((size_t)H * W);
            for (int y = 0; y < H; ++y) {                                            // k_mf_rows: a row of its own, as the LDS copy is
                const std::vector<uint32_t> row(rec.begin() + (size_t)y * W, rec.begin() + (size_t)(y + 1) * W);
                for (int x = 0; x < W; ++x) key[(size_t)y * W + x] = mf_row_search(row.data(), W, x);
            }
            std::printf(" |");
            for (uint64_t q : key) std::printf(" %d", (int)mf_key_nearest(q, W));
            std::printf(" |");
            for (uint64_t q : key) std::printf(" %u", (unsigned)mf_key_dist2(q));
            std::printf("\n");
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
