// event_filter_check.cpp — the HIP-free rules of the refractory and polarity-aware event filter (DESIGN.md section 24;
// csrc/eincm_event_filter.h) as a program of its own: the argument checks, the refractory rule at its edges, and a sequential filter
// built from the header's functions and walked chunk by chunk.  tests/test_host_event_filter.py builds it with the sanitizers and
// compares its lines with numpy.
//
// One case per input line:
//   args n refractory tau radius full_support flags has_p            ->  args fault |
//   kept t prev_any refractory masked                                ->  kept 0|1 |
//   filter H W refractory tau r k polarity has_p has_mask nchunks len[nchunks] n  x[n] y[n] t[n] p[n]? mask[H W]?
//          ->  filter | keep .. | support .. | weights (as float bits) .. | last_any, last_kept[0], last_kept[1] (as double bits) ..
// filter walks the chunks as the kernels do: a pixel's previous event, and a neighbour's last kept event of a class, is the one in
// the current chunk where it has one, else the carried map's; the maps take the chunk's last ones after the chunk.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_event_filter.h"

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
        if (tok[0] == "args") {
            const int64_t n = (int64_t)num();
            const double rho = num(), tau = num();
            const int radius = (int)num(), fs = (int)num(), flags = (int)num(), has_p = (int)num();
            std::printf("args %d |\n", (int)ef_check_args(n, rho, tau, radius, fs, flags, has_p != 0));
        } else if (tok[0] == "kept") {
            const double t = num(), prev = num(), rho = num();
            const int masked = (int)num();
            std::printf("kept %d |\n", ef_kept(t, prev, rho, masked != 0) ? 1 : 0);
        } else if (tok[0] == "filter") {
            const int H = (int)num(), W = (int)num();
            const double rho = num(), tau = num();
            const int r = (int)num(), fs = (int)num(), polarity = (int)num(), has_p = (int)num(), has_mask = (int)num(), nchunks = (int)num();
            if (ef_check_args(0, rho, tau, r, fs, polarity ? EF_POLARITY : 0, has_p != 0) != EF_ARG_OK) return 8;
            std::vector<int64_t> len((size_t)nchunks);
            for (auto& v : len) v = (int64_t)num();
            const int64_t n = (int64_t)num();
            std::vector<int16_t> x((size_t)n), y((size_t)n);
            std::vector<double> t((size_t)n);
            std::vector<int8_t> p;
            for (auto& v : x) v = (int16_t)num();
            for (auto& v : y) v = (int16_t)num();
            for (auto& v : t) v = num();
            if (has_p) { p.resize((size_t)n); for (auto& v : p) v = (int8_t)num(); }
            std::vector<uint8_t> mask;
            if (has_mask) { mask.resize((size_t)H * W); for (auto& v : mask) v = (uint8_t)num(); }
            const size_t npix = (size_t)H * W;
            std::vector<double> any(npix, es_no_event()), lk[2] = {std::vector<double>(npix, es_no_event()), std::vector<double>(npix, es_no_event())};
            std::vector<int64_t> last(npix), lastk[2] = {std::vector<int64_t>(npix), std::vector<int64_t>(npix)};
            std::vector<int> keep((size_t)n), sup((size_t)n);
            std::vector<float> wt((size_t)n);
            double carried = es_no_event();
            int64_t e0 = 0;
            for (int c = 0; c < nchunks; ++c) {
                const int64_t e1 = e0 + len[(size_t)c];
                if (e1 > n) return 5;
                if (es_first_offender(H, W, x.data() + e0, y.data() + e0, t.data() + e0, e1 - e0, carried)) return 6;
                std::fill(last.begin(), last.end(), (int64_t)-1);
                for (auto& v : lastk) std::fill(v.begin(), v.end(), (int64_t)-1);
                for (int64_t e = e0; e < e1; ++e) {
                    const size_t px = (size_t)(y[(size_t)e] * W + x[(size_t)e]);
                    const double te = t[(size_t)e];
                    const int cls = has_p ? ef_class(p[(size_t)e]) : 0;
                    const double prev = last[px] >= 0 ? t[(size_t)last[px]] : any[px];
                    const bool kept = ef_kept(te, prev, rho, has_mask && mask[px]);
                    int cnt = 0;
                    if (kept && r > 0) {
                        const EsWindow w = es_window(H, W, x[(size_t)e], y[(size_t)e], r);
                        for (int qy = w.y0; qy <= w.y1; ++qy)
                            for (int qx = w.x0; qx <= w.x1; ++qx) {
                                const size_t q = (size_t)(qy * W + qx);
                                if (q == px || (has_mask && mask[q])) continue;
                                // the later of the two classes' in-chunk events is the later index; an in-chunk event is never older
                                // than the carried map's
                                const int64_t j = polarity ? lastk[cls][q] : std::max(lastk[0][q], lastk[1][q]);
                                const double tp = j >= 0 ? t[(size_t)j] : ef_last_kept(lk[0][q], lk[1][q], cls, polarity != 0);
                                cnt += es_supported(te, tp, tau) ? 1 : 0;
                            }
                    }
                    keep[(size_t)e] = kept ? 1 : 0;
                    sup[(size_t)e] = cnt;
                    wt[(size_t)e] = ef_weight(kept, cnt, r, fs);
                    last[px] = e;
                    if (kept) lastk[cls][px] = e;
                }
                for (size_t q = 0; q < npix; ++q) {
                    if (last[q] >= 0) any[q] = t[(size_t)last[q]];
                    for (int cl = 0; cl < 2; ++cl) if (lastk[cl][q] >= 0) lk[cl][q] = t[(size_t)lastk[cl][q]];
                }
                if (e1 > e0) carried = t[(size_t)e1 - 1];
                e0 = e1;
            }
            if (e0 != n) return 7;
            std::printf("filter |");
            for (int64_t e = 0; e < n; ++e) std::printf(" %d", keep[(size_t)e]);
            std::printf(" |");
            for (int64_t e = 0; e < n; ++e) std::printf(" %d", sup[(size_t)e]);
            std::printf(" |");
            for (int64_t e = 0; e < n; ++e) { uint32_t u; std::memcpy(&u, &wt[(size_t)e], 4); std::printf(" %u", u); }
            std::printf(" |");
            for (const std::vector<double>* mp : {&any, &lk[0], &lk[1]})
                for (size_t q = 0; q < npix; ++q) { uint64_t u; std::memcpy(&u, &(*mp)[q], 8); std::printf(" %llu", (unsigned long long)u); }
            std::printf("\n");
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
