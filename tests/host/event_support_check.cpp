// event_support_check.cpp — the HIP-free rules of the event-support filter (csrc/eincm_event_support.h) as a
// program of its own: the argument checks, the geometry of the sort by pixel (es_sort_plan; fits: every number on the way fits the
// type it is used in), the first refused event, the neighbour window clipped to the sensor, and the carried-time rule walked chunk by
// chunk.  tests/test_host_event_support.py builds it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   args n tau radius full_support                                   ->  args fault |
//   plan n npix                                                      ->  plan nblk nhist ntiles passes fits |
//   first H W carried n  x[n] y[n] t[n]                              ->  first index fault |
//   window H W r npts  x[npts] y[npts]                               ->  window | x0 x1 y0 y1 neighbours  (per point)
//   filter H W tau r k has_mask nchunks len[nchunks] n  x[n] y[n] t[n] mask[H W]?
//                                                                    ->  filter | support .. | weights (as float bits) .. | map (as double bits) ..
// filter walks the chunks as the kernels do: a neighbour's previous event is its last one in the current chunk where it has one, else
// the carried map's; the map takes every pixel's last time after the chunk.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_event_support.h"

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
            const double tau = num();
            const int radius = (int)num(), fs = (int)num();
            std::printf("args %d |\n", (int)es_check_args(n, tau, radius, fs));
        } else if (tok[0] == "plan") {
            const int64_t n = (int64_t)num(), npix = (int64_t)num();
            const EsSortPlan p = es_sort_plan(n, npix);
            // the same numbers in 64-bit unsigned arithmetic that cannot wrap at these sizes, and whether each fits where it is used:
            // nblk an int and a grid, nhist the int64_t length of the histogram whose uint32_t entries sum to n, ntiles a grid, the
            // key bits covered by the passes' shifts inside a uint32_t
            const uint64_t un = (uint64_t)n, nblk = (un + (uint64_t)ES_SORT_BLOCK - 1) / (uint64_t)ES_SORT_BLOCK;
            const uint64_t nhist = (uint64_t)ES_RADIX * nblk, ntiles = (nhist + (uint64_t)ES_SCAN_TILE - 1) / (uint64_t)ES_SCAN_TILE;
            const uint64_t hist_bytes = nhist * sizeof(uint32_t);
            const bool same = (uint64_t)p.nblk == nblk && (uint64_t)p.nhist == nhist && (uint64_t)p.ntiles == ntiles && p.nblk >= 0;
            const bool fits = nblk <= (uint64_t)INT32_MAX && nhist <= (uint64_t)INT32_MAX && ntiles <= (uint64_t)INT32_MAX &&
                              hist_bytes <= (uint64_t)INT64_MAX && un <= (uint64_t)UINT32_MAX && p.passes * ES_RADIX_BITS <= 32 &&
                              (npix <= 1 || ((uint64_t)(npix - 1) >> (p.passes * ES_RADIX_BITS - 1)) <= 1u) &&
                              nblk * (uint64_t)ES_SORT_BLOCK >= un && ntiles * (uint64_t)ES_SCAN_TILE >= nhist;
            std::printf("plan %d %lld %lld %d %d |\n", p.nblk, (long long)p.nhist, (long long)p.ntiles, p.passes, (int)(same && fits));
        } else if (tok[0] == "first") {
            const int H = (int)num(), W = (int)num();
            const double carried = num();
            const int64_t n = (int64_t)num();
            std::vector<int16_t> x((size_t)n), y((size_t)n);
            std::vector<double> t((size_t)n);
            for (auto& v : x) v = (int16_t)num();
            for (auto& v : y) v = (int16_t)num();
            for (auto& v : t) v = num();
            const EsRefusal r = es_first_offender(H, W, x.data(), y.data(), t.data(), n, carried);
            std::printf("first %lld %d |\n", (long long)r.index, r.fault);
        } else if (tok[0] == "window") {
            const int H = (int)num(), W = (int)num(), r = (int)num(), npts = (int)num();
            std::vector<int> x((size_t)npts), y((size_t)npts);
            for (auto& v : x) v = (int)num();
            for (auto& v : y) v = (int)num();
            std::printf("window |");
            for (int i = 0; i < npts; ++i) {
                const EsWindow w = es_window(H, W, x[(size_t)i], y[(size_t)i], r);
                std::printf(" %d %d %d %d %d", w.x0, w.x1, w.y0, w.y1, (w.x1 - w.x0 + 1) * (w.y1 - w.y0 + 1) - 1);
            }
            std::printf("\n");
        } else if (tok[0] == "filter") {
            const int H = (int)num(), W = (int)num();
            const double tau = num();
            const int r = (int)num(), fs = (int)num(), has_mask = (int)num(), nchunks = (int)num();
            std::vector<int64_t> len((size_t)nchunks);
            for (auto& v : len) v = (int64_t)num();
            const int64_t n = (int64_t)num();
            std::vector<int16_t> x((size_t)n), y((size_t)n);
            std::vector<double> t((size_t)n);
            for (auto& v : x) v = (int16_t)num();
            for (auto& v : y) v = (int16_t)num();
            for (auto& v : t) v = num();
            std::vector<uint8_t> mask;
            if (has_mask) { mask.resize((size_t)H * W); for (auto& v : mask) v = (uint8_t)num(); }
            std::vector<double> map((size_t)H * W, es_no_event());
            std::vector<int64_t> last((size_t)H * W);
            std::vector<int> sup((size_t)n);
            std::vector<float> wt((size_t)n);
            double carried = es_no_event();
            int64_t e0 = 0;
            for (int c = 0; c < nchunks; ++c) {
                const int64_t e1 = e0 + len[(size_t)c];
                if (e1 > n) return 5;
                if (es_first_offender(H, W, x.data() + e0, y.data() + e0, t.data() + e0, e1 - e0, carried)) return 6;
                std::fill(last.begin(), last.end(), (int64_t)-1);
                for (int64_t e = e0; e < e1; ++e) {
                    const int p = y[(size_t)e] * W + x[(size_t)e];
                    int cnt = 0;
                    if (!(has_mask && mask[(size_t)p])) {
                        const EsWindow w = es_window(H, W, x[(size_t)e], y[(size_t)e], r);
                        for (int qy = w.y0; qy <= w.y1; ++qy)
                            for (int qx = w.x0; qx <= w.x1; ++qx) {
                                const int q = qy * W + qx;
                                if (q == p || (has_mask && mask[(size_t)q])) continue;
                                const bool in_chunk = last[(size_t)q] >= 0;
                                const double tp = es_prev_time(in_chunk, in_chunk ? t[(size_t)last[(size_t)q]] : 0.0, map[(size_t)q]);
                                cnt += es_supported(t[(size_t)e], tp, tau) ? 1 : 0;
                            }
                    }
                    sup[(size_t)e] = cnt;
                    wt[(size_t)e] = es_weight(cnt, fs);
                    last[(size_t)p] = e;
                }
                for (size_t q = 0; q < map.size(); ++q) if (last[q] >= 0) map[q] = t[(size_t)last[q]];
                if (e1 > e0) carried = t[(size_t)e1 - 1];
                e0 = e1;
            }
            if (e0 != n) return 7;
            std::printf("filter |");
            for (int64_t e = 0; e < n; ++e) std::printf(" %d", sup[(size_t)e]);
            std::printf(" |");
            for (int64_t e = 0; e < n; ++e) { uint32_t u; std::memcpy(&u, &wt[(size_t)e], 4); std::printf(" %u", u); }
            std::printf(" |");
            for (size_t q = 0; q < map.size(); ++q) { uint64_t u; std::memcpy(&u, &map[q], 8); std::printf(" %llu", (unsigned long long)u); }
            std::printf("\n");
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
