// weights_check.cpp — the HIP-free rules of a weighted staging (csrc/eincm_plan.h) as a program of its own:
// batch_weighted and the plan's decision, check_weights' first refusal, and bin_events carrying the weights through the host
// counting sort.  tests/test_host_event_weights.py builds it with the sanitizers and compares its lines with numpy.
//
// One case per input line:
//   stage H W B null_array  n_0 .. n_{B-1}  has_0 .. has_{B-1}  then per window: x[n] y[n] t[n] and, where has_b, w[n]
// ->  stage batch_weighted plan_weighted refused_win refused_index | sxy .. | sw (as float bits) .. | cntmax ..      (the lists only where nothing is refused)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_plan.h"

using namespace eincm;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::vector<std::string> tok;
        for (std::string t; s >> t;) tok.push_back(t);
        if (tok.empty() || tok[0] != "stage") return 3;
        size_t k = 1;
        auto num = [&]() { return std::strtod(tok.at(k++).c_str(), nullptr); };      // (strtod reads nan and inf)
        const int H = (int)num(), W = (int)num(), B = (int)num(), null_array = (int)num();
        std::vector<int64_t> n((size_t)B);
        std::vector<int> has((size_t)B);
        for (auto& v : n) v = (int64_t)num();
        for (auto& v : has) v = (int)num();
        std::vector<std::vector<int16_t>> xs((size_t)B), ys((size_t)B);
        std::vector<std::vector<double>> ts((size_t)B);
        std::vector<std::vector<float>> ws((size_t)B);
        for (int b = 0; b < B; ++b) {
            for (int64_t i = 0; i < n[b]; ++i) xs[b].push_back((int16_t)num());
            for (int64_t i = 0; i < n[b]; ++i) ys[b].push_back((int16_t)num());
            for (int64_t i = 0; i < n[b]; ++i) ts[b].push_back(num());
            if (has[b]) for (int64_t i = 0; i < n[b]; ++i) ws[b].push_back((float)num());
        }
        if (k != tok.size()) return 4;
        std::vector<const int16_t*> xp, yp;
        std::vector<const double*> tp;
        std::vector<const float*> wp;
        static const float none = 0.0f;                   // a non-NULL address for the weights of a window without events
        for (int b = 0; b < B; ++b) {
            xp.push_back(xs[b].data()); yp.push_back(ys[b].data()); tp.push_back(ts[b].data());
            wp.push_back(has[b] ? (n[b] ? ws[b].data() : &none) : nullptr);
        }
        const float* const* weights = null_array ? nullptr : wp.data();
        PlanCtx c;
        c.H = H; c.W = W;
        const int R = 2;
        const StagePlan P = plan_staging(c, B, R, n.data(), 0u, StageKnobs{}, weights);
        const WeightRefusal r = check_weights(B, n.data(), weights);
        std::printf("stage %d %d %d %lld |", batch_weighted(B, n.data(), weights) ? 1 : 0, P.weighted ? 1 : 0, r.win, (long long)r.index);
        if (!r) {
            std::vector<int32_t> tilecount;
            std::vector<uint32_t> sxy;
            std::vector<double> st, dtmax((size_t)B, 0.0), edge_ts((size_t)B * R, 0.0);
            std::vector<unsigned> cntmax((size_t)B, 0u);
            std::vector<float> sw;
            const EventRefusal e = bin_events(P.g, n.data(), xp.data(), yp.data(), tp.data(), edge_ts.data(), P.N, tilecount, sxy, st, cntmax,
                                              dtmax, weights, P.weighted ? &sw : nullptr);
            if (e) return 5;
            for (int64_t i = 0; i < P.N; ++i) std::printf(" %u", sxy[(size_t)i]);
            std::printf(" |");
            if (P.weighted)
                for (int64_t i = 0; i < P.N; ++i) { uint32_t u; std::memcpy(&u, &sw[(size_t)i], 4); std::printf(" %u", u); }
            std::printf(" |");
            for (int b = 0; b < B; ++b) std::printf(" %u", cntmax[(size_t)b]);
        } else {
            std::printf(" | |");
        }
        std::printf("\n");
    }
    return 0;
}
