// reweight.cpp — the HIP-free side of a keep-order staging (csrc/eincm_plan.h) as a program of its own: the
// plan's decision (EINCM_SW_KEEP_ORDER makes a weighted batch of any batch), bin_events carrying the index of every sorted slot back
// into the batch as it was handed over, and most_on_one_pixel, which a re-weighting of a host-binned batch counts with.
// tests/test_host_reweight.py builds it with the sanitizers, checks the counts below and compares the index with numpy.
//
// One case per input line:
//   order H W B  n_0 .. n_{B-1}  has_0 .. has_{B-1}  then per window: x[n] y[n] t[n] and, where has_b, w[n]
// ->  order plan_keep plan_weighted plan_weighted_without_the_flag
//       | not_a_permutation leaves_its_window xy_differs t_differs w_differs descends_inside_a_tile cntmax_differs    (counts: all 0)
//       | idx ..
//
//   payload B  n_0 .. n_{B-1}  has_0 .. has_{B-1}  keep
// ->  payload state weighted keep_order      (StagePlan.payload as a number: 0 none, 1 weights, 2 weights and order; the two flags set from it)
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
        if (tok.empty() || (tok[0] != "order" && tok[0] != "payload")) return 3;
        size_t k = 1;
        auto num = [&]() { return std::strtod(tok.at(k++).c_str(), nullptr); };
        if (tok[0] == "payload") {
            const int B = (int)num();
            std::vector<int64_t> n((size_t)B);
            std::vector<const float*> wp((size_t)B, nullptr);
            static const float some = 0.5f;               // the plan reads which windows have weights, never the values
            for (auto& v : n) v = (int64_t)num();
            bool any = false;
            for (auto& w : wp) if ((int)num()) { w = &some; any = true; }
            const uint32_t flags = (int)num() ? EINCM_SW_KEEP_ORDER : 0u;
            if (k != tok.size()) return 4;
            PlanCtx c;
            c.H = 70; c.W = 100;
            const StagePlan P = plan_staging(c, B, 2, n.data(), flags, StageKnobs{}, any ? wp.data() : nullptr);
            static_assert(PAYLOAD_NONE == 0 && PAYLOAD_WEIGHTS == 1 && PAYLOAD_WEIGHTS_ORDER == 2, "the payload state indexes the staging kernels");
            std::printf("payload %d %d %d\n", (int)P.payload, P.weighted ? 1 : 0, P.keep_order ? 1 : 0);
            continue;
        }
        const int H = (int)num(), W = (int)num(), B = (int)num();
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
        PlanCtx c;
        c.H = H; c.W = W;
        const int R = 2;
        const StagePlan P = plan_staging(c, B, R, n.data(), EINCM_SW_KEEP_ORDER, StageKnobs{}, nullptr);      // (handed no weights at all)
        const StagePlan P0 = plan_staging(c, B, R, n.data(), 0u, StageKnobs{}, nullptr);
        std::printf("order %d %d %d |", P.keep_order ? 1 : 0, P.weighted ? 1 : 0, P0.weighted || P0.keep_order ? 1 : 0);
        std::vector<int32_t> tilecount;
        std::vector<uint32_t> sxy, sidx;
        std::vector<double> st, dtmax((size_t)B, 0.0), edge_ts((size_t)B * R, 0.0);
        std::vector<unsigned> cntmax((size_t)B, 0u);
        std::vector<float> sw;
        if (bin_events(P.g, n.data(), xp.data(), yp.data(), tp.data(), edge_ts.data(), P.N, tilecount, sxy, st, cntmax, dtmax, wp.data(), &sw, &sidx))
            return 5;
        const int64_t N = P.N;
        // the batch as handed over, window after window: what the index points into
        std::vector<uint32_t> rxy; std::vector<double> rt; std::vector<float> rw; std::vector<int> rwin;
        for (int b = 0; b < B; ++b)
            for (int64_t i = 0; i < n[b]; ++i) {
                rxy.push_back((uint32_t)(uint16_t)xs[b][(size_t)i] | ((uint32_t)(uint16_t)ys[b][(size_t)i] << 16));
                rt.push_back(ts[b][(size_t)i]); rw.push_back(has[b] ? ws[b][(size_t)i] : 1.0f); rwin.push_back(b);
            }
        long long not_perm = 0, leaves = 0, dxy = 0, dt = 0, dw = 0, descends = 0, dcnt = 0;
        std::vector<int> seen((size_t)N, 0);
        int64_t slot = 0;
        for (int b = 0; b < B; ++b)
            for (int64_t i = 0; i < n[b]; ++i, ++slot) {
                const uint32_t e = sidx[(size_t)slot];
                if ((int64_t)e >= N) { ++not_perm; continue; }
                if (seen[e]++) ++not_perm;
                if (rwin[e] != b) ++leaves;
                if (rxy[e] != sxy[(size_t)slot]) ++dxy;
                if (std::memcmp(&rt[e], &st[(size_t)slot], 8) != 0) ++dt;
                if (std::memcmp(&rw[e], &sw[(size_t)slot], 4) != 0) ++dw;
            }
        slot = 0;
        for (int b = 0; b < B; ++b)
            for (int tile = 0; tile < P.g.ntiles; ++tile) {
                const int cnt = tilecount[(size_t)b * P.g.ntiles + tile];
                for (int i = 1; i < cnt; ++i)
                    if (sidx[(size_t)slot + i] <= sidx[(size_t)slot + i - 1]) ++descends;       // stable: a tile's events keep their order
                slot += cnt;
            }
        int64_t off = 0;
        for (int b = 0; b < B; ++b) {
            if (most_on_one_pixel(H, W, n[b], rxy.data() + off, has[b] ? rw.data() + off : nullptr) != cntmax[(size_t)b]) ++dcnt;
            off += n[b];
        }
        std::printf(" %lld %lld %lld %lld %lld %lld %lld |", not_perm, leaves, dxy, dt, dw, descends, dcnt);
        for (int64_t i = 0; i < N; ++i) std::printf(" %u", sidx[(size_t)i]);
        std::printf("\n");
    }
    return 0;
}
