// theta_advect_check.cpp — the HIP-free rules of the theta transport (csrc/eincm_theta_advect.h) as a program
// of its own: the argument check in its order, the value-range rule with the taps' gain, the quantisers, and the scales with the
// worst case of the overflow proof in 128-bit integers.  tests/test_theta_advect_interface.py builds it with the sanitizers and
// compares its lines with the witness.
//
// One case per input line:
//   check has_theta has_tau has_gain has_out n h w H W method fill min_coverage tau_all tau_at tau_val gain_all gain_at gain_val
//          (tau[b] = tau_all, but tau[tau_at] = tau_val where tau_at >= 0; likewise gain)      ->  check fault code |
//   range h w H W method count v[count]     ->  range ok tap_gain |
//   quant v                                 ->  quant Q dequantised |
//   landing x y vx vy tau H W               ->  landing ok x0 y0 ix iy | w00 w10 w01 w11
//   scales                                  ->  scales K S one full max_pixels theta_max | q_worst fits
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_theta_advect.h"

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
            TaArgs a{};
            a.has_theta = num() != 0; a.has_tau = num() != 0; a.has_gain = num() != 0; a.has_out = num() != 0;
            a.n = (int)num(); a.h = (int)num(); a.w = (int)num(); a.H = (int)num(); a.W = (int)num();
            a.method = (int)num(); a.fill = (int)num(); a.min_coverage = num();
            const size_t len = (size_t)(a.n >= 1 && a.n <= 65535 ? a.n : 1);         // (the arrays are read only for an n in range)
            std::vector<double> tau(len), gain(len);
            for (std::vector<double>* v : {&tau, &gain}) {
                const double all = num(); const int at = (int)num(); const double val = num();
                for (auto& e : *v) e = all;
                if (at >= 0) v->at((size_t)at) = val;
            }
            a.tau = a.has_tau ? tau.data() : nullptr;
            a.gain = a.has_gain ? gain.data() : nullptr;
            const TaFault f = ta_check(a);
            if ((f == TA_OK) != (ta_why(f)[0] == '\0')) return 5;                    // every refusal has its sentence
            std::printf("check %d %d |\n", (int)f, ta_code(f));
        } else if (tok[0] == "range") {
            const int h = (int)num(), w = (int)num(), H = (int)num(), W = (int)num(), method = (int)num();
            const size_t count = (size_t)num();
            std::vector<double> v(count);
            for (auto& e : v) e = num();
            double g = 1.0;
            if (h != H || w != W) { TapTables t; build_taps(h, w, H, W, method, t); g = ta_tap_gain(t, H, W); }
            std::printf("range %d %.17g |\n", ta_range_ok(v.data(), v.size(), g) ? 1 : 0, g);
        } else if (tok[0] == "quant") {
            const int64_t q = ta_quantise(num());
            std::printf("quant %lld %.17g |\n", (long long)q, ta_dequantise(q));
        } else if (tok[0] == "landing") {
            const int x = (int)num(), y = (int)num();
            const double vx = num(), vy = num(), tau = num();
            const int H = (int)num(), W = (int)num();
            TaLanding l{};
            const bool ok = ta_landing(x, y, vx, vy, tau, H, W, l);
            std::printf("landing %d %d %d %lld %lld |", ok ? 1 : 0, l.x0, l.y0, (long long)l.ix, (long long)l.iy);
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) std::printf(" %lld", ok ? (long long)ta_weight(l, dx, dy) : 0ll);
            std::printf("\n");
        } else if (tok[0] == "scales") {
            // the worst case of the proof: every source of the largest sensor on one pixel with the largest weight and value
            const int64_t q_worst = ta_quantise(TA_THETA_MAX + 0.5);
            const __int128 worst = (__int128)TA_MAX_PIXELS * TA_FULL * q_worst;
            std::printf("scales %d %d %lld %lld %lld %.17g | %lld %d\n", TA_K, TA_S, (long long)TA_ONE, (long long)TA_FULL,
                        (long long)TA_MAX_PIXELS, TA_THETA_MAX, (long long)q_worst, worst < ((__int128)1 << 63) ? 1 : 0);
        } else {
            return 3;
        }
        if (k != tok.size()) return 4;
    }
    return 0;
}
