// motion_fused_check — runs the HIP-free rules of the fused motion-model evaluation on the CPU: the support
// predicate and the slot order of the moment partials (csrc/eincm_motion.h) and the MOTION plan (csrc/eincm_plan.h).
// tests/test_host_motion_fused.py builds it with the address and undefined-behaviour sanitizers, hands it a file of cases (one per
// line: a keyword, then numbers) and compares the line it prints for each with numpy, bit for bit.  Nothing of ROCm is included or linked.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_motion.h"
#include "eincm_plan.h"

using namespace eincm;

namespace {

struct Args {                       // the numbers of one case, read in order
    std::vector<std::string> tok; size_t k = 1;
    bool more() const { return k < tok.size(); }
    void need() const { if (!more()) { std::fprintf(stderr, "motion_fused_check: '%s' case is short of arguments\n", tok[0].c_str()); std::exit(2); } }
    double f() { need(); return std::strtod(tok[k++].c_str(), nullptr); }
    int64_t i() { need(); return std::strtoll(tok[k++].c_str(), nullptr, 10); }
};

void put(double v) { std::printf(" %.17g", v); }
void put_i(int64_t v) { std::printf(" %lld", (long long)v); }

// supported fp64 model_set staged constants_pending device_results in_flight splat_size flags cur_pyr_lvl gamma: code | the reason's words
void supported(Args& a) {
    MotionCtxState s{};
    s.fp64 = a.i() != 0; s.model_set = a.i() != 0; s.staged = a.i() != 0; s.constants_pending = a.i() != 0;
    s.device_results = a.i() != 0; s.in_flight = a.i() != 0; s.splat_size = (int)a.i();
    eincm_params p{};
    p.alpha = 20.0; p.beta = 35.0;
    p.flags = (uint32_t)a.i(); p.cur_pyr_lvl = (int)a.i(); p.gamma = a.f();
    const MotionRefusal r = motion_fused_supported(s, &p);
    put_i(r.code);
    std::printf(" | %s", r ? r.why : "ok");
}

// usable bound q[12]: 1 if the window takes part in the kernels
void usable(Args& a) {
    const double bound = a.f();
    double q[MOTION_NQ];
    for (double& v : q) v = a.f();
    put_i(motion_q_usable(q, bound) ? 1 : 0);
}

// plan H W R B vmax want_grad cur_pyr_lvl delta all_r_knob counts[B * ntiles]: the MOTION plan of a context that staged these tile
// populations | the thirteen fields of eincm_get_launch_policy after it
void plan(Args& a) {
    PlanCtx c;
    c.H = (int)a.i(); c.W = (int)a.i();
    const int R = (int)a.i(), B = (int)a.i();
    const double vmax = a.f();
    const bool want_grad = a.i() != 0;
    eincm_params p{};
    p.alpha = 20.0; p.beta = 35.0; p.contrast_kind = EINCM_CONTRAST_GRAD_MAG;
    p.cur_pyr_lvl = (int)a.i(); p.delta = a.f();
    EvalKnobs knobs;
    knobs.all_r = (int)a.i();
    std::vector<int32_t> counts;
    while (a.more()) counts.push_back((int32_t)a.i());
    const int ntiles = ((c.W + TS - 1) / TS) * ((c.H + TS - 1) / TS);
    if (counts.size() != (size_t)B * ntiles) { std::fprintf(stderr, "motion_fused_check: plan wants %d x %d counts\n", B, ntiles); std::exit(2); }
    std::vector<int64_t> n_events((size_t)B, 0);
    for (int b = 0; b < B; ++b) for (int t = 0; t < ntiles; ++t) n_events[b] += counts[(size_t)b * ntiles + t];
    c.stage = plan_staging(c, B, R, n_events.data(), 0u, StageKnobs{});
    c.g = c.stage.g;
    std::vector<int32_t> lens;
    const StagePlan& S = c.stage;                                      // the four lists, as stage_windows cuts them
    cut_segments(counts.data(), counts.size(), ntiles, S.seg, S.N, false, c.gather, lens); c.gather.n = (int)lens.size();
    cut_segments(counts.data(), counts.size(), ntiles, S.seg_s, S.N, false, c.splat, lens); c.splat.n = (int)lens.size();
    cut_segments(counts.data(), counts.size(), ntiles, S.seg_2, S.N, true, c.gather_2, lens); c.gather_2.n = (int)lens.size();
    if (S.splat_short) { cut_segments(counts.data(), counts.size(), ntiles, SEG_SHORT, S.N, true, c.splat_sh, lens); c.splat_sh.n = (int)lens.size(); }
    const EvalPlan P = plan_motion(c, knobs, vmax, &p, want_grad);
    for (const int64_t v : {(int64_t)P.shape, (int64_t)P.theta_src, (int64_t)P.use_arg, (int64_t)P.need_theta_image, (int64_t)P.host_asm,
                            (int64_t)P.zero_copy_out, (int64_t)P.all_r, (int64_t)P.ep.identity, (int64_t)P.nsrc, (int64_t)P.events_projected,
                            (int64_t)P.proj, (int64_t)P.grid_tail, (int64_t)P.ep.want_tv, (int64_t)P.ep.want_div, (int64_t)P.div_grad,
                            (int64_t)S.wide, (int64_t)c.gather.n, (int64_t)P.nth})
        put_i(v);
    std::printf(" |");
    double out[EINCM_LP_SPLAT_SHORT + 1] = {};
    launch_policy(c, P, true, out);
    for (const double v : out) put(v);
}

// slots B ntiles seg slots_per_segment counts[B * ntiles]: segments in all | first slot of every window (B + 1)
void slots(Args& a) {
    const int B = (int)a.i(), ntiles = (int)a.i(), seg = (int)a.i(), sps = (int)a.i();
    std::vector<int32_t> counts((size_t)B * ntiles);
    for (int32_t& v : counts) v = (int32_t)a.i();
    std::vector<int64_t> s0((size_t)B + 1);
    put_i(motion_slot_offsets(counts.data(), B, ntiles, seg, sps, s0.data()));
    std::printf(" |");
    for (const int64_t v : s0) put_i(v);
}

// sum n parts[n * 12]: mu (12), the n partials of one window added in index order
void sum(Args& a) {
    const int64_t n = a.i();
    std::vector<double> parts((size_t)n * MOTION_NQ);
    for (double& v : parts) v = a.f();
    double mu[MOTION_NQ];
    motion_sum_slots(parts.data(), n, mu);
    for (const double v : mu) put(v);
}

// consts: the sizes the plan and the kernels share
void consts(Args&) { put_i(MOTION_PLAN_ARG_WINDOWS); put_i(THETA_ARG_MAX); put_i((int64_t)EvalPlan::MOTION); put_i((int64_t)EvalPlan::THETA_ARGS); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: motion_fused_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "motion_fused_check: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        Args a;
        std::istringstream ss(line);
        for (std::string t; ss >> t; ) a.tok.push_back(t);
        if (a.tok.empty()) continue;
        const std::string& w = a.tok[0];
        std::printf("%s", w.c_str());
        if (w == "supported") supported(a);
        else if (w == "usable") usable(a);
        else if (w == "plan") plan(a);
        else if (w == "slots") slots(a);
        else if (w == "sum") sum(a);
        else if (w == "consts") consts(a);
        else { std::fprintf(stderr, "motion_fused_check: unknown case '%s'\n", w.c_str()); return 2; }
        if (a.more()) { std::fprintf(stderr, "motion_fused_check: '%s' case has arguments left over\n", w.c_str()); return 2; }
        std::printf("\n");
    }
    return 0;
}
