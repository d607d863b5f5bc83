// plan_check — runs the host's planning (csrc/eincm_plan.h) on the CPU: tests/test_host_plan.py builds it with the address and
// undefined-behaviour sanitizers, hands it a file of cases (one per line: a keyword, then numbers) and compares the line it prints
// for each.  Nothing of ROCm is included or linked.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_plan.h"

using namespace eincm;

namespace {

struct Args {                       // the numbers of one case, read in order
    std::vector<std::string> tok; size_t k = 1;
    bool more() const { return k < tok.size(); }
    double f() { if (!more()) { std::fprintf(stderr, "plan_check: '%s' case is short of arguments\n", tok[0].c_str()); std::exit(2); } return std::strtod(tok[k++].c_str(), nullptr); }
    int64_t i() { if (!more()) { std::fprintf(stderr, "plan_check: '%s' case is short of arguments\n", tok[0].c_str()); std::exit(2); } return std::strtoll(tok[k++].c_str(), nullptr, 10); }
};

void put(double v) { std::printf(" %.17g", v); }
void put_i(int64_t v) { std::printf(" %lld", (long long)v); }
template <typename T> void put_all(const std::vector<T>& v) { std::printf(" |"); for (const T& x : v) put_i((int64_t)x); }

// The context of a staged batch of these tile populations (counts: B * ntiles): plan_staging, and the four lists as stage_windows cuts them
void stage_counts(PlanCtx& c, int R, int B, const std::vector<int32_t>& counts, const StageKnobs& sk, const char* who) {
    const int ntiles = ((c.W + TS - 1) / TS) * ((c.H + TS - 1) / TS);
    if (counts.size() != (size_t)B * ntiles) { std::fprintf(stderr, "plan_check: %s wants %d x %d counts\n", who, B, ntiles); std::exit(2); }
    std::vector<int64_t> n_events((size_t)B, 0);
    for (int b = 0; b < B; ++b) for (int t = 0; t < ntiles; ++t) n_events[b] += counts[(size_t)b * ntiles + t];
    c.stage = plan_staging(c, B, R, n_events.data(), 0u, sk);
    c.g = c.stage.g;
    std::vector<int32_t> lens;
    const StagePlan& S = c.stage;
    cut_segments(counts.data(), counts.size(), ntiles, S.seg, S.N, false, c.gather, lens); c.gather.n = (int)lens.size();
    cut_segments(counts.data(), counts.size(), ntiles, S.seg_s, S.N, false, c.splat, lens); c.splat.n = (int)lens.size();
    cut_segments(counts.data(), counts.size(), ntiles, S.seg_2, S.N, true, c.gather_2, lens); c.gather_2.n = (int)lens.size();
    if (S.splat_short) { cut_segments(counts.data(), counts.size(), ntiles, SEG_SHORT, S.N, true, c.splat_sh, lens); c.splat_sh.n = (int)lens.size(); }
}

// a (B, h, w, 2) theta whose largest magnitude is vmax
std::vector<double> theta_of(int B, int h, int w, double vmax) {
    std::vector<double> theta((size_t)B * h * w * 2);
    for (size_t i = 0; i < theta.size(); ++i) theta[i] = (i % 3 == 0 ? -0.5 : 0.75) * vmax;
    theta[theta.size() / 2] = -vmax;
    return theta;
}

eincm_params level2_params() {
    eincm_params p{};
    p.alpha = 20.0; p.beta = 35.0; p.cur_pyr_lvl = 2; p.contrast_kind = EINCM_CONTRAST_GRAD_MAG;
    return p;
}

// policy H W R B rad pitch_env(-1: unset) vmax(< 0: staged only) h w counts[B * ntiles]: the thirteen fields of
// eincm_get_launch_policy for a context that staged these tile populations and evaluated a (h, w) theta of that maximum
void policy(Args& a) {
    PlanCtx c;
    c.H = (int)a.i(); c.W = (int)a.i();
    const int R = (int)a.i(), B = (int)a.i();
    c.splat_rad = (int)a.i();
    StageKnobs sk;
    const int pitch_env = (int)a.i();
    if (pitch_env >= 0) { sk.has_pitch = true; sk.pitch = pitch_env; }
    const double vmax = a.f();
    const int h = (int)a.i(), w = (int)a.i();
    std::vector<int32_t> counts;
    while (a.more()) counts.push_back((int32_t)a.i());
    stage_counts(c, R, B, counts, sk, "policy");
    EvalPlan P;
    if (vmax >= 0.0) {
        const std::vector<double> theta = theta_of(B, h, w, vmax);
        const eincm_params p = level2_params();
        P = plan_eval(c, DevIo{}, EvalKnobs{}, theta.data(), h, w, &p, true);
    }
    double out[EINCM_LP_SPLAT_SHORT + 1] = {};
    launch_policy(c, P, vmax >= 0.0, out);
    for (const double v : out) put(v);
}

// forms H W R B rad weighted wide(-1: as staged) proj_in_gather itembase_valid n_gather n_splat n_splat_sh n_gather_2 all_r(-1: unset)
// no_host_asm motion h w vmax want_grad [counts[B * ntiles]]: the launch forms of the event kernels (plan_forms) for a context in that
// state - the four lists hold that many segments, or, with counts, the staged batch of these tile populations (the four n_ are then
// not read) - that evaluates a (h, w) theta of that maximum, or (motion) a motion model whose field has that bound.
//   splat: mode rad threads weighted row lds list wincap winmaxw
// | gather: mode rad wide threads proj all_r weighted row lds list copy wg_per_seg wincap winmaxw pitch_aligned (row -1: none planned)
// | plan: wincap winmaxw wincap_a winmaxw_a pitch_aligned win_2.cap win_2.maxw win_2.pal splat_short proj all_r host_asm
void forms(Args& a) {
    PlanCtx c;
    c.H = (int)a.i(); c.W = (int)a.i();
    const int R = (int)a.i(), B = (int)a.i();
    c.splat_rad = (int)a.i();
    const bool weighted = a.i() != 0;
    const int wide = (int)a.i();
    c.proj_in_gather = a.i() != 0; c.itembase_valid = a.i() != 0;
    const int n_list[4] = {(int)a.i(), (int)a.i(), (int)a.i(), (int)a.i()};
    EvalKnobs knobs;
    knobs.all_r = (int)a.i(); knobs.no_host_asm = a.i() != 0;
    const bool motion = a.i() != 0;
    const int h = (int)a.i(), w = (int)a.i();
    const double vmax = a.f();
    const bool want_grad = a.i() != 0;
    std::vector<int32_t> counts;
    while (a.more()) counts.push_back((int32_t)a.i());
    if (!counts.empty()) {
        stage_counts(c, R, B, counts, StageKnobs{}, "forms");
    } else {
        const std::vector<int64_t> n_events((size_t)B, 100000);
        c.stage = plan_staging(c, B, R, n_events.data(), 0u, StageKnobs{});
        c.g = c.stage.g;
        c.gather.n = n_list[0]; c.splat.n = n_list[1]; c.splat_sh.n = n_list[2]; c.gather_2.n = n_list[3];
    }
    c.stage.weighted = weighted;
    if (wide >= 0) c.stage.wide = wide != 0;
    const eincm_params p = level2_params();
    EvalPlan P;
    if (motion) {
        P = plan_motion(c, knobs, vmax, &p, want_grad);
    } else {
        const std::vector<double> theta = theta_of(B, h, w, vmax);
        P = plan_eval(c, DevIo{}, knobs, theta.data(), h, w, &p, want_grad);
    }
    const SplatForm& s = P.splat;
    for (const int64_t v : {(int64_t)s.key.mode, (int64_t)s.key.rad, (int64_t)s.key.threads, (int64_t)s.key.weighted, (int64_t)s.row, (int64_t)s.lds,
                            (int64_t)s.list, (int64_t)s.wincap, (int64_t)s.winmaxw}) put_i(v);
    std::printf(" |");
    const GatherForm& g = P.gather;
    for (const int64_t v : {(int64_t)g.key.mode, (int64_t)g.key.rad, (int64_t)g.key.wide, (int64_t)g.key.threads, (int64_t)g.key.proj,
                            (int64_t)g.key.all_r, (int64_t)g.key.weighted, (int64_t)g.row, (int64_t)g.lds, (int64_t)g.list, (int64_t)g.copy,
                            (int64_t)g.wg_per_seg, (int64_t)g.wincap, (int64_t)g.winmaxw, (int64_t)g.pitch_aligned}) put_i(v);
    std::printf(" |");
    for (const int64_t v : {(int64_t)P.wincap, (int64_t)P.winmaxw, (int64_t)P.wincap_a, (int64_t)P.winmaxw_a, (int64_t)P.pitch_aligned,
                            (int64_t)P.win_2.cap, (int64_t)P.win_2.maxw, (int64_t)P.win_2.pal, (int64_t)P.splat_short, (int64_t)P.proj,
                            (int64_t)P.all_r, (int64_t)P.host_asm}) put_i(v);
}

// formrows: the rows of the four form lists, k_splat's (mode rad threads weighted) | k_splat_r's | k_gather's (mode rad wide threads
// proj all_r weighted) | k_gather_r's
void formrows() {
    for (const SplatKey& k : SPLAT_FORMS) { put_i(k.mode); put_i(k.rad); put_i(k.threads); put_i(k.weighted); }
    std::printf(" |");
    for (const SplatKey& k : SPLAT_R_FORMS) { put_i(k.mode); put_i(k.rad); put_i(k.threads); put_i(k.weighted); }
    std::printf(" |");
    for (const GatherKey& k : GATHER_FORMS) { put_i(k.mode); put_i(k.rad); put_i(k.wide); put_i(k.threads); put_i(k.proj); put_i(k.all_r); put_i(k.weighted); }
    std::printf(" |");
    for (const GatherKey& k : GATHER_R_FORMS) { put_i(k.mode); put_i(k.rad); put_i(k.wide); put_i(k.threads); put_i(k.proj); put_i(k.all_r); put_i(k.weighted); }
}

// cut seg ntiles N want_items counts[]: n, tspan | lens | order | win_item0 | items (win, tile, begin, count)
void cut(Args& a) {
    const int seg = (int)a.i(), ntiles = (int)a.i();
    const int64_t N = a.i();
    const bool want_items = a.i() != 0;
    std::vector<int32_t> counts, lens;
    while (a.more()) counts.push_back((int32_t)a.i());
    SegList L;
    cut_segments(counts.data(), counts.size(), ntiles, seg, N, want_items, L, lens);
    put_i((int64_t)lens.size()); put(L.tspan);
    put_all(lens); put_all(L.h_order); put_all(L.h_win_item0);
    std::printf(" |");
    for (const Item& it : L.h_items) { put_i(it.win); put_i(it.tile); put_i(it.begin); put_i(it.count); }
}

// resample method h w H W: AH | AW | row taps | column taps | tile ranges | fits
void resample(Args& a) {
    const int method = (int)a.i(), h = (int)a.i(), w = (int)a.i(), H = (int)a.i(), W = (int)a.i();
    ResampleTables t;
    build_resample(h, w, H, W, method, t);
    for (const double v : t.AH) put(v);
    std::printf(" |"); for (const double v : t.AW) put(v);
    std::printf(" |"); for (const Int2& q : t.rowtap) { put_i(q.x); put_i(q.y); }
    std::printf(" |"); for (const Int2& q : t.coltap) { put_i(q.x); put_i(q.y); }
    std::printf(" |"); for (const TileRange& q : t.tilerng) { put_i(q.ilo); put_i(q.ni); put_i(q.jlo); put_i(q.nj); }
    std::printf(" | %d", t.fits ? 1 : 0);
}

// taps method h w H W: rstride cstride | rlo | rcnt | clo | ccnt | row weights | column weights, read back out of the packed block
void taps(Args& a) {
    const int method = (int)a.i(), h = (int)a.i(), w = (int)a.i(), H = (int)a.i(), W = (int)a.i();
    TapTables t;
    build_taps(h, w, H, W, method, t);
    const char* base = t.tab.buf.data();
    put_i(t.rstride); put_i(t.cstride);
    const size_t off[4] = {t.o_rlo, t.o_rcnt, t.o_clo, t.o_ccnt};
    for (int k = 0; k < 4; ++k) { std::printf(" |"); for (int i = 0; i < (k < 2 ? H : W); ++i) put_i(Packer::i32(base, off[k])[i]); }
    std::printf(" |"); for (int i = 0; i < H * t.rstride; ++i) put(Packer::f64(base, 0)[i]);
    std::printf(" |"); for (int i = 0; i < W * t.cstride; ++i) put(Packer::f64(base, t.o_cw)[i]);
    put_i((int64_t)t.tab.buf.size());
}

// bin H W R B n_events[B] edge_ts[B * R] then x y t per event: "refused win index bad_xy", or
// ok | tile counts | sorted xy words | sorted t | cntmax | dtmax
void bin(Args& a) {
    Geom g{};
    g.H = (int)a.i(); g.W = (int)a.i(); g.R = (int)a.i(); g.B = (int)a.i();
    g.tilesX = (g.W + TS - 1) / TS; g.tilesY = (g.H + TS - 1) / TS; g.ntiles = g.tilesX * g.tilesY;
    std::vector<int64_t> n((size_t)g.B);
    int64_t N = 0;
    for (int64_t& v : n) { v = a.i(); N += v; }
    std::vector<double> edge_ts((size_t)g.B * g.R);
    for (double& v : edge_ts) v = a.f();
    std::vector<std::vector<int16_t>> xs((size_t)g.B), ys((size_t)g.B);
    std::vector<std::vector<double>> ts((size_t)g.B);
    std::vector<const int16_t*> xp, yp; std::vector<const double*> tp;
    for (int b = 0; b < g.B; ++b) {
        for (int64_t i = 0; i < n[b]; ++i) { xs[b].push_back((int16_t)a.i()); ys[b].push_back((int16_t)a.i()); ts[b].push_back(a.f()); }
        xp.push_back(xs[b].data()); yp.push_back(ys[b].data()); tp.push_back(ts[b].data());
    }
    std::vector<int32_t> tilecount; std::vector<uint32_t> sxy; std::vector<double> st;
    std::vector<unsigned> cntmax((size_t)g.B, 0u); std::vector<double> dtmax((size_t)g.B, 0.0);
    const EventRefusal r = bin_events(g, n.data(), xp.data(), yp.data(), tp.data(), edge_ts.data(), N, tilecount, sxy, st, cntmax, dtmax);
    if (r) { std::printf(" refused %d %lld %d", r.win, (long long)r.index, r.bad_xy ? 1 : 0); return; }
    sxy.resize((size_t)N); st.resize((size_t)N);                       // (both hold one slot for an empty batch)
    std::printf(" ok");
    put_all(tilecount); put_all(sxy);
    std::printf(" |"); for (const double v : st) put(v);
    put_all(cntmax);
    std::printf(" |"); for (const double v : dtmax) put(v);
}

// edges v[]: sum, sum of squares and largest magnitude of the fp32 values | the fp32 values
void edges(Args& a) {
    std::vector<double> e;
    while (a.more()) e.push_back(a.f());
    std::vector<float> o(e.size());
    double s, ss, mx;
    edge_moments(e.data(), e.size(), o.data(), s, ss, mx);
    put(s); put(ss); put(mx);
    std::printf(" |"); for (const float v : o) put((double)v);
}

// packer (bytes align)[]: every piece's offset | the block in hex.  Piece k holds the bytes k + 1.
void packer(Args& a) {
    Packer p;
    for (int k = 1; a.more(); ++k) {
        const size_t bytes = (size_t)a.i(), align = (size_t)a.i();
        const std::vector<char> piece(bytes, (char)k);
        put_i((int64_t)p.add(piece.data(), bytes, align));
    }
    std::printf(" | ");
    for (const char ch : p.buf) std::printf("%02x", (unsigned)(unsigned char)ch);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: plan_check <cases file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "plan_check: cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        Args a;
        std::istringstream ss(line);
        for (std::string t; ss >> t;) a.tok.push_back(t);
        if (a.tok.empty()) continue;
        const std::string& what = a.tok[0];
        std::printf("%s", what.c_str());
        if (what == "policy") policy(a);
        else if (what == "forms") forms(a);
        else if (what == "formrows") formrows();
        else if (what == "cut") cut(a);
        else if (what == "resample") resample(a);
        else if (what == "taps") taps(a);
        else if (what == "bin") bin(a);
        else if (what == "edges") edges(a);
        else if (what == "packer") packer(a);
        else if (what == "mrw") { const int R = (int)a.i(); std::vector<double> w((size_t)R); multi_ref_weights(R, w.data()); for (const double v : w) put(v); }
        else if (what == "ishift") put_i(f64_ishift(a.i()));
        else if (what == "nlm") put_i(nlm_shift((int)a.i()));
        else { std::fprintf(stderr, "plan_check: unknown case '%s'\n", what.c_str()); return 2; }
        std::printf("\n");
    }
    return 0;
}
