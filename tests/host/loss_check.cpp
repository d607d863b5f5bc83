// loss_check — runs csrc/eincm_loss.h (the loss's scalar assembly) on the cases of tests/test_host_loss.py.  A stand-alone program:
// built with -fsanitize=address,undefined -ffp-contract=off and run as a child process; one input line per case, one output line per
// case: the case's first word, then numbers printed with 17 significant digits (they read back to the same doubles), groups split by '|'.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "eincm_loss.h"

using namespace eincm;

namespace {

struct In {
    std::istringstream s;
    explicit In(const std::string& line) : s(line) {}
    double d() { std::string t; s >> t; return strtod(t.c_str(), nullptr); }      // (strtod reads nan, inf and -0.0)
    int i() { long long v = 0; s >> v; return (int)v; }
    std::vector<double> ds(size_t n) { std::vector<double> v(n); for (double& x : v) x = d(); return v; }
};
void put(double v) { printf(" %.17g", v); }
void put(const double* v, size_t n) { for (size_t k = 0; k < n; ++k) put(v[k]); }
void bar() { printf(" |"); }

EvalParams params(In& in) {
    EvalParams ep{};
    ep.alpha = in.d(); ep.beta = in.d(); ep.gamma = in.d(); ep.delta = in.d();
    ep.cur_pyr_lvl = in.i(); ep.contrast_kind = in.i(); ep.want_div = in.i(); ep.want_tv = in.i();
    return ep;
}
WinConst constants(In& in, int R) {
    WinConst wc{};
    wc.c0_gradmag = in.d(); wc.c0_var = in.d(); wc.d0 = in.d();
    for (int r = 0; r < R; ++r) wc.zc[r] = in.d();
    for (int r = 0; r < R; ++r) wc.sE[r] = in.d();
    for (int r = 0; r < R; ++r) wc.sEE[r] = in.d();
    for (int r = 0; r < R; ++r) wc.mrw[r] = in.d();
    return wc;
}
void put_out(const OutScal& o, int R) {
    put(o.value); put(o.mean_rel_corr); put(o.mean_rel_contrast); put(o.mean_rel_div); put(o.tv); put(o.nonfinite);
    put(o.corr, R); put(o.contrast_gm, R); put(o.var, R); put(o.div, R);
}

// window: ep R tv theta_bad tv_direct | constants | per image (contrast, correlation, divergence) through the F64Scal front end
void window(In& in) {
    const EvalParams ep = params(in);
    const int R = in.i();
    const double tv = in.d();
    const bool bad = in.i() != 0, direct = in.i() != 0;
    const WinConst wc = constants(in, R);
    OutScal o{};
    double sc = 0.0, sr = 0.0, sd = 0.0;
    for (int r = 0; r < R; ++r) {
        F64Scal s{};
        s.g2 = s.var = in.d(); s.mse = -in.d(); s.div = in.d();
        const ImageTerms t = image_terms(ep, wc, r, s);
        store_terms(o, r, t);
        sc += t.rel_con; sr += t.rel_corr; sd += t.rel_div;
    }
    assemble_window(ep, R, sc, sr, ep.want_div ? sd / (double)R : NAN, tv_reported(ep, tv), bad, direct, o);
    put_out(o, R);
}

// the fp32 front end (through pack / unpack), the objective kinds' front end, mse_from_moments
void image(In& in) {
    const EvalParams ep = params(in);
    const WinConst wc = constants(in, 1);
    const std::vector<double> q = in.ds(IMGSCAL_N);
    ImgScal s{};
    s.m = q[0]; s.M = q[1]; s.D = q[2]; s.cm = q[3]; s.cM = q[4]; s.sI = q[5]; s.sII = q[6]; s.sEI = q[7]; s.sG2 = q[8];
    double packed[IMGSCAL_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -7.0};
    pack(s, packed);
    const double g2 = in.d(), dsum = in.d(), HW = in.d();
    const ImageTerms t = image_terms(ep, wc, 0, unpack(packed), g2, dsum, HW);
    put(t.corr); put(t.contrast_gm); put(t.var); put(t.div); put(t.rel_con); put(t.rel_corr); put(t.rel_div);
    bar(); put(packed, IMGSCAL_N); put(unpack(packed).sG2);
    bar(); put(mse_from_moments(s, wc.sE[0], wc.sEE[0], HW));
    const ImageTerms k = image_terms(wc.mrw[0], g2, dsum, wc.c0_var, wc.zc[0]);
    bar(); put(k.rel_con); put(k.rel_corr); put(rel_term(wc.mrw[0], g2, dsum));
}

void weights(In& in) {
    const EvalParams ep = params(in);
    const double mrw = in.d(), R = in.d(), c0 = in.d(), zc = in.d(), d0 = in.d(), hw = in.d();
    const LossWeights w = loss_weights(ep, mrw, R, c0, zc, d0, hw);
    put(w.a); put(w.b); put(w.e);
}

void tv(In& in) {
    const EvalParams ep = params(in);
    const double a = in.d(), nz = in.d();
    put(tv_value(a, nz)); put(tv_reported(ep, tv_value(a, nz))); put(tv_grad_scale(ep.gamma, nz));
}

void sum4(In& in) {
    const size_t n = (size_t)in.i();
    const std::vector<double> p = in.ds(2 * n);           // exactly 2 n doubles on the heap: ASan sees a read past them
    double out[2];
    sum_partials_4(p.data(), n, out);
    put(out, 2);
}

void scan(In& in) {
    const size_t n = (size_t)in.i();
    const bool with_dst = in.i() != 0;
    const std::vector<double> src = in.ds(n);
    std::vector<double> dst(n, -1.0);
    put(copy_scan_finite(with_dst ? dst.data() : nullptr, src.data(), n) ? 1.0 : 0.0);
    bar(); put(dst.data(), n);
}

void handover(In& in) {
    const size_t B = (size_t)in.i(), nth = (size_t)in.i();
    const std::vector<double> a = in.ds(B), prev = in.ds(B * nth), theta = in.ds(B * nth), grad = in.ds(B * nth);
    std::vector<double> tho(B * nth), dv(B);
    handover_blend(a.data(), prev.data(), theta.data(), B, nth, tho.data());
    handover_chain(grad.data(), prev.data(), theta.data(), B, nth, dv.data());
    put(tho.data(), tho.size()); bar(); put(dv.data(), B);
}

// A whole evaluation's way through host_assemble (mode 0), f64_assemble (1), each followed by obj_assemble (+2), then hand_over
void assemble(In& in) {
    const int mode = in.i();
    EvalParams ep = params(in);
    Geom g{};
    g.R = in.i(); g.B = in.i(); g.wmask = (unsigned long long)in.i(); g.H = in.i(); g.W = in.i(); g.nig = in.i(); g.ntiles = in.i();
    const bool two_dof = in.i() != 0;
    const size_t nth = (size_t)in.i();
    const int nwg = (g.nig + IG_NT / 64 - 1) / (IG_NT / 64), ck = in.i(), rk = in.i();
    const size_t B = (size_t)g.B, BR = B * g.R;
    std::vector<WinConst> wc;
    std::vector<ObjConst> oc(B);
    std::vector<int64_t> nev;
    std::vector<int32_t> item0(1, 0);
    std::vector<double> theta, tvparts, img, g2, g11, ovals, grad(B * nth, 5.0);
    std::vector<F64Scal> scal(BR);
    for (size_t b = 0; b < B; ++b) {
        nev.push_back(in.i());
        item0.push_back(item0.back() + in.i());
        for (double x : in.ds(nth)) theta.push_back(x);
        wc.push_back(constants(in, g.R));
        for (int k = 0; k < 4; ++k) oc[b].c0[k] = in.d();
        for (int k = 0; k < 4; ++k) for (int r = 0; r < g.R; ++r) oc[b].zc[k][r] = in.d();
        for (double x : in.ds((size_t)g.ntiles * 3)) tvparts.push_back(x);
        for (int r = 0; r < g.R; ++r) {
            for (double x : in.ds(IMGSCAL_N)) img.push_back(x);
            for (double x : in.ds(nwg)) g2.push_back(x);
            F64Scal& s = scal[b * g.R + r];
            s.var = in.d(); s.g2 = in.d(); s.mse = in.d(); s.div = in.d();
            for (double x : in.ds(2)) ovals.push_back(x);
        }
    }
    for (double x : in.ds((size_t)item0.back() * g.R * 2)) g11.push_back(x);
    std::vector<uint8_t> theta_nan(B, 0);
    scan_theta(theta.data(), g.B, nth, theta_nan.data());
    std::vector<OutScal> outs(B);
    const LossView v{&g, &ep, two_dof, nth, wc.data(), outs.data(), grad.data(), theta_nan.data(), tvparts.data(), img.data(), g2.data(),
                     g11.data(), item0.data(), nev.data(), scal.data(), oc.data(), ovals.data(), ck, rk, (mode & 1) == 0};
    if (mode & 1) f64_assemble(v); else host_assemble(v);
    if (mode & 2) obj_assemble(v);
    std::vector<double> value(B);
    std::vector<eincm_aux> aux(B);
    const bool nonfinite = hand_over(v, true, value.data(), aux.data());
    put(nonfinite ? 1.0 : 0.0);
    for (size_t b = 0; b < B; ++b) {
        bar(); put(value[b]); put(aux[b].final_loss); put(aux[b].mean_rel_corr); put(aux[b].mean_rel_contrast);
        put(aux[b].mean_rel_iwe_divergence); put(aux[b].theta_total_variation);
        bar(); put_out(outs[b], g.R);
        bar(); put(grad.data() + b * nth, nth);
    }
}

// the window constants from a zero pass, and objectives()' block
void constants_case(In& in) {
    Geom g{};
    g.R = in.i(); g.H = in.i(); g.W = in.i(); g.ntiles = in.i();
    OutScal o{};
    o.tv = in.d();
    for (int r = 0; r < g.R; ++r) { o.corr[r] = in.d(); o.contrast_gm[r] = in.d(); o.var[r] = in.d(); o.div[r] = in.d(); }
    const std::vector<double> tvp = in.ds((size_t)g.ntiles * 3);
    WinConst wc{};
    for (int r = 0; r < g.R; ++r) wc.mrw[r] = in.d();
    constants_from_zero_pass(o, g.R, wc);
    put(wc.c0_gradmag); put(wc.c0_var); put(wc.d0); put(wc.inv_c0_gradmag); put(wc.inv_c0_var); put(wc.zc, g.R); put(wc.inv_zc, g.R);
    eincm_objectives_out q;
    fill_objectives(g, o, wc, tvp.data(), q);
    bar(); put((double)q.n_refs); put(q.zero_contrast); put(q.zero_variance); put(q.zero_iwe_divergence); put(q.theta_total_variation);
    put(q.theta_divergence);
    bar(); put(q.correlations, g.R); put(q.zero_correlations, g.R); put(q.rel_correlations, g.R); put(q.contrasts, g.R);
    put(q.rel_contrasts, g.R); put(q.iwe_divergences, g.R); put(q.rel_iwe_divergences, g.R); put(q.variances, g.R);
    put(q.flow_warp_losses, g.R); put(q.multi_ref_weights, g.R);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: loss_check CASES.txt\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        In in(line);
        std::string word;
        in.s >> word;
        printf("%s", word.c_str());
        if (word == "window") window(in);
        else if (word == "image") image(in);
        else if (word == "weights") weights(in);
        else if (word == "tv") tv(in);
        else if (word == "sum4") sum4(in);
        else if (word == "scan") scan(in);
        else if (word == "handover") handover(in);
        else if (word == "assemble") assemble(in);
        else if (word == "constants") constants_case(in);
        else { fprintf(stderr, "unknown case %s\n", word.c_str()); return 2; }
        if (in.s.fail()) { fprintf(stderr, "%s: the line ran out\n", word.c_str()); return 2; }
        printf("\n");
    }
    return 0;
}
