// eincm_loss.h — the one statement of the loss's scalar assembly (losses.py:176-203):
//     L = alpha * (-mean_r rel_con_r) + beta * (-mean_r rel_corr_r) + gamma * TV + delta * mean_r rel_div_r,   rel_x_r = mrw_r * x_r / (x0 + eps)
// and of its derivative, the weights a_r, b_r, e_r on dcon_r, dcorr_r, ddiv_r.  The EINCM_HD functions run on both sides: k_final,
// k_imgrad, k64_grad1, k_obj_grad, the gather's tail and k64_gfin call them, and so do the host's assemblies below.  Plain C++17: no
// HIP header and no getenv, so tests/host/loss_check.cpp builds it with any compiler, under the sanitizers.  Every expression keeps
// its operation order: the bit-reproducibility of DESIGN.md 4.1 rests on it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "eincm.h"
#include "eincm_types.h"

namespace eincm {

EINCM_HD double rel_term(double mrw, double term, double zero) { return mrw * term / (zero + EPSN); }

// dL/dcon_r, dL/dcorr_r, dL/ddiv_r (the last over `hw`: k_imgrad and k_obj_grad fold the pixel count in; the fp64 kernel passes 1.0)
struct LossWeights { double a, b, e; };
EINCM_HD LossWeights loss_weights(const EvalParams& ep, double mrw, double R, double c0, double zc, double d0, double hw) {
    LossWeights w;
    w.a = -ep.alpha * mrw / (R * (c0 + EPSN));
    w.b = -ep.beta * mrw / (R * (zc + EPSN));
    w.e = ep.delta * mrw / (R * (d0 + EPSN) * hw);
    return w;
}

// mean((E - n)^2) with n = (I - m)/D from the moments (correlation_objectives.py:25-26 on img_utils.py:24-25)
EINCM_HD double mse_from_moments(const ImgScal& s, double sE, double sEE, double HW) {
    const double a = s.m / s.D;
    return (sEE + HW * a * a + s.sII / (s.D * s.D) + 2.0 * a * sE - 2.0 * s.sEI / s.D - 2.0 * a * s.sI / s.D) / HW;
}

// The TV term (regularizers.py:14-38) from the sums of k_tv's partials: a = sum |grad theta|, nz = the non-zero pixels
EINCM_HD double tv_value(double a, double nz) { return a / (nz + EPSN); }
EINCM_HD double tv_grad_scale(double gamma, double nz) { return gamma * 0.25 / (nz + EPSN); }
// ... as the aux reports it (losses.py:171): 0 above level 0, NAN where it was not computed
EINCM_HD double tv_reported(const EvalParams& ep, double tv) { return (ep.cur_pyr_lvl <= 0) ? (ep.want_tv ? tv : NAN) : 0.0; }

// The image scalars k_imgrad hands to the host: IMGSCAL_N slots, the last (sG2) left to the per-strip contrast energies
EINCM_HD void pack(const ImgScal& s, double* o) {
    o[0] = s.m; o[1] = s.M; o[2] = s.D; o[3] = s.cm; o[4] = s.cM; o[5] = s.sI; o[6] = s.sII; o[7] = s.sEI;
}
EINCM_HD ImgScal unpack(const double* q) {
    ImgScal s{};
    s.m = q[0]; s.M = q[1]; s.D = q[2]; s.cm = q[3]; s.cM = q[4]; s.sI = q[5]; s.sII = q[6]; s.sEI = q[7];
    return s;
}

// One image's entries of OutScal and its three terms of the sums over reference times (rel_div: 0 where the divergence is not wanted)
struct ImageTerms { double corr, contrast_gm, var, div, rel_con, rel_corr, rel_div; };
EINCM_HD ImageTerms image_terms_of(const EvalParams& ep, const WinConst& c, int r, double corr, double cgm, double var, double div) {
    ImageTerms t;
    const double con = (ep.contrast_kind == EINCM_CONTRAST_VARIANCE) ? var : cgm;
    const double c0 = (ep.contrast_kind == EINCM_CONTRAST_VARIANCE) ? c.c0_var : c.c0_gradmag;
    t.corr = corr; t.contrast_gm = cgm; t.var = var; t.div = div;
    t.rel_con = rel_term(c.mrw[r], con, c0);
    t.rel_corr = rel_term(c.mrw[r], corr, c.zc[r]);
    t.rel_div = ep.want_div ? rel_term(c.mrw[r], div, c.d0) : 0.0;
    return t;
}
// fp32 path (host_assemble and k_final): the reduced moments, the contrast energy sum(gx^2 + gy^2) and the sum of |div n|
EINCM_HD ImageTerms image_terms(const EvalParams& ep, const WinConst& c, int r, const ImgScal& s, double g2, double dsum, double HW) {
    const double mse = mse_from_moments(s, c.sE[r], c.sEE[r], HW);
    const double mean = s.sI / HW;
    const double var = s.sII / HW - mean * mean;
    return image_terms_of(ep, c, r, -mse, g2 / HW, var, ep.want_div ? dsum / HW : NAN);
}
// float64 path: k64_scal's means
EINCM_HD ImageTerms image_terms(const EvalParams& ep, const WinConst& c, int r, const F64Scal& s) {
    return image_terms_of(ep, c, r, -s.mse, s.g2, s.var, ep.want_div ? s.div : NAN);
}
// objective kinds: k_obj_grad's (contrast, signed correlation) against the kinds' zero-warp values; the OutScal entries stay the default kinds'
EINCM_HD ImageTerms image_terms(double mrw, double con, double corr, double c0, double zc) {
    ImageTerms t{};
    t.rel_con = rel_term(mrw, con, c0);
    t.rel_corr = rel_term(mrw, corr, zc);
    return t;
}
EINCM_HD void store_terms(OutScal& o, int r, const ImageTerms& t) { o.corr[r] = t.corr; o.contrast_gm[r] = t.contrast_gm; o.var[r] = t.var; o.div[r] = t.div; }

// One window's value and aux entries (losses.py:176-203) from the sums over reference times of the rel_* terms; mrd, tv: NAN where
// not computed.  host_assemble (tv_direct) adds gamma * TV straight to the value where the TV was computed, the others add the
// regularisers' sum: with delta == 0 (every host-assembled evaluation) the two differ in the sign of a zero value only.
EINCM_HD void assemble_window(const EvalParams& ep, int R, double sum_con, double sum_corr, double mrd, double tv, bool theta_bad, bool tv_direct,
                              OutScal& o) {
    const double mrc = sum_con / (double)R, mrr = sum_corr / (double)R;
    double val = ep.alpha * (-mrc) + ep.beta * (-mrr);
    if (tv_direct) {
        if (ep.want_tv && ep.gamma != 0.0) val += ep.gamma * tv;
    } else {
        double reg = 0.0;
        if (ep.gamma != 0.0) reg += ep.gamma * ((ep.cur_pyr_lvl <= 0) ? tv : 0.0);
        if (ep.delta != 0.0) reg += ep.delta * mrd;
        val += reg;
    }
    if (theta_bad) val = NAN;
    o.mean_rel_contrast = mrc; o.mean_rel_corr = mrr; o.mean_rel_div = mrd; o.tv = tv;
    o.value = val;
    o.nonfinite = (val - val == 0.0) ? 0.0 : 1.0;
}

// ---- host only: the assemblies eval_end_collect runs, on a view of the context's pinned memory ----

// Window b sits the evaluation out (eincm_loss_grad_masked): the host's form of the kernels' !win_active(g, b)
inline bool window_sat_out(const Geom& g, int b) { return b < 64 && !((g.wmask >> b) & 1ull); }

// Is a NaN / Inf among src[0..n)?  Copies src to dst on the way unless dst is null.  Branch-free, so that it vectorises: an OR over the
// exponent bits (an early-exit std::isfinite loop does not: 0.6 ms of a 1.8 ms dense-theta evaluation at 480x640).  No __restrict__:
// with it the compiler splits the copying loop into a memcpy and a second pass over the source (+0.1 ms on that evaluation).
inline bool copy_scan_finite(double* dst, const double* src, size_t n) {
    uint64_t bad = 0;
    if (dst) for (size_t i = 0; i < n; ++i) { uint64_t u; memcpy(&u, src + i, sizeof u); dst[i] = src[i]; bad |= (uint64_t)((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull); }
    else     for (size_t i = 0; i < n; ++i) { uint64_t u; memcpy(&u, src + i, sizeof u); bad |= (uint64_t)((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull); }
    return bad != 0;
}
// theta_nan[b]: a NaN / Inf somewhere in window b's theta (host-assembled and float64 evaluations)
inline void scan_theta(const double* theta, int B, size_t nth, uint8_t* theta_nan) {
    for (int b = 0; b < B; ++b) theta_nan[b] = copy_scan_finite(nullptr, theta + (size_t)b * nth, nth);   // (4096 values at 16x16 x 8 windows)
}

// Sum of n (x, y) pairs in four interleaved chains per component (a fixed association, so still a function of the partials alone): one
// chain is bound by the latency of the add, 4000 partials of the 8-window batch took 6 us
inline void sum_partials_4(const double* p, size_t n, double* out) {
    double ax[4] = {0.0, 0.0, 0.0, 0.0}, ay[4] = {0.0, 0.0, 0.0, 0.0};
    size_t k = 0;
    for (; k + 4 <= n; k += 4) {
        ax[0] += p[2 * k]; ay[0] += p[2 * k + 1]; ax[1] += p[2 * k + 2]; ay[1] += p[2 * k + 3];
        ax[2] += p[2 * k + 4]; ay[2] += p[2 * k + 5]; ax[3] += p[2 * k + 6]; ay[3] += p[2 * k + 7];
    }
    for (; k < n; ++k) { ax[0] += p[2 * k]; ay[0] += p[2 * k + 1]; }
    out[0] = (ax[0] + ax[1]) + (ax[2] + ax[3]); out[1] = (ay[0] + ay[1]) + (ay[2] + ay[3]);
}

struct LossView {
    const Geom* g; const EvalParams* ep;
    bool two_dof; size_t nth;                   // theta's shape
    const WinConst* wc; OutScal* outs; double* grad; const uint8_t* theta_nan;
    const double* tvparts;                      // (B,ntiles,3) k_tv's partials
    const double* img; const double* g2; const double* g11; const int32_t* win_item0; const int64_t* win_events;    // host assembly
    const F64Scal* scal;                        // float64
    const ObjConst* objc; const double* ovals; int ck, rk; bool host_asm;       // objective kinds
};

// Window b's TV term as the aux reports it, from k_tv's partials in tile order
inline double window_tv(const LossView& v, int b) {
    const double* q = v.tvparts + (size_t)b * v.g->ntiles * 3;
    double a = 0.0, nz = 0.0;
    if (v.ep->want_tv) for (int i = 0; i < v.g->ntiles; ++i) { a += q[(size_t)i * 3]; nz += q[(size_t)i * 3 + 1]; }
    return tv_reported(*v.ep, tv_value(a, nz));
}

// Host-assembled evaluations (plan.host_asm): what k_final does for them, in fp64 on the host from the partials the kernels wrote
// into pinned memory - the image scalars of k_imgrad (img), its per-workgroup contrast energies (g2) and the per-workgroup partials
// of the 2-DoF gradient (g11) - every sum in index order, so the result is a function of the partials alone (bit-reproducible).
// Without the divergence term (the planner routes those evaluations to k_final).
inline void host_assemble(const LossView& v) {
    const Geom& g = *v.g;
    const double HW = (double)g.H * (double)g.W;
    const int nwg = (g.nig + IG_NT / 64 - 1) / (IG_NT / 64);          // one contrast-energy partial per k_imgrad workgroup
    for (int b = 0; b < g.B; ++b) {
        OutScal& o = v.outs[b];
        memset(&o, 0, sizeof o);
        if (window_sat_out(g, b)) continue;       // sat this evaluation out (hand_over marks its outputs)
        double sum_rel_con = 0.0, sum_rel_corr = 0.0;
        for (int r = 0; r < g.R; ++r) {
            const double* g2p = v.g2 + ((size_t)b * g.R + r) * nwg;
            double g2 = 0.0;
            for (int i = 0; i < nwg; ++i) g2 += g2p[i];
            const ImageTerms t = image_terms(*v.ep, v.wc[b], r, unpack(v.img + ((size_t)b * g.R + r) * IMGSCAL_N), g2, 0.0, HW);
            store_terms(o, r, t);
            sum_rel_con += t.rel_con; sum_rel_corr += t.rel_corr;
        }
        assemble_window(*v.ep, g.R, sum_rel_con, sum_rel_corr, NAN, window_tv(v, b), v.theta_nan[b] != 0, true, o);
        if (v.two_dof) {                            // 2-DoF: the gather's per-workgroup partials, added in index order
            const int lo = v.win_item0[b], hi = v.win_item0[b + 1];
            sum_partials_4(v.g11 + (size_t)lo * g.R * 2, (size_t)(hi - lo) * g.R, v.grad + (size_t)b * 2);
        } else if (v.win_events[b] == 0) {          // theta grid: the gather's tail wrote dL/dtheta, unless the window has no workgroup
            for (size_t i = 0; i < v.nth; ++i) v.grad[(size_t)b * v.nth + i] = 0.0;
        }
    }
}

// What k_final does, for a float64 evaluation: from the per-image scalars and k_tv's partials, sums in index order
inline void f64_assemble(const LossView& v) {
    const Geom& g = *v.g;
    for (int b = 0; b < g.B; ++b) {
        OutScal& o = v.outs[b];
        memset(&o, 0, sizeof o);
        if (window_sat_out(g, b)) continue;
        double src = 0.0, srr = 0.0, srd = 0.0;
        for (int r = 0; r < g.R; ++r) {
            const ImageTerms t = image_terms(*v.ep, v.wc[b], r, v.scal[(size_t)b * g.R + r]);
            store_terms(o, r, t);
            src += t.rel_con; srr += t.rel_corr; srd += t.rel_div;
        }
        assemble_window(*v.ep, g.R, src, srr, v.ep->want_div ? srd / (double)g.R : NAN, window_tv(v, b), v.theta_nan[b] != 0, false, o);
    }
}

// After the kernels of an evaluation with a new kind: the assembly with the kinds' values (k_obj_grad's per-image values, the
// zero-warp values), on top of what k_final / host_assemble left for the TV and divergence terms.
inline void obj_assemble(const LossView& v) {
    const Geom& g = *v.g;
    for (int b = 0; b < g.B; ++b) {
        if (window_sat_out(g, b)) continue;
        OutScal& o = v.outs[b];
        // a NaN theta: host_assemble marks it in theta_nan, k_final in its (default-kind) value
        const bool bad = v.host_asm ? v.theta_nan[b] != 0 : o.value != o.value;
        double sum_rel_con = 0.0, sum_rel_corr = 0.0;
        for (int r = 0; r < g.R; ++r) {
            const double* q = v.ovals + ((size_t)b * g.R + r) * 2;
            const ImageTerms t = image_terms(v.wc[b].mrw[r], q[0], q[1], v.objc[b].c0[v.ck], v.objc[b].zc[v.rk][r]);
            sum_rel_con += t.rel_con; sum_rel_corr += t.rel_corr;
        }
        assemble_window(*v.ep, g.R, sum_rel_con, sum_rel_corr, o.mean_rel_div, o.tv, bad, false, o);
    }
}

// The results' way out: value and aux per window (a window that sat out: NaN value, zero gradient, no verdict).  True: a value is not finite.
inline bool hand_over(const LossView& v, bool whole_grad, double* value, eincm_aux* aux) {
    OutScal sat_out{};
    sat_out.value = sat_out.mean_rel_corr = sat_out.mean_rel_contrast = sat_out.mean_rel_div = sat_out.tv = NAN;
    bool nonfinite = false;
    for (int b = 0; b < v.g->B; ++b) {
        const bool out = window_sat_out(*v.g, b);
        if (out && whole_grad) for (size_t i = 0; i < v.nth; ++i) v.grad[(size_t)b * v.nth + i] = 0.0;
        const OutScal& o = out ? sat_out : v.outs[b];
        if (value) value[b] = o.value;
        if (aux) {
            aux[b].final_loss = o.value;
            aux[b].mean_rel_corr = o.mean_rel_corr;
            aux[b].mean_rel_contrast = o.mean_rel_contrast;
            aux[b].mean_rel_iwe_divergence = o.mean_rel_div;
            aux[b].theta_total_variation = o.tv;
        }
        if (o.nonfinite != 0.0) nonfinite = true;
    }
    return nonfinite;
}

// The window constants from the outputs of the theta = 0 pass (every IWE_r then equals the IUE)
inline void constants_from_zero_pass(const OutScal& o, int R, WinConst& wc) {
    wc.c0_gradmag = o.contrast_gm[0];
    wc.c0_var = o.var[0];
    wc.d0 = o.div[0];
    for (int r = 0; r < R; ++r) { wc.zc[r] = o.corr[r]; wc.inv_zc[r] = 1.0 / (wc.zc[r] + EPSN); }     // -MSE(E_r, n0)
    wc.inv_c0_gradmag = 1.0 / (wc.c0_gradmag + EPSN); wc.inv_c0_var = 1.0 / (wc.c0_var + EPSN);
}

// Handover (losses.py:269): theta_o = a theta_prev + (1 - a) theta, and dL/da = <dL/dtheta_o, theta_prev - theta>
inline void handover_blend(const double* a, const double* prev, const double* theta, size_t B, size_t nth, double* out) {
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < nth; ++i) out[b * nth + i] = a[b] * prev[b * nth + i] + (1.0 - a[b]) * theta[b * nth + i];
}
inline void handover_chain(const double* grad, const double* prev, const double* theta, size_t B, size_t nth, double* dvalue_da) {
    for (size_t b = 0; b < B; ++b) {
        double s = 0.0;
        for (size_t i = 0; i < nth; ++i) s += grad[b * nth + i] * (prev[b * nth + i] - theta[b * nth + i]);
        dvalue_da[b] = s;
    }
}

// compute_loss_objectives (losses.py:89-105) of window b from a full-aux evaluation's outputs; tvp: the window's (ntiles,3) partials of k_tv
inline void fill_objectives(const Geom& g, const OutScal& s, const WinConst& wc, const double* tvp, eincm_objectives_out& o) {
    memset(&o, 0, sizeof o);
    o.n_refs = g.R;
    o.zero_contrast = wc.c0_gradmag; o.zero_variance = wc.c0_var; o.zero_iwe_divergence = wc.d0;
    for (int r = 0; r < g.R; ++r) {
        o.correlations[r] = s.corr[r];
        o.zero_correlations[r] = wc.zc[r];
        o.rel_correlations[r] = rel_term(1.0, s.corr[r], wc.zc[r]);
        o.contrasts[r] = s.contrast_gm[r];
        o.rel_contrasts[r] = rel_term(1.0, s.contrast_gm[r], wc.c0_gradmag);
        o.iwe_divergences[r] = s.div[r];
        o.rel_iwe_divergences[r] = rel_term(1.0, s.div[r], wc.d0);
        o.variances[r] = s.var[r];
        o.flow_warp_losses[r] = s.var[r] / wc.c0_var;          // contrast_metrics.py:17
        o.multi_ref_weights[r] = wc.mrw[r];
    }
    o.theta_total_variation = s.tv;
    double td = 0.0;
    for (int k = 0; k < g.ntiles; ++k) td += tvp[(size_t)k * 3 + 2];
    o.theta_divergence = td / ((double)g.H * g.W);
}

}  // namespace eincm
