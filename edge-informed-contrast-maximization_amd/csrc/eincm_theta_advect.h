// eincm_theta_advect.h — the rules of the theta transport between windows that need no GPU: what a call
// refuses, in which order, the two fixed-point scales with the proof that no accepted input overflows an accumulator, and the
// quantisers the host's checks and the kernels (eincm_theta_advect.hip.h) both run.  eincm_api.hip runs the checks;
// tests/test_theta_advect_interface.py runs them through tests/host/theta_advect_check.cpp and compares the quantisers with the
// witness (tests/_theta_advect_witness.py).
//
// As eincm_event_scores.h: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU under the sanitizers.
//
// The scales.  A source pixel deposits Q = llrint(Theta 2^S) with four integer weights that sum to 2^(2K), into i64 accumulators:
//   TA_K = 10   bits of each of the two bilinear fractions: a weight is a product of two integers in [0, 2^10], at most 2^20
//   TA_S = 13   a value step is 2^-13 px
//   TA_MAX_PIXELS = 2^21   the largest sensor (H W) a call accepts
//   TA_THETA_MAX = 511     the largest |theta| L a call accepts, L = ta_tap_gain (1 for a dense theta and for bilinear)
// Proof.  |Theta(p)| = |sum_i a_i sum_j b_j theta_ij| <= L max|theta| (1 + 2^-52)^n, L = (max_y sum_i |a_i|)(max_x sum_j |b_j|),
// for the n < 2^17 rounded operations of the two sums (h + w <= 65534 taps), so |Theta| <= 511 (1 + 2^-34) < 511.5 and
// |Q| <= 511.5 2^13 + 0.5 < 2^22.  The four
// taps of one source lie on four different pixels, so a pixel receives at most one tap, of weight <= 2^20, per source, from at most
// H W <= 2^21 sources: Wacc <= 2^41 and |Uacc|, |Vacc| < 2^21 2^20 2^22 = 2^63, strictly, even if every source of the sensor lands
// on one pixel.  Every partial sum has the same bound, so the order the atomics arrive in does not matter.
// Resolution.  The transported value is sum(w Q) / sum(w) 2^-13: the values are held to 2^-14 px (half a step), and a landing
// position to 2^-11 px (half a weight step of 2^-10) in each axis.
#pragma once
#include <cstdint>

#include "eincm.h"
#include "eincm_plan.h"

// Every sum and product below is rounded on its own, on both sides (hipcc contracts a * b + c by default)
#if defined(__clang__)
#define EINCM_TA_UNFUSED _Pragma("clang fp contract(off)")
#else
#define EINCM_TA_UNFUSED
#endif

namespace eincm {

constexpr int TA_K = 10;
constexpr int TA_S = 13;
constexpr int64_t TA_ONE = (int64_t)1 << TA_K;             // the weight of a whole fraction
constexpr int64_t TA_FULL = TA_ONE * TA_ONE;               // what the four taps of a source sum to
constexpr int64_t TA_MAX_PIXELS = (int64_t)1 << 21;
constexpr double TA_THETA_MAX = 511.0;
constexpr double TA_VALUE_SCALE = (double)((int64_t)1 << TA_S);
constexpr double TA_VALUE_STEP = 1.0 / TA_VALUE_SCALE;
constexpr double TA_COVERAGE_STEP = 1.0 / (double)TA_FULL;

// ---- the quantisers (host checks and kernels alike; every operation is exact or one IEEE rounding) ----
// Q(v) = llrint(v 2^S), ties to even; |v| <= 512 on every accepted input
EINCM_HD int64_t ta_quantise(double v) { return (int64_t)__builtin_rint(v * TA_VALUE_SCALE); }
EINCM_HD double ta_dequantise(int64_t q) { return (double)q * TA_VALUE_STEP; }

// Where source (x, y) with flow (vx, vy) lands after tau: the pixel (x0, y0) above and left of q, in [-1, W - 1] x [-1, H - 1], and
// the two fractions in units of 2^-K, in [0, 2^K].  false: q is not finite or lies outside (-1, W) x (-1, H); nothing is deposited.
struct TaLanding { int x0, y0; int64_t ix, iy; };
EINCM_HD bool ta_landing(int x, int y, double vx, double vy, double tau, int H, int W, TaLanding& l) {
    EINCM_TA_UNFUSED
    const double px = vx * tau, py = vy * tau;
    const double qx = (double)x + px, qy = (double)y + py;
    if (!(qx > -1.0 && qx < (double)W && qy > -1.0 && qy < (double)H)) return false;       // false for NaN and +-inf
    const double fx = __builtin_floor(qx), fy = __builtin_floor(qy);
    l.x0 = (int)fx; l.y0 = (int)fy;
    l.ix = (int64_t)__builtin_rint((qx - fx) * (double)TA_ONE);
    l.iy = (int64_t)__builtin_rint((qy - fy) * (double)TA_ONE);
    return true;
}
// the weight of tap (dx, dy) in {0, 1}^2 of a landing: the four sum to TA_FULL exactly
EINCM_HD int64_t ta_weight(const TaLanding& l, int dx, int dy) { return (dx ? l.ix : TA_ONE - l.ix) * (dy ? l.iy : TA_ONE - l.iy); }

// ---- what a call refuses ----
struct TaArgs {
    bool has_theta, has_tau, has_gain, has_out;            // the four pointers that must not be NULL
    int n, h, w, H, W, method, fill;
    const double* tau;                                     // n each (read only where has_tau / has_gain)
    const double* gain;
    double min_coverage;
};

// The order of the checks is the order of the enum.  TA_RANGE is ta_range_ok's, run last (it reads every value of theta).
enum TaFault { TA_OK = 0, TA_NULL, TA_N, TA_SHAPE, TA_SENSOR, TA_METHOD, TA_FILL, TA_TAU, TA_GAIN, TA_MIN_COVERAGE, TA_RANGE };

inline TaFault ta_check(const TaArgs& a) {
    if (!a.has_theta || !a.has_tau || !a.has_gain || !a.has_out) return TA_NULL;
    if (a.n < 1 || a.n > 65535) return TA_N;
    if (a.h < 1 || a.w < 1 || a.h > a.H || a.w > a.W) return TA_SHAPE;
    if ((int64_t)a.H * a.W > TA_MAX_PIXELS) return TA_SENSOR;
    if (a.method < 0 || a.method > EINCM_METHOD_CUBIC) return TA_METHOD;
    if (a.fill != EINCM_TA_FILL_SOURCE && a.fill != EINCM_TA_FILL_ZERO) return TA_FILL;
    for (int b = 0; b < a.n; ++b) if (!__builtin_isfinite(a.tau[b])) return TA_TAU;
    for (int b = 0; b < a.n; ++b) if (!__builtin_isfinite(a.gain[b])) return TA_GAIN;
    if (!(a.min_coverage > 0.0 && a.min_coverage <= 1.0)) return TA_MIN_COVERAGE;          // false for NaN
    return TA_OK;
}

// L of the proof: (max over sensor rows of sum |a_i|) (max over sensor columns of sum |b_j|) of the tap tables the kernels read.
// The runs are padded with zeros to their strides, which add nothing.
inline double ta_tap_gain(const TapTables& t, int H, int W) {
    auto most = [](const double* wt, int n_out, int stride) {
        double m = 0.0;
        for (int o = 0; o < n_out; ++o) {
            double s = 0.0;
            for (int k = 0; k < stride; ++k) s += std::fabs(wt[(size_t)o * stride + k]);
            m = std::max(m, s);
        }
        return m;
    };
    return most(Packer::f64(t.tab.buf.data(), 0), H, t.rstride) * most(Packer::f64(t.tab.buf.data(), t.o_cw), W, t.cstride);
}

// The value-range rule: every component of theta is finite and |theta| L <= TA_THETA_MAX (tap_gain: 1.0 for a dense theta)
inline bool ta_range_ok(const double* theta, size_t count, double tap_gain) {
    for (size_t k = 0; k < count; ++k)
        if (!(std::fabs(theta[k]) * tap_gain <= TA_THETA_MAX)) return false;                // false for NaN; inf fails the bound
    return true;
}

inline int ta_code(TaFault f) { return f == TA_OK ? EINCM_OK : EINCM_ERR_ARG; }

inline const char* ta_why(TaFault f) {
    switch (f) {
        case TA_NULL: return "null pointer argument (theta, tau, gain, out_theta)";
        case TA_N: return "n outside 1..65535";
        case TA_SHAPE: return "theta shape outside 1x1 .. the sensor's";
        case TA_SENSOR: return "the sensor has more than 2^21 pixels";
        case TA_METHOD: return "method unknown";
        case TA_FILL: return "fill is neither EINCM_TA_FILL_SOURCE nor EINCM_TA_FILL_ZERO";
        case TA_TAU: return "tau must be finite";
        case TA_GAIN: return "gain must be finite";
        case TA_MIN_COVERAGE: return "min_coverage outside (0, 1]";
        case TA_RANGE: return "a theta value is not finite, or scales beyond the 511 px the fixed-point accumulators hold";
        default: return "";
    }
}

}   // namespace eincm
