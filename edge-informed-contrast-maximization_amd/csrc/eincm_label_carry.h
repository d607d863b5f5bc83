// eincm_label_carry.h — the rules of the label prior carried along the models' own motions to the next window (DESIGN.md section 33;
// eincm_carry_label_prior, eincm_adopt_carried_prior) that need no GPU: what the calls refuse, in which order, the fixed-point scale of
// the forward splat with the proof that no accepted input overflows an accumulator, the resolve rule as a plain function, and where a
// (group, model)'s block of every output lies.  eincm_api.hip runs the checks and derives its copies from the layout; the kernels
// (eincm_label_carry.hip.h) call the same lc_resolve, and the landing and the tap weights are eincm_theta_advect.h's, reused as they
// are; engine.py restates the layout (label_carry_layout) and tests/test_host_label_carry.py compares the two through
// tests/host/label_carry_check.cpp.
//
// As eincm_label_prior.h, whose checks it runs first: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU
// under the sanitizers.
//
// The scale.  A source pixel p of model l with mass M_l(p) > 0 (uint32: k_ml_mass) lands at q = p + f_l(p) tau (ta_landing) and
// deposits M_l(p) w into the uint64 accumulator A_l at each of the up to four pixels around q, w = ta_weight, the four summing to
// LC_FULL = 2^20.  C_l = lc_resolve(A_l) = min((A_l + 2^19) >> 20, 2^32 - 1): half up, saturating.
// Proof.  Whatever the field does - all of a model's mass may land on one pixel - a cell of A_l holds at most
//   LC_FULL * (total mass of model l) <= 2^20 * ML_Q_ONE * n_events = 2^32 n_events
// with n_events the events of the model's window (every event adds at most ML_Q_ONE = 4096 to one pixel's mass).  Staging accepts at
// most LC_STAGING_EVENTS_MAX = 2 * 10^9 < 2^31 events in a batch (eincm_create's max_events_total), so A < 2^63.  lc_check refuses a
// window above LC_EVENTS_MAX = 2^32 - 1 all the same, the largest count with 2^32 n < 2^64, so the proof stands on this header alone
// if staging's limit ever moves.  `dropped` sums the same products over fewer terms, so it has the same bound.  Every partial sum has
// the bound too and integer adds commute, so the order the atomics arrive in does not matter.  C < 2^32 by the saturation, which is
// what lp_prior's proof (T < 2^53) needs of the masses it is handed.
#pragma once
#include <cstdint>

#include "eincm.h"
#include "eincm_label_prior.h"
#include "eincm_theta_advect.h"

namespace eincm {

constexpr unsigned LC_FLAGS = 0u;                                  // every flag bit the call knows: none yet
constexpr int LC_SHIFT = 2 * TA_K;                                 // 20
constexpr uint64_t LC_FULL = (uint64_t)TA_FULL;                    // what the four taps of a source sum to: 2^20
constexpr uint64_t LC_HALF = LC_FULL >> 1;
constexpr uint64_t LC_CARRIED_MAX = 0xFFFFFFFFull;                 // where lc_resolve saturates
constexpr int64_t LC_STAGING_EVENTS_MAX = 2000000000;              // eincm_create refuses a larger max_events_total
constexpr int64_t LC_EVENTS_MAX = 0xFFFFFFFFll;                    // the largest n with LC_FULL * ML_Q_ONE * n < 2^64
static_assert(LC_FULL == (1ull << LC_SHIFT), "the four weights of ta_weight sum to 2^(2 TA_K)");
static_assert(LC_FULL * ML_Q_ONE == (1ull << 32) && (uint64_t)LC_EVENTS_MAX <= ~0ull / (LC_FULL * ML_Q_ONE), "the overflow proof");
static_assert(LC_STAGING_EVENTS_MAX <= LC_EVENTS_MAX, "staging's own limit already keeps the accumulators below 2^64");

// ---- the resolve rule: the kernel runs this very function ----
// (a + 2^19) >> 20 written as the quotient plus the bit below it, which is the same number and cannot wrap: the rule holds for every
// uint64, not only for the a < 2^63 of the proof
EINCM_HD uint32_t lc_resolve(uint64_t a) {
    const uint64_t c = (a >> LC_SHIFT) + ((a >> (LC_SHIFT - 1)) & 1ull);
    return c > LC_CARRIED_MAX ? (uint32_t)LC_CARRIED_MAX : (uint32_t)c;
}

// ---- what eincm_carry_label_prior refuses ----
struct LcArgs {
    bool has_coeffs, has_tau, model_set;
    int n_coeffs, model_coeffs;        // the caller's K_c, the model's (anything when none is set)
    const double* tau;                 // (G), read only where has_tau and lp_check has passed
    unsigned flags;
};

// lp_check's faults keep their numbers (an LcFault below LC_NULL is that LpFault); the call's own follow in the order of the checks
enum LcFault { LC_OK = 0, LC_NULL = 64, LC_TAU, LC_NO_MODEL, LC_WIDTH, LC_BAD_FLAGS, LC_EVENTS };

// An LP_CROWDED leaves the window and the tile in *where_b / *where_i, an LC_TAU the group, an LC_EVENTS the window; any other -1.
// flags go to the call's own check, not to lp_check (whose known bits are another call's).
inline int lc_check(const LpState& s, const LcArgs& a, int n_models, int radius, int* where_b, int64_t* where_i) {
    if (const LpFault f = lp_check(s, n_models, radius, 0u, where_b, where_i)) return (int)f;
    if (!a.has_coeffs || !a.has_tau) return LC_NULL;
    const int G = s.n_windows / n_models;
    for (int g = 0; g < G; ++g) if (!__builtin_isfinite(a.tau[g])) { *where_b = g; return LC_TAU; }
    if (!a.model_set) return LC_NO_MODEL;
    if (a.n_coeffs != a.model_coeffs) return LC_WIDTH;
    if (a.flags & ~LC_FLAGS) return LC_BAD_FLAGS;
    for (int b = 0; b < s.n_windows; ++b) if (s.n_events[b] > LC_EVENTS_MAX) { *where_b = b; return LC_EVENTS; }
    return LC_OK;
}

inline int lc_code(int f) {
    if (f < LC_NULL) return lp_code((LpFault)f);
    switch (f) {
        case LC_NO_MODEL: return EINCM_ERR_STATE;
        case LC_EVENTS: return EINCM_ERR_UNSUPPORTED;
        default: return EINCM_ERR_ARG;
    }
}

inline const char* lc_why(int f) {
    if (f < LC_NULL) return lp_why((LpFault)f);
    switch (f) {
        case LC_NULL: return "null pointer argument (coeffs, tau)";
        case LC_TAU: return "tau must be finite";
        case LC_NO_MODEL: return "needs a motion model (eincm_set_motion_model)";
        case LC_WIDTH: return "n_coeffs is not the motion model's";
        case LC_BAD_FLAGS: return "unknown flag bits (the call has none yet)";
        case LC_EVENTS: return "a window holds more than 2^32 - 1 events: a uint64 accumulator could overflow";
        default: return "";
    }
}

// ---- what eincm_adopt_carried_prior refuses ----
struct LcCarried {                     // what the context remembers of the carried prior
    bool valid;
    int n_models, n_windows, H, W;
};
enum LcAdoptFault { LCA_OK = 0, LCA_IN_FLIGHT, LCA_NOT_STAGED, LCA_NONE, LCA_MODELS, LCA_WINDOWS, LCA_SENSOR };

inline LcAdoptFault lc_adopt_check(bool in_flight, bool staged, const LcCarried& k, int n_models, int n_windows, int H, int W) {
    if (in_flight) return LCA_IN_FLIGHT;
    if (!staged) return LCA_NOT_STAGED;
    if (!k.valid) return LCA_NONE;
    if (k.n_models != n_models) return LCA_MODELS;
    if (k.n_windows != n_windows) return LCA_WINDOWS;
    if (k.H != H || k.W != W) return LCA_SENSOR;
    return LCA_OK;
}

inline int lc_adopt_code(LcAdoptFault f) { return f == LCA_OK ? EINCM_OK : f <= LCA_NONE ? EINCM_ERR_STATE : EINCM_ERR_ARG; }

inline const char* lc_adopt_why(LcAdoptFault f) {
    switch (f) {
        case LCA_IN_FLIGHT: return ml_why(ML_IN_FLIGHT);
        case LCA_NOT_STAGED: return lp_why(LP_NOT_STAGED);
        case LCA_NONE: return "no carried prior (eincm_carry_label_prior)";
        case LCA_MODELS: return "the carried prior was formed with another n_models";
        case LCA_WINDOWS: return "the carried prior was formed on a batch of another number of windows";
        case LCA_SENSOR: return "the carried prior was formed on another sensor";
        default: return "";
    }
}

// The layout, in elements of each output's own type, row-major inside a block.
//   prior (B, H, W) float: window b = g * n_models + l is model l of group g | carried (G, n_models, H, W) uint32
//   accum (G, n_models, H, W) uint64 | dropped (G, n_models) uint64
inline int64_t lc_prior_offset(int b, int H, int W) { return lp_prior_offset(b, H, W); }
inline int64_t lc_carried_offset(int g, int l, int n_models, int H, int W) { return ((int64_t)g * n_models + l) * H * W; }
inline int64_t lc_accum_offset(int g, int l, int n_models, int H, int W) { return ((int64_t)g * n_models + l) * H * W; }
inline int64_t lc_dropped_offset(int g, int l, int n_models) { return (int64_t)g * n_models + l; }

}   // namespace eincm
