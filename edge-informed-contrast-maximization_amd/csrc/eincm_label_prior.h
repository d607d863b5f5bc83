// eincm_label_prior.h — the rules of the per-pixel label prior (eincm_label_prior) that need no GPU: what a call
// refuses, in which order, where a window's block of `prior` and a (group, model)'s block of `smoothed` lie, and the per-pixel rule
// lp_prior as a plain function.  eincm_api.hip runs the check and derives its copies from the layout; the kernel
// (eincm_label_prior.hip.h) calls the same lp_prior, so host and device cannot drift apart; engine.py restates the layout
// (label_prior_layout) and tests/test_host_label_prior.py compares the two through tests/host/label_prior_check.cpp.
//
// As eincm_motion_layers.h, whose mass images it smooths: no HIP, no environment.  Plain C++17, so the checker runs all of it on the
// CPU under the sanitizers.
#pragma once
#include <cstdint>

#include "eincm.h"
#include "eincm_motion_layers.h"

namespace eincm {

constexpr unsigned LP_FLAGS = 0u;                   // every flag bit the call knows: none yet

// What the call sees of the context before anything is written (both outputs may be NULL: the prior is staged all the same)
struct LpState {
    bool in_flight, staged, fp64, sharded;
    int n_windows;             // B of the staged batch (anything when nothing is staged)
    const int64_t* n_events;   // (B), or anything when nothing is staged
    const int32_t* tilecount;  // (B, ntiles) events per (window, 32x32 source tile) of the staged batch, as staging left them
    int64_t n_tilecounts;      // B * ntiles
};

// The order of the checks is the order of the enum, and that of ml_check for the faults the two share
enum LpFault { LP_OK = 0, LP_IN_FLIGHT, LP_NOT_STAGED, LP_FP64, LP_SHARDED, LP_MODELS, LP_GROUPS, LP_UNEQUAL, LP_RADIUS, LP_BAD_FLAGS,
               LP_CROWDED };

// An LP_CROWDED leaves the window in *where_b and the tile in *where_i; any other fault leaves both at -1.
inline LpFault lp_check(const LpState& s, int n_models, int radius, unsigned flags, int* where_b, int64_t* where_i) {
    *where_b = -1; *where_i = -1;
    if (s.in_flight) return LP_IN_FLIGHT;
    if (!s.staged) return LP_NOT_STAGED;
    if (s.fp64) return LP_FP64;
    if (s.sharded) return LP_SHARDED;
    if (n_models < 1 || n_models > EINCM_RS_MAX_MODELS) return LP_MODELS;
    if (s.n_windows % n_models != 0) return LP_GROUPS;
    for (int b = 0; b < s.n_windows; ++b)
        if (s.n_events[b] != s.n_events[b - b % n_models]) return LP_UNEQUAL;
    if (radius < 0 || radius > EINCM_LP_MAX_RADIUS) return LP_RADIUS;
    if (flags & ~LP_FLAGS) return LP_BAD_FLAGS;
    const int64_t ntiles = s.n_windows > 0 ? s.n_tilecounts / s.n_windows : 0;
    for (int64_t i = 0; i < s.n_tilecounts; ++i)
        if (s.tilecount[i] >= ML_TILE_EVENTS_MAX) { *where_b = (int)(i / ntiles); *where_i = i % ntiles; return LP_CROWDED; }
    return LP_OK;
}

inline int lp_code(LpFault f) {
    switch (f) {
        case LP_OK: return EINCM_OK;
        case LP_IN_FLIGHT: case LP_NOT_STAGED: return EINCM_ERR_STATE;
        case LP_FP64: case LP_SHARDED: case LP_CROWDED: return EINCM_ERR_UNSUPPORTED;
        default: return EINCM_ERR_ARG;
    }
}

inline const char* lp_why(LpFault f) {
    switch (f) {
        case LP_IN_FLIGHT: return ml_why(ML_IN_FLIGHT);
        case LP_NOT_STAGED: return "needs staged windows (eincm_set_windows)";
        case LP_FP64: return ml_why(ML_FP64);
        case LP_SHARDED: return ml_why(ML_SHARDED);
        case LP_MODELS: return ml_why(ML_MODELS);
        case LP_GROUPS: return ml_why(ML_GROUPS);
        case LP_UNEQUAL: return ml_why(ML_UNEQUAL);
        case LP_RADIUS: return "radius must lie within 0 .. EINCM_LP_MAX_RADIUS";
        case LP_BAD_FLAGS: return "unknown flag bits (the call has none yet)";
        case LP_CROWDED: return ml_why(ML_CROWDED);
        default: return "";
    }
}

// The layout, in elements of each output's own type, row-major inside a block.
//   prior (B, H, W) float: window b = g * n_models + l is model l of group g | smoothed (G, n_models, H, W) uint64
inline int64_t lp_prior_offset(int b, int H, int W) { return (int64_t)b * H * W; }
inline int64_t lp_smoothed_offset(int g, int l, int n_models, int H, int W) { return ((int64_t)g * n_models + l) * H * W; }

// ---- the per-pixel rule: the kernel runs this very function ----

// n_l = S[l] + floor_mass, T = n_0 + ... + n_{K-1}, out[l] = T == 0 ? 1 : (float)((double)n_l / (double)T).  S[l] is a box sum of at
// most 17 x 17 pixel masses below 2^32 and K <= 8, so T < 2^53 and both conversions are exact: one rounded fp64 division and one
// rounding to float.  The loops run to a K the kernel knows at compile time, so they unroll there and nothing is indexed at run time.
EINCM_HD void lp_prior(const uint64_t* S, int K, uint32_t floor_mass, float* out) {
    uint64_t T = 0;
    for (int l = 0; l < K; ++l) T += S[l] + floor_mass;
    for (int l = 0; l < K; ++l) out[l] = T == 0 ? 1.0f : (float)((double)(S[l] + floor_mass) / (double)T);
}

}   // namespace eincm
