// eincm_motion_layers.h — the rules of the composition of a motion segmentation into one flow field and a label image (DESIGN.md
// section 30; eincm_compose_motions) that need no GPU: what a call refuses, in which order, where a group's block of every output
// lies, and the four per-pixel rules - the quantised weight, the label, the dominant model and the soft blend - as plain functions.
// eincm_api.hip runs the check and derives its copies from the layout; the kernels (eincm_motion_layers.hip.h) call the same four
// functions, so host and device cannot drift apart; engine.py restates the layout (compose_motions_layout) and
// tests/test_motion_layers_interface.py compares the two through tests/host/motion_layers_check.cpp.
//
// As eincm_responsibilities.h: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU under the sanitizers
// (tests/test_host_motion_layers.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "eincm.h"
#include "eincm_types.h"

namespace eincm {

constexpr int ML_TILE_EVENTS_MAX = 1 << 20;         // a (window, tile) with this many events is refused: (2^20 - 1) * 4096 < 2^32
constexpr uint32_t ML_Q_ONE = 4096u;                // q(1): the quantised weight of an event of an unweighted batch
constexpr unsigned ML_FLAGS = EINCM_ML_SOFT | EINCM_ML_FILL_DOMINANT;      // every flag bit the call knows

// What the call sees of the context, and of its own arguments, before anything is written
struct MlState {
    bool in_flight, has_outputs, staged, model_set, fp64, sharded;
    int n_windows;             // B of the staged batch (anything when nothing is staged)
    const int64_t* n_events;   // (B), or anything when nothing is staged
    int n_coeffs;              // K_c of the model (anything when none is set)
    const int32_t* tilecount;  // (B, ntiles) events per (window, 32x32 source tile) of the staged batch, as staging left them
    int64_t n_tilecounts;      // B * ntiles
};

// The order of the checks is the order of the enum
enum MlFault { ML_OK = 0, ML_IN_FLIGHT, ML_NULL_OUTPUTS, ML_NOT_READY, ML_FP64, ML_SHARDED, ML_MODELS, ML_GROUPS, ML_UNEQUAL, ML_COEFFS,
               ML_BAD_FLAGS, ML_CROWDED };

// coeffs: (B, K_c) doubles.  An ML_COEFFS for a value that is not finite leaves the window in *where_b and the coefficient's index in
// *where_i; for a NULL coeffs both are -1.  An ML_CROWDED leaves the window and the tile there.
inline MlFault ml_check(const MlState& s, int n_models, const double* coeffs, unsigned flags, int* where_b, int64_t* where_i) {
    *where_b = -1; *where_i = -1;
    if (s.in_flight) return ML_IN_FLIGHT;
    if (!s.has_outputs) return ML_NULL_OUTPUTS;
    if (!s.staged || !s.model_set) return ML_NOT_READY;
    if (s.fp64) return ML_FP64;
    if (s.sharded) return ML_SHARDED;
    if (n_models < 1 || n_models > EINCM_RS_MAX_MODELS) return ML_MODELS;
    if (s.n_windows % n_models != 0) return ML_GROUPS;
    for (int b = 0; b < s.n_windows; ++b)
        if (s.n_events[b] != s.n_events[b - b % n_models]) return ML_UNEQUAL;
    if (!coeffs) return ML_COEFFS;
    for (int b = 0; b < s.n_windows; ++b)
        for (int k = 0; k < s.n_coeffs; ++k)
            if (!std::isfinite(coeffs[(int64_t)b * s.n_coeffs + k])) { *where_b = b; *where_i = k; return ML_COEFFS; }
    if (flags & ~ML_FLAGS) return ML_BAD_FLAGS;
    const int64_t ntiles = s.n_windows > 0 ? s.n_tilecounts / s.n_windows : 0;
    for (int64_t i = 0; i < s.n_tilecounts; ++i)
        if (s.tilecount[i] >= ML_TILE_EVENTS_MAX) { *where_b = (int)(i / ntiles); *where_i = i % ntiles; return ML_CROWDED; }
    return ML_OK;
}

inline int ml_code(MlFault f) {
    switch (f) {
        case ML_OK: return EINCM_OK;
        case ML_IN_FLIGHT: case ML_NOT_READY: return EINCM_ERR_STATE;
        case ML_FP64: case ML_SHARDED: case ML_CROWDED: return EINCM_ERR_UNSUPPORTED;
        default: return EINCM_ERR_ARG;
    }
}

inline const char* ml_why(MlFault f) {
    switch (f) {
        case ML_IN_FLIGHT: return "an evaluation is in flight";
        case ML_NULL_OUTPUTS: return "null pointer argument (theta, labels, mass and total all)";
        case ML_NOT_READY: return "needs staged windows (eincm_set_windows) and a motion model (eincm_set_motion_model)";
        case ML_FP64: return "not supported in fp64 mode (EINCM_CF_FP64)";
        case ML_SHARDED: return "not supported on an event-sharded staging (EINCM_SW_DEFER_CONSTANTS)";
        case ML_MODELS: return "n_models must lie within 1 .. EINCM_RS_MAX_MODELS";
        case ML_GROUPS: return "the staged windows are not a whole number of groups of n_models";
        case ML_UNEQUAL: return "the windows of a group must have equal n_events";
        case ML_COEFFS: return "coeffs is required and must be finite";
        case ML_BAD_FLAGS: return "unknown flag bits (EINCM_ML_SOFT and EINCM_ML_FILL_DOMINANT are all there is)";
        case ML_CROWDED: return "a 32x32 source tile of one window holds 2^20 events or more: a pixel's uint32 mass could overflow";
        default: return "";
    }
}

// The layout, in elements of each output's own type: a group's block after the previous group's, row-major inside.
//   theta (G, H, W, 2) double | labels (G, H, W) uint8 | mass (G, n_models, H, W) uint32 | total (G, n_models) uint64
inline int64_t ml_theta_offset(int g, int H, int W) { return (int64_t)g * H * W * 2; }
inline int64_t ml_labels_offset(int g, int H, int W) { return (int64_t)g * H * W; }
inline int64_t ml_mass_offset(int g, int l, int n_models, int H, int W) { return ((int64_t)g * n_models + l) * H * W; }
inline int64_t ml_total_offset(int g, int l, int n_models) { return (int64_t)g * n_models + l; }

// ---- the per-pixel rules: the kernels run these very functions ----

// q(w) = (uint32) rintf(w * 4096): the scaling by 2^12 is exact in fp32, the rounding is half to even (the default rounding mode;
// v_rndne_f32 on the device).  w lies in [0, 1] (staging refuses anything else), so q <= 4096.
EINCM_HD uint32_t ml_q(float w) { return (uint32_t)rintf(w * 4096.0f); }

// The lowest l with the largest mass[l * stride], if that mass is > 0; else EINCM_ML_NO_LABEL
EINCM_HD int ml_label(const uint32_t* mass, int n_models, int64_t stride = 1) {
    int lab = 0; uint32_t best = mass[0];
    for (int l = 1; l < n_models; ++l) { const uint32_t m = mass[(int64_t)l * stride]; if (m > best) { best = m; lab = l; } }
    return best > 0u ? lab : EINCM_ML_NO_LABEL;
}

// The lowest l with the largest total[l], if that total is > 0; else -1 (the fill is then (0, 0))
EINCM_HD int ml_dominant(const uint64_t* total, int n_models) {
    int d = 0; uint64_t best = total[0];
    for (int l = 1; l < n_models; ++l) if (total[l] > best) { best = total[l]; d = l; }
    return best > 0u ? d : -1;
}

// One step of the soft blend of one component: l == 0 starts the sum at a_0 f_0, every later l adds a_l f_l, with
// a_l = (double)mass_l / (double)S.  The division, the product and the sum are rounded on their own.  S > 0.
EINCM_HD double ml_blend_step(double acc, int l, uint32_t mass_l, uint64_t S, double f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = (double)mass_l / (double)S;
    const double t = a * f;
    return l == 0 ? t : acc + t;
}

// The blend of one pixel written out: f (n_models, 2), out (2).  S = sum_l mass[l] > 0.
inline void ml_soft_blend(const uint32_t* mass, int n_models, const double* f, double* out) {
    uint64_t S = 0;
    for (int l = 0; l < n_models; ++l) S += mass[l];
    for (int a = 0; a < 2; ++a) {
        double acc = 0.0;
        for (int l = 0; l < n_models; ++l) acc = ml_blend_step(acc, l, mass[l], S, f[l * 2 + a]);
        out[a] = acc;
    }
}

}   // namespace eincm
