// eincm_event_scores.h — the rules of the per-event scores that need no GPU: what a call refuses, in which
// order, and where window b's block of `scores` / `selfs` lies in both output forms.  eincm_api.hip runs the check and derives its
// copies from the layout; engine.py restates the layout (event_scores_layout) and tests/test_event_scores_interface.py compares the
// two through tests/host/event_scores_check.cpp.
//
// As eincm_event_filter.h: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU under the sanitizers
// (tests/test_host_event_scores.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "eincm.h"

namespace eincm {

// What the call sees of the context, and of its own arguments, before anything is written
struct ScState {
    bool in_flight;        // an evaluation begun and not collected
    bool has_scores;       // scores != NULL
    bool staged, have_eval;
    bool fp64;             // EINCM_CF_FP64
    int splat_size;        // eincm_set_splat_window
    bool sharded;          // staged with EINCM_SW_DEFER_CONSTANTS
    bool has_images;       // images != NULL
    bool masked;           // the last evaluation left windows out (eincm_loss_grad_masked and its kin)
};

// The order of the checks is the order of the enum
enum ScFault { SC_OK = 0, SC_IN_FLIGHT, SC_NULL_SCORES, SC_NO_EVAL, SC_FP64, SC_SPLAT, SC_SHARDED, SC_REF_WEIGHT, SC_MASKED };

// ref_weights: NULL (the per-reference form) or n_refs doubles (the combined form), every one finite
inline ScFault sc_check(const ScState& s, const double* ref_weights, int n_refs) {
    if (s.in_flight) return SC_IN_FLIGHT;
    if (!s.has_scores) return SC_NULL_SCORES;
    if (!s.staged || !s.have_eval) return SC_NO_EVAL;
    if (s.fp64) return SC_FP64;
    if (s.splat_size != 3) return SC_SPLAT;
    if (s.sharded) return SC_SHARDED;
    for (int r = 0; ref_weights && r < n_refs; ++r)
        if (!std::isfinite(ref_weights[r])) return SC_REF_WEIGHT;
    if (!s.has_images && s.masked) return SC_MASKED;
    return SC_OK;
}

inline int sc_code(ScFault f) {
    switch (f) {
        case SC_OK: return EINCM_OK;
        case SC_NULL_SCORES: case SC_REF_WEIGHT: return EINCM_ERR_ARG;
        case SC_IN_FLIGHT: case SC_NO_EVAL: case SC_MASKED: return EINCM_ERR_STATE;
        default: return EINCM_ERR_UNSUPPORTED;
    }
}

inline const char* sc_why(ScFault f) {
    switch (f) {
        case SC_IN_FLIGHT: return "an evaluation is in flight";
        case SC_NULL_SCORES: return "null pointer argument (scores)";
        case SC_NO_EVAL: return "no evaluation yet";
        case SC_FP64: return "not supported in fp64 mode (EINCM_CF_FP64)";
        case SC_SPLAT: return "the scores have the 3x3 splat window only (eincm_set_splat_window)";
        case SC_SHARDED: return "not supported on an event-sharded staging (EINCM_SW_DEFER_CONSTANTS)";
        case SC_REF_WEIGHT: return "ref_weights must be finite";
        case SC_MASKED: return "the last evaluation left windows out, so their IWEs are not current: pass images, or evaluate every window first";
        default: return "";
    }
}

// The layout: window after window, (n_refs, n_events[b]) floats per window, or (n_events[b]) in the combined form
inline int64_t sc_block_len(int64_t n_b, int n_refs, bool combined) { return combined ? n_b : (int64_t)n_refs * n_b; }
inline int64_t sc_block_offset(const int64_t* n_events, int b, int n_refs, bool combined) {
    int64_t off = 0;
    for (int i = 0; i < b; ++i) off += sc_block_len(n_events[i], n_refs, combined);
    return off;
}
inline int64_t sc_total(const int64_t* n_events, int n_windows, int n_refs, bool combined) {
    return sc_block_offset(n_events, n_windows, n_refs, combined);
}

}   // namespace eincm
