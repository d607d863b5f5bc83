// eincm_responsibilities.h — the rules of the E-step operator (eincm_event_responsibilities) that need no GPU:
// what a call refuses, in which order, and where a window's block of `weights_out` and a group's block of `labels` lie.
// eincm_api.hip runs the check and derives its copies from the layout; engine.py restates the layout
// (event_responsibilities_layout) and tests/test_responsibilities_interface.py compares the two through
// tests/host/responsibilities_check.cpp.
//
// As eincm_event_scores.h, whose state it extends: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU
// under the sanitizers (tests/test_host_responsibilities.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "eincm.h"
#include "eincm_event_scores.h"

namespace eincm {

// What the call sees of the context, and of its own arguments, before anything is written: sc_check's state (has_scores: any of the
// four outputs is not NULL) and the staged batch
struct RsState {
    ScState sc;
    int n_windows;             // B of the staged batch
    const int64_t* n_events;   // (B), or anything when nothing is staged
};

// The order of the checks is the order of the enum
enum RsFault { RS_OK = 0, RS_IN_FLIGHT, RS_NULL_OUTPUTS, RS_NO_EVAL, RS_FP64, RS_SPLAT, RS_SHARDED, RS_MODELS, RS_GROUPS, RS_UNEQUAL,
               RS_REF_WEIGHT, RS_PRIOR, RS_MASKED };

// ref_weights: n_refs finite doubles.  prior: NULL (ones) or n_windows doubles, each finite and >= 0 as the float the kernel takes,
// every group of n_models consecutive ones with a float sum > 0 that is finite.
inline RsFault rs_check(const RsState& s, int n_models, const double* ref_weights, int n_refs, const double* prior) {
    if (s.sc.in_flight) return RS_IN_FLIGHT;
    if (!s.sc.has_scores) return RS_NULL_OUTPUTS;
    if (!s.sc.staged || !s.sc.have_eval) return RS_NO_EVAL;
    if (s.sc.fp64) return RS_FP64;
    if (s.sc.splat_size != 3) return RS_SPLAT;
    if (s.sc.sharded) return RS_SHARDED;
    if (n_models < 1 || n_models > EINCM_RS_MAX_MODELS) return RS_MODELS;
    if (s.n_windows % n_models != 0) return RS_GROUPS;
    for (int b = 0; b < s.n_windows; ++b)
        if (s.n_events[b] != s.n_events[b - b % n_models]) return RS_UNEQUAL;
    if (!ref_weights) return RS_REF_WEIGHT;
    for (int r = 0; r < n_refs; ++r)
        if (!std::isfinite(ref_weights[r])) return RS_REF_WEIGHT;
    for (int b = 0; prior && b < s.n_windows; b += n_models) {
        float sum = 0.0f;
        for (int l = 0; l < n_models; ++l) {
            const double v = prior[b + l];
            if (!std::isfinite(v) || v < 0.0 || !std::isfinite((float)v)) return RS_PRIOR;
            sum = sum + (float)v;
        }
        if (!(sum > 0.0f) || !std::isfinite(sum)) return RS_PRIOR;
    }
    if (!s.sc.has_images && s.sc.masked) return RS_MASKED;
    return RS_OK;
}

inline int rs_code(RsFault f) {
    switch (f) {
        case RS_OK: return EINCM_OK;
        case RS_NULL_OUTPUTS: case RS_MODELS: case RS_GROUPS: case RS_UNEQUAL: case RS_REF_WEIGHT: case RS_PRIOR: return EINCM_ERR_ARG;
        case RS_IN_FLIGHT: case RS_NO_EVAL: case RS_MASKED: return EINCM_ERR_STATE;
        default: return EINCM_ERR_UNSUPPORTED;
    }
}

inline const char* rs_why(RsFault f) {
    switch (f) {
        case RS_IN_FLIGHT: return sc_why(SC_IN_FLIGHT);
        case RS_NULL_OUTPUTS: return "null pointer argument (weights_out, labels, mass and n_unsupported all)";
        case RS_NO_EVAL: return sc_why(SC_NO_EVAL);
        case RS_FP64: return sc_why(SC_FP64);
        case RS_SPLAT: return sc_why(SC_SPLAT);
        case RS_SHARDED: return sc_why(SC_SHARDED);
        case RS_MODELS: return "n_models must lie within 1 .. EINCM_RS_MAX_MODELS";
        case RS_GROUPS: return "the staged windows are not a whole number of groups of n_models";
        case RS_UNEQUAL: return "the windows of a group must have equal n_events";
        case RS_REF_WEIGHT: return "ref_weights is required and must be finite";
        case RS_PRIOR: return "prior must be finite and >= 0 as floats, with a positive finite sum in every group";
        case RS_MASKED: return sc_why(SC_MASKED);
        default: return "";
    }
}

// ---- the E-step with a prior image (eincm_event_responsibilities_spatial) ----
// What it refuses beyond rs_check, after it and in the order of the enum: the prior stack comes from exactly one source, the caller's
// prior_images or (EINCM_RS_PRIOR_STAGED) the context's staged prior, and every value of the caller's is finite and >= 0.
enum RsSpatialFault { RSS_OK = 0, RSS_BOTH, RSS_NEITHER, RSS_NOT_STAGED, RSS_VALUE };

// prior_images: NULL or n_windows * npix floats.  An RSS_VALUE leaves the window in *where_b and the pixel (y * W + x) in *where_p.
inline RsSpatialFault rs_spatial_check(const float* prior_images, uint32_t flags, bool prior_staged, int n_windows, int64_t npix,
                                       int* where_b, int64_t* where_p) {
    *where_b = -1; *where_p = -1;
    const bool staged_asked = (flags & EINCM_RS_PRIOR_STAGED) != 0;
    if (prior_images && staged_asked) return RSS_BOTH;
    if (!prior_images && !staged_asked) return RSS_NEITHER;
    if (staged_asked) return prior_staged ? RSS_OK : RSS_NOT_STAGED;
    for (int b = 0; b < n_windows; ++b)
        for (int64_t p = 0; p < npix; ++p) {
            const float v = prior_images[(int64_t)b * npix + p];
            if (!std::isfinite(v) || v < 0.0f) { *where_b = b; *where_p = p; return RSS_VALUE; }
        }
    return RSS_OK;
}

inline int rs_spatial_code(RsSpatialFault f) { return f == RSS_OK ? EINCM_OK : f == RSS_NOT_STAGED ? EINCM_ERR_STATE : EINCM_ERR_ARG; }

inline const char* rs_spatial_why(RsSpatialFault f) {
    switch (f) {
        case RSS_BOTH: return "prior_images must be NULL with EINCM_RS_PRIOR_STAGED: the prior stack has one source";
        case RSS_NEITHER: return "no prior stack: hand prior_images over, or set EINCM_RS_PRIOR_STAGED for the staged prior";
        case RSS_NOT_STAGED: return "EINCM_RS_PRIOR_STAGED without a staged prior (eincm_label_prior since the last eincm_set_windows)";
        case RSS_VALUE: return "prior_images must be finite and >= 0";
        default: return "";
    }
}

// The layout.  weights_out: the combined form of sc_block_offset, window b's block is n_events[b] floats.  labels: one byte per event of
// a group, group after group; a group's event count is that of its first window.
inline int64_t rs_weights_offset(const int64_t* n_events, int b) { return sc_block_offset(n_events, b, 1, true); }
inline int64_t rs_weights_total(const int64_t* n_events, int n_windows) { return sc_total(n_events, n_windows, 1, true); }
inline int64_t rs_group_events(const int64_t* n_events, int g, int n_models) { return n_events[(int64_t)g * n_models]; }
inline int64_t rs_labels_offset(const int64_t* n_events, int g, int n_models) {
    int64_t off = 0;
    for (int i = 0; i < g; ++i) off += rs_group_events(n_events, i, n_models);
    return off;
}
inline int64_t rs_labels_total(const int64_t* n_events, int n_windows, int n_models) {
    return rs_labels_offset(n_events, n_windows / n_models, n_models);
}

}   // namespace eincm
