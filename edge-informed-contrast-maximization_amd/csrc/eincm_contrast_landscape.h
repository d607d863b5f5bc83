// eincm_contrast_landscape.h — the rules of the contrast landscape (eincm_contrast_landscape) that need no GPU:
// what a call refuses, in which order, and how the image of cell counts is cut into the bands that one workgroup each holds in LDS.
// eincm_api.hip runs the check and sizes its launch from the plan; the kernel (eincm_contrast_landscape.hip.h) reads the plan's
// numbers and recomputes none.
//
// As eincm_responsibilities.h: no HIP, no environment.  Plain C++17, so tests/host/contrast_landscape_check.cpp runs all of it on the
// CPU under the sanitizers (tests/test_host_contrast_landscape.py).
//
// The operator counts where events land, nothing else: an event warped outside the sensor is DROPPED.  The reference's image of warped
// events lets Python's negative indices wrap such an event to the far side of the image; that wrap does not apply here, because a
// landscape that rewards a candidate for throwing its events over the edge would mislead the search it exists to seed.
#pragma once
#include <cmath>
#include <cstdint>

#include "eincm.h"

namespace eincm {

constexpr int CL_NT = 1024;                         // threads per workgroup of k_contrast_landscape: 16 waves
constexpr int CL_LDS_BYTES = 65536;                 // what a workgroup may use in all: the static limit, no function attribute
constexpr int CL_RED_BYTES = 2 * (CL_NT / 64) * 8;  // the waves' two 64-bit partials
constexpr int CL_TABLE_MAX = 2048;                  // the W + H table of normalised coordinates is kept up to this many doubles (a quarter
                                                    // of the LDS); a larger sensor divides per event instead

// What the call sees of the context before anything is written
struct ClState {
    bool in_flight, has_outputs, staged, model_set, sharded;
    int n_windows;             // B of the staged batch (anything when nothing is staged)
    int n_coeffs;              // K of the model (anything when none is set)
};

// The order of the checks is the order of the enum
enum ClFault { CL_OK = 0, CL_IN_FLIGHT, CL_NULL_OUTPUTS, CL_NOT_STAGED, CL_NO_MODEL, CL_SHARDED, CL_RANGE, CL_NULL_INPUT, CL_NONFINITE };

inline int cl_log2_cell(int cell) { return cell == 1 ? 0 : cell == 2 ? 1 : cell == 4 ? 2 : cell == 8 ? 3 : -1; }

// coeffs: (B, V, K) doubles, t_ref: (B) doubles.  A CL_NONFINITE leaves the window in *where_b and the index in *where_i: the flat
// index j * K + k of the coefficient inside its window, or -1 for the window's t_ref (the coefficients are looked at first).
inline ClFault cl_check(const ClState& s, int n_candidates, int cell, const double* coeffs, const double* t_ref, int* where_b,
                        int64_t* where_i) {
    if (s.in_flight) return CL_IN_FLIGHT;
    if (!s.has_outputs) return CL_NULL_OUTPUTS;
    if (!s.staged) return CL_NOT_STAGED;
    if (!s.model_set) return CL_NO_MODEL;
    if (s.sharded) return CL_SHARDED;
    if (n_candidates < 1 || n_candidates > EINCM_CL_MAX_CANDIDATES || cl_log2_cell(cell) < 0) return CL_RANGE;
    if (!coeffs || !t_ref) return CL_NULL_INPUT;
    const int64_t per = (int64_t)n_candidates * s.n_coeffs;
    for (int b = 0; b < s.n_windows; ++b) {
        for (int64_t i = 0; i < per; ++i)
            if (!std::isfinite(coeffs[(int64_t)b * per + i])) { *where_b = b; *where_i = i; return CL_NONFINITE; }
        if (!std::isfinite(t_ref[b])) { *where_b = b; *where_i = -1; return CL_NONFINITE; }
    }
    return CL_OK;
}

inline int cl_code(ClFault f) {
    switch (f) {
        case CL_OK: return EINCM_OK;
        case CL_IN_FLIGHT: case CL_NOT_STAGED: case CL_NO_MODEL: return EINCM_ERR_STATE;
        case CL_SHARDED: return EINCM_ERR_UNSUPPORTED;
        default: return EINCM_ERR_ARG;
    }
}

inline const char* cl_why(ClFault f) {
    switch (f) {
        case CL_IN_FLIGHT: return "an evaluation is in flight";
        case CL_NULL_OUTPUTS: return "null pointer argument (sumsq and n_in both)";
        case CL_NOT_STAGED: return "called before eincm_set_windows";
        case CL_NO_MODEL: return "no motion model set (eincm_set_motion_model)";
        case CL_SHARDED: return "not supported on an event-sharded staging (EINCM_SW_DEFER_CONSTANTS)";
        case CL_RANGE: return "n_candidates must lie within 1 .. EINCM_CL_MAX_CANDIDATES and cell must be 1, 2, 4 or 8";
        case CL_NULL_INPUT: return "null pointer argument (coeffs or t_ref)";
        case CL_NONFINITE: return "coeffs and t_ref must be finite";
        default: return "";
    }
}

// The band plan.  The image of counts has Hc x Wc cells (Hc = ceil(H / cell), Wc = ceil(W / cell)), a uint32 each.  A band is `rows`
// consecutive cell rows by `cols` consecutive cell columns and belongs to one workgroup, whose LDS holds the table (if kept), the
// band's counts and the reduction's partials, CL_LDS_BYTES at the most.  Wherever a whole cell row fits, cols = Wc and a band is whole
// rows, as many as fit: the fewest bands, because every band's workgroup streams all of the window's events.  Only a sensor wider than
// the LDS (more than ~16000 cells in a row) is cut along its rows too, each row band then one cell row high.  Band i of the launch is
// row band i / n_col_bands, column band i % n_col_bands; every cell lies in exactly one band.
struct ClBands {
    int Hc, Wc;
    int rows, n_row_bands;     // cell rows per row band (the last may hold fewer), row bands
    int cols, n_col_bands;     // cell columns per column band (the last may hold fewer), column bands
    int table;                 // doubles of the coordinate table in LDS: W + H, or 0 where it is not kept
    int n_bands() const { return n_row_bands * n_col_bands; }
    int lds_bytes() const { return table * 8 + ((rows * cols + 1) & ~1) * 4 + CL_RED_BYTES; }   // (the partials are 8-byte aligned)
};

inline ClBands cl_bands(int H, int W, int cell) {
    ClBands p{};
    p.Hc = (H + cell - 1) / cell;
    p.Wc = (W + cell - 1) / cell;
    p.table = W + H <= CL_TABLE_MAX ? W + H : 0;
    const int words = (CL_LDS_BYTES - CL_RED_BYTES - p.table * 8) / 4;
    if (p.Wc <= words) {
        p.cols = p.Wc;
        p.rows = words / p.Wc < p.Hc ? words / p.Wc : p.Hc;
    } else {
        p.cols = words;
        p.rows = 1;
    }
    p.n_row_bands = (p.Hc + p.rows - 1) / p.rows;
    p.n_col_bands = (p.Wc + p.cols - 1) / p.cols;
    return p;
}

}   // namespace eincm
