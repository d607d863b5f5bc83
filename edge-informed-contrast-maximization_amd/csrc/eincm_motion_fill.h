// eincm_motion_fill.h — the rules of the dense composition of a motion segmentation (eincm_densify_motions) that
// need no GPU: what a call refuses, in which order, where a group's block of every output lies, and the exact Euclidean feature
// transform - which labelled pixel is nearest, not only how far - as plain functions: the packed column record, the 64-bit key whose
// unsigned minimum is the tie rule, one step of either column sweep, and the row search.  eincm_api.hip runs the check; the kernels
// (eincm_motion_fill.hip.h) call the same functions, so host and device cannot drift apart; engine.py restates the layout
// (densify_motions_layout) and tests/test_host_motion_fill.py compares the two through tests/host/motion_fill_check.cpp.
//
// The rule: the nearest site of pixel (x, y) is the site (x', y') with the smallest key (d2, y', x') in lexicographic order,
// d2 = (x - x')^2 + (y - y')^2.  The separable form is exact under it.  Fix a column x': over that column's sites (x - x')^2 is a
// constant, so the smallest (d2, y') there is the site of the smallest |y - y'|, the upper one of an up/down pair at equal distance -
// what the two sweeps leave in the column record.  Every site lies in one column, so the smallest key over all sites is the smallest
// over x' of the column keys (d2, y', x'), and the unsigned order of d2 << 32 | y' << 16 | x' is that lexicographic order.
//
// As eincm_motion_layers.h: no HIP, no environment.  Plain C++17, so the checker runs all of it on the CPU under the sanitizers.
#pragma once
#include <cstdint>

#include "eincm.h"
#include "eincm_motion_layers.h"
#include "eincm_types.h"

namespace eincm {

constexpr int MF_MAX_W = 16384;                     // the row kernel keeps one row of column records in LDS: 4 * 16384 = 64 KiB
constexpr uint32_t MF_REC_NONE = 0xFFFFFFFFu;       // a column record: no site in this column (distance 0xFFFF, y' = -1)
constexpr uint64_t MF_KEY_NONE = ~0ull;             // a key: no candidate; above every key of a site (d2 < 2^31)

// The faults of ml_check keep their numbers, order, codes and sentences (ML_NULL_OUTPUTS: all five outputs here); the new ones follow
enum MfFault { MF_OK = 0, MF_SITE_MASS = ML_CROWDED + 1, MF_WIDE };

// s.has_outputs: any of theta, labels, dist2, nearest, n_sites.  W: the sensor's width.  Returns an MlFault or an MfFault.
inline int mf_check(const MlState& s, int W, int n_models, const double* coeffs, unsigned flags, uint32_t min_site_mass, int* where_b,
                    int64_t* where_i) {
    if (const MlFault f = ml_check(s, n_models, coeffs, flags, where_b, where_i)) return (int)f;
    if (min_site_mass == 0u) return MF_SITE_MASS;
    if (W > MF_MAX_W) return MF_WIDE;
    return MF_OK;
}

inline int mf_code(int f) {
    switch (f) {
        case MF_SITE_MASS: return EINCM_ERR_ARG;
        case MF_WIDE: return EINCM_ERR_UNSUPPORTED;
        default: return ml_code((MlFault)f);
    }
}

inline const char* mf_why(int f) {
    switch (f) {
        case ML_NULL_OUTPUTS: return "null pointer argument (theta, labels, dist2, nearest and n_sites all)";
        case MF_SITE_MASS: return "min_site_mass must be at least 1";
        case MF_WIDE: return "a sensor wider than 16384 pixels is not supported (the row search keeps one row in LDS)";
        default: return ml_why((MlFault)f);
    }
}

// The layout, in elements of each output's own type: a group's block after the previous group's, row-major inside.
//   theta (G, H, W, 2) double | labels (G, H, W) uint8 | dist2 (G, H, W) uint32 | nearest (G, H, W) int32 | n_sites (G) uint32
inline int64_t mf_theta_offset(int g, int H, int W) { return ml_theta_offset(g, H, W); }
inline int64_t mf_labels_offset(int g, int H, int W) { return ml_labels_offset(g, H, W); }
inline int64_t mf_dist2_offset(int g, int H, int W) { return (int64_t)g * H * W; }
inline int64_t mf_nearest_offset(int g, int H, int W) { return (int64_t)g * H * W; }
inline int64_t mf_nsites_offset(int g) { return g; }

// ---- the feature transform: the kernels run these very functions ----

// S >= min_site_mass, S the uint64 sum of the pixel's K masses (mass[l * stride])
EINCM_HD bool mf_is_site(const uint32_t* mass, int n_models, int64_t stride, uint32_t min_site_mass) {
    uint64_t S = 0;
    for (int l = 0; l < n_models; ++l) S += mass[(int64_t)l * stride];
    return S >= (uint64_t)min_site_mass;
}

// The column record of a pixel: the vertical distance to the nearest site of its column in the low half (0 .. 32767: sensor sides are
// below 32768), that site's row y' in the high half
EINCM_HD uint32_t mf_pack(int dist, int y) { return (uint32_t)dist | ((uint32_t)y << 16); }
EINCM_HD int mf_rec_dist(uint32_t rec) { return (int)(rec & 0xFFFFu); }
EINCM_HD int mf_rec_y(uint32_t rec) { return (int)(rec >> 16); }

// One step of the downward sweep, rows 0 .. H - 1: `above` is the row of the nearest site at or above row y (-1 before the first one;
// the caller starts it at -1).  Returns the record of (column, y) as far as the rows above know.
EINCM_HD uint32_t mf_col_down(bool site, int y, int& above) {
    if (site) above = y;
    return above >= 0 ? mf_pack(y - above, above) : MF_REC_NONE;
}

// One step of the upward sweep, rows H - 1 .. 0: `down` is what the downward sweep left at (column, y), `below` the row of the nearest
// site at or below row y (-1 before the first one).  A site below wins only if it is strictly nearer: a tie keeps the upper one.
EINCM_HD uint32_t mf_col_up(uint32_t down, int y, int& below) {
    if (down != MF_REC_NONE && mf_rec_dist(down) == 0) below = y;
    if (below < 0) return down;
    if (down == MF_REC_NONE || below - y < mf_rec_dist(down)) return mf_pack(below - y, below);
    return down;
}

// The key of column xs's record as seen from a pixel dx columns away
EINCM_HD uint64_t mf_key(uint32_t rec, uint32_t dx, int xs) {
    if (rec == MF_REC_NONE) return MF_KEY_NONE;
    const uint32_t d = (uint32_t)mf_rec_dist(rec);
    return ((uint64_t)(d * d + dx * dx) << 32) | ((uint64_t)mf_rec_y(rec) << 16) | (uint64_t)xs;
}

// One step of the row search at distance k >= 1 from x: the better of `best` and the candidates k columns to the left and to the right
EINCM_HD uint64_t mf_row_step(const uint32_t* row, int W, int x, uint32_t k, uint64_t best) {
    const int xl = x - (int)k, xr = x + (int)k;
    if (xl >= 0) { const uint64_t c = mf_key(row[xl], k, xl); best = c < best ? c : best; }
    if (xr < W) { const uint64_t c = mf_key(row[xr], k, xr); best = c < best ? c : best; }
    return best;
}

// The smallest key over the row's W records as seen from column x.  The search goes on while k^2 <= the best d2: a candidate at an
// equal d2 may still win on (y', x'), so the bound of a plain distance transform, k^2 < best, stops one step early.  Without a
// candidate yet the best d2 reads 2^32 - 1 > k^2 (k < 2^14), and the search ends with the row.
EINCM_HD uint64_t mf_row_search(const uint32_t* row, int W, int x) {
    uint64_t best = mf_key(row[x], 0u, x);
    for (uint32_t k = 1; (uint64_t)k * k <= (best >> 32); ++k) {
        if (x - (int)k < 0 && x + (int)k >= W) break;
        best = mf_row_step(row, W, x, k, best);
    }
    return best;
}

EINCM_HD uint32_t mf_key_dist2(uint64_t key) { return key == MF_KEY_NONE ? EINCM_MD_NONE : (uint32_t)(key >> 32); }
EINCM_HD int32_t mf_key_nearest(uint64_t key, int W) {
    return key == MF_KEY_NONE ? -1 : (int32_t)((key >> 16) & 0xFFFFu) * W + (int32_t)(key & 0xFFFFu);
}

// p is reached: it has a nearest site no farther than max_dist2 (EINCM_MD_UNBOUNDED: any distance)
EINCM_HD bool mf_reached(int32_t nearest, uint32_t dist2, uint32_t max_dist2) { return nearest >= 0 && dist2 <= max_dist2; }

}   // namespace eincm
