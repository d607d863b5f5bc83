// eincm_event_support.h — the rules of the event-support filter that need no GPU: the argument checks, the
// per-event refusals and their first offender, the neighbour window clipped to the sensor, the carried-time rule, the weight, and
// the geometry of the sort by pixel.  The kernels of eincm_event_support.hip.h run the EINCM_HD functions below per event;
// eincm_api.hip runs the argument checks and launches the sort from es_sort_plan.
//
// As eincm_plan.h: no HIP, no environment.  Plain C++17, so tests/host/event_support_check.cpp runs all of it on the CPU under the
// sanitizers (tests/test_host_event_support.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "eincm_types.h"

namespace eincm {

constexpr int ES_MAX_RADIUS = 3;
constexpr int64_t ES_MAX_N = (int64_t)1 << 30;

// What a call refuses before it looks at an event (the order of the checks is the order of the enum)
enum EsArgFault { ES_ARG_OK = 0, ES_ARG_N, ES_ARG_TAU, ES_ARG_RADIUS, ES_ARG_FULL_SUPPORT };

inline int es_max_support(int radius) { return (2 * radius + 1) * (2 * radius + 1) - 1; }

inline EsArgFault es_check_args(int64_t n, double tau, int radius, int full_support) {
    if (n < 0 || n > ES_MAX_N) return ES_ARG_N;
    if (!std::isfinite(tau) || tau < 0.0) return ES_ARG_TAU;
    if (radius < 1 || radius > ES_MAX_RADIUS) return ES_ARG_RADIUS;
    if (full_support < 1 || full_support > es_max_support(radius)) return ES_ARG_FULL_SUPPORT;
    return ES_ARG_OK;
}

// What an event is refused for; an event with several faults reports the first of this order
enum EsEventFault { ES_EV_OK = 0, ES_EV_COORD = 1, ES_EV_TIME = 2, ES_EV_ORDER = 3 };

// Event (x, y, t) after an event of time t_prev (the carried last time for the first event of a chunk; -inf: nothing before it).
// t - t == 0 is false for NaN and for +-inf.  A non-finite t_prev belongs to the predecessor's own refusal and orders nothing.
EINCM_HD int es_event_fault(int H, int W, int x, int y, double t, double t_prev) {
    if (x < 0 || x >= W || y < 0 || y >= H) return ES_EV_COORD;
    if (!(t - t == 0.0)) return ES_EV_TIME;
    if (t < t_prev) return ES_EV_ORDER;
    return ES_EV_OK;
}

struct EsRefusal {
    int64_t index = -1;            // the first offender; -1: none
    int fault = ES_EV_OK;
    explicit operator bool() const { return index >= 0; }
};

// The first event of a chunk that is refused, as the validation kernel reports it (the smallest index over all faults)
inline EsRefusal es_first_offender(int H, int W, const int16_t* x, const int16_t* y, const double* t, int64_t n, double carried_last_t) {
    double prev = carried_last_t;
    for (int64_t e = 0; e < n; ++e) {
        const int f = es_event_fault(H, W, x[e], y[e], t[e], prev);
        if (f) { EsRefusal r; r.index = e; r.fault = f; return r; }
        prev = t[e];
    }
    return EsRefusal{};
}

// The neighbour window of pixel (x, y): Chebyshev distance <= r, clipped to the sensor; both bounds inclusive.  (The pixel itself
// lies inside and is skipped by the caller.)
struct EsWindow { int x0, x1, y0, y1; };
EINCM_HD EsWindow es_window(int H, int W, int x, int y, int r) {
    EsWindow w;
    w.x0 = x - r < 0 ? 0 : x - r;
    w.x1 = x + r > W - 1 ? W - 1 : x + r;
    w.y0 = y - r < 0 ? 0 : y - r;
    w.y1 = y + r > H - 1 ? H - 1 : y + r;
    return w;
}

// "No event": the value the carried map holds for a pixel that has not fired
EINCM_HD double es_no_event() { return -std::numeric_limits<double>::infinity(); }

// The carried-time rule: a neighbour's most recent event before e is its last one in the current chunk where it has one, else what
// the carried map holds for it
EINCM_HD double es_prev_time(bool in_chunk, double t_chunk, double t_map) { return in_chunk ? t_chunk : t_map; }

// One double subtraction, one compare.  t_prev = -inf gives +inf <= tau: false.
EINCM_HD bool es_supported(double t_e, double t_prev, double tau) { return t_e - t_prev <= tau; }

// One float32 division
EINCM_HD float es_weight(int support, int full_support) {
    return (float)(support < full_support ? support : full_support) / (float)full_support;
}

// ---- the geometry of the sort by pixel (the kernels: eincm_event_support.hip.h) ----
constexpr int ES_RADIX_BITS = 8;
constexpr int ES_RADIX = 1 << ES_RADIX_BITS;       // 256 digits: 4 per lane
constexpr int ES_SORT_BLOCK = 1024;                // events per wave of the sort: 16 trips of 64
constexpr int ES_SCAN_NT = 1024;
constexpr int ES_SCAN_TILE = ES_SCAN_NT * 4;       // histogram entries per workgroup of the tile scan

// Passes of ES_RADIX_BITS bits that cover every pixel key below npix
inline int es_sort_passes(int64_t npix) {
    int bits = 1;
    while (((int64_t)1 << bits) < npix) ++bits;
    return (bits + ES_RADIX_BITS - 1) / ES_RADIX_BITS;
}

// What the host launches the sort of n events (0 <= n <= ES_MAX_N) over npix pixels with: nblk waves of ES_SORT_BLOCK events, the
// digit-major histogram of nhist = ES_RADIX nblk entries (at most 2^28: an int, and every entry and every sum of entries counts
// events, so stays <= 2^30 in a uint32_t), its ntiles tiles of ES_SCAN_TILE entries, and the passes.
struct EsSortPlan { int nblk; int64_t nhist, ntiles; int passes; };
inline EsSortPlan es_sort_plan(int64_t n, int64_t npix) {
    EsSortPlan p;
    p.nblk = (int)((n + ES_SORT_BLOCK - 1) / ES_SORT_BLOCK);
    p.nhist = (int64_t)ES_RADIX * p.nblk;
    p.ntiles = (p.nhist + ES_SCAN_TILE - 1) / ES_SCAN_TILE;
    p.passes = es_sort_passes(npix);
    return p;
}

}   // namespace eincm
