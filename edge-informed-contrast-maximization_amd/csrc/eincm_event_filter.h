// eincm_event_filter.h — the rules of the refractory and polarity-aware event filter that need no GPU: the
// argument checks, the polarity class, the refractory rule, which carried time a neighbour is asked for, and the weight.  Everything
// the event-support filter already states (the per-event refusals, the neighbour window, the support compare, "no event") is
// eincm_event_support.h's and is called from there.  The kernels of eincm_event_filter.hip.h run the EINCM_HD functions below per
// event; eincm_api.hip runs the argument checks.
//
// As eincm_event_support.h: no HIP, no environment.  Plain C++17, so tests/host/event_filter_check.cpp runs all of it on the CPU under
// the sanitizers (tests/test_host_event_filter.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "eincm_event_support.h"

namespace eincm {

constexpr int EF_POLARITY = 1;             // EINCM_EF_POLARITY (include/eincm.h)
constexpr int EF_KNOWN_FLAGS = EF_POLARITY;

// What a call refuses before it looks at an event (the order of the checks is the order of the enum)
enum EfArgFault { EF_ARG_OK = 0, EF_ARG_N, EF_ARG_REFRACTORY, EF_ARG_TAU, EF_ARG_RADIUS, EF_ARG_FULL_SUPPORT, EF_ARG_FLAGS };

// radius 0 switches the support stage off: nothing to count, so full_support has one meaningful value.  has_p: a polarity array was
// handed over (the polarity flag without one is a flags fault).
inline EfArgFault ef_check_args(int64_t n, double refractory, double tau, int radius, int full_support, int flags, bool has_p) {
    if (n < 0 || n > ES_MAX_N) return EF_ARG_N;
    if (!std::isfinite(refractory) || refractory < 0.0) return EF_ARG_REFRACTORY;
    if (!std::isfinite(tau) || tau < 0.0) return EF_ARG_TAU;
    if (radius < 0 || radius > ES_MAX_RADIUS) return EF_ARG_RADIUS;
    if (full_support < 1 || full_support > (radius == 0 ? 1 : es_max_support(radius))) return EF_ARG_FULL_SUPPORT;
    if ((flags & ~EF_KNOWN_FLAGS) || ((flags & EF_POLARITY) && !has_p)) return EF_ARG_FLAGS;
    return EF_ARG_OK;
}

// The polarity class: {0, 1} and {-1, +1} recordings alike
EINCM_HD int ef_class(int p) { return p > 0 ? 1 : 0; }

// The refractory rule: one double subtraction, one compare.  prev_any is the time of the pixel's previous event, kept or not (-inf:
// none, which gives +inf < rho: false).  rho = 0 keeps every unmasked event; t - prev_any == rho keeps.
EINCM_HD bool ef_kept(double t, double prev_any, double rho, bool masked) { return !masked && !(t - prev_any < rho); }

// The time of a neighbour's last kept event that supports class cls: its own class's with the polarity flag, the later of the two
// without (an exact max: no rounding)
EINCM_HD double ef_last_kept(double l0, double l1, int cls, bool polarity) { return polarity ? (cls ? l1 : l0) : (l0 > l1 ? l0 : l1); }

// One float32 division (es_weight) for a kept event with the support stage on; kept -> 1 with it off; a dropped event weighs nothing
EINCM_HD float ef_weight(bool kept, int support, int radius, int full_support) {
    if (!kept) return 0.0f;
    return radius == 0 ? 1.0f : es_weight(support, full_support);
}

}   // namespace eincm
