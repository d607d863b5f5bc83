// eincm_motion.h — the host's rules of the parametric motion-field models: validation of a model, q = M c,
// the bound of |Theta| that picks the LDS capacities, the order in which the moment partials of k_motion_moments are added, and
// M^T mu; and of their fused evaluation inside the event kernels (section 21): the support predicate, which windows take part, the
// slots of the gather's moment partials and the order they are added in, the rule of 'auto'.  eincm_api.hip owns the memory, enqueues
// the kernels (eincm_motion.hip.h, eincm_kernels.hip.h) and words the refusals' codes.
//
// As eincm_plan.h: no HIP, no environment; plain C++17, so tests/host/motion_check.cpp runs all of it on the CPU under the sanitizers
// (tests/test_host_motion.py).  Every sum below is written out in the order the contract names, unfused, so that numpy reproduces it
// bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "eincm.h"
#include "eincm_types.h"

namespace eincm {

constexpr int MOTION_NQ = EINCM_MOTION_NQ;          // polynomial coefficients: q0..q5 of Theta_x, q6..q11 of Theta_y
constexpr int MOTION_NM = 6;                        // monomials 1, u, v, u u, u v, v v
constexpr int MOTION_MAX_K = EINCM_MOTION_MAX_COEFFS;
constexpr int MOTION_PARTS = 64;                    // workgroups (= partials) per window of k_motion_moments
constexpr int MOTION_ARG_WINDOWS = 64;              // windows whose q rides in k_motion_expand's arguments (6 KiB); more: pinned memory

struct MotionQArg { double q[MOTION_ARG_WINDOWS * MOTION_NQ]; };

// Null if the model can be used, else what is wrong with it.
inline const char* motion_model_error(const eincm_motion_model& m) {
    if (m.n_coeffs < 1 || m.n_coeffs > MOTION_MAX_K) return "n_coeffs outside 1 .. EINCM_MOTION_MAX_COEFFS";
    if (!std::isfinite(m.cx) || !std::isfinite(m.cy)) return "the centre (cx, cy) is not finite";
    if (!(m.scale > 0.0) || !std::isfinite(m.scale)) return "scale is not a positive finite number";
    for (int i = 0; i < MOTION_NQ * m.n_coeffs; ++i)
        if (!std::isfinite(m.M[i])) return "M holds a NaN or an infinity";
    return nullptr;
}

// q = M c of one window: q_j = (..((M_j0 c_0 + M_j1 c_1) + M_j2 c_2) ..), every product rounded
inline void motion_q(const eincm_motion_model& m, const double* c, double* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int K = m.n_coeffs;
    for (int j = 0; j < MOTION_NQ; ++j) {
        double s = m.M[j * K] * c[0];
        for (int k = 1; k < K; ++k) { const double t = m.M[j * K + k] * c[k]; s = s + t; }
        q[j] = s;
    }
}

// max |m_j| over the H x W sensor: [1, U, V, U U, U V, V V] with U = max |u|, V = max |v| (attained in a corner)
inline void motion_monomial_bounds(const eincm_motion_model& m, int H, int W, double* mm) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double U = std::fmax(std::fabs(0.0 - m.cx), std::fabs((double)(W - 1) - m.cx)) / m.scale;
    const double V = std::fmax(std::fabs(0.0 - m.cy), std::fabs((double)(H - 1) - m.cy)) / m.scale;
    mm[0] = 1.0; mm[1] = U; mm[2] = V; mm[3] = U * U; mm[4] = U * V; mm[5] = V * V;
}

// A bound of |Theta_x| and |Theta_y| of one window: the larger of sum_j |q_j| max|m_j| over the two components (left to right).
// A NaN among q makes it NaN: the caller then passes "unknown".
inline double motion_abs_bound(const double* q, const double* mm) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double b[2];
    for (int a = 0; a < 2; ++a) {
        double s = std::fabs(q[a * MOTION_NM]) * mm[0];
        for (int j = 1; j < MOTION_NM; ++j) { const double t = std::fabs(q[a * MOTION_NM + j]) * mm[j]; s = s + t; }
        b[a] = s;
    }
    return (b[0] != b[0] || b[1] != b[1]) ? NAN : (b[0] > b[1] ? b[0] : b[1]);
}

// mu = the MOTION_PARTS partials (P, 12) of one window added in index order
inline void motion_sum_partials(const double* parts, int P, double* mu) {
    for (int j = 0; j < MOTION_NQ; ++j) {
        double s = parts[j];
        for (int g = 1; g < P; ++g) s = s + parts[(size_t)g * MOTION_NQ + j];
        mu[j] = s;
    }
}

// grad = M^T mu: grad_k = (..((M_0k mu_0 + M_1k mu_1) + M_2k mu_2) ..), every product rounded
inline void motion_project(const eincm_motion_model& m, const double* mu, double* grad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int K = m.n_coeffs;
    for (int k = 0; k < K; ++k) {
        double s = m.M[k] * mu[0];
        for (int j = 1; j < MOTION_NQ; ++j) { const double t = m.M[j * K + k] * mu[j]; s = s + t; }
        grad[k] = s;
    }
}

// ---- the fused evaluation: the polynomial inside the event kernels, no Theta image ----

// What the support predicate reads of a context
struct MotionCtxState {
    bool fp64, model_set, staged, constants_pending, device_results, in_flight;
    int splat_size;                                 // eincm_set_splat_window's window_size
    bool weighted = false;                          // the staged batch carries per-event weights
};
struct MotionRefusal {
    int code;                                       // EINCM_OK: the fused path applies
    const char* why;
    explicit operator bool() const { return code != EINCM_OK; }
};
// Does eincm_loss_grad_motion_fused apply to this context and these parameters?  The first four refusals are eincm_loss_grad_motion's
// own; the others name what needs the Theta image during the evaluation (the TV term, the full aux) or has no polynomial mode (another
// splat window's kernels).
inline MotionRefusal motion_fused_supported(const MotionCtxState& s, const eincm_params* p) {
    if (s.fp64) return {EINCM_ERR_UNSUPPORTED, "not supported in fp64 mode (EINCM_CF_FP64): the device-resident evaluation does not exist there"};
    if (!s.model_set) return {EINCM_ERR_STATE, "no motion model set (eincm_set_motion_model)"};
    if (!s.staged) return {EINCM_ERR_STATE, "called before eincm_set_windows"};
    if (s.constants_pending) return {EINCM_ERR_STATE, "window constants pending (eincm_finish_constants)"};
    if (s.device_results) return {EINCM_ERR_STATE, "eincm_set_device_results is on (the split finishing half owns the results)"};
    if (s.in_flight) return {EINCM_ERR_STATE, "an evaluation is in flight"};
    if (s.splat_size != 3) return {EINCM_ERR_UNSUPPORTED, "the fused path has the 3x3 splat window only (eincm_set_splat_window): use eincm_loss_grad_motion"};
    if (p && (p->flags & EINCM_PF_FULL_AUX)) return {EINCM_ERR_UNSUPPORTED, "EINCM_PF_FULL_AUX needs the Theta image during the evaluation: use eincm_loss_grad_motion"};
    if (p && p->cur_pyr_lvl <= 0 && p->gamma != 0.0)
        return {EINCM_ERR_UNSUPPORTED, "the TV term (level 0, gamma != 0) needs the Theta image during the evaluation: use eincm_loss_grad_motion"};
    if (s.weighted) return {EINCM_ERR_UNSUPPORTED, "the fused path has no weighted form (the staged batch carries per-event weights): use eincm_loss_grad_motion"};
    return {EINCM_OK, nullptr};
}

// Which path 'auto' takes where the fused one applies.  The rule follows profiles/motion_fused.md (MI355X; the fused path against the
// parent commit's eincm_loss_grad_motion on the same coefficients; faster = the median below the parent's by more than the parent's
// own min-max range): the fused path was the faster one in every cell measured - 8 x [260x346, 10^6 events] by 5.6 us of 347,
// 1 x [480x640, 10^6 events] by 18 us of 154, 64 x [256x336, 3 10^4 events] by 184 us of 982 - so 'auto' takes it wherever it
// applies.  A regime found slower later gets its test here; engine.motion_auto_takes_fused states the same rule for Python.
// n_windows, n_events: the staged batch; n_refs: its reference times.
inline bool motion_auto_takes_fused(int n_windows, int64_t n_events, int n_refs) {
    (void)n_windows; (void)n_events; (void)n_refs;
    return true;
}

// A window takes part in the kernels of a fused evaluation only if its q and the bound of its field are finite; otherwise it sits the
// launch out like a masked window and its outputs are NaN.
inline bool motion_q_usable(const double* q, double bound) {
    for (int j = 0; j < MOTION_NQ; ++j) if (!std::isfinite(q[j])) return false;
    return std::isfinite(bound);
}

// First slot of every window's moment partials (B + 1 entries): the gather's list holds the segments of the bins (window, tile) in bin
// order, a bin of n events cut at `seg` into ceil(n / balanced_seg_len(n, seg)) segments (cut_segments, k_items); a segment is one
// slot (all_r) or R of them.  Returns the segments in all.
inline int64_t motion_slot_offsets(const int32_t* tilecount, int B, int ntiles, int seg, int slots_per_segment, int64_t* win_slot0) {
    int64_t n = 0;
    for (int b = 0; b < B; ++b) {
        win_slot0[b] = n * slots_per_segment;
        for (int k = 0; k < ntiles; ++k) {
            const int cnt = tilecount[(size_t)b * ntiles + k];
            if (cnt <= 0) continue;
            const int len = balanced_seg_len(cnt, seg);
            const int nseg = (cnt + len - 1) / len;
            n += nseg;
        }
    }
    win_slot0[B] = n * slots_per_segment;
    return n;
}

// mu = a window's n moment partials (n, 12) added in index order; zero for a window without a segment.  One pass over the slots with
// the twelve chains side by side: every chain still adds its partials in index order, so the bits are those of twelve separate loops.
inline void motion_sum_slots(const double* parts, int64_t n, double* mu) {
    for (int j = 0; j < MOTION_NQ; ++j) mu[j] = n > 0 ? parts[j] : 0.0;
    for (int64_t g = 1; g < n; ++g)
        for (int j = 0; j < MOTION_NQ; ++j) mu[j] = mu[j] + parts[(size_t)g * MOTION_NQ + j];
}

}  // namespace eincm
