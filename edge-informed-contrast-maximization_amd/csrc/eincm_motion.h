// eincm_motion.h — the host's rules of the parametric motion-field models: validation of a model, q = M c,
// the bound of |Theta| that picks the LDS capacities, the order in which the moment partials of k_motion_moments are added, and
// M^T mu.  eincm_api.hip owns the memory, enqueues the kernels (eincm_motion.hip.h) and words the refusals' codes.
//
// As eincm_plan.h: no HIP, no environment; plain C++17, so tests/host/motion_check.cpp runs all of it on the CPU under the sanitizers
// (tests/test_host_motion.py).  Every sum below is written out in the order the contract names, unfused, so that numpy reproduces it
// bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "eincm.h"

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

}  // namespace eincm
