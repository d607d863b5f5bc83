// eincm_event_scores.hip.h — k_event_scores: the adjoint of the splat applied to an image stack.  For every
// staged event e of window b and every reference time r
//     s[r, e]    = sum over the nine taps d of  k_{e,r}(d) * F_{b,r}[ wrap_drop(round(x'_{e,r}) + d) ]
//     self[r, e] = sum over the undropped taps of  k_{e,r}(d)^2
// with the evaluation's warp (warp_axis), the splat's tap weights (taps3x2 at scale 1/(2 pi)) and the splat's index rule (wrap_drop
// after clamp_far), all three reused unchanged from eincm_kernels.hip.h: the rounded coordinate has the evaluation's bits by
// construction.  Not on the evaluation path; the rules that need no GPU are in eincm_event_scores.h.
//
// Arithmetic: fp32 after the fp64 warp.  k(d) = ky[dy] * kx[dx], one rounded product.  The taps are summed in ONE order, rows dy = -1,
// 0, +1 and within a row dx = -1, 0, +1, each by one fused multiply-add onto the running sum (s = fma(k, F, s), self = fma(k, k, self)),
// both sums starting at +0; a dropped tap is skipped.  The combined form adds (float)omega_r * s[r, e] (product rounded, then the add)
// in ascending r.  One thread owns an output cell from first to last operation: no atomics, no reduction across threads, the same
// bytes on every run.  An event whose taps are all dropped scores +0 exactly.
#pragma once
#include "eincm_kernels.hip.h"

namespace eincm {

// One (event, reference time) cell: the warp, the nine tap weights and the two sums s and self in the order stated above, both from +0.
// F is the image of that (window, r).  Shared by k_event_scores and k_responsibilities (eincm_responsibilities.hip.h), so that both
// have the same operations in the same order: the same bits.
__device__ __forceinline__ void sc_event_ref(const Geom& g, int x, int y, double2 v, double dt, const float* __restrict__ F, float& s_out,
                                             float& q_out)
{
#pragma clang fp contract(off)
    int irx, iry; float fx, fy;
    warp_axis(x, v.x, dt, irx, fx);
    warp_axis(y, v.y, dt, iry, fy);
    f2v km, k0, kp;                                  // .x = x-axis weight, .y = y-axis weight (carries the 1/(2 pi))
    taps3x2(fx, fy, INV_2PI, km, k0, kp);
    const float kx[3] = {km.x, k0.x, kp.x}, ky[3] = {km.y, k0.y, kp.y};
    const int sx = clamp_far(irx), sy = clamp_far(iry);
    float s = 0.0f, q = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int gy = wrap_drop(sy - 1 + dy, g.H);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int gx = wrap_drop(sx - 1 + dx, g.W);
            if (gx >= 0 && gy >= 0) {
                const float k = ky[dy] * kx[dx];
                s = fmaf(k, F[(size_t)gy * g.W + gx], s);
                q = fmaf(k, k, q);
            }
        }
    }
    s_out = s; q_out = q;
}

// One thread per event, the Theta pair loaded once (as k_warp_events), a loop over the reference times in the thread.  grid
// (ceil(max_b n_b / NT), B): blockIdx.y is the window.  (One grid row per reference time, so that a workgroup stays inside one image,
// was measured and not kept: 2 to 7 % slower on every batch of profiles/event_scores.md; the combined output
// needs the loop anyway, its sum over r stays in one thread.)
//   evoff (B + 1): the windows' event offsets in the raw arrays.  images (B, R, H, W).  rw: (R) floats, or nullptr for the
//   per-reference form.  scores / selfs: window b's block starts at evoff[b] * (rw ? 1 : R) (sc_block_offset); selfs may be nullptr.
__global__ __launch_bounds__(NT) void k_event_scores(Geom g, const int64_t* __restrict__ evoff, const int16_t* __restrict__ xs,
                                                      const int16_t* __restrict__ ys, const double* __restrict__ ts,
                                                      const double* __restrict__ Theta, const double* __restrict__ edge_ts,
                                                      const float* __restrict__ images, const float* __restrict__ rw,
                                                      float* __restrict__ scores, float* __restrict__ selfs)
{
#pragma clang fp contract(off)
    const int win = blockIdx.y;
    const int64_t e0 = evoff[win], n = evoff[win + 1] - e0;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int x = xs[e0 + i], y = ys[e0 + i];
    const double t = ts[e0 + i];
    const size_t npix = (size_t)g.H * g.W;
    const double2 v = *reinterpret_cast<const double2*>(Theta + ((size_t)win * npix + (size_t)y * g.W + x) * 2);
    const int64_t base = e0 * (rw ? 1 : g.R);
    float S = 0.0f, Q = 0.0f;                        // the combined form's sums over r
    for (int r = 0; r < g.R; ++r) {
        float s, q;
        sc_event_ref(g, x, y, v, t - edge_ts[win * g.R + r], images + ((size_t)win * g.R + r) * npix, s, q);
        if (rw) {
            const float w = rw[r];
            S = S + w * s;
            Q = Q + w * q;
        } else {
            scores[base + (int64_t)r * n + i] = s;
            if (selfs) selfs[base + (int64_t)r * n + i] = q;
        }
    }
    if (rw) {
        scores[base + i] = S;
        if (selfs) selfs[base + i] = Q;
    }
}

}   // namespace eincm
