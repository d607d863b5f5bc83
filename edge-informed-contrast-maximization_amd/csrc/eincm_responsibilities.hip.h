// eincm_responsibilities.hip.h — k_responsibilities and k_rs_mass: the E-step of a segmentation into K motions.
// The staged batch is G groups of K consecutive windows; window g*K + l is model l of group g, and event i of every window of a group
// is one event seen under K motions.  For that event
//     s_l, q_l = the combined score and self of k_event_scores for window g*K + l (sc_event_ref, the same operations in the same order)
//     a_l = s_l - w_l * q_l   (EINCM_RS_EXCLUDE_SELF; else s_l),   a_l = a_l > 0 ? a_l : +0   (a NaN becomes +0)
//     p_l = pi_l * a_l,   T = ((0 + p_0) + p_1) + ...
//     T not > 0 or not finite: the event is unsupported, p_l = pi_l and T is summed again
//     w'_l = p_l / T,   label = the lowest l with the largest p_l
// all in fp32 with contraction off, every operation rounded once.  The division is the plain `/`: without fast-math flags the compiler
// emits the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence for it, and the build must stay that way (no -ffast-math,
// no __fdividef, no reciprocal).  The rules that need no GPU are in eincm_responsibilities.h.
//
// mass[b] = sum_i w' in fp64 in one fixed order and without atomics: a wave adds its 64 values by halving (lane j += lane j + 32, 16,
// ... 1), a block adds its four waves in ascending order (k_responsibilities, one partial per window and block), and k_rs_mass adds
// a window's partials in ascending block order from +0.  The unsupported events are counted by an integer atomic per wave: exact.
#pragma once
#include "eincm_event_scores.hip.h"

namespace eincm {

// (the one argument of k_responsibilities' pack)
__device__ inline const float* rs_prior_stack(const float* prior_img) { return prior_img; }

// One thread per event of a group, a loop over the models and over the reference times in the thread; p_l stays in registers (the
// model loop is unrolled over the template's K, so p[] is never indexed at run time: no scratch).  grid (ceil(max_g n_g / NT), G):
// blockIdx.y is the group; a block beyond its group's events leaves at once, as one.
//   evoff (B + 1) as k_event_scores; the windows of a group have equal counts, so window g*K + l starts at evoff[g*K] + l * n_g and
//   the group's labels at evoff[g*K] / K.  rw (R) floats.  w_in: the batch's weights in the layout of wout, or nullptr for ones;
//   w_has (B): 0 where a window's weights are ones.  pi (B) floats.  wout, labels, part (B, gridDim.x), uns (G, zeroed): any may be
//   nullptr.
// SP = 1 is the E-step with a prior image: one more argument, prior_img (B, H, W) floats, and
//     c_l = pi_l * prior_img[g*K + l, y_e, x_e],   p_l = c_l * a_l
//     unsupported: p_l = c_l and T is summed again; if that T is not > 0 or not finite either, p_l = pi_l and T is summed once more
// with the event's raw pixel, the xs / ys read for the warp.  The event counts as unsupported once.  SP = 0 takes no such argument
// (the pack is empty) and compiles to the instructions it had before SP existed (profiles/label_prior.md).
template <int K, int SP = 0, typename... PriorImg>
__global__ __launch_bounds__(NT) void k_responsibilities(Geom g, const int64_t* __restrict__ evoff, const int16_t* __restrict__ xs,
                                                          const int16_t* __restrict__ ys, const double* __restrict__ ts,
                                                          const double* __restrict__ Theta, const double* __restrict__ edge_ts,
                                                          const float* __restrict__ images, const float* __restrict__ rw,
                                                          const float* __restrict__ w_in, const uint8_t* __restrict__ w_has,
                                                          const float* __restrict__ pi, uint32_t flags, float* __restrict__ wout,
                                                          uint8_t* __restrict__ labels, double* __restrict__ part,
                                                          unsigned long long* __restrict__ uns, PriorImg... prior_img)
{
#pragma clang fp contract(off)
    static_assert(sizeof...(PriorImg) == (SP ? 1 : 0), "SP = 1 takes the prior stack, SP = 0 nothing");
    __shared__ double sm[K][NT / 64];
    const int grp = blockIdx.y, w0 = grp * K;
    const int64_t e0 = evoff[w0], n = evoff[w0 + 1] - e0;
    if ((int64_t)blockIdx.x * NT >= n) return;       // (the whole block: nobody waits at the barrier below)
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    const bool live = i < n;
    const size_t npix = (size_t)g.H * g.W;
    float p[K];
    [[maybe_unused]] float c[SP ? K : 1];            // SP: c_l, the first fallback's shares
    bool unsupported = false;
    if (live) {
#pragma unroll
        for (int l = 0; l < K; ++l) {
            const int win = w0 + l;
            const int64_t e = e0 + (int64_t)l * n + i;
            const int x = xs[e], y = ys[e];
            const double t = ts[e];
            const double2 v = *reinterpret_cast<const double2*>(Theta + ((size_t)win * npix + (size_t)y * g.W + x) * 2);
            float S = 0.0f, Q = 0.0f;
            for (int r = 0; r < g.R; ++r) {
                float s, q;
                sc_event_ref(g, x, y, v, t - edge_ts[win * g.R + r], images + ((size_t)win * g.R + r) * npix, s, q);
                const float w = rw[r];
                S = S + w * s;
                Q = Q + w * q;
            }
            float a = S;
            if (flags & EINCM_RS_EXCLUDE_SELF) {
                const float w = (w_in && w_has[win]) ? w_in[e] : 1.0f;
                a = S - w * Q;
            }
            a = a > 0.0f ? a : 0.0f;
            if constexpr (SP) {
                c[l] = pi[win] * rs_prior_stack(prior_img...)[(size_t)win * npix + (size_t)y * g.W + x];
                p[l] = c[l] * a;
            } else {
                p[l] = pi[win] * a;
            }
        }
        float T = 0.0f;
#pragma unroll
        for (int l = 0; l < K; ++l) T = T + p[l];
        if (!(T > 0.0f) || !(fabsf(T) <= 3.402823466e38f)) {
            unsupported = true;
            T = 0.0f;
            if constexpr (SP) {
#pragma unroll
                for (int l = 0; l < K; ++l) { p[l] = c[l]; T = T + p[l]; }
                if (!(T > 0.0f) || !(fabsf(T) <= 3.402823466e38f)) {
                    T = 0.0f;
#pragma unroll
                    for (int l = 0; l < K; ++l) { p[l] = pi[w0 + l]; T = T + p[l]; }
                }
            } else {
#pragma unroll
                for (int l = 0; l < K; ++l) { p[l] = pi[w0 + l]; T = T + p[l]; }
            }
        }
        int lab = 0; float best = p[0];
#pragma unroll
        for (int l = 1; l < K; ++l)
            if (p[l] > best) { best = p[l]; lab = l; }
#pragma unroll
        for (int l = 0; l < K; ++l) {
            p[l] = p[l] / T;
            if (wout) wout[e0 + (int64_t)l * n + i] = p[l];
        }
        if (labels) labels[e0 / K + i] = (uint8_t)lab;
    } else {
#pragma unroll
        for (int l = 0; l < K; ++l) p[l] = 0.0f;
    }
    if (uns) {
        const unsigned long long m = __ballot(unsupported);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(uns + grp, (unsigned long long)__popcll(m));
    }
    if (part) {
#pragma unroll
        for (int l = 0; l < K; ++l) {
            double d = (double)p[l];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) d = d + __shfl_down(d, off, 64);
            if ((threadIdx.x & 63) == 0) sm[l][threadIdx.x >> 6] = d;
        }
        __syncthreads();
        if (threadIdx.x < K) {
            double d = sm[threadIdx.x][0];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) d = d + sm[threadIdx.x][w];
            part[(size_t)(w0 + threadIdx.x) * gridDim.x + blockIdx.x] = d;
        }
    }
}

// k_responsibilities<K> for a call's K (1 .. EINCM_RS_MAX_MODELS, checked by rs_check before)
template <int K = 1> static auto rs_kernel(int n_models) -> decltype(&k_responsibilities<1>) {
    if constexpr (K < EINCM_RS_MAX_MODELS) { if (n_models != K) return rs_kernel<K + 1>(n_models); }
    return k_responsibilities<K>;
}
template <int K = 1> static auto rs_spatial_kernel(int n_models) -> decltype(&k_responsibilities<1, 1, const float*>) {
    if constexpr (K < EINCM_RS_MAX_MODELS) { if (n_models != K) return rs_spatial_kernel<K + 1>(n_models); }
    return k_responsibilities<K, 1, const float*>;
}

// mass[b] = a window's block partials added in ascending block order from +0.  One thread per window; n_part is the row length of
// part (the grid x of k_responsibilities), of which window b wrote its first ceil(n_b / NT).
__global__ __launch_bounds__(NT) void k_rs_mass(int B, const int64_t* __restrict__ evoff, const double* __restrict__ part, int64_t n_part,
                                                double* __restrict__ mass)
{
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= B) return;
    const int64_t nb = (evoff[b + 1] - evoff[b] + NT - 1) / NT;
    double d = 0.0;
    for (int64_t j = 0; j < nb; ++j) d = d + part[(size_t)b * n_part + j];
    mass[b] = d;
}

}   // namespace eincm
