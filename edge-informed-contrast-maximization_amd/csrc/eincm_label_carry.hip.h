// eincm_label_carry.hip.h — k_lc_splat and k_lc_resolve: a segmentation's per-model mass images carried along each model's own motion
// field to the next window (eincm_carry_label_prior).  k_ml_mass (eincm_motion_layers.hip.h) has left M
// (G, K, H, W), every model's quantised staged weights summed per pixel; k_label_prior (eincm_label_prior.hip.h) runs unchanged on what
// these two kernels leave.  The rules that need no GPU - the refusals, the scale with its overflow proof, lc_resolve, the layout - are
// in eincm_label_carry.h; the landing and the tap weights are eincm_theta_advect.h's.
//
//   k_lc_splat    grid (pixel blocks, G K), one thread per SOURCE pixel p of one (group, model): where M_l(p) > 0 it forms the model's
//                 field f_l(p) (motion_monomials / motion_poly: the bits of k_ml_compose's hard mode and of eincm_motion_field), lands
//                 it at q = p + f_l(p) tau (ta_landing) and adds M_l(p) w to the u64 plane A_l at the up to four pixels around q,
//                 w = ta_weight.  Taps outside the sensor, and the whole M_l(p) 2^20 of a source ta_landing rejects, go to the
//                 (group, model)'s `dropped` instead: one wave reduction by shuffles, one LDS word per wave, one atomic per workgroup.
//   k_lc_resolve  one thread per cell: C = lc_resolve(A).
// Every sum is an integer one (64-bit atomics on A and on dropped: the sums do not depend on the order of arrival, and
// eincm_label_carry.h proves that no accepted input overflows them), so every run leaves the same bytes.
//
// Atomics: as k_ta_splat's (the HIP guide's Guideline 12 and scatter-add appendix), a smooth field moves neighbouring sources to
// neighbouring pixels, so a wave's adds fall in a few rows of one plane.  Only pixels with mass add at all - about one in four at the
// reference's window sizes - and one plane takes 4 taps x 8 B per such source.  profiles/label_carry.md records what the kernel reaches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_label_carry.h"
#include "eincm_motion.hip.h"
#include "eincm_theta_advect.hip.h"

namespace eincm {

struct LcGeom {
    int H, W, K;                       // K: the models of a group
    double cx, cy, s;                  // the motion model's centre and scale
};

// u64 += with no value returned (as ta_add)
__device__ __forceinline__ void lc_add(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }

// grid (ceil(H W / NT), G K).  mass (G, K, H W) as k_ml_mass wrote it; q (G K, 12): motion_q of every window's coefficients; tau (G);
// acc (G, K, H W) u64 and dropped (G K) u64, both zero on entry.
// q + 12 (group, model) and tau + group are the same address for the whole workgroup, so the compiler reads them once, by scalar
// loads, and no thread reads them where its mass is 0: such a thread goes straight to the reduction with 0.
__global__ __launch_bounds__(NT) void k_lc_splat(LcGeom g, const uint32_t* __restrict__ mass, const double* __restrict__ q,
                                                 const double* __restrict__ tau, unsigned long long* __restrict__ acc,
                                                 unsigned long long* __restrict__ dropped)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long wdrop[NWAVE];
    const int gk = blockIdx.y, grp = gk / g.K;
    const int npix = g.H * g.W;                             // (as k_ml_compose: pixel indices fit 32 bits)
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    const uint32_t m = p < npix ? mass[(size_t)gk * npix + p] : 0u;
    unsigned long long lost = 0ull;
    if (m > 0u) {
        const MotionGeom mg{g.H, g.W, 0, ~0ull, g.cx, g.cy, g.s};
        double u, v, uu, uv, vv;
        motion_monomials(mg, p, u, v, uu, uv, vv);
        const double2 f = motion_poly(q + (size_t)gk * MOTION_NQ, u, v, uu, uv, vv);
        const int y = p / g.W, x = p - y * g.W;
        TaLanding l;
        if (!ta_landing(x, y, f.x, f.y, tau[grp], g.H, g.W, l)) {
            lost = (unsigned long long)m * LC_FULL;
        } else {
            unsigned long long* const a = acc + (size_t)gk * npix;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int tx = l.x0 + dx, ty = l.y0 + dy;
                    const unsigned long long d = (unsigned long long)m * (unsigned long long)ta_weight(l, dx, dy);
                    if (d == 0ull) continue;
                    if (tx < 0 || tx >= g.W || ty < 0 || ty >= g.H) { lost += d; continue; }
                    lc_add(a + ((size_t)ty * g.W + tx), d);        // in [0, npix): both coordinates were just checked
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lost += __shfl_down(lost, o, 64);
    if ((threadIdx.x & 63) == 0) wdrop[threadIdx.x >> 6] = lost;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = wdrop[0];
#pragma unroll
        for (int w = 1; w < NWAVE; ++w) t += wdrop[w];
        if (t) lc_add(dropped + gk, t);
    }
}

// grid (ceil(n / NT)): one thread per cell of acc (G, K, H W) -> carried, the same shape
__global__ __launch_bounds__(NT) void k_lc_resolve(size_t n, const unsigned long long* __restrict__ acc, uint32_t* __restrict__ carried)
{
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) carried[i] = lc_resolve(acc[i]);
}

}   // namespace eincm
