// eincm_floweval.hip.h — flow errors of a batch of solved thetas against staged ground truth: what
// sparse_flow_error (src/evaluations/flow_eval.py:14-76) computes on per_pix_theta_to_flow (theta_utils.py:40-73) of one window, for
// every window of a batch in one launch.
//
//   staging (once per batch)
//     k_fe_events  one thread per evaluation event: the byte of its pixel becomes 1 (racing writers all store the same value, so no
//                  atomics); counts the events whose coordinate lies outside the sensor (the call then fails)
//     k_fe_flags   one thread per pixel: flag byte = bit 0 "an event sits here AND (no eval mask OR eval mask != 0)" | bit 1 "GT valid";
//                  counts the GT-valid pixels of the window
//   evaluation (once per theta batch)
//     k_flow_error grid (FE_PARTS, n): thread t of workgroup g owns pixels p = g NT + t + k (FE_PARTS NT), k = 0, 1, ... ascending.
//                  Where bit 0 is set it forms the predicted flow (theta itself at sensor size, else the unfused tap sums of
//                  k_flow_encode), tests it, and in the intersection with bit 1 adds ee and ree to its float64 chains and the counts
//                  to its integers.  The workgroup reduces with wave_sum / block_sum and STORES its partial in slot (window, g);
//                  the host adds the FE_PARTS partials in index order.  No atomic on any float.
// "valid" is flow_eval.py's mask: both components not +-inf and sqrt(x x + y y) > 0 (false for NaN and for a norm that underflows).
// The two staging counters are integer atomicAdd: their final value does not depend on the order of the additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int FE_PARTS = 32;                       // workgroups (= partials) per window
constexpr int FE_NOVER = 6;                        // thresholds of A{N}PE: N = 1, 2, 3, 5, 10, 20
constexpr uint8_t FE_EVENT = 1, FE_GT = 2;         // the bits of a flag byte

struct FlowErrPart {                               // what one workgroup of k_flow_error leaves
    double sum_ee, sum_ree;
    uint32_t n_ee, n_pred, n_over[FE_NOVER];
};

// both components are not +-inf and the norm, formed as numpy / jnp.linalg.norm does, is positive
__device__ __forceinline__ bool fe_valid(double x, double y) {
#pragma clang fp contract(off)
    return !isinf(x) && !isinf(y) && __dsqrt_rn(x * x + y * y) > 0.0;
}

// grid (ceil(max events of a window / NT), n).  Window b's events are xs / ys [off[b], off[b + 1]); plane (n, npix) is zero on entry.
__global__ __launch_bounds__(NT) void k_fe_events(int H, int W, const int64_t* __restrict__ off, const int16_t* __restrict__ xs,
                                                  const int16_t* __restrict__ ys, uint8_t* __restrict__ plane,
                                                  unsigned long long* __restrict__ oob) {
    const int b = blockIdx.y;
    const int64_t e = off[b] + (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= off[b + 1]) return;
    const int x = xs[e], y = ys[e];
    if (x < 0 || x >= W || y < 0 || y >= H) { atomicAdd(oob, 1ull); return; }
    plane[(int64_t)b * H * W + (int64_t)y * W + x] = 1;
}

// grid (ceil(npix / NT), n).  flags holds the event plane on entry and the flag bytes on exit; n_gt[b] += GT-valid pixels.
__global__ __launch_bounds__(NT) void k_fe_flags(int npix, const double2* __restrict__ gt, const uint8_t* __restrict__ eval_mask,
                                                 uint8_t* __restrict__ flags, unsigned long long* __restrict__ n_gt) {
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    bool ok = false;
    if (p < npix) {
        const int64_t q = (int64_t)blockIdx.y * npix + p;
        const double2 g = gt[q];
        ok = fe_valid(g.x, g.y);
        const bool ev = flags[q] != 0 && (!eval_mask || eval_mask[q] != 0);
        flags[q] = (uint8_t)((ev ? FE_EVENT : 0) | (ok ? FE_GT : 0));
    }
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_gt + blockIdx.y, (unsigned long long)__popcll(m));
}

// grid (FE_PARTS, n).  theta (n, h, w, 2); full: (h, w) == (H, W) and the tap tables are not read.  Tap tables as k_flow_encode's.
// parts (n, FE_PARTS); ee_map (n, npix) or null: ee in the intersection, NaN elsewhere (every pixel is written by its owner).
__global__ __launch_bounds__(NT) void k_flow_error(int H, int W, int h, int w, int full, const double2* __restrict__ gt,
                                                   const uint8_t* __restrict__ flags, const double2* __restrict__ theta,
                                                   const int32_t* __restrict__ rlo, const int32_t* __restrict__ rcnt,
                                                   const double* __restrict__ rwt, int rstride, const int32_t* __restrict__ clo,
                                                   const int32_t* __restrict__ ccnt, const double* __restrict__ cwt, int cstride,
                                                   FlowErrPart* __restrict__ parts, double* __restrict__ ee_map) {
#pragma clang fp contract(off)
    __shared__ double scratch[NWAVE];
    __shared__ uint32_t cred[NWAVE][2 + FE_NOVER];
    const int npix = H * W;                        // H, W <= 32767: pixel indices fit 32 bits
    const int b = blockIdx.y;
    const double2* g_b = gt + (int64_t)b * npix;
    const uint8_t* f_b = flags + (int64_t)b * npix;
    const double2* th = theta + (int64_t)b * h * w;
    double* map_b = ee_map ? ee_map + (int64_t)b * npix : nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double s_ee = 0.0, s_ree = 0.0;
    uint32_t cnt[2 + FE_NOVER] = {};               // n_ee, n_pred, n_over[6]
    for (int p = (int)(blockIdx.x * NT + threadIdx.x); p < npix; p += FE_PARTS * NT) {
        const double2 g = g_b[p];
        const uint8_t f = f_b[p];
        double ee = nan;
        if (f & FE_EVENT) {
            double vx, vy;
            if (full) {
                const double2 t = th[p];
                vx = t.x; vy = t.y;
            } else {
                const int y = p / W, x = p - y * W;
                const int i0 = rlo[y], ni = rcnt[y], j0 = clo[x], nj = ccnt[x];
                vx = 0.0; vy = 0.0;
                for (int i = 0; i < ni; ++i) {
                    double sx = 0.0, sy = 0.0;
                    for (int j = 0; j < nj; ++j) {
                        const double2 t = th[(int64_t)(i0 + i) * w + (j0 + j)];
                        const double bw = cwt[(int64_t)x * cstride + j];
                        sx += bw * t.x;
                        sy += bw * t.y;
                    }
                    const double aw = rwt[(int64_t)y * rstride + i];
                    vx += aw * sx;
                    vy += aw * sy;
                }
            }
            if (fe_valid(vx, vy)) {
                ++cnt[1];
                if (f & FE_GT) {
                    const double dx = vx - g.x, dy = vy - g.y;
                    ee = __dsqrt_rn(dx * dx + dy * dy);
                    const double ree = __ddiv_rn(ee, __dsqrt_rn(g.x * g.x + g.y * g.y) + EPSN);
                    s_ee += ee;
                    s_ree += ree;
                    ++cnt[0];
                    cnt[2] += ee > 1.0; cnt[3] += ee > 2.0; cnt[4] += ee > 3.0;
                    cnt[5] += ee > 5.0; cnt[6] += ee > 10.0; cnt[7] += ee > 20.0;
                }
            }
        }
        if (map_b) map_b[p] = ee;
    }
    s_ee = block_sum(s_ee, scratch);
    s_ree = block_sum(s_ree, scratch);
#pragma unroll
    for (int k = 0; k < 2 + FE_NOVER; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt[k] += __shfl_xor(cnt[k], d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 2 + FE_NOVER; ++k) cred[wave][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        FlowErrPart o;
        o.sum_ee = s_ee; o.sum_ree = s_ree;
        uint32_t t[2 + FE_NOVER];
        for (int k = 0; k < 2 + FE_NOVER; ++k) { t[k] = 0; for (int v = 0; v < NWAVE; ++v) t[k] += cred[v][k]; }
        o.n_ee = t[0]; o.n_pred = t[1];
        for (int k = 0; k < FE_NOVER; ++k) o.n_over[k] = t[2 + k];
        parts[(int64_t)b * FE_PARTS + blockIdx.x] = o;
    }
}

}  // namespace eincm
