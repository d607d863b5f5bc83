// eincm_motion_layers.hip.h — k_ml_mass, k_ml_total and k_ml_compose: a motion segmentation composed into one flow field and a label
// image (eincm_compose_motions).  The staged batch is G groups of K consecutive windows that hold the same events
// under K motions with complementary weights; per sensor pixel the operator asks which model owns the events that fired there and
// writes that model's flow.  The rules that need no GPU - the refusals, the layout, and the four per-pixel functions the kernels call -
// are in eincm_motion_layers.h.
//
// What is read of the staging (eincm_binning.hip.h): the gather's copy of the events, ev_xy = x | y << 16 with the RAW sensor pixel of
// every event and ev_w its weight, both contiguous per (window, tile) in the order (window, tile) - k_bin_scatter places a bin's events
// from tilebase on, k_segsort permutes inside a segment of a bin, the host path (bin_events) sorts by the same key - so the events of bin
// i are the slots [off[i], off[i + 1]) with off the exclusive scan of the tile populations, which the host holds and uploads.  Nothing
// is assumed about the order inside a bin, nor about the K windows of a group sharing a layout: every window's own bins are walked.
//
// Everything up to the last step is integer: uint32 masses by LDS integer atomics inside one workgroup, uint64 totals by shuffles and
// plain stores, no global atomics, no float atomics.  The fp64 blend is one thread's own sequence of rounded operations.  Any launch
// shape therefore gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_motion.hip.h"
#include "eincm_motion_layers.h"

namespace eincm {

constexpr int ML_TILE_PIX = TS * TS;

struct MlGeom {
    int H, W, tilesX, ntiles, K;       // K: the models of a group
    unsigned flags;                    // EINCM_ML_*
    double cx, cy, s;                  // the motion model's centre and scale
};

// grid (ntiles, G), ML_NT threads, K * 1024 uint32 of dynamic LDS: the masses of one source tile under the K models of one group.
//   off (B * ntiles + 1): where every (window, tile)'s events start in ev_xy / ev_w.  ev_w: nullptr for an unweighted batch (w = 1,
//   q = 4096).
//   mass (G, K, H, W): this workgroup's 32x32 block of every model's image, clipped to the sensor, zeros included.
//   part (G, K, ntiles): the block's sum per model.
// An event's pixel lies in its tile (staging binned it by y / TS, x / TS), so its LDS slot is (y & 31) * 32 + (x & 31) < 1024.
// The walk is bound by the latency of its loads, not by their bytes (a bin of a 10^6-event window holds a few thousand events): 16
// waves per workgroup and ML_UNROLL loads per thread in flight before the first atomic took the kernel from 100 to 25 us at 4 x 10^6
// events on 480x640, against 4 waves and one load at a time; on bins of a few hundred events most of the 16 waves idle and the same
// change costs 3 us of 8 (profiles/motion_layers.md).
constexpr int ML_NT = 1024, ML_UNROLL = 4;
static_assert(ML_NT == ML_TILE_PIX, "the write-out owns one pixel of the tile per thread");
__global__ __launch_bounds__(ML_NT) void k_ml_mass(MlGeom g, const int32_t* __restrict__ off, const uint32_t* __restrict__ ev_xy,
                                                   const float* __restrict__ ev_w, uint32_t* __restrict__ mass,
                                                   unsigned long long* __restrict__ part)
{
    extern __shared__ uint32_t ml_acc[];
    __shared__ unsigned long long wsum[ML_NT / 64];
    const int tile = blockIdx.x, grp = blockIdx.y, K = g.K;
    for (int i = threadIdx.x; i < K * ML_TILE_PIX; i += ML_NT) ml_acc[i] = 0u;
    __syncthreads();
    for (int l = 0; l < K; ++l) {
        const size_t bin = (size_t)(grp * K + l) * g.ntiles + tile;
        const int e0 = off[bin], e1 = off[bin + 1];
        uint32_t* acc = ml_acc + l * ML_TILE_PIX;
        for (int e = e0 + (int)threadIdx.x; e < e1; e += ML_NT * ML_UNROLL) {
            uint32_t xy[ML_UNROLL]; float w[ML_UNROLL];
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {           // every load of the trip before its first use; a slot past the bin weighs 0
                const int i = e + u * ML_NT;
                xy[u] = i < e1 ? ev_xy[i] : 0u;
                w[u] = i < e1 ? (ev_w ? ev_w[i] : 1.0f) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < ML_UNROLL; ++u) {
                const uint32_t q = ml_q(w[u]);
                if (q) atomicAdd(&acc[((xy[u] >> 16) & (TS - 1)) * TS + (xy[u] & (TS - 1))], q);
            }
        }
    }
    __syncthreads();
    const int p = threadIdx.x;                              // this thread's pixel of the tile
    const int x = (tile % g.tilesX) * TS + (p & (TS - 1)), y = (tile / g.tilesX) * TS + p / TS;
    const bool inside = x < g.W && y < g.H;
    const size_t npix = (size_t)g.H * g.W;
    for (int l = 0; l < K; ++l) {
        const uint32_t m = ml_acc[l * ML_TILE_PIX + p];     // (a slot outside the sensor holds 0: no event lies there)
        if (inside) mass[((size_t)grp * K + l) * npix + (size_t)y * g.W + x] = m;
        unsigned long long sum = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = wsum[0];
#pragma unroll
            for (int w = 1; w < ML_NT / 64; ++w) t += wsum[w];
            part[((size_t)grp * K + l) * g.ntiles + tile] = t;
        }
        __syncthreads();                                    // wsum is reused by the next model
    }
}

// total[g, l] = the tile partials of one (group, model) added up: integers, so the order is free.  One wave per (group, model).
__global__ __launch_bounds__(64) void k_ml_total(int ntiles, const unsigned long long* __restrict__ part, unsigned long long* __restrict__ total)
{
    const size_t i = blockIdx.x;
    unsigned long long t = 0ull;
    for (int k = threadIdx.x; k < ntiles; k += 64) t += part[i * ntiles + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (threadIdx.x == 0) total[i] = t;
}

// grid (ceil(H W / NT), G): one thread per (group, pixel).  q (B, 12): motion_q of every window's coefficients.  theta (G, H, W)
// double2 and labels (G, H, W), either may be nullptr.
__global__ __launch_bounds__(NT) void k_ml_compose(MlGeom g, const uint32_t* __restrict__ mass, const unsigned long long* __restrict__ total,
                                                   const double* __restrict__ q, double2* __restrict__ theta, uint8_t* __restrict__ labels)
{
#pragma clang fp contract(off)
    const int grp = blockIdx.y, K = g.K;
    const int npix = g.H * g.W;                             // (as k_motion_expand: pixel indices fit 32 bits)
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    const uint32_t* m = mass + (size_t)grp * K * npix + p;  // model l's mass of this pixel: m[l * npix]
    const int lab = ml_label(m, K, npix);
    if (labels) labels[(size_t)grp * npix + p] = (uint8_t)lab;
    if (!theta) return;
    const MotionGeom mg{g.H, g.W, 0, ~0ull, g.cx, g.cy, g.s};
    double u, v, uu, uv, vv;
    motion_monomials(mg, p, u, v, uu, uv, vv);
    const double* qg = q + (size_t)grp * K * MOTION_NQ;
    double2 out; out.x = 0.0; out.y = 0.0;
    if (lab == EINCM_ML_NO_LABEL) {
        const int d = (g.flags & EINCM_ML_FILL_DOMINANT) ? ml_dominant((const uint64_t*)total + (size_t)grp * K, K) : -1;
        if (d >= 0) out = motion_poly(qg + (size_t)d * MOTION_NQ, u, v, uu, uv, vv);
    } else if (g.flags & EINCM_ML_SOFT) {
        unsigned long long S = 0ull;
        for (int l = 0; l < K; ++l) S += m[(size_t)l * npix];
        for (int l = 0; l < K; ++l) {
            const double2 f = motion_poly(qg + (size_t)l * MOTION_NQ, u, v, uu, uv, vv);
            const uint32_t ml = m[(size_t)l * npix];
            out.x = ml_blend_step(out.x, l, ml, S, f.x);
            out.y = ml_blend_step(out.y, l, ml, S, f.y);
        }
    } else {
        out = motion_poly(qg + (size_t)lab * MOTION_NQ, u, v, uu, uv, vv);
    }
    theta[(size_t)grp * npix + p] = out;
}

}   // namespace eincm
