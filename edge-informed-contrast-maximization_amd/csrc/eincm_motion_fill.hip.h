// eincm_motion_fill.hip.h — k_mf_sites, k_mf_count, k_mf_cols, k_mf_rows and k_mf_compose: a motion segmentation composed into a DENSE
// flow field and label image (eincm_densify_motions).  k_ml_mass and k_ml_total (eincm_motion_layers.hip.h) give
// the per-pixel masses and the groups' totals as they do for eincm_compose_motions; a pixel whose summed mass reaches min_site_mass is a
// site; an exact Euclidean feature transform finds every pixel's nearest site under the tie rule of eincm_motion_fill.h; and the
// composition of k_ml_compose runs with the mass vector read at that site and the models' fields evaluated at the pixel itself.
//
// The transform is separable, as the distance transform of eincm_edges.hip.h: a column pass leaves, per pixel, the nearest site of its
// own column (distance and row in one 32-bit word); a row pass searches outwards from x over those records and keeps the smallest
// 64-bit key.  The functions that decide anything are eincm_motion_fill.h's, which the CPU checker runs too.
//
// Everything but the last step is integer; the fp64 composition is one thread's own sequence of rounded operations.  No global atomics,
// no float atomics: any launch shape gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_motion.hip.h"
#include "eincm_motion_fill.h"
#include "eincm_motion_layers.hip.h"

namespace eincm {

// grid (ceil(H W / NT), G): one thread per (group, pixel).  mass (G, K, H, W).  site (G, H, W): 1 where the pixel's summed mass reaches
// min_site_mass.  part (G, gridDim.x): this workgroup's sites, one plain store; k_mf_count adds them.
__global__ __launch_bounds__(NT) void k_mf_sites(int npix, int K, uint32_t min_site_mass, const uint32_t* __restrict__ mass,
                                                 uint8_t* __restrict__ site, uint32_t* __restrict__ part)
{
    __shared__ uint32_t wcnt[NWAVE];
    const int grp = blockIdx.y;
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    bool s = false;
    if (p < npix) {                                         // (lanes past the image stay for the reduction)
        s = mf_is_site(mass + (size_t)grp * K * npix + p, K, npix, min_site_mass);
        site[(size_t)grp * npix + p] = s ? 1 : 0;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(s));
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = wcnt[0];
#pragma unroll
        for (int w = 1; w < NWAVE; ++w) t += wcnt[w];
        part[(size_t)grp * gridDim.x + blockIdx.x] = t;
    }
}

// n_sites[g] = the workgroup partials of one group added up: integers, so the order is free.  One wave per group.
__global__ __launch_bounds__(64) void k_mf_count(int nparts, const uint32_t* __restrict__ part, uint32_t* __restrict__ n_sites)
{
    const size_t g = blockIdx.x;
    uint32_t t = 0u;
    for (int k = threadIdx.x; k < nparts; k += 64) t += part[g * nparts + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += (uint32_t)__shfl_down((int)t, o, 64);
    if (threadIdx.x == 0) n_sites[g] = t;
}

// grid (ceil(W / NT), G): one thread per (group, column), loads and stores coalesced across the columns.  rec (G, H, W): the column
// record of every pixel (mf_pack), MF_REC_NONE in a column without a site.
// A thread walks its column twice and is bound by the latency of its loads (W x G threads in all, a few waves per CU at most): one
// load per step, each waiting for the step before it, took 145 us at 8 x 256x336 and 270 us at 480x640.  So MF_COL_BATCH rows are
// loaded before the first of them is used; the steps themselves still run in row order, which is all the sweeps ask for.
constexpr int MF_COL_BATCH = 8;
__global__ __launch_bounds__(NT) void k_mf_cols(int H, int W, const uint8_t* __restrict__ site, uint32_t* __restrict__ rec)
{
    const int x = (int)(blockIdx.x * NT + threadIdx.x);
    if (x >= W) return;
    const size_t base = (size_t)blockIdx.y * H * W + x;
    int above = -1, below = -1;
    for (int y0 = 0; y0 < H; y0 += MF_COL_BATCH) {
        uint8_t s[MF_COL_BATCH];
#pragma unroll
        for (int u = 0; u < MF_COL_BATCH; ++u) s[u] = y0 + u < H ? site[base + (size_t)(y0 + u) * W] : (uint8_t)0;
#pragma unroll
        for (int u = 0; u < MF_COL_BATCH; ++u)
            if (y0 + u < H) rec[base + (size_t)(y0 + u) * W] = mf_col_down(s[u] != 0, y0 + u, above);
    }
    for (int y0 = H - 1; y0 >= 0; y0 -= MF_COL_BATCH) {
        uint32_t r[MF_COL_BATCH];
#pragma unroll
        for (int u = 0; u < MF_COL_BATCH; ++u) r[u] = y0 - u >= 0 ? rec[base + (size_t)(y0 - u) * W] : MF_REC_NONE;
#pragma unroll
        for (int u = 0; u < MF_COL_BATCH; ++u)
            if (y0 - u >= 0) rec[base + (size_t)(y0 - u) * W] = mf_col_up(r[u], y0 - u, below);
    }
}

// grid (H, G), NT threads, W uint32 of dynamic LDS: one workgroup per (group, row).  The row's records go into LDS once, coalesced;
// every thread then searches outwards from its own x (mf_row_search), so the work per pixel is its distance and the LDS reads of a wave
// are at stride 1.  nearest (G, H, W) and dist2 (G, H, W), either may be nullptr.
__global__ __launch_bounds__(NT) void k_mf_rows(int H, int W, const uint32_t* __restrict__ rec, int32_t* __restrict__ nearest,
                                                uint32_t* __restrict__ dist2)
{
    extern __shared__ uint32_t mf_row[];
    const size_t base = ((size_t)blockIdx.y * H + blockIdx.x) * W;
    for (int x = threadIdx.x; x < W; x += NT) mf_row[x] = rec[base + x];
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += NT) {
        const uint64_t key = mf_row_search(mf_row, W, x);
        if (nearest) nearest[base + x] = mf_key_nearest(key, W);
        if (dist2) dist2[base + x] = mf_key_dist2(key);
    }
}

// grid (ceil(H W / NT), G): one thread per (group, pixel): k_ml_compose's arithmetic with the mass vector of the pixel's nearest site,
// the monomials of the pixel itself, and the reach test.  theta (G, H, W) double2 and labels (G, H, W), either may be nullptr.
__global__ __launch_bounds__(NT) void k_mf_compose(MlGeom g, uint32_t max_dist2, const uint32_t* __restrict__ mass,
                                                   const unsigned long long* __restrict__ total, const double* __restrict__ q,
                                                   const int32_t* __restrict__ nearest, const uint32_t* __restrict__ dist2,
                                                   double2* __restrict__ theta, uint8_t* __restrict__ labels)
{
#pragma clang fp contract(off)
    const int grp = blockIdx.y, K = g.K;
    const int npix = g.H * g.W;                             // (as k_ml_compose: pixel indices fit 32 bits)
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    const int32_t s = nearest[(size_t)grp * npix + p];
    const bool reached = mf_reached(s, dist2[(size_t)grp * npix + p], max_dist2);
    const uint32_t* m = mass + (size_t)grp * K * npix + (reached ? s : 0);    // model l's mass of the site: m[l * npix]
    const int lab = reached ? ml_label(m, K, npix) : EINCM_ML_NO_LABEL;
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
