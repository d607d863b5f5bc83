// eincm_contrast_landscape.hip.h — k_contrast_landscape and k_cl_sum_bands: the contrast of the image of warped events on a grid of
// candidate motion coefficients.  Every result is an integer with one right answer: events are counted per cell
// with LDS integer atomics, the squares are summed in 64-bit integers, no float is accumulated anywhere and no workgroup adds to
// another's result, so every run gives the same bytes.
//
//   k_contrast_landscape   grid (bands, V, B), CL_NT threads: one workgroup owns one (window, candidate, band) and holds the band's
//                          uint32 counts in LDS beside the W + H table of normalised coordinates (the bits of motion_coord, built once
//                          per workgroup: the two fp64 divisions leave the event loop).  It streams ALL of the window's events: for an
//                          event that takes part, Theta at the event's own pixel by motion_products and motion_poly, dt = t - t_ref,
//                          w = (double)x - Theta * dt with the product rounded first (warp_axis's rule, fp contract off), r = rint(w),
//                          in the sensor iff 0 <= r_x < W and 0 <= r_y < H as doubles (false for a NaN; the convert that follows sees
//                          in-range values only), cell (r_y >> log2 cell, r_x >> log2 cell), and one ds_add_u32 if the cell is the
//                          band's.  Outside the sensor the event is dropped: no wrap.  Then sum count^2 and sum count over the band's
//                          cells in 64-bit integers, lanes by shuffles, waves through LDS, and one plain store of the pair.
//   k_cl_sum_bands         one thread per (window, candidate): the bands' pairs added in band order.  Integers: any order is exact.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_contrast_landscape.h"
#include "eincm_kernels.hip.h"

namespace eincm {

struct ClGeom {
    int H, W, V;
    int shift;                          // log2 cell
    int rows, cols, n_col_bands;        // ClBands
    int Hc, Wc;
    int table;                          // W + H, or 0: divide per event
    double cx, cy, s;
};

// evoff (B + 1): window b's events are [evoff[b], evoff[b + 1]) of xs, ys, ts and keep.  q (B, V, 12).  t_ref (B).  keep: nullptr (all
// events), else bytes in the events' layout, read for the windows with has_keep[b] != 0.  part (B, V, bands, 2) u64: sum count^2, sum count.
__global__ __launch_bounds__(CL_NT) void k_contrast_landscape(ClGeom g, const int64_t* __restrict__ evoff, const int16_t* __restrict__ xs,
                                                              const int16_t* __restrict__ ys, const double* __restrict__ ts,
                                                              const double* __restrict__ q_all, const double* __restrict__ t_ref,
                                                              const uint8_t* __restrict__ keep, const uint8_t* __restrict__ has_keep,
                                                              unsigned long long* __restrict__ part)
{
#pragma clang fp contract(off)
    extern __shared__ double cl_lds[];                                   // table | counts | the waves' partials
    double* tab = cl_lds;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(cl_lds + g.table);
    const int band = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int rb = band / g.n_col_bands, cb = band - rb * g.n_col_bands;
    const int row0 = rb * g.rows, col0 = cb * g.cols;
    const int nrows = min(g.rows, g.Hc - row0), ncols = min(g.cols, g.Wc - col0);
    const int ncell = nrows * ncols;                                     // <= rows * cols: inside the LDS the host sized
    unsigned long long* red = reinterpret_cast<unsigned long long*>(cnt + (((size_t)g.rows * g.cols + 1) & ~(size_t)1));
    for (int i = threadIdx.x; i < g.table; i += CL_NT) tab[i] = i < g.W ? motion_coord(i, g.cx, g.s) : motion_coord(i - g.W, g.cy, g.s);
    for (int i = threadIdx.x; i < ncell; i += CL_NT) cnt[i] = 0u;
    double q[POLY_NQ];
#pragma unroll
    for (int k = 0; k < POLY_NQ; ++k) q[k] = q_all[((size_t)b * g.V + j) * POLY_NQ + k];
    const double tr = t_ref[b];
    const int64_t e0 = evoff[b], n = evoff[b + 1] - e0;
    const uint8_t* kp = (keep && has_keep[b]) ? keep + e0 : nullptr;
    const double Wd = (double)g.W, Hd = (double)g.H;
    __syncthreads();
#pragma unroll 4
    for (int64_t i = threadIdx.x; i < n; i += CL_NT) {
        if (kp && !kp[i]) continue;
        const int x = xs[e0 + i], y = ys[e0 + i];                       // staged events lie inside the sensor (eincm_set_windows refuses others)
        const double u = g.table ? tab[x] : motion_coord(x, g.cx, g.s);
        const double v = g.table ? tab[g.W + y] : motion_coord(y, g.cy, g.s);
        double uu, uv, vv;
        motion_products(u, v, uu, uv, vv);
        const double2 th = motion_poly(q, u, v, uu, uv, vv);
        const double dt = ts[e0 + i] - tr;
        const double wx = (double)x - th.x * dt, wy = (double)y - th.y * dt;
        const double rx = rint(wx), ry = rint(wy);
        if (!(rx >= 0.0 && rx < Wd && ry >= 0.0 && ry < Hd)) continue;  // (on the doubles: a NaN fails every comparison)
        const int cr = ((int)ry >> g.shift) - row0, cc = ((int)rx >> g.shift) - col0;
        if ((unsigned)cr < (unsigned)nrows && (unsigned)cc < (unsigned)ncols) atomicAdd(cnt + cr * ncols + cc, 1u);
    }
    __syncthreads();
    unsigned long long s2 = 0ull, s1 = 0ull;
    for (int i = threadIdx.x; i < ncell; i += CL_NT) {
        const unsigned long long c = cnt[i];
        s2 += c * c;
        s1 += c;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s2 += __shfl_down(s2, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = s2; red[2 * (threadIdx.x >> 6) + 1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CL_NT / 64; ++w) { s2 += red[2 * w]; s1 += red[2 * w + 1]; }
        unsigned long long* o = part + (((size_t)b * g.V + j) * gridDim.x + band) * 2;
        o[0] = s2;
        o[1] = s1;
    }
}

// sumsq, n_in (B * V), either may be nullptr.  part (B * V, n_bands, 2).
__global__ __launch_bounds__(NT) void k_cl_sum_bands(int n, int n_bands, const unsigned long long* __restrict__ part,
                                                     unsigned long long* __restrict__ sumsq, uint32_t* __restrict__ n_in)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    unsigned long long s2 = 0ull, s1 = 0ull;
    for (int k = 0; k < n_bands; ++k) {
        s2 += part[((size_t)i * n_bands + k) * 2];
        s1 += part[((size_t)i * n_bands + k) * 2 + 1];
    }
    if (sumsq) sumsq[i] = s2;
    if (n_in) n_in[i] = (uint32_t)s1;                                    // <= the window's events, which an int32 counts
}

}   // namespace eincm
