// eincm_splat_window.hip.h — gfx950 event kernels for splat window sizes other than 3.
//
// events_to_pdf_frame(xs, ys, sensor_size, window_size) (event_utils.py:13-61) adds exp(-|q|^2 / 2) / (2 pi) at the (2w+1)^2 pixels
// round(x) + d, d in [-w, w]^2, q = round(x) + d - x, w = window_size // 2.  Radius 1 (sizes 2 and 3) keeps k_splat / k_gather of
// eincm_kernels.hip.h; radius 0, 2 and 3 (sizes 1, 4-5, 6-7) take the two kernels below, templated on the radius:
//   k_splat_r   warp + (2w+1)^2 taps of every event at every reference time into an LDS window of u64 at the IWE accumulator's own
//               scale 2^ACC_SHIFT, flushed once per (segment, reference time)                                 [event_utils.py:31-59]
//   k_gather_r  backward of the splat: dL/dw from the (2w+1)^2 neighbourhood of dL/dIWE (G staged in LDS), then either a per-workgroup
//               partial of dL/dtheta (2-DoF theta, the slots k_final / the host sum) or an i64 per-source-pixel sum flushed into the
//               dL/dTheta image that k_project / k_final_dense consume                                         [reverse of event_utils.py:59]
// Both walk one segment list plainly (thread i takes events i, i + NT, ...), like the fp64 kernels; the theta-grid gather never projects
// onto the cells itself.  Destination windows get the radius as their margin; they are derived per workgroup from the per-tile
// velocity bounds (k_theta) or the 2-DoF theta, not read from the tables k_theta fills for the radius-1 kernels.
//
// Bounds (radius w):
//   IWE.  Every tap is rounded once, rint(tap * 2^30), whether it lands in LDS or goes to HBM, so the image is the exact integer sum of
//     the rounded taps whatever the segmentation, batch or order.  One tap <= 1 / (2 pi).  An LDS word takes at most one tap per event
//     (the window is in unwrapped coordinates; the flush applies the wrap / drop rule), so it holds <= MAX_CHUNK * 0.16 * 2^30 < 2^42.
//     In HBM a sensor side <= 2w lets one event wrap two taps per axis onto one pixel (p and p + n both in [c - w, c + w]): <= 4 taps
//     per event and pixel, pixel * 2^30 <= 4 * 0.16 * N * 2^30 < 2^63 for N < 1.3e10 events (event offsets are int32).
//   Gradient.  |dL/dw_x| <= max|G| sum_d |d - f| k(d) = max|G| S1(f) S0(f) / (2 pi) with S0 = sum_d exp(-(d - f)^2 / 2) <= 2.51 and
//     S1 = sum_d |d - f| exp(-(d - f)^2 / 2) <= 2.10 for |f| <= 1/2 and ANY radius: <= 0.84 max|G| per component, under the 2.15 max|G|
//     that grad_shift_pixel / grad_shift assume for radius 1.  The fixed-point scales of the radius-1 path hold unchanged.
#pragma once
#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int SPLAT_RADIUS_MAX = 3;          // window size 7

// item_window with the margin of radius `rad` (+rad for the taps, +1 for the rounding) and the row pitch equal to the width
__device__ __forceinline__ Window item_window_r(const Geom& g, const Item& it, const double* mm4, double tau, int wincap, int winmaxw, int rad) {
    const int tx = it.tile % g.tilesX, ty = it.tile / g.tilesX;
    const int x0 = tx * TS, y0 = ty * TS;
    const int x1 = min(x0 + TS, g.W) - 1, y1 = min(y0 + TS, g.H) - 1;
    const double dlo = it.t_lo - tau, dhi = it.t_hi - tau;
    const double LIM = 4096.0;
    double lo[2], hi[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double vmin = mm4[2 * c], vmax = mm4[2 * c + 1];
        const double a = -vmin * dlo, b = -vmin * dhi, cc = -vmax * dlo, d = -vmax * dhi;
        double mn = fmin(fmin(a, b), fmin(cc, d)), mx = fmax(fmax(a, b), fmax(cc, d));
        if (!(mn == mn) || !(mx == mx)) { mn = 0.0; mx = 0.0; }          // NaN theta: any window is correct
        lo[c] = floor(fmin(fmax(mn, -LIM), LIM));
        hi[c] = ceil(fmin(fmax(mx, -LIM), LIM));
    }
    const int m = rad + 1;
    int bx0 = x0 + (int)lo[0] - m, bx1 = x1 + (int)hi[0] + m;
    int by0 = y0 + (int)lo[1] - m, by1 = y1 + (int)hi[1] + m;
    int ww = bx1 - bx0 + 1, wh = by1 - by0 + 1;
    if (ww * wh > wincap || ww > winmaxw) {          // clamped: the taps outside take the direct-to-HBM path (any window is correct)
        const int nww = min(ww, winmaxw);
        const int nwh = min(wh, wincap / nww);
        bx0 = (bx0 + bx1) / 2 - nww / 2;
        by0 = (by0 + by1) / 2 - nwh / 2;
        ww = nww; wh = nwh;
    }
    Window w; w.ox = bx0; w.oy = by0; w.ww = ww; w.wh = wh;
    return w;
}

// k(d) = exp(-(d - f)^2 / 2), d = -RAD..RAD: 2 RAD + 1 exponentials per axis (the (2 RAD + 1)^2 taps are their products)
template <int RAD>
__device__ __forceinline__ void taps_axis(float f, float* k) {
    constexpr float HL2E = 0.5f * 1.4426950408889634f;
#pragma unroll
    for (int d = -RAD; d <= RAD; ++d) {
        const float q = (float)d - f;
        k[d + RAD] = __builtin_amdgcn_exp2f(-(q * q) * HL2E);
    }
}

// the window's velocity bounds: the 2-DoF theta itself, or the tile's bounds k_theta wrote
template <int TM>
__device__ __forceinline__ double2 window_velocity(const Geom& g, const Item& it, int use_arg, const double* __restrict__ theta_c,
                                                   const ThetaArg& targ, const double* __restrict__ tmm, double mm4[4]) {
    if (TM == THETA_CONST) {
        const double2 v = use_arg ? make_double2(targ.v[2 * it.win], targ.v[2 * it.win + 1])
                                  : make_double2(theta_c[2 * it.win], theta_c[2 * it.win + 1]);
        mm4[0] = v.x; mm4[1] = v.x; mm4[2] = v.y; mm4[3] = v.y;
        return v;
    }
    const double* mm = tmm + ((size_t)it.win * g.ntiles + it.tile) * 4;
    mm4[0] = mm[0]; mm4[1] = mm[1]; mm4[2] = mm[2]; mm4[3] = mm[3];
    return make_double2(0.0, 0.0);
}

// the source tile's velocities into LDS (theta grids / dense theta)
__device__ __forceinline__ void stage_theta_tile(const Geom& g, const Item& it, const double* __restrict__ Theta, double2* thtile) {
    const int tx0 = (it.tile % g.tilesX) * TS, ty0 = (it.tile / g.tilesX) * TS;
    const double* __restrict__ ThW = Theta + (size_t)it.win * g.H * g.W * 2;
    for (int p = threadIdx.x; p < TS * TS; p += NT) {
        const int y = ty0 + p / TS, x = tx0 + p % TS;
        thtile[p] = (y < g.H && x < g.W) ? *reinterpret_cast<const double2*>(ThW + ((size_t)y * g.W + x) * 2) : make_double2(0.0, 0.0);
    }
}

// ------------------------------------------------------------------------------------------------
// k_splat_r: grid ceil(n_items/8)*8*R blocks (block_to_work), LDS g.wincap u64 (+ the Theta tile for THETA_TILE).
// ------------------------------------------------------------------------------------------------
template <int TM, int RAD>
__global__ __launch_bounds__(NT) void k_splat_r(Geom g, int n_items, const Item* __restrict__ items,
        const uint32_t* __restrict__ ev_xy, const double* __restrict__ ev_t,
        const double* __restrict__ Theta,      // (B,H,W,2), THETA_TILE
        const double* __restrict__ tmm,        // (B,ntiles,4) velocity bounds, THETA_TILE
        const double* __restrict__ edge_ts,    // (B,R)
        unsigned long long* __restrict__ acc,  // (B,R,H,W) u64 at 2^ACC_SHIFT, zero on entry (cleared by its consumer)
        const int32_t* __restrict__ order,
        int use_arg, const double* __restrict__ theta_c, ThetaArg targ)
{
    constexpr int K = 2 * RAD + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds64[];
    double2* thtile = reinterpret_cast<double2*>(lds64 + g.wincap);
    int item, r;
    if (!block_to_work(n_items, g.R, order, item, r)) return;
    const Item it = items[item];
    if (!win_active(g, it.win)) return;
    const double tau = edge_ts[it.win * g.R + r];
    double mm4[4];
    const double2 vconst = window_velocity<TM>(g, it, use_arg, theta_c, targ, tmm, mm4);
    if (TM == THETA_TILE) stage_theta_tile(g, it, Theta, thtile);
    const Window wn = item_window_r(g, it, mm4, tau, g.wincap, g.winmaxw, RAD);
    const int nwin = wn.ww * wn.wh;
    for (int i = threadIdx.x; i < nwin; i += NT) lds64[i] = 0ull;
    __syncthreads();

    unsigned long long* __restrict__ img = acc + ((size_t)it.win * g.R + r) * g.H * g.W;
    const float scy = INV_2PI * 1073741824.0f;      // 2^ACC_SHIFT / (2 pi): a tap * 2^30 < 2^28
    for (int e = threadIdx.x; e < it.count; e += NT) {
        const uint32_t xy = ev_xy[it.begin + e];
        const double dt = ev_t[it.begin + e] - tau;
        const int x = xy & 0xffff, y = xy >> 16;
        const double2 v = (TM == THETA_CONST) ? vconst : thtile[((xy >> 11) & (31u << 5)) | (xy & 31u)];
        int irx, iry; float fx, fy;
        warp_axis(x, v.x, dt, irx, fx);
        warp_axis(y, v.y, dt, iry, fy);
        float kx[K], ky[K];
        taps_axis<RAD>(fx, kx);
        taps_axis<RAD>(fy, ky);
#pragma unroll
        for (int d = 0; d < K; ++d) ky[d] *= scy;
        const int sx = clamp_far(irx), sy = clamp_far(iry);
        const int lx0 = sx - RAD - wn.ox, ly0 = sy - RAD - wn.oy;      // window coordinates of the top-left tap
        if (lx0 >= 0 && ly0 >= 0 && lx0 + K <= wn.ww && ly0 + K <= wn.wh) {
            unsigned long long* p = lds64 + ly0 * wn.ww + lx0;
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) atomicAdd(p + dx, (unsigned long long)fix_u32(ky[dy], kx[dx]));
                p += wn.ww;
            }
        } else {
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const unsigned long long q = (unsigned long long)fix_u32(ky[dy], kx[dx]);
                    const int cx = lx0 + dx, cy = ly0 + dy;
                    if (cx >= 0 && cy >= 0 && cx < wn.ww && cy < wn.wh) {
                        atomicAdd(lds64 + cy * wn.ww + cx, q);
                    } else {
                        const int gx = wrap_drop(sx - RAD + dx, g.W), gy = wrap_drop(sy - RAD + dy, g.H);
                        if (gx >= 0 && gy >= 0) atomicAdd(img + (size_t)gy * g.W + gx, q);
                    }
                }
            }
        }
    }
    __syncthreads();
    // flush: the window's exact integer sums, already at the accumulator's scale; the wrap / drop rule per pixel
    for (WinWalk w(threadIdx.x, wn.ww); w.i < nwin; w.next()) {
        const unsigned long long q = lds64[w.i];
        if (q == 0ull) continue;
        const int gx = wrap_drop(wn.ox + w.col, g.W), gy = wrap_drop(wn.oy + w.row, g.H);
        if (gx >= 0 && gy >= 0) atomicAdd(img + (size_t)gy * g.W + gx, q);
    }
}

// ------------------------------------------------------------------------------------------------
// k_gather_r: grid as k_splat_r.  For every event of the segment and this reference time
//   dL/dwx = sum_taps G[p] k (dx - fx) / (2 pi),  dL/dwy likewise,  then  dL/dTheta[y,x,:] += -dt * (dL/dwx, dL/dwy).
// 2-DoF theta: fp32 per thread, the workgroup's fp64 sum in a fixed order STORED into its own slot of g11 (k_final / the host add the
// slots in index order).  Otherwise: i64 per source pixel in LDS at grad_shift_pixel's scale (61 bits when `wide`), flushed with i64
// atomics into gTheta.  LDS: [G window g.wincap_a floats][i64 sums TS*TS*2, THETA_TILE][Theta tile TS*TS double2, THETA_TILE].
// ------------------------------------------------------------------------------------------------
template <int TM, int RAD>
__global__ __launch_bounds__(NT) void k_gather_r(Geom g, int n_items, const Item* __restrict__ items,
        const uint32_t* __restrict__ ev_xy, const double* __restrict__ ev_t,
        const double* __restrict__ Theta, const double* __restrict__ tmm, const double* __restrict__ edge_ts,
        const float* __restrict__ G,           // (B,R,H,W) dL/dIWE
        long long* __restrict__ gTheta,        // (B,H,W,2) i64 fixed point, zero on entry (cleared by its consumer)
        double* __restrict__ g11,              // 2-DoF theta: (n_items, R, 2) per-workgroup partials of dL/dtheta
        const WinConst* __restrict__ wc, const unsigned* __restrict__ gmax, int wide,
        int use_arg, const double* __restrict__ theta_c, ThetaArg targ)
{
    constexpr int K = 2 * RAD + 1;
    constexpr bool direct11 = TM == THETA_CONST;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[NWAVE];
    __shared__ unsigned gms[NWAVE];
    unsigned long long* accum = reinterpret_cast<unsigned long long*>(lds + g.wincap_a);
    double2* thtile = reinterpret_cast<double2*>(lds + g.wincap_a + TS * TS * 4);
    int item, r;
    if (!block_to_work(n_items, g.R, nullptr, item, r)) return;
    const Item it = items[item];
    if (!win_active(g, it.win)) return;
    const double tau = edge_ts[it.win * g.R + r];
    double mm4[4];
    const double2 vconst = window_velocity<TM>(g, it, use_arg, theta_c, targ, tmm, mm4);
    const Window wn = item_window_r(g, it, mm4, tau, g.wincap_a, g.winmaxw_a, RAD);
    const float* __restrict__ Gi = G + ((size_t)it.win * g.R + r) * g.H * g.W;
    const int x0 = (it.tile % g.tilesX) * TS, y0 = (it.tile / g.tilesX) * TS;
    if (!direct11) {
        stage_theta_tile(g, it, Theta, thtile);
        for (int i = threadIdx.x; i < TS * TS * 2; i += NT) accum[i] = 0ull;
    }
    for (WinWalk w(threadIdx.x, wn.ww); w.i < wn.ww * wn.wh; w.next()) {       // the G window, zero where the index rule drops
        const int gx = wrap_drop(wn.ox + w.col, g.W), gy = wrap_drop(wn.oy + w.row, g.H);
        lds[w.i] = (gx >= 0 && gy >= 0) ? Gi[(size_t)gy * g.W + gx] : 0.0f;
    }
    double gscale = 0.0;
    if (!direct11) gscale = ldexp(1.0, grad_shift_pixel(wc[it.win], gmax_of(gmax + (size_t)it.win * g.gmax_n, g.gmax_n, gms), g.R, wide != 0));
    __syncthreads();

    float f11x = 0.0f, f11y = 0.0f;
    for (int e = threadIdx.x; e < it.count; e += NT) {
        const uint32_t xy = ev_xy[it.begin + e];
        const double dt = ev_t[it.begin + e] - tau;
        const int x = xy & 0xffff, y = xy >> 16;
        const uint32_t key = ((xy >> 11) & (31u << 5)) | (xy & 31u);
        const double2 v = direct11 ? vconst : thtile[key];
        int irx, iry; float fx, fy;
        warp_axis(x, v.x, dt, irx, fx);
        warp_axis(y, v.y, dt, iry, fy);
        float kx[K], ky[K];
        taps_axis<RAD>(fx, kx);
        taps_axis<RAD>(fy, ky);
        const int sx = clamp_far(irx), sy = clamp_far(iry);
        const int lx0 = sx - RAD - wn.ox, ly0 = sy - RAD - wn.oy;
        const bool inside = lx0 >= 0 && ly0 >= 0 && lx0 + K <= wn.ww && ly0 + K <= wn.wh;
        // c[dx] = sum_dy ky G, rr[dy] = sum_dx kx G: dL/dwx = sum_dx kx (dx - fx) c[dx], dL/dwy = sum_dy ky (dy - fy) rr[dy]
        float c[K];
#pragma unroll
        for (int d = 0; d < K; ++d) c[d] = 0.0f;
        float gy_acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
            float rr = 0.0f;
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                float gv;
                if (inside) {
                    gv = lds[(ly0 + dy) * wn.ww + lx0 + dx];
                } else {
                    const int cx = lx0 + dx, cy = ly0 + dy;
                    if (cx >= 0 && cy >= 0 && cx < wn.ww && cy < wn.wh) {
                        gv = lds[cy * wn.ww + cx];
                    } else {
                        const int gx = wrap_drop(sx - RAD + dx, g.W), gy = wrap_drop(sy - RAD + dy, g.H);
                        gv = (gx >= 0 && gy >= 0) ? Gi[(size_t)gy * g.W + gx] : 0.0f;
                    }
                }
                rr = fmaf(kx[dx], gv, rr);
                c[dx] = fmaf(ky[dy], gv, c[dx]);
            }
            gy_acc = fmaf(ky[dy] * ((float)(dy - RAD) - fy), rr, gy_acc);
        }
        float gx_acc = 0.0f;
#pragma unroll
        for (int dx = 0; dx < K; ++dx) gx_acc = fmaf(kx[dx] * ((float)(dx - RAD) - fx), c[dx], gx_acc);
        const float gwx = gx_acc * INV_2PI, gwy = gy_acc * INV_2PI;
        if (direct11) {
            const float ndt = (float)(-dt);
            f11x = fmaf(ndt, gwx, f11x); f11y = fmaf(ndt, gwy, f11y);
        } else {
            const double sdt = -dt * gscale;
            const double vx = sdt * (double)gwx, vy = sdt * (double)gwy;
            unsigned long long* a = accum + (key << 1);
            atomicAdd(a, (unsigned long long)(wide ? fix64_wide(vx) : fix64(vx)));
            atomicAdd(a + 1, (unsigned long long)(wide ? fix64_wide(vy) : fix64(vy)));
        }
    }
    if (direct11) {
        const double sx = block_sum((double)f11x, red);
        const double sy = block_sum((double)f11y, red);
        if (threadIdx.x == 0) {
            double* dst = g11 + ((size_t)item * g.R + r) * 2;
            dst[0] = sx; dst[1] = sy;
        }
        return;
    }
    __syncthreads();
    unsigned long long* __restrict__ gT = reinterpret_cast<unsigned long long*>(gTheta) + (size_t)it.win * g.H * g.W * 2;
    const int tw = min(TS, g.W - x0), th = min(TS, g.H - y0);
    for (int i = threadIdx.x; i < TS * TS * 2; i += NT) {
        const int cc = i & 1, px = (i >> 1) % TS, py = (i >> 1) / TS;
        const unsigned long long q = accum[i];
        if (px < tw && py < th && q != 0ull) atomicAdd(gT + ((size_t)(y0 + py) * g.W + (x0 + px)) * 2 + cc, q);
    }
}

}  // namespace eincm
