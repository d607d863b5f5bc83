// eincm_kernels_f64.hip.h — gfx950 device code of the float64 mode (EINCM_CF_FP64).
//
// The same objective and gradient as eincm_kernels.hip.h, with every quantity after the warp in fp64:
//   k64_splat    warp (the fp32 path's operations: fp64, product rounded first) + nine fp64 taps, summed in an LDS window, -> u64 IWE
//                accumulator at the per-window scale 2^ishift[b] (>= 2^40, from the bound N_b / (2 pi) on any pixel)            [event_utils.py:31-59]
//   k64_img_a    accumulator -> fp64 IWE stack (consumer clears) + per-workgroup min / max / sum
//   k64_img_b    tie counts, centred second moment, Scharr energy, MSE against the fp64 edges, |div n| (+ its sign image)
//   k64_scal     per-image scalars from the partials, in index order
//   k64_grad1    dL/dIWE without the min / max tie terms + the two sums those terms need              [reverse of losses.py:61-81]
//   k64_grad2    the tie terms; max |dL/dIWE| per window (scale of the gradient accumulator)
//   k64_gather   per-event dL/dw in fp64, summed over the reference times in the thread, added to a 128-bit fixed-point
//                accumulator per source pixel and component (in LDS for the segment's source tile, flushed once per segment)                                           [reverse of event_utils.py:59]
//   k64_gfin     accumulator -> fp64 dL/dTheta (+ gamma * TV gradient of k_tv) (consumer clears); NaN where a window was flagged
//                non-finite (k64_grad2, k64_gather), so the fp32 path's NONFINITE contract holds
//   k64_proj_w / k64_proj_h   separable adjoint resample dL/dTheta -> dL/dtheta, sequential sums     [reverse of theta_utils.py:25-35]
//                (k64_proj_h_first / k64_proj_w_second: the rows first, for theta grids wider than the sensor)
// The staging (event copies, segment lists), k_theta's Theta image and k_tv are shared with the fp32 path.  Every cross-workgroup
// sum is integer (u64 IWE, i128 gradient) or a per-workgroup partial reduced in index order, so results are bit-reproducible.
// A first pass: both event kernels sum in LDS and flush once per segment, the image passes are plain pixel-parallel kernels;
// DESIGN.md section 10 has what it costs.
#pragma once
#include "eincm_kernels.hip.h"
#include <cfloat>

namespace eincm {

constexpr int F64_PIX = 2048;          // pixels per workgroup of the image passes (NT threads x 8)
constexpr int F64_PA = 3;              // partials of k64_img_a: min, max, sum I
constexpr int F64_PB = 6;              // partials of k64_img_b: #min, #max, sum (I - mean)^2, sum gx^2 + gy^2, sum (E - n)^2, sum |div n|
constexpr int F64_PC = 2;              // partials of k64_grad1: sum Gn (n - 1), sum Gn n
constexpr double INV_2PI_D = 0.15915494309189535;    // exp(-log(2 pi)) (event_utils.py:56)
constexpr double EXP_M1_D = 0.36787944117144233;

// fixed-order block reduction (waves, then the waves in index order); the result is returned to every thread
template <typename Op>
__device__ __forceinline__ double block_reduce64(double v, double* scratch, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o, 64));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[wv] = v;
    __syncthreads();
    double r = scratch[0];
#pragma unroll
    for (int i = 1; i < NWAVE; ++i) r = op(r, scratch[i]);
    __syncthreads();
    return r;
}
struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// warp_axis with the fraction kept in fp64: the same operations (no contraction), hence the same rounding decisions
__device__ __forceinline__ void warp_axis64(int x, double v, double dt, int& ir, double& f) {
#pragma clang fp contract(off)
    const double w = (double)x - v * dt;
    const double r = rint(w);
    f = w - r;
    ir = (int)r;
}

// k(d) = exp(-0.5 (d - f)^2), d = -1, 0, 1, centre-factorised: k(0) = exp(-f^2 / 2), k(+1) = k(0) exp(f - 1/2), k(-1) = k(0) e^-1 / exp(f - 1/2)
// (two fp64 exp per axis instead of three: gfx950 has no fp64 exp instruction, ocml's is a software routine)
__device__ __forceinline__ void taps64(double f, double k[3]) {
    const double e0 = exp(-0.5 * f * f);
    const double bp = exp(f - 0.5);
    k[0] = e0 * (EXP_M1_D / bp);
    k[1] = e0;
    k[2] = e0 * bp;
}

// Scharr pair of an image given by an accessor A(y, x) that is 0 outside the image (difference-first form of oracle scharr_grads)
template <typename A>
__device__ __forceinline__ void scharr64(const A& a, int y, int x, double& gx, double& gy) {
    const double pp = a(y + 1, x + 1), pm = a(y + 1, x - 1), mp = a(y - 1, x + 1), mm = a(y - 1, x - 1);
    gx = 3.0 * (pp - pm) + 10.0 * (a(y, x + 1) - a(y, x - 1)) + 3.0 * (mp - mm);
    gy = 3.0 * (pp - mp) + 10.0 * (a(y + 1, x) - a(y - 1, x)) + 3.0 * (pm - mm);
}
__device__ __constant__ const double DIVK64[3][3] = {{1.0 / 12, 1.0 / 6, 1.0 / 12}, {1.0 / 6, 0.0, 1.0 / 6}, {1.0 / 12, 1.0 / 6, 1.0 / 12}};

// ------------------------------------------------------------------------------------------------
// k64_splat: one workgroup per (segment, reference time) as k_count.  A first pass over the segment's events finds the bounding box
// of their rounded destinations; where that box (+ the tap margin, clipped to the sensor) fits F64_WIN words of LDS, the taps are
// summed there as u64 (ds_add_u64) and the window is flushed with one global atomic per touched pixel.  Taps outside the box's
// in-frame part (the JAX wrap of index -1, drops) and segments whose box is too large take one global u64 atomic per tap.  Integer
// sums in both places: the result does not depend on which path a tap took.
// ------------------------------------------------------------------------------------------------
constexpr int F64_WIN = 4096;          // u64 words of the LDS window (32 KiB)

__global__ __launch_bounds__(NT) void k64_splat(Geom g, int n_items, const Item* __restrict__ items, const uint32_t* __restrict__ ev_xy,
                                                 const double* __restrict__ ev_t, const double* __restrict__ Theta,
                                                 const double* __restrict__ edge_ts, const int* __restrict__ ishift,
                                                 unsigned long long* __restrict__ acc)
{
    __shared__ unsigned long long win[F64_WIN];
    __shared__ double scratch[NWAVE];
    int item, r;
    if (!block_to_work(n_items, g.R, nullptr, item, r)) return;
    const Item it = items[item];
    if (!win_active(g, it.win)) return;
    const double tau = edge_ts[it.win * g.R + r];
    const double scale = ldexp(INV_2PI_D, ishift[it.win]);
    const double* __restrict__ Th = Theta + (size_t)it.win * g.H * g.W * 2;
    unsigned long long* __restrict__ img = acc + ((size_t)it.win * g.R + r) * g.H * g.W;
    // pass 1: bounding box of the rounded destinations (warp only)
    double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
    for (int i = threadIdx.x; i < it.count; i += NT) {
        const uint32_t xy = ev_xy[it.begin + i];
        const double dt = ev_t[it.begin + i] - tau;
        const int x = xy & 0xffff, y = xy >> 16;
        const double2 v = *reinterpret_cast<const double2*>(Th + ((size_t)y * g.W + x) * 2);
        int irx, iry; double fx, fy;
        warp_axis64(x, v.x, dt, irx, fx);
        warp_axis64(y, v.y, dt, iry, fy);
        const double cx = (double)clamp_far(irx), cy = (double)clamp_far(iry);
        mnx = fmin(mnx, cx); mxx = fmax(mxx, cx); mny = fmin(mny, cy); mxy = fmax(mxy, cy);
    }
    mnx = block_reduce64(mnx, scratch, OpMin()); mxx = block_reduce64(mxx, scratch, OpMax());
    mny = block_reduce64(mny, scratch, OpMin()); mxy = block_reduce64(mxy, scratch, OpMax());
    if (!(mnx <= mxx)) return;                      // no events
    // the in-frame part of the box with the tap margin: [ox, ox + ww) x [oy, oy + wh)
    const int ox = (int)fmax(mnx - 1.0, 0.0), ex = (int)fmin(mxx + 1.0, (double)(g.W - 1));
    const int oy = (int)fmax(mny - 1.0, 0.0), ey = (int)fmin(mxy + 1.0, (double)(g.H - 1));
    const int ww = ex - ox + 1, wh = ey - oy + 1;
    const bool use_lds = ww > 0 && wh > 0 && ww * wh <= F64_WIN;      // (ww <= W, wh <= H: no overflow)
    if (use_lds) {
        for (int k = threadIdx.x; k < ww * wh; k += NT) win[k] = 0ull;
        __syncthreads();
    }
    // pass 2: the taps
    for (int i = threadIdx.x; i < it.count; i += NT) {
        const uint32_t xy = ev_xy[it.begin + i];
        const double dt = ev_t[it.begin + i] - tau;
        const int x = xy & 0xffff, y = xy >> 16;
        const double2 v = *reinterpret_cast<const double2*>(Th + ((size_t)y * g.W + x) * 2);
        int irx, iry; double fx, fy;
        warp_axis64(x, v.x, dt, irx, fx);
        warp_axis64(y, v.y, dt, iry, fy);
        const int cx = clamp_far(irx), cy = clamp_far(iry);
        double kx[3], ky[3];
        taps64(fx, kx);
        taps64(fy, ky);
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int py = wrap_drop(cy + dy, g.H);
            if (py < 0) continue;
            const double sy = ky[dy + 1] * scale;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int px = wrap_drop(cx + dx, g.W);
                if (px < 0) continue;
                const unsigned long long q = (unsigned long long)rint(kx[dx + 1] * sy);
                const int lx = px - ox, ly = py - oy;
                if (use_lds && (unsigned)lx < (unsigned)ww && (unsigned)ly < (unsigned)wh) atomicAdd(&win[ly * ww + lx], q);
                else atomicAdd(img + (size_t)py * g.W + px, q);
            }
        }
    }
    if (use_lds) {                                  // flush: one global atomic per touched window pixel
        __syncthreads();
        for (int k = threadIdx.x; k < ww * wh; k += NT) {
            const unsigned long long q = win[k];
            if (q) atomicAdd(img + (size_t)(oy + k / ww) * g.W + ox + k % ww, q);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// image passes: grid (P, R, B), workgroup p covers pixels [p * F64_PIX, (p + 1) * F64_PIX) of image (b, r)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k64_img_a(Geom g, const int* __restrict__ ishift, unsigned long long* __restrict__ acc,
                                                 double* __restrict__ iwe, double* __restrict__ partA)
{
    __shared__ double scratch[NWAVE];
    const int p = blockIdx.x, r = blockIdx.y, b = blockIdx.z, P = gridDim.x;
    if (!win_active(g, b)) return;
    const int HW = g.H * g.W;
    const size_t base = ((size_t)b * g.R + r) * HW;
    const double inv = ldexp(1.0, -ishift[b]);
    double mn = INFINITY, mx = -INFINITY, s = 0.0;
    const int hi = min((p + 1) * F64_PIX, HW);
    for (int i = p * F64_PIX + threadIdx.x; i < hi; i += NT) {
        const unsigned long long q = acc[base + i];
        if (q) acc[base + i] = 0ull;
        const double v = (double)q * inv;
        iwe[base + i] = v;
        mn = fmin(mn, v); mx = fmax(mx, v); s += v;
    }
    mn = block_reduce64(mn, scratch, OpMin());
    mx = block_reduce64(mx, scratch, OpMax());
    s = block_reduce64(s, scratch, OpSum());
    if (threadIdx.x == 0) {
        double* o = partA + (((size_t)b * g.R + r) * P + p) * F64_PA;
        o[0] = mn; o[1] = mx; o[2] = s;
    }
}

// m, M, sum I of one image from k64_img_a's partials (every thread gets them; fixed order)
__device__ __forceinline__ void reduce_a64(const double* __restrict__ partA, int P, double* scratch, double& m, double& M, double& s) {
    double mn = INFINITY, mx = -INFINITY, sm = 0.0;
    for (int k = threadIdx.x; k < P; k += NT) { mn = fmin(mn, partA[k * F64_PA]); mx = fmax(mx, partA[k * F64_PA + 1]); sm += partA[k * F64_PA + 2]; }
    m = block_reduce64(mn, scratch, OpMin());
    M = block_reduce64(mx, scratch, OpMax());
    s = block_reduce64(sm, scratch, OpSum());
}

// v = conv(gx_n, K) + conv(gy_n, K) at (y, x): the divergence image of event_collapse_objectives.py:10-20 on the normalised IWE
template <typename A>
__device__ __forceinline__ double div_at64(const A& nrm, int y, int x, int H, int W) {
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
        for (int c = -1; c <= 1; ++c) {
            const int qy = y + a, qx = x + c;
            if (qy < 0 || qy >= H || qx < 0 || qx >= W || (a == 0 && c == 0)) continue;
            double gx, gy;
            scharr64(nrm, qy, qx, gx, gy);
            sx += DIVK64[a + 1][c + 1] * gx;
            sy += DIVK64[a + 1][c + 1] * gy;
        }
    return sx + sy;
}

__global__ __launch_bounds__(NT) void k64_img_b(Geom g, const double* __restrict__ iwe, const double* __restrict__ edges,
                                                 const double* __restrict__ partA, double* __restrict__ partB, int want_div,
                                                 double* __restrict__ sgn /* (B,R,H,W) sign of the divergence image, or nullptr */)
{
    __shared__ double scratch[NWAVE];
    const int p = blockIdx.x, r = blockIdx.y, b = blockIdx.z, P = gridDim.x;
    if (!win_active(g, b)) return;
    const int H = g.H, W = g.W, HW = H * W;
    const size_t base = ((size_t)b * g.R + r) * HW;
    double m, M, sI;
    reduce_a64(partA + ((size_t)b * g.R + r) * P * F64_PA, P, scratch, m, M, sI);
    const double mean = sI / (double)HW, D = M - m + EPSN;
    const double* __restrict__ I = iwe + base;
    const double* __restrict__ E = edges + base;
    auto img = [&](int y, int x) -> double { return (y < 0 || y >= H || x < 0 || x >= W) ? 0.0 : I[y * W + x]; };
    auto nrm = [&](int y, int x) -> double { return (y < 0 || y >= H || x < 0 || x >= W) ? 0.0 : (I[y * W + x] - m) / D; };
    double cm = 0.0, cM = 0.0, sv = 0.0, sg = 0.0, se = 0.0, sd = 0.0;
    const int hi = min((p + 1) * F64_PIX, HW);
    for (int i = p * F64_PIX + threadIdx.x; i < hi; i += NT) {
        const int y = i / W, x = i - y * W;
        const double v = I[i];
        cm += (v == m) ? 1.0 : 0.0;
        cM += (v == M) ? 1.0 : 0.0;
        const double dv = v - mean;
        sv += dv * dv;
        double gx, gy;
        scharr64(img, y, x, gx, gy);
        sg += gx * gx + gy * gy;
        const double e = E[i] - (v - m) / D;
        se += e * e;
        if (want_div) {
            const double dvg = div_at64(nrm, y, x, H, W);
            sd += fabs(dvg);
            if (sgn) sgn[base + i] = (dvg > 0.0) ? 1.0 : ((dvg < 0.0) ? -1.0 : 0.0);
        }
    }
    double vals[F64_PB] = {cm, cM, sv, sg, se, sd};
    double* o = partB + (((size_t)b * g.R + r) * P + p) * F64_PB;
#pragma unroll
    for (int k = 0; k < F64_PB; ++k) {
        const double t = block_reduce64(vals[k], scratch, OpSum());
        if (threadIdx.x == 0) o[k] = t;
    }
}

// grid (R, B): the image scalars, every sum in index order
__global__ __launch_bounds__(NT) void k64_scal(Geom g, int P, const double* __restrict__ partA, const double* __restrict__ partB,
                                                F64Scal* __restrict__ scal)
{
    __shared__ double scratch[NWAVE];
    const int r = blockIdx.x, b = blockIdx.y;
    if (!win_active(g, b)) return;
    const double HW = (double)g.H * g.W;
    const size_t img = (size_t)b * g.R + r;
    double m, M, sI;
    reduce_a64(partA + img * P * F64_PA, P, scratch, m, M, sI);
    double acc[F64_PB];
#pragma unroll
    for (int k = 0; k < F64_PB; ++k) {
        double s = 0.0;
        for (int q = threadIdx.x; q < P; q += NT) s += partB[(img * P + q) * F64_PB + k];
        acc[k] = block_reduce64(s, scratch, OpSum());
    }
    if (threadIdx.x == 0) {
        F64Scal o;
        o.m = m; o.M = M; o.D = M - m + EPSN; o.cm = acc[0]; o.cM = acc[1]; o.mean = sI / HW;
        o.var = acc[2] / HW; o.g2 = acc[3] / HW; o.mse = acc[4] / HW; o.div = acc[5] / HW;
        scal[img] = o;
    }
}

// dL/dIWE without the tie terms (oracle loss_and_grad): G0 = a_r dc/dI + Gn / D, Gn = b_r (2/HW)(E - n) [+ e_r d|div n|/dn];
// partials of sum Gn (n - 1) and sum Gn n for the tie terms
__global__ __launch_bounds__(NT) void k64_grad1(Geom g, EvalParams ep, const double* __restrict__ iwe, const double* __restrict__ edges,
                                                 const F64Scal* __restrict__ scal, const WinConst* __restrict__ wcs,
                                                 const double* __restrict__ sgn /* or nullptr: delta = 0 */, double* __restrict__ G,
                                                 double* __restrict__ partC)
{
    __shared__ double scratch[NWAVE];
    const int p = blockIdx.x, r = blockIdx.y, b = blockIdx.z, P = gridDim.x;
    if (!win_active(g, b)) return;
    const int H = g.H, W = g.W, HW = H * W;
    const double HWd = (double)HW, Rd = (double)g.R;
    const size_t base = ((size_t)b * g.R + r) * HW;
    const F64Scal s = scal[(size_t)b * g.R + r];
    const WinConst& wc = wcs[b];
    const bool var_kind = ep.contrast_kind == 1;
    const double c0 = var_kind ? wc.c0_var : wc.c0_gradmag;
    const LossWeights lw = loss_weights(ep, wc.mrw[r], Rd, c0, wc.zc[r], wc.d0, 1.0);
    const double a_r = lw.a, b_r = lw.b, e_r = lw.e;
    const double* __restrict__ I = iwe + base;
    const double* __restrict__ E = edges + base;
    const double* __restrict__ S = sgn ? sgn + base : nullptr;
    auto inside = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W; };
    auto img = [&](int y, int x) -> double { return inside(y, x) ? I[y * W + x] : 0.0; };
    auto gxf = [&](int y, int x) -> double { if (!inside(y, x)) return 0.0; double gx, gy; scharr64(img, y, x, gx, gy); return gx; };
    auto gyf = [&](int y, int x) -> double { if (!inside(y, x)) return 0.0; double gx, gy; scharr64(img, y, x, gx, gy); return gy; };
    // t = conv(sign(v) / HW, K) (the kernel is symmetric: its adjoint is itself), zero outside
    auto tf = [&](int y, int x) -> double {
        if (!inside(y, x)) return 0.0;
        double t = 0.0;
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
            for (int c = -1; c <= 1; ++c)
                if (!(a == 0 && c == 0) && inside(y + a, x + c)) t += DIVK64[a + 1][c + 1] * (S[(y + a) * W + x + c] / HWd);
        return t;
    };
    double sa = 0.0, sb = 0.0;
    const int hi = min((p + 1) * F64_PIX, HW);
    for (int i = p * F64_PIX + threadIdx.x; i < hi; i += NT) {
        const int y = i / W, x = i - y * W;
        const double v = I[i];
        const double n = (v - s.m) / s.D;
        double Gn = b_r * (2.0 / HWd) * (E[i] - n);
        if (S) {
            // adjoint of a Scharr stencil = minus the stencil itself (Scharr kernels are antisymmetric)
            double tx, ty;
            scharr64(tf, y, x, tx, ty);
            Gn += e_r * (-(tx + ty));
        }
        double dc;
        if (var_kind) {
            dc = (2.0 / HWd) * (v - s.mean);
        } else {
            double ux, uy, wx, wy;
            scharr64(gxf, y, x, ux, uy);       // Scharr-x of the gx image
            scharr64(gyf, y, x, wx, wy);       // Scharr-y of the gy image
            (void)uy; (void)wx;
            dc = -(2.0 / HWd) * (ux + wy);
        }
        G[base + i] = a_r * dc + Gn / s.D;
        sa += Gn * (n - 1.0);
        sb += Gn * n;
    }
    sa = block_reduce64(sa, scratch, OpSum());
    sb = block_reduce64(sb, scratch, OpSum());
    if (threadIdx.x == 0) {
        double* o = partC + (((size_t)b * g.R + r) * P + p) * F64_PC;
        o[0] = sa; o[1] = sb;
    }
}

// the tie terms of n = (I - m) / (M - m + eps) (S4: the cotangent of min / max shared equally among the tied pixels); max |G| per window
__global__ __launch_bounds__(NT) void k64_grad2(Geom g, const double* __restrict__ iwe, const F64Scal* __restrict__ scal,
                                                 const double* __restrict__ partC, double* __restrict__ G,
                                                 unsigned long long* __restrict__ gmax, unsigned* __restrict__ bad)
{
    __shared__ double scratch[NWAVE];
    const int p = blockIdx.x, r = blockIdx.y, b = blockIdx.z, P = gridDim.x;
    if (!win_active(g, b)) return;
    const int HW = g.H * g.W;
    const size_t img = (size_t)b * g.R + r, base = img * HW;
    const F64Scal s = scal[img];
    double sa = 0.0, sb = 0.0;
    for (int k = threadIdx.x; k < P; k += NT) { sa += partC[(img * P + k) * F64_PC]; sb += partC[(img * P + k) * F64_PC + 1]; }
    sa = block_reduce64(sa, scratch, OpSum());
    sb = block_reduce64(sb, scratch, OpSum());
    const double dm = sa / s.D, dM = -sb / s.D;
    double gm = 0.0, nf = 0.0;
    const int hi = min((p + 1) * F64_PIX, HW);
    for (int i = p * F64_PIX + threadIdx.x; i < hi; i += NT) {
        const double v = iwe[base + i];
        double Gv = G[base + i];
        if (v == s.m) Gv += dm / s.cm;
        if (v == s.M) Gv += dM / s.cM;
        G[base + i] = Gv;
        if (fabs(Gv) <= DBL_MAX) gm = fmax(gm, fabs(Gv)); else nf = 1.0;
    }
    gm = block_reduce64(gm, scratch, OpMax());
    nf = block_reduce64(nf, scratch, OpMax());
    if (threadIdx.x == 0 && gm > 0.0) atomicMax(gmax + b, (unsigned long long)__double_as_longlong(gm));   // non-negative: bit order = value order
    if (threadIdx.x == 0 && nf != 0.0) atomicOr(bad + b, 1u);      // a NaN / Inf in dL/dIWE: the window's gradient is NaN (k64_gfin)
}

// Scale of the 128-bit gradient accumulator of window b: 2^S with bound * 2^S < 2^116, bound >= the sum of the magnitudes of everything
// added to one pixel (events * refs * max|t - tau| * max|G| * sum_taps k |q|, the last < 9 * 0.16 * 1.5 < 3).  The high word then stays
// below 2^52 (exact in fp64) and one event's contribution is resolved to 2^-116 of the bound.
__device__ __forceinline__ int gshift64(const WinConst& wc, unsigned long long gmax_bits, int R) {
    const double gm = __longlong_as_double((long long)gmax_bits);
    const double bound = wc.nev * (double)R * wc.dtmax * gm * 3.0;
    if (!(bound > 0.0) || !(bound < 1e300)) return 0;
    return 115 - ilogb(bound);
}

// (lo, hi) added modulo 2^128 into p[0] / p[1] (LDS or global)
__device__ __forceinline__ void add_u128(unsigned long long* p, unsigned long long lo, unsigned long long hi) {
    if (lo) {
        const unsigned long long old = atomicAdd(p, lo);
        if (old + lo < old) ++hi;                // carry out of the low word
    }
    if (hi) atomicAdd(p + 1, hi);
}
// two's-complement 128-bit add of an integer-valued double (|x| < 2^116) into p[0] (low) / p[1] (high): integer adds commute.
// false for a value the accumulator cannot hold (NaN, Inf, beyond the bound): the caller flags the window
__device__ __forceinline__ bool add_i128(unsigned long long* p, double x) {
    if (x == 0.0) return true;
    if (!(fabs(x) < 0x1p116)) return false;
    const double ax = fabs(x);
    const double hd = floor(ax * 0x1p-64);
    const double ld = ax - hd * 0x1p64;          // exact: a multiple of ulp(ax) below 2^64
    unsigned long long lo = (unsigned long long)ld, hi = (unsigned long long)hd;
    if (x < 0.0) { lo = ~lo + 1ull; hi = ~hi + (lo == 0ull ? 1ull : 0ull); }
    add_u128(p, lo, hi);
    return true;
}
__device__ __forceinline__ double i128_to_double(unsigned long long lo, unsigned long long hi) {
    const bool neg = (long long)hi < 0;
    if (neg) { lo = ~lo + 1ull; hi = ~hi + (lo == 0ull ? 1ull : 0ull); }
    const double v = (double)hi * 0x1p64 + (double)lo;
    return neg ? -v : v;
}

// ------------------------------------------------------------------------------------------------
// k64_gather: one workgroup per segment of the gather's list; per event sum_r -dt_r * sum_taps G k q in fp64, one i128 add per component
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k64_gather(Geom g, int n_items, const Item* __restrict__ items, const uint32_t* __restrict__ ev_xy,
                                                  const double* __restrict__ ev_t, const double* __restrict__ Theta,
                                                  const double* __restrict__ edge_ts, const double* __restrict__ G,
                                                  const WinConst* __restrict__ wcs, const unsigned long long* __restrict__ gmax,
                                                  unsigned long long* __restrict__ gacc /* (B,H,W,2) x 2 words */, unsigned* __restrict__ bad)
{
    // the segment's events all come from one 32x32 source tile: their i128 sums are kept per source pixel and component in LDS
    // (32 KiB) and flushed once per segment; an event outside the tile (none, by construction of the segments) would go to HBM directly
    __shared__ unsigned long long lacc[TS * TS * 2 * 2];
    if ((int)blockIdx.x >= n_items) return;
    const Item it = items[blockIdx.x];
    const int b = it.win;
    if (!win_active(g, b)) return;
    const int tx0 = (it.tile % g.tilesX) * TS, ty0 = (it.tile / g.tilesX) * TS;
    for (int k = threadIdx.x; k < TS * TS * 4; k += NT) lacc[k] = 0ull;
    __syncthreads();
    bool flag = false;
    const int H = g.H, W = g.W, R = g.R;
    const size_t HW = (size_t)H * W;
    const double scale = ldexp(1.0, gshift64(wcs[b], gmax[b], R));
    const double* __restrict__ Th = Theta + (size_t)b * HW * 2;
    const double* __restrict__ Gb = G + (size_t)b * R * HW;
    for (int i = threadIdx.x; i < it.count; i += NT) {
        const uint32_t xy = ev_xy[it.begin + i];
        const double t = ev_t[it.begin + i];
        const int x = xy & 0xffff, y = xy >> 16;
        const double2 v = *reinterpret_cast<const double2*>(Th + ((size_t)y * W + x) * 2);
        double cx = 0.0, cy = 0.0;
        for (int r = 0; r < R; ++r) {
            const double dt = t - edge_ts[b * R + r];
            int irx, iry; double fx, fy;
            warp_axis64(x, v.x, dt, irx, fx);
            warp_axis64(y, v.y, dt, iry, fy);
            const int ix = clamp_far(irx), iy = clamp_far(iry);
            double kx[3], ky[3];
            taps64(fx, kx);
            taps64(fy, ky);
            const double* __restrict__ Gr = Gb + (size_t)r * HW;
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int py = wrap_drop(iy + dy, H);
                if (py < 0) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int px = wrap_drop(ix + dx, W);
                    if (px < 0) continue;
                    const double gk = Gr[(size_t)py * W + px] * (kx[dx + 1] * ky[dy + 1] * INV_2PI_D);
                    sx += gk * ((double)dx - fx);
                    sy += gk * ((double)dy - fy);
                }
            }
            cx += -dt * sx;
            cy += -dt * sy;
        }
        const int lx = x - tx0, ly = y - ty0;
        unsigned long long* a = ((unsigned)lx < (unsigned)TS && (unsigned)ly < (unsigned)TS) ? lacc + (ly * TS + lx) * 4
                                                                                            : gacc + (((size_t)b * HW + (size_t)y * W + x) * 2) * 2;
        const bool okx = add_i128(a, rint(cx * scale));
        const bool oky = add_i128(a + 2, rint(cy * scale));
        flag = flag || !(okx && oky);
    }
    if (flag) atomicOr(bad + b, 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < TS * TS * 2; k += NT) {          // flush: (pixel, component) k, both words
        const int pix = k >> 1, y = ty0 + pix / TS, x = tx0 + pix % TS;
        const unsigned long long lo = lacc[2 * k], hi = lacc[2 * k + 1];
        if ((lo | hi) && y < H && x < W) add_u128(gacc + (((size_t)b * HW + (size_t)y * W + x) * 2 + (k & 1)) * 2, lo, hi);
    }
}

// accumulator -> dL/dTheta (fp64) + tv_scale * k_tv's gradient image; clears the accumulator.  grid (nblk, B), grid-stride.
__global__ __launch_bounds__(NT) void k64_gfin(Geom g, int use_tv, double gamma, const double* __restrict__ tvparts,
                                                const double* __restrict__ tvg, const WinConst* __restrict__ wcs,
                                                const unsigned long long* __restrict__ gmax, unsigned long long* __restrict__ gacc,
                                                const unsigned* __restrict__ bad, double* __restrict__ gTh)
{
    __shared__ double scratch[NWAVE];
    const int b = blockIdx.y;
    if (!win_active(g, b)) return;
    const size_t n = (size_t)g.H * g.W * 2;
    double tvs = 0.0;
    if (use_tv) {              // gamma * 0.25 / (count + eps), regularizers.py:26-38 (the count from k_tv's partials, index order)
        double nz = 0.0;
        for (int k = threadIdx.x; k < g.ntiles; k += NT) nz += tvparts[((size_t)b * g.ntiles + k) * 3 + 1];
        nz = block_reduce64(nz, scratch, OpSum());
        tvs = tv_grad_scale(gamma, nz);
    }
    const double inv = ldexp(1.0, -gshift64(wcs[b], gmax[b], g.R));
    const bool nonfinite = bad[b] != 0u;           // a NaN / Inf the integer accumulator could not carry: the whole window's gradient is NaN
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        unsigned long long* a = gacc + ((size_t)b * n + i) * 2;
        const unsigned long long lo = a[0], hi = a[1];
        if (lo | hi) { a[0] = 0ull; a[1] = 0ull; }
        double v = i128_to_double(lo, hi) * inv;
        if (use_tv) v += tvs * tvg[(size_t)b * n + i];
        if (nonfinite) v = NAN;
        gTh[(size_t)b * n + i] = v;
    }
}

// adjoint of Theta = A_H theta A_W^T, per component: T[b,y,j,c] = sum_x AW[x,j] gTh[b,y,x,c], then out[b,i,j,c] = sum_y AH[y,i] T[b,y,j,c]
__global__ __launch_bounds__(NT) void k64_proj_w(Geom g, int w, const double* __restrict__ AW, const double* __restrict__ gTh,
                                                  double* __restrict__ T)
{
    const size_t n = (size_t)g.B * g.H * w * 2;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < n; k += (size_t)gridDim.x * NT) {
        const int c = (int)(k & 1);
        const size_t q = k >> 1;
        const int j = (int)(q % w);
        const size_t by = q / w;                        // b * H + y
        const int b = (int)(by / g.H);
        if (!win_active(g, b)) continue;
        const double* __restrict__ row = gTh + by * g.W * 2 + c;
        double s = 0.0;
        for (int x = 0; x < g.W; ++x) s += AW[(size_t)x * w + j] * row[(size_t)x * 2];
        T[k] = s;
    }
}
__global__ __launch_bounds__(NT) void k64_proj_h(Geom g, int h, int w, const double* __restrict__ AH, const double* __restrict__ T,
                                                  double* __restrict__ out)
{
    const size_t n = (size_t)g.B * h * w * 2;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < n; k += (size_t)gridDim.x * NT) {
        const int c = (int)(k & 1);
        const size_t q = k >> 1;
        const int j = (int)(q % w);
        const size_t bi = q / w;                        // b * h + i
        const int i = (int)(bi % h), b = (int)(bi / h);
        if (!win_active(g, b)) continue;
        const double* __restrict__ col = T + ((size_t)b * g.H * w + j) * 2 + c;
        double s = 0.0;
        for (int y = 0; y < g.H; ++y) s += AH[(size_t)y * h + i] * col[(size_t)y * w * 2];
        out[k] = s;
    }
}

// The same adjoint rows first, for a grid finer than the sensor in x (w > W, so h < H since h * w <= H * W): the intermediate
// (B,h,W,2) fits T's (B,H,W,2) capacity where k64_proj_w's (B,H,w,2) would overrun it.
__global__ __launch_bounds__(NT) void k64_proj_h_first(Geom g, int h, const double* __restrict__ AH, const double* __restrict__ gTh,
                                                        double* __restrict__ T)
{
    const size_t n = (size_t)g.B * h * g.W * 2;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < n; k += (size_t)gridDim.x * NT) {
        const int c = (int)(k & 1);
        const size_t q = k >> 1;
        const int x = (int)(q % g.W);
        const size_t bi = q / g.W;                      // b * h + i
        const int i = (int)(bi % h), b = (int)(bi / h);
        if (!win_active(g, b)) continue;
        const double* __restrict__ col = gTh + ((size_t)b * g.H * g.W + x) * 2 + c;
        double s = 0.0;
        for (int y = 0; y < g.H; ++y) s += AH[(size_t)y * h + i] * col[(size_t)y * g.W * 2];
        T[k] = s;
    }
}
__global__ __launch_bounds__(NT) void k64_proj_w_second(Geom g, int h, int w, const double* __restrict__ AW, const double* __restrict__ T,
                                                         double* __restrict__ out)
{
    const size_t n = (size_t)g.B * h * w * 2;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < n; k += (size_t)gridDim.x * NT) {
        const int c = (int)(k & 1);
        const size_t q = k >> 1;
        const int j = (int)(q % w);
        const size_t bi = q / w;                        // b * h + i
        const int b = (int)(bi / h);
        if (!win_active(g, b)) continue;
        const double* __restrict__ row = T + bi * g.W * 2 + c;
        double s = 0.0;
        for (int x = 0; x < g.W; ++x) s += AW[(size_t)x * w + j] * row[(size_t)x * 2];
        out[k] = s;
    }
}

}  // namespace eincm
