// eincm_theta_advect.hip.h — a solved theta carried along its own flow to the next window: the field that
// belongs at a pixel of the next window is the flow of whatever moved into it.  For a batch of n fields, each with its own tau and
// gain, in four launches:
//
//   k_ta_splat        grid (pixel blocks, n), one thread per SOURCE pixel p = (x, y): forms Theta(p) (theta itself at sensor size,
//                     else the unfused tap sums of k_flow_encode / k_flow_error: ta_expand), lands it at q = p + Theta tau
//                     (ta_landing) and adds (w, w Qx, w Qy) to the three i64 planes Wacc | Uacc | Vacc at the up to four pixels
//                     around q, w = ta_weight, Q = ta_quantise(Theta).  Taps outside the sensor and taps of weight 0 add nothing.
//                     64-bit integer atomics: the sums do not depend on the order of arrival, so every run leaves the same bytes;
//                     eincm_theta_advect.h proves that no accepted input overflows them.
//   k_ta_resolve      one thread per pixel: coverage c = Wacc 2^-2K; where c >= min_coverage the difference from the pixel's own
//                     QUANTISED value D = Uacc / Wacc 2^-S - Q(Theta(p)) 2^-S (IEEE division, every step unfused), elsewhere the
//                     fill (0, or -Theta(p)).  Writes what is asked for: D (the reducer's input), the dense field Theta + D, the
//                     coverage as float32, and for a dense theta the result gain (theta + D) itself.
//   k_ta_reduce_cols  S[b][y][j] = sum over the non-zero run of row j of resample_matrix(W -> w) of  weight * D[b][y][x], in run
//                     order from +0.0, every product rounded before it is added
//   k_ta_reduce_rows  R[b][i][j] = the same over row i of resample_matrix(H -> h) of weight * S[b][y][j]; out = gain (theta + R)
// The two reducers walk columns, then rows, as the expansion does; each output is one thread's ordered fp64 chain, so there is no
// atomic on any float and nothing depends on the launch shape.
//
// Atomics (the HIP guide's Guideline 12 and scatter-add appendix): a smooth flow moves neighbouring sources to neighbouring pixels,
// so a wave's 64 adds into one plane mostly fall in one or two rows, 512 contiguous bytes each: the shape the memory side serves at
// its full rate.  Per 480x640 field that is 4 taps x 3 planes x 8 B x 307200 = 29.5 MB of added bytes.  The rate of 64-bit integer
// atomics is not among the measured ones (float and packed bf16 are); profiles/theta_advect.md records what this kernel reaches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_theta_advect.h"

namespace eincm {

// the tap tables of the (h, w) -> (H, W) expansion, as k_flow_error reads them (build_taps)
struct TaTaps {
    const int32_t* rlo; const int32_t* rcnt; const double* rwt; int rstride;
    const int32_t* clo; const int32_t* ccnt; const double* cwt; int cstride;
};

// Theta at sensor pixel (x, y) of field th (h, w, 2): k_flow_error's arithmetic, term for term
__device__ __forceinline__ double2 ta_expand(const double2* __restrict__ th, int w, int full, int W, int x, int y, const TaTaps& t) {
#pragma clang fp contract(off)
    if (full) return th[(int64_t)y * W + x];
    const int i0 = t.rlo[y], ni = t.rcnt[y], j0 = t.clo[x], nj = t.ccnt[x];
    double vx = 0.0, vy = 0.0;
    for (int i = 0; i < ni; ++i) {
        double sx = 0.0, sy = 0.0;
        for (int j = 0; j < nj; ++j) {
            const double2 v = th[(int64_t)(i0 + i) * w + (j0 + j)];
            const double bw = t.cwt[(int64_t)x * t.cstride + j];
            sx += bw * v.x;
            sy += bw * v.y;
        }
        const double aw = t.rwt[(int64_t)y * t.rstride + i];
        vx += aw * sx;
        vy += aw * sy;
    }
    return make_double2(vx, vy);
}

// i64 += through the u64 atomic (two's complement: the same bits)
__device__ __forceinline__ void ta_add(int64_t* p, int64_t v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// grid (ceil(H W / NT), n).  theta (n, h, w, 2); tau (n); acc (n, 3, H W) i64, zero on entry: the planes Wacc | Uacc | Vacc.
__global__ __launch_bounds__(NT) void k_ta_splat(int H, int W, int h, int w, int full, const double2* __restrict__ theta, TaTaps taps,
                                                 const double* __restrict__ tau, int64_t* __restrict__ acc) {
    const int npix = H * W;                        // <= 2^21 (ta_check)
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    const int b = blockIdx.y;
    const int y = p / W, x = p - y * W;
    const double2 v = ta_expand(theta + (int64_t)b * h * w, w, full, W, x, y, taps);
    TaLanding l;
    if (!ta_landing(x, y, v.x, v.y, tau[b], H, W, l)) return;
    const int64_t qx = ta_quantise(v.x), qy = ta_quantise(v.y);
    int64_t* const wacc = acc + (int64_t)b * 3 * npix;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int tx = l.x0 + dx, ty = l.y0 + dy;
            const int64_t wt = ta_weight(l, dx, dy);
            if (tx < 0 || tx >= W || ty < 0 || ty >= H || wt == 0) continue;
            const int64_t at = (int64_t)ty * W + tx;               // in [0, npix): both coordinates were just checked
            ta_add(wacc + at, wt);
            ta_add(wacc + npix + at, wt * qx);
            ta_add(wacc + 2 * (int64_t)npix + at, wt * qy);
        }
    }
}

// grid (ceil(H W / NT), n).  Every output is NULL where it is not wanted: D (n, H W) double2, dense (n, H W) double2, coverage
// (n, H W) float, out (n, H W) double2 (a dense theta only: the call's result).
__global__ __launch_bounds__(NT) void k_ta_resolve(int H, int W, int h, int w, int full, const double2* __restrict__ theta, TaTaps taps,
                                                   const double* __restrict__ gain, const int64_t* __restrict__ acc, int fill_zero,
                                                   double min_coverage, double2* __restrict__ D, double2* __restrict__ dense,
                                                   float* __restrict__ coverage, double2* __restrict__ out) {
#pragma clang fp contract(off)
    const int npix = H * W;
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    const int b = blockIdx.y;
    const int y = p / W, x = p - y * W;
    const double2 v = ta_expand(theta + (int64_t)b * h * w, w, full, W, x, y, taps);
    const int64_t* const wacc = acc + (int64_t)b * 3 * npix;
    const int64_t sw = wacc[p];
    const double c = (double)sw * TA_COVERAGE_STEP;
    double dx, dy;
    if (c >= min_coverage) {
        const double dw = (double)sw;
        dx = __ddiv_rn((double)wacc[npix + p], dw) * TA_VALUE_STEP - ta_dequantise(ta_quantise(v.x));
        dy = __ddiv_rn((double)wacc[2 * (int64_t)npix + p], dw) * TA_VALUE_STEP - ta_dequantise(ta_quantise(v.y));
    } else {
        dx = fill_zero ? -v.x : 0.0;
        dy = fill_zero ? -v.y : 0.0;
    }
    const int64_t at = (int64_t)b * npix + p;
    const double rx = v.x + dx, ry = v.y + dy;
    if (D) D[at] = make_double2(dx, dy);
    if (dense) dense[at] = make_double2(rx, ry);
    if (coverage) coverage[at] = (float)c;
    if (out) { const double g = gain[b]; out[at] = make_double2(g * rx, g * ry); }
}

// grid (ceil(H w / NT), n): one thread per (sensor row y, coarse column j).  clo / ccnt / cwt: the runs of resample_matrix(W -> w).
__global__ __launch_bounds__(NT) void k_ta_reduce_cols(int H, int W, int w, const double2* __restrict__ D, const int32_t* __restrict__ clo,
                                                       const int32_t* __restrict__ ccnt, const double* __restrict__ cwt, int cstride,
                                                       double2* __restrict__ S) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k >= (int64_t)H * w) return;
    const int b = blockIdx.y;
    const int y = (int)(k / w), j = (int)(k - (int64_t)y * w);
    const double2* row = D + ((int64_t)b * H + y) * W;
    const int x0 = clo[j], nx = ccnt[j];
    double sx = 0.0, sy = 0.0;
    for (int t = 0; t < nx; ++t) {
        const double2 d = row[x0 + t];
        const double bw = cwt[(int64_t)j * cstride + t];
        sx += bw * d.x;
        sy += bw * d.y;
    }
    S[((int64_t)b * H + y) * w + j] = make_double2(sx, sy);
}

// grid (ceil(h w / NT), n): one thread per coarse cell (i, j).  rlo / rcnt / rwt: the runs of resample_matrix(H -> h).
__global__ __launch_bounds__(NT) void k_ta_reduce_rows(int H, int h, int w, const double2* __restrict__ S, const int32_t* __restrict__ rlo,
                                                       const int32_t* __restrict__ rcnt, const double* __restrict__ rwt, int rstride,
                                                       const double2* __restrict__ theta, const double* __restrict__ gain,
                                                       double2* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t k = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (k >= (int64_t)h * w) return;
    const int b = blockIdx.y;
    const int i = (int)(k / w), j = (int)(k - (int64_t)i * w);
    const int y0 = rlo[i], ny = rcnt[i];
    double vx = 0.0, vy = 0.0;
    for (int t = 0; t < ny; ++t) {
        const double2 s = S[((int64_t)b * H + (y0 + t)) * w + j];
        const double aw = rwt[(int64_t)i * rstride + t];
        vx += aw * s.x;
        vy += aw * s.y;
    }
    const int64_t at = (int64_t)b * h * w + k;
    const double2 th = theta[at];
    const double g = gain[b];
    out[at] = make_double2(g * (th.x + vx), g * (th.y + vy));
}

}  // namespace eincm
