// eincm_motion.hip.h — parametric motion-field models as a theta mode: the map from a window's polynomial
// coefficients q = M c (host, eincm_motion.h) to the dense field Theta, and the adjoint of that map on the dense gradient.
//
//   k_motion_expand   grid (ceil(npix / NT), B): one pixel per thread.  u = (x - cx) / s, v = (y - cy) / s,
//                     Theta_x = ((((q0 + q1 u) + q2 v) + q3 (u u)) + q4 (u v)) + q5 (v v), Theta_y likewise from q6..q11: correctly
//                     rounded division, every product rounded, the sums left to right (fp contract off), so the numpy witness
//                     (motion.py) gives the same bits.  q rides in the arguments (up to MOTION_ARG_WINDOWS windows) or is read from
//                     pinned host memory.  The workgroups of a window outside the mask leave at once.
//   k_motion_moments  grid (MOTION_PARTS, B): thread t of workgroup g owns the pixels p = g NT + t + k (MOTION_PARTS NT), k ascending,
//                     and adds m_j dL/dTheta_x (j < 6) and m_j dL/dTheta_y to its twelve float64 chains.  The workgroup reduces each
//                     with block_sum (lanes by the fixed tree, waves in index order) and thread 0 STORES the twelve partials in slot
//                     (window, g) of pinned host memory; a workgroup whose range is empty stores zeros.  The host adds the partials in
//                     index order (motion_sum_partials).  No atomic on any float.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_motion.h"

namespace eincm {

struct MotionGeom {
    int H, W, B;
    unsigned long long wmask;          // as Geom::wmask: bit b clear = window b sits this call out (b < 64)
    double cx, cy, s;
};

__device__ __forceinline__ bool motion_active(const MotionGeom& g, int b) { return b >= 64 || ((g.wmask >> b) & 1ull) != 0ull; }

// the monomials of pixel p (m[0] = 1 is implied), by the helpers the event kernels' THETA_POLY mode shares (eincm_kernels.hip.h)
__device__ __forceinline__ void motion_monomials(const MotionGeom& g, int p, double& u, double& v, double& uu, double& uv, double& vv) {
#pragma clang fp contract(off)
    const int y = p / g.W, x = p - y * g.W;
    u = motion_coord(x, g.cx, g.s);
    v = motion_coord(y, g.cy, g.s);
    motion_products(u, v, uu, uv, vv);
}

// Theta (B, H, W) double2.  use_arg: q of window b is qarg.q[12 b ..], else q_mem[12 b ..].
__global__ __launch_bounds__(NT) void k_motion_expand(MotionGeom g, int use_arg, MotionQArg qarg, const double* __restrict__ q_mem,
                                                      double2* __restrict__ Theta) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    if (!motion_active(g, b)) return;
    const int npix = g.H * g.W;                    // H, W <= 32767 and the dense theta fits memory: pixel indices fit 32 bits
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    double q[MOTION_NQ];
#pragma unroll
    for (int j = 0; j < MOTION_NQ; ++j) q[j] = use_arg ? qarg.q[b * MOTION_NQ + j] : q_mem[(int64_t)b * MOTION_NQ + j];
    double u, v, uu, uv, vv;
    motion_monomials(g, p, u, v, uu, uv, vv);
    Theta[(int64_t)b * npix + p] = motion_poly(q, u, v, uu, uv, vv);       // (the expression the event kernels' THETA_POLY mode evaluates)
}

// grad (B, H, W) double2: the dense dL/dTheta of the evaluation.  parts (B, MOTION_PARTS, 12) in pinned host memory.
__global__ __launch_bounds__(NT) void k_motion_moments(MotionGeom g, const double2* __restrict__ grad, double* __restrict__ parts) {
#pragma clang fp contract(off)
    __shared__ double scratch[NWAVE];
    const int b = blockIdx.y;
    if (!motion_active(g, b)) return;
    const int npix = g.H * g.W;
    const double2* g_b = grad + (int64_t)b * npix;
    double a[MOTION_NQ];
#pragma unroll
    for (int j = 0; j < MOTION_NQ; ++j) a[j] = 0.0;
    for (int p = (int)(blockIdx.x * NT + threadIdx.x); p < npix; p += MOTION_PARTS * NT) {
        double u, v, uu, uv, vv;
        motion_monomials(g, p, u, v, uu, uv, vv);
        const double2 d = g_b[p];
        a[0] += d.x; a[1] += u * d.x; a[2] += v * d.x; a[3] += uu * d.x; a[4] += uv * d.x; a[5] += vv * d.x;
        a[6] += d.y; a[7] += u * d.y; a[8] += v * d.y; a[9] += uu * d.y; a[10] += uv * d.y; a[11] += vv * d.y;
    }
#pragma unroll
    for (int j = 0; j < MOTION_NQ; ++j) a[j] = block_sum(a[j], scratch);
    if (threadIdx.x == 0) {
        double* o = parts + ((int64_t)b * MOTION_PARTS + blockIdx.x) * MOTION_NQ;
#pragma unroll
        for (int j = 0; j < MOTION_NQ; ++j) o[j] = a[j];
    }
}

}  // namespace eincm
