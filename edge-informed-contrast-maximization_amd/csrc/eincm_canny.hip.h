// eincm_canny.hip.h — SURVEY row f-4: Canny edge detection, the step from a grayscale frame to the binary edge image that the
// smoothing of eincm_edges.hip.h turns into `edges` (src/utils/img_utils.py:192-208: cv.Canny(img, th1, th2, None, 3, True)).
//
// The semantics are OpenCV's generic integer Canny for 8-bit input (imgproc/src/canny.cpp, non-IPP, non-OpenCL), aperture 3:
//   Sobel dx = [-1 0 1] x [1 2 1]^T, dy its transpose, BORDER_REPLICATE; magnitude m = dx^2 + dy^2 (L2) or |dx| + |dy| (L1), 0
//   outside the image; non-maximum suppression along the gradient sector with the tan(22.5) / tan(67.5) tests in 15-bit fixed
//   point and OpenCV's asymmetric tie rule (> before, >= after); a survivor (m > low after NMS) is strong if m > high; the output
//   is 255 at every survivor 8-connected through survivors to a strong one.
//
// Four launches per call, whatever the image holds (no host loop, no bounded propagation):
//   k_canny_nms      one 64x16 tile per workgroup: the uint8 source with a 2-pixel replicate halo and the magnitude with a 1-pixel
//                    halo live in LDS; writes state (0 none, 1 weak, 2 strong) and the union-find parent (own index, -1 if none)
//   k_canny_merge    union of every survivor with its already-visited 8-neighbours (left, upper row): lock-free union-find with
//                    atomicMin links to the smaller index (Playne & Hawick 2018), path halving by atomicMin
//   k_canny_resolve  parent := root for every survivor; a strong survivor marks its root strong (state 2)
//   k_canny_output   255 where the survivor's root is strong
// Labels are per-image indices (int32: sensors are below 32768 x 32768).  Every step is integer work: the output is exact and
// does not depend on the order in which atomics retire.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int CANNY_TW = 64;                  // tile width  (output pixels): one wave per row
constexpr int CANNY_TH = 16;                  // tile height (output pixels): 4 rows per wave
constexpr int CANNY_SW = CANNY_TW + 4;        // source tile: 2-pixel halo (Sobel of the 1-pixel magnitude halo)
constexpr int CANNY_SH = CANNY_TH + 4;
constexpr int CANNY_MW = CANNY_TW + 2;        // magnitude tile: 1-pixel halo (the NMS neighbours)
constexpr int CANNY_MH = CANNY_TH + 2;

__device__ __forceinline__ void canny_sobel(const int (*s)[CANNY_SW], int i, int j, int& dx, int& dy) {
    // (i, j) is the centre in source-tile coordinates
    dx = (s[i - 1][j + 1] + 2 * s[i][j + 1] + s[i + 1][j + 1]) - (s[i - 1][j - 1] + 2 * s[i][j - 1] + s[i + 1][j - 1]);
    dy = (s[i + 1][j - 1] + 2 * s[i + 1][j] + s[i + 1][j + 1]) - (s[i - 1][j - 1] + 2 * s[i - 1][j] + s[i - 1][j + 1]);
}

// grid (ceil(W/64), ceil(H/16), n).  src (n,H,W) uint8; state (n,H,W) uint8; parent (n,H,W) int32.
__global__ __launch_bounds__(NT) void k_canny_nms(int H, int W, int low, int high, int l2, const uint8_t* __restrict__ src,
                                                   uint8_t* __restrict__ state, int32_t* __restrict__ parent)
{
    __shared__ int s_src[CANNY_SH][CANNY_SW];
    __shared__ int s_mag[CANNY_MH][CANNY_MW + 1];
    const int x0 = blockIdx.x * CANNY_TW, y0 = blockIdx.y * CANNY_TH;
    const size_t npix = (size_t)H * W;
    const uint8_t* __restrict__ S = src + (size_t)blockIdx.z * npix;
    for (int k = threadIdx.x; k < CANNY_SH * CANNY_SW; k += NT) {
        const int i = k / CANNY_SW, j = k % CANNY_SW;
        const int y = min(max(y0 - 2 + i, 0), H - 1), x = min(max(x0 - 2 + j, 0), W - 1);     // BORDER_REPLICATE
        s_src[i][j] = S[(size_t)y * W + x];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CANNY_MH * CANNY_MW; k += NT) {
        const int i = k / CANNY_MW, j = k % CANNY_MW;
        const int y = y0 - 1 + i, x = x0 - 1 + j;
        int m = 0;                                                                             // 0 outside the image
        if (y >= 0 && y < H && x >= 0 && x < W) {
            int dx, dy;
            canny_sobel(s_src, i + 1, j + 1, dx, dy);
            m = l2 ? dx * dx + dy * dy : abs(dx) + abs(dy);
        }
        s_mag[i][j] = m;
    }
    __syncthreads();
    uint8_t* __restrict__ St = state + (size_t)blockIdx.z * npix;
    int32_t* __restrict__ P = parent + (size_t)blockIdx.z * npix;
    for (int k = threadIdx.x; k < CANNY_TH * CANNY_TW; k += NT) {
        const int ti = k / CANNY_TW, tj = k % CANNY_TW;
        const int y = y0 + ti, x = x0 + tj;
        if (y >= H || x >= W) continue;
        const int i = ti + 1, j = tj + 1;                       // magnitude-tile coordinates
        const int m = s_mag[i][j];
        int st = 0;
        if (m > low) {
            int dx, dy;
            canny_sobel(s_src, i + 1, j + 1, dx, dy);
            const int ax = abs(dx), ay = abs(dy) << 15;
            const int tg22x = ax * 13573;                        // tan(22.5 deg) * 2^15
            const int tg67x = tg22x + (ax << 16);                // tan(67.5 deg) * 2^15 = (tan 22.5 + 2) * 2^15
            bool keep;
            if (ay < tg22x) {
                keep = m > s_mag[i][j - 1] && m >= s_mag[i][j + 1];
            } else if (ay > tg67x) {
                keep = m > s_mag[i - 1][j] && m >= s_mag[i + 1][j];
            } else {
                const int s = ((dx ^ dy) < 0) ? -1 : 1;
                keep = m > s_mag[i - 1][j - s] && m > s_mag[i + 1][j + s];
            }
            if (keep) st = (m > high) ? 2 : 1;
        }
        const size_t p = (size_t)y * W + x;
        St[p] = (uint8_t)st;
        P[p] = st ? (int32_t)p : -1;
    }
}

// Root of x.  Parents only ever decrease (atomicMin) and always point into x's own set, so a stale read is an ancestor and the
// halving step (an atomicMin too: a plain store could undo a concurrent link to a smaller index) never splits a set.
__device__ __forceinline__ int32_t canny_find(int32_t* P, int32_t x) {
    int32_t p = __hip_atomic_load(&P[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) {
        const int32_t gp = __hip_atomic_load(&P[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gp != p) atomicMin(&P[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

// Link the roots of a and b, the larger under the smaller; retried when another thread moved a root in between.
__device__ __forceinline__ void canny_union(int32_t* P, int32_t a, int32_t b) {
    for (;;) {
        a = canny_find(P, a);
        b = canny_find(P, b);
        if (a == b) return;
        if (a > b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(&P[b], a);
        if (old == b) return;                                   // b was still a root: linked
        b = old;
    }
}

// grid (nb, n), grid-stride over the pixels of image blockIdx.y.  Only the neighbours already visited in row-major order are
// joined; one joined through another survivor is skipped (left covers up-left; up covers up-left and up-right).
__global__ __launch_bounds__(NT) void k_canny_merge(int H, int W, const uint8_t* __restrict__ state, int32_t* __restrict__ parent)
{
    const int npix = H * W;
    const uint8_t* __restrict__ St = state + (size_t)blockIdx.y * npix;
    int32_t* P = parent + (size_t)blockIdx.y * npix;
    for (int p = blockIdx.x * NT + threadIdx.x; p < npix; p += gridDim.x * NT) {
        if (!St[p]) continue;
        const int y = p / W, x = p - y * W;
        const bool l = x > 0 && St[p - 1];
        if (l) canny_union(P, p, p - 1);
        if (y == 0) continue;
        const int u = p - W;
        if (St[u]) { canny_union(P, p, u); continue; }
        if (!l && x > 0 && St[u - 1]) canny_union(P, p, u - 1);
        if (x + 1 < W && St[u + 1]) canny_union(P, p, u + 1);
    }
}

// grid (nb, n).  parent := root; a strong survivor marks its root 2 (every writer stores the same value).
__global__ __launch_bounds__(NT) void k_canny_resolve(int H, int W, uint8_t* __restrict__ state, int32_t* __restrict__ parent)
{
    const int npix = H * W;
    uint8_t* St = state + (size_t)blockIdx.y * npix;
    int32_t* P = parent + (size_t)blockIdx.y * npix;
    for (int p = blockIdx.x * NT + threadIdx.x; p < npix; p += gridDim.x * NT) {
        const int s = St[p];
        if (!s) continue;
        const int32_t r = canny_find(P, p);
        P[p] = r;
        if (s == 2) St[r] = 2;
    }
}

// grid (nb, n).  dst may alias the source of k_canny_nms (no longer read).
__global__ __launch_bounds__(NT) void k_canny_output(int H, int W, const uint8_t* __restrict__ state, const int32_t* __restrict__ parent,
                                                      uint8_t* __restrict__ dst)
{
    const int npix = H * W;
    const uint8_t* __restrict__ St = state + (size_t)blockIdx.y * npix;
    const int32_t* __restrict__ P = parent + (size_t)blockIdx.y * npix;
    uint8_t* __restrict__ D = dst + (size_t)blockIdx.y * npix;
    for (int p = blockIdx.x * NT + threadIdx.x; p < npix; p += gridDim.x * NT) {
        const int32_t r = P[p];
        D[p] = (r >= 0 && St[r] == 2) ? 255 : 0;
    }
}

}  // namespace eincm
