// eincm_gtflow.hip.h — ground-truth flow of an MVSEC evaluation window: MVSECDataLoader.estimate_gt_flow
// (src/dataloaders/mvsec_loader.py:322-408) and its per-frame step _prop_flow (:411-433), for a batch of windows in one launch.
//
// A window is one of two modes:
//   direct     one step (f, num, den): out = ((double)g[f][p] * num) / den, x and y; no mask (mvsec_loader.py:335-337)
//   propagate  steps (f, s) in order; the pixel's float32 position (cx, cy) starts at (x, y) and, per step, reads the frame's flow at
//              (rintf(cx), rintf(cy)) (cv.remap INTER_NEAREST: cvRound, constant 0 border; NaN or out of range reads 0), clears the
//              x / y mask where the read x / y flow is 0, and moves by cx = (float)((double)cx + fx * s) (the reference's float32
//              coordinates += a float64 product: numpy computes the sum in float64 and casts).  At the end
//              out = mask ? (double)(cx - (float)x) : 0.0, per component, the subtraction in float32.
// Every pixel's chain is independent: one thread per pixel, grid (pixel blocks, windows).  No reduction, no atomics, every float
// expression unfused (fp contract off): the output is the same bytes on every run and in fp32 and EINCM_CF_FP64 contexts.
//
// The frames are read in the stack's own type T (float or double) and widened exactly; a float32 stack and the same stack widened to
// float64 give the same output.  The step lists are wave-uniform (one window per block row), the flow reads near-identity gathers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int GTF_DIRECT = 0;          // EINCM_GTF_DIRECT
constexpr int GTF_PROPAGATE = 1;       // EINCM_GTF_PROPAGATE
constexpr int GTF_MAX_WINDOWS_PER_LAUNCH = 65535;     // grid.y

// grid (ceil(H*W / NT), windows of this launch); window b of the launch is window w0 + b of the batch.
// gx, gy (n_frames, H, W) of T; mode (n_windows); step_off (n_windows + 1): window b's steps are [step_off[b], step_off[b + 1]);
// step_frame / step_num / step_den (n_steps); out (n_windows, H, W, 2) float64.  The host has checked every index and value.
template <typename T>
__global__ __launch_bounds__(NT) void k_gt_flow(int H, int W, int w0, const T* __restrict__ gx, const T* __restrict__ gy,
                                                const int32_t* __restrict__ mode, const int32_t* __restrict__ step_off,
                                                const int32_t* __restrict__ step_frame, const double* __restrict__ step_num,
                                                const double* __restrict__ step_den, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t npix = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const int b = w0 + (int)blockIdx.y;
    const int s0 = step_off[b], s1 = step_off[b + 1];
    double ox, oy;
    if (mode[b] == GTF_DIRECT) {
        const int64_t at = (int64_t)step_frame[s0] * npix + p;
        const double num = step_num[s0], den = step_den[s0];
        ox = ((double)gx[at] * num) / den;
        oy = ((double)gy[at] * num) / den;
    } else {
        const int x = (int)(p % W), y = (int)(p / W);
        const float xf = (float)x, yf = (float)y;
        const float xmax = (float)(W - 1), ymax = (float)(H - 1);
        float cx = xf, cy = yf;
        bool mx = true, my = true;
        for (int k = s0; k < s1; ++k) {
            const float rx = rintf(cx), ry = rintf(cy);
            double fx = 0.0, fy = 0.0;
            if (rx >= 0.0f && rx <= xmax && ry >= 0.0f && ry <= ymax) {      // false for NaN
                const int64_t at = (int64_t)step_frame[k] * npix + (int64_t)(int)ry * W + (int)rx;
                fx = (double)gx[at];
                fy = (double)gy[at];
            }
            if (fx == 0.0) mx = false;
            if (fy == 0.0) my = false;
            const double s = step_num[k];
            cx = (float)((double)cx + fx * s);
            cy = (float)((double)cy + fy * s);
        }
        ox = mx ? (double)(cx - xf) : 0.0;
        oy = my ? (double)(cy - yf) : 0.0;
    }
    reinterpret_cast<double2*>(out)[((int64_t)b * npix + p)] = make_double2(ox, oy);
}

}  // namespace eincm
