// eincm_preprocess.hip.h — SURVEY row f-4: the photometric clean-up in front of Canny, the reference's preprocess_image
// (src/utils/img_utils.py:131-189): cv.fastNlMeansDenoising -> CLAHE -> unsharp mask (GaussianBlur + addWeighted) ->
// cv.bilateralFilter, on 8-bit grayscale images, each stage reading the previous stage's uint8 output.
//
// The contract is OpenCV 4.x's generic CPU code as written there; borders are reflect101, iterated.
//   k_nlm<TW>        one 64x32 output tile per workgroup, its (tile + 2 border) source in LDS; a thread owns 8 rows of one
//                    column, keeps their template rows in registers and, per search offset, forms the TW-wide row sums once
//                    and the TW-high box sums from them (integer, exact); the weight table is in global memory (L2-resident)
//   k_clahe_lut      one workgroup per (tile, image): LDS histogram by integer atomics, clip + redistribution, scan, LUT
//   k_clahe_interp   per pixel: bilinear blend of the four neighbouring tiles' LUTs, float32 in the contract's order
//   k_unsharp_rows   per pixel: the fixed-point row pass (taps sum to 256), exact in uint16
//   k_unsharp_cols   per pixel: the column pass (+2^15 >> 16) fused with addWeighted (float32, half-to-even)
//   k_bilateral      one 64x16 output tile per workgroup, source with an r halo and the colour table in LDS; float32 sums in
//                    tap order
// Every float expression is unfused (fp contract off in each kernel): the bytes do not depend on the context's precision.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int NLM_TW = 64;                 // output tile width: one wave per row of columns
constexpr int NLM_ROWS = 8;                // output rows per thread
constexpr int NLM_TH = NLM_ROWS * (NT / NLM_TW);     // 32
constexpr int NLM_MAX_TEMPLATE = 7;
constexpr int NLM_MAX_SEARCH = 21;
constexpr int CLAHE_BINS = 256;
constexpr int UNSHARP_MAX_TAPS = 129;      // sigma up to ~21 (cvRound(6 sigma + 1) | 1 taps)
constexpr int BIL_TW = 64;
constexpr int BIL_ROWS = 4;
constexpr int BIL_TH = BIL_ROWS * (NT / BIL_TW);     // 16
constexpr int BIL_MAX_RADIUS = 32;

// cv::borderInterpolate(p, n, BORDER_REFLECT_101), iterated: a border wider than the image folds back again.
__host__ __device__ __forceinline__ int pre_reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__device__ __forceinline__ uint8_t rne_u8(float x) {
    const float r = fminf(fmaxf(rintf(x), 0.0f), 255.0f);       // cvRound (half to even), saturate_cast<uchar>
    return (uint8_t)(int)r;
}

// ---------------------------------------------------------------------------------------------------- NL-means
// grid (ceil(W/64), ceil(H/32), n), NT threads, dynamic LDS (NLM_TH + 2b) x (NLM_TW + 2b) ints, b = sr + TW/2.
template <int TW>
__global__ __launch_bounds__(NT) void k_nlm(int H, int W, int sr, const int32_t* __restrict__ table, const uint8_t* __restrict__ src,
                                            uint8_t* __restrict__ dst)
{
    constexpr int TR = TW / 2;
    constexpr int SHIFT = TW == 1 ? 0 : TW == 3 ? 4 : TW == 5 ? 5 : 6;     // min p with 2^p >= TW^2
    constexpr int NR = NLM_ROWS + 2 * TR;                                  // template rows a thread needs
    extern __shared__ int s_nlm[];
    const int b = sr + TR;
    const int SW = NLM_TW + 2 * b, SH = NLM_TH + 2 * b;
    const int x0 = blockIdx.x * NLM_TW, y0 = blockIdx.y * NLM_TH;
    const size_t npix = (size_t)H * W;
    const uint8_t* __restrict__ S = src + (size_t)blockIdx.z * npix;
    for (int k = threadIdx.x; k < SH * SW; k += NT) {
        const int i = k / SW, j = k - (k / SW) * SW;
        s_nlm[k] = S[(size_t)pre_reflect101(y0 - b + i, H) * W + pre_reflect101(x0 - b + j, W)];
    }
    __syncthreads();
    const int col = threadIdx.x % NLM_TW, strip = threadIdx.x / NLM_TW;
    const int x = x0 + col;
    if (x >= W) return;
    const int li = b + strip * NLM_ROWS, lj = b + col;               // LDS position of the thread's first output
    int c[NR][TW];                                                   // the template rows around the outputs
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int t = 0; t < TW; ++t) c[r][t] = s_nlm[(li - TR + r) * SW + lj - TR + t];
    uint32_t est[NLM_ROWS], wsum[NLM_ROWS];
#pragma unroll
    for (int r = 0; r < NLM_ROWS; ++r) { est[r] = 0; wsum[r] = 0; }
    for (int dy = -sr; dy <= sr; ++dy) {
        for (int dx = -sr; dx <= sr; ++dx) {
            const int* __restrict__ q = s_nlm + (li - TR + dy) * SW + lj - TR + dx;
            int rs[NR];                                              // TW-wide sums of squared differences, per template row
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                int acc = 0;
#pragma unroll
                for (int t = 0; t < TW; ++t) { const int e = c[r][t] - q[r * SW + t]; acc += e * e; }
                rs[r] = acc;
            }
#pragma unroll
            for (int r = 0; r < NLM_ROWS; ++r) {
                int D = 0;
#pragma unroll
                for (int t = 0; t < TW; ++t) D += rs[r + t];
                const uint32_t w = (uint32_t)table[D >> SHIFT];
                est[r] += w * (uint32_t)q[(r + TR) * SW + TR];
                wsum[r] += w;
            }
        }
    }
    uint8_t* __restrict__ Dst = dst + (size_t)blockIdx.z * npix;
#pragma unroll
    for (int r = 0; r < NLM_ROWS; ++r) {
        const int y = y0 + strip * NLM_ROWS + r;
        if (y < H) Dst[(size_t)y * W + x] = (uint8_t)((est[r] + wsum[r] / 2) / wsum[r]);
    }
}

// ---------------------------------------------------------------------------------------------------- CLAHE
// grid (tiles_x, tiles_y, n), NT threads.  Tile (tx, ty) of the bottom/right-padded image; lut (n, tiles_y, tiles_x, 256).
// limit <= 0: no clipping.
__global__ __launch_bounds__(NT) void k_clahe_lut(int H, int W, int tile_h, int tile_w, int limit, const uint8_t* __restrict__ src,
                                                  uint8_t* __restrict__ lut)
{
#pragma clang fp contract(off)
    __shared__ int s_hist[CLAHE_BINS];
    __shared__ int s_clipped;
    const int i = threadIdx.x;                                       // NT == CLAHE_BINS: one bin per thread
    s_hist[i] = 0;
    if (i == 0) s_clipped = 0;
    __syncthreads();
    const uint8_t* __restrict__ S = src + (size_t)blockIdx.z * H * W;
    const int px0 = blockIdx.x * tile_w, py0 = blockIdx.y * tile_h;
    const int total = tile_w * tile_h;
    for (int k = i; k < total; k += NT) {
        const int ty = k / tile_w, tx = k - (k / tile_w) * tile_w;
        const int y = pre_reflect101(py0 + ty, H), x = pre_reflect101(px0 + tx, W);
        atomicAdd(&s_hist[S[(size_t)y * W + x]], 1);
    }
    __syncthreads();
    int h = s_hist[i];
    if (limit > 0) {
        const int over = h - limit;
        if (over > 0) { atomicAdd(&s_clipped, over); h = limit; }
    }
    __syncthreads();
    if (limit > 0) {
        const int clipped = s_clipped;
        const int batch = clipped / CLAHE_BINS, res = clipped - batch * CLAHE_BINS;
        h += batch;
        if (res > 0) {
            const int step = max(CLAHE_BINS / res, 1);
            if (i % step == 0 && i / step < res) h += 1;             // bins 0, step, 2 step, ... while the residual lasts
        }
    }
    s_hist[i] = h;
    __syncthreads();
    for (int off = 1; off < CLAHE_BINS; off <<= 1) {                 // inclusive scan (Hillis-Steele)
        const int v = i >= off ? s_hist[i - off] : 0;
        __syncthreads();
        s_hist[i] += v;
        __syncthreads();
    }
    const float scale = 255.0f / (float)total;
    const size_t t = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    lut[t * CLAHE_BINS + i] = rne_u8((float)s_hist[i] * scale);
}

// grid (ceil(W/NT), H, n).
__global__ __launch_bounds__(NT) void k_clahe_interp(int H, int W, int tile_h, int tile_w, int tiles_x, int tiles_y,
                                                     const uint8_t* __restrict__ lut, const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const float inv_tw = 1.0f / (float)tile_w, inv_th = 1.0f / (float)tile_h;
    const float txf = (float)x * inv_tw - 0.5f;
    const int tx1u = (int)floorf(txf);
    const float xa = txf - (float)tx1u, xa1 = 1.0f - xa;
    const int tx1 = min(max(tx1u, 0), tiles_x - 1), tx2 = min(tx1u + 1, tiles_x - 1);     // the upper clamp never binds
    const float tyf = (float)y * inv_th - 0.5f;
    const int ty1u = (int)floorf(tyf);
    const float ya = tyf - (float)ty1u, ya1 = 1.0f - ya;
    const int ty1 = min(max(ty1u, 0), tiles_y - 1), ty2 = min(ty1u + 1, tiles_y - 1);
    const size_t p = (size_t)blockIdx.z * H * W + (size_t)y * W + x;
    const int v = src[p];
    const uint8_t* __restrict__ Lz = lut + (size_t)blockIdx.z * tiles_y * tiles_x * CLAHE_BINS;
    const float L11 = Lz[((size_t)ty1 * tiles_x + tx1) * CLAHE_BINS + v], L12 = Lz[((size_t)ty1 * tiles_x + tx2) * CLAHE_BINS + v];
    const float L21 = Lz[((size_t)ty2 * tiles_x + tx1) * CLAHE_BINS + v], L22 = Lz[((size_t)ty2 * tiles_x + tx2) * CLAHE_BINS + v];
    const float top = L11 * xa1 + L12 * xa;
    const float bot = L21 * xa1 + L22 * xa;
    dst[p] = rne_u8(top * ya1 + bot * ya);
}

// ---------------------------------------------------------------------------------------------------- unsharp mask
// grid (ceil(W/NT), H, n).  rows (n,H,W) uint16 = sum_i k_i src[y][pre_reflect101(x + i - r)], in 1/256.
__global__ __launch_bounds__(NT) void k_unsharp_rows(int H, int W, int radius, const int32_t* __restrict__ taps,
                                                     const uint8_t* __restrict__ src, uint16_t* __restrict__ rows)
{
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t row = (size_t)blockIdx.z * H * W + (size_t)y * W;
    const uint8_t* __restrict__ S = src + row;
    uint32_t acc = 0;
    if (x >= radius && x + radius < W) {
        for (int i = -radius; i <= radius; ++i) acc += (uint32_t)taps[i + radius] * S[x + i];
    } else {
        for (int i = -radius; i <= radius; ++i) acc += (uint32_t)taps[i + radius] * S[pre_reflect101(x + i, W)];
    }
    rows[row + x] = (uint16_t)acc;
}

// grid (ceil(W/NT), H, n).  blur = (sum_j k_j rows[pre_reflect101(y + j - r)][x] + 2^15) >> 16; dst = addWeighted(src, alpha, blur,
// beta, 0).  dst may not alias src.
__global__ __launch_bounds__(NT) void k_unsharp_cols(int H, int W, int radius, const int32_t* __restrict__ taps, float alpha,
                                                     float beta, const uint16_t* __restrict__ rows, const uint8_t* __restrict__ src,
                                                     uint8_t* __restrict__ dst)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t img = (size_t)blockIdx.z * H * W;
    const uint16_t* __restrict__ R = rows + img + x;
    uint32_t acc = 0;
    if (y >= radius && y + radius < H) {
        for (int j = -radius; j <= radius; ++j) acc += (uint32_t)taps[j + radius] * R[(size_t)(y + j) * W];
    } else {
        for (int j = -radius; j <= radius; ++j) acc += (uint32_t)taps[j + radius] * R[(size_t)pre_reflect101(y + j, H) * W];
    }
    const uint32_t blur = (acc + (1u << 15)) >> 16;
    const size_t p = img + (size_t)y * W + x;
    const float t = (float)src[p] * alpha;
    const float u = (float)blur * beta;
    const float s = t + u;
    dst[p] = rne_u8(s + 0.0f);
}

// ---------------------------------------------------------------------------------------------------- bilateral
// grid (ceil(W/64), ceil(H/16), n), NT threads, dynamic LDS (BIL_TH + 2r) x (BIL_TW + 2r) ints.  taps: n_taps (dy, dx) pairs
// and weights, row-major over the disc; cw: 256 colour weights.
__global__ __launch_bounds__(NT) void k_bilateral(int H, int W, int radius, int n_taps, const int32_t* __restrict__ tap_ofs,
                                                  const float* __restrict__ tap_w, const float* __restrict__ cw,
                                                  const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
#pragma clang fp contract(off)
    extern __shared__ int s_bil[];
    __shared__ float s_cw[256];
    const int SW = BIL_TW + 2 * radius, SH = BIL_TH + 2 * radius;
    const int x0 = blockIdx.x * BIL_TW, y0 = blockIdx.y * BIL_TH;
    const size_t npix = (size_t)H * W;
    const uint8_t* __restrict__ S = src + (size_t)blockIdx.z * npix;
    for (int k = threadIdx.x; k < SH * SW; k += NT) {
        const int i = k / SW, j = k - (k / SW) * SW;
        s_bil[k] = S[(size_t)pre_reflect101(y0 - radius + i, H) * W + pre_reflect101(x0 - radius + j, W)];
    }
    s_cw[threadIdx.x] = cw[threadIdx.x];                              // NT == 256
    __syncthreads();
    const int col = threadIdx.x % BIL_TW, strip = threadIdx.x / BIL_TW;
    const int x = x0 + col;
    if (x >= W) return;
    const int li = radius + strip * BIL_ROWS, lj = radius + col;
    int v0[BIL_ROWS];
    float sum[BIL_ROWS], wsum[BIL_ROWS];
#pragma unroll
    for (int r = 0; r < BIL_ROWS; ++r) { v0[r] = s_bil[(li + r) * SW + lj]; sum[r] = 0.0f; wsum[r] = 0.0f; }
    for (int k = 0; k < n_taps; ++k) {
        const int dy = tap_ofs[2 * k], dx = tap_ofs[2 * k + 1];
        const float sw = tap_w[k];
        const int* __restrict__ q = s_bil + (li + dy) * SW + lj + dx;
#pragma unroll
        for (int r = 0; r < BIL_ROWS; ++r) {
            const int v = q[r * SW];
            const float w = sw * s_cw[abs(v - v0[r])];
            wsum[r] += w;
            const float vw = (float)v * w;
            sum[r] += vw;
        }
    }
    uint8_t* __restrict__ Dst = dst + (size_t)blockIdx.z * npix;
#pragma unroll
    for (int r = 0; r < BIL_ROWS; ++r) {
        const int y = y0 + strip * BIL_ROWS + r;
        if (y < H) Dst[(size_t)y * W + x] = rne_u8(sum[r] / wsum[r]);
    }
}

}  // namespace eincm
