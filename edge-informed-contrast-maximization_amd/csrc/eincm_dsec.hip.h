// eincm_dsec.hip.h — the DSEC data path: what DSECDataLoader (src/dataloaders/dsec_loader.py) does per event
// and per pixel before a window reaches the loss, and what dsec_npz_to_png.py does to a solved theta after it.
//
//   event rectification (dsec_loader.py:145-171)
//     k_rect_map      once per map: (rx, ry) float32 -> (rint(rx), rint(ry)) packed as int16 x 2; counts the entries that are not finite
//                     or whose rounding does not fit int16.  The per-event gather then moves 4 bytes, not 8, and rounds nothing.
//     k_rect_count    per block of RECT_BLOCK events: gather, in-sensor test, keep mask bytes, the block's kept count; counts the
//                     events whose input coordinate lies outside the sensor (the reference asserts on them)
//     k_rect_scan     one workgroup: exclusive scan of the block counts, the total
//     k_rect_scatter  per block: gather again, rank = block offset + ranks of the lower waves + ballot / popcount rank inside the
//                     wave + rank inside the thread; kept (rec_x, rec_y) go to their place
//     Each is its own launch on one stream: the kernel boundary carries the ordering, no workgroup waits on another, no atomics decide
//     a position.  The compaction is STABLE (ranks follow the event index) and the output the same bytes on every run.  A thread owns
//     RECT_EPT = 8 consecutive events: one 16-byte load of x and one of y.
//   frame -> rectified event camera (dsec_loader.py:188-245: cv.remap, INTER_CUBIC, constant 0 border)
//     k_remap_cubic   one thread per output pixel: its fixed-point coordinate (5 fractional bits) and the row of 16 integer weights
//                     of its fraction pair once, then the 4 x 4 taps of every image of the stack
//   16-bit flow codec (dsec_loader.py:247-266, dsec_npz_to_png.py:84-96)
//     k_flow_decode   (c - 2^15) / 128 where channel 2 is 1, 0 elsewhere; counts pixels whose channel 2 is neither 0 nor 1
//     k_flow_encode   bilinear scale_and_translate of theta (h, w, 2) to (H, W) and uint16(trunc(v * 128 + 2^15)) in one pass: the
//                     float64 (H, W, 2) image is never stored.  Counts the values with no defined encoding.
// The counters are integer atomicAdd: their final value does not depend on the order of the additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"

namespace eincm {

constexpr int RECT_EPT = 8;                        // events per thread: one 16-byte load of each coordinate array
constexpr int RECT_BLOCK = NT * RECT_EPT;          // events per workgroup (2048)
constexpr int RECT_SCAN_NT = 1024;
constexpr int RECT_OUTSIDE = -32768;               // packed map entry of a refused map value (never read: the call fails first)

struct alignas(16) Short8 { int16_t v[RECT_EPT]; };

// map (npix, 2) float32, channel 0 = x  ->  packed (npix) uint32: low half rint(x) as int16, high half rint(y).  bad[0] += entries
// that are NaN / Inf or round outside [-32768, 32767].  rintf: round half to even, numpy's np.round on float32.
__global__ __launch_bounds__(NT) void k_rect_map(int64_t npix, const float2* __restrict__ map, uint32_t* __restrict__ packed,
                                                 unsigned long long* __restrict__ bad) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const float2 m = map[p];
    const float rx = rintf(m.x), ry = rintf(m.y);
    const bool ok = rx >= -32768.0f && rx <= 32767.0f && ry >= -32768.0f && ry <= 32767.0f;      // false for NaN
    const int ix = ok ? (int)rx : RECT_OUTSIDE, iy = ok ? (int)ry : RECT_OUTSIDE;
    packed[p] = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
    if (!ok) atomicAdd(bad, 1ull);
}

// The 8 events of a thread: loads, gathers and in-sensor tests.  Events at or past n, and events whose input coordinate is outside
// the sensor (counted in n_oob), are not kept and read nothing.  Returns the keep bits (bit j: event e0 + j).
__device__ __forceinline__ uint32_t rect_thread(int H, int W, int64_t n, int64_t e0, const int16_t* __restrict__ xs,
                                                const int16_t* __restrict__ ys, const uint32_t* __restrict__ packed,
                                                uint32_t (&rec)[RECT_EPT], uint32_t& n_oob) {
    Short8 x8{}, y8{};
    if (e0 + RECT_EPT <= n) {                      // the arrays are 16-byte aligned (the host allocates them) and e0 is a multiple of 8
        x8 = *reinterpret_cast<const Short8*>(xs + e0);
        y8 = *reinterpret_cast<const Short8*>(ys + e0);
    } else {
#pragma unroll
        for (int j = 0; j < RECT_EPT; ++j)
            if (e0 + j < n) { x8.v[j] = xs[e0 + j]; y8.v[j] = ys[e0 + j]; }
    }
    uint32_t keep = 0u;
    n_oob = 0u;
#pragma unroll
    for (int j = 0; j < RECT_EPT; ++j) {
        const int x = x8.v[j], y = y8.v[j];
        const bool live = e0 + j < n;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        rec[j] = 0u;
        if (live && in) rec[j] = packed[(int64_t)y * W + x];
        if (live && !in) ++n_oob;
    }
#pragma unroll
    for (int j = 0; j < RECT_EPT; ++j) {
        const int rx = (int16_t)(rec[j] & 0xffffu), ry = (int16_t)(rec[j] >> 16);
        const bool live = e0 + j < n;
        const int x = x8.v[j], y = y8.v[j];
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        if (live && in && rx >= 0 && rx < W && ry >= 0 && ry < H) keep |= 1u << j;
    }
    return keep;
}

// grid ceil(n / RECT_BLOCK).  keep (n) bytes 0 / 1; blockcount (grid); oob[0] += events with an input coordinate outside the sensor.
__global__ __launch_bounds__(NT) void k_rect_count(int H, int W, int64_t n, const int16_t* __restrict__ xs, const int16_t* __restrict__ ys,
                                                   const uint32_t* __restrict__ packed, uint8_t* __restrict__ keep,
                                                   uint32_t* __restrict__ blockcount, unsigned long long* __restrict__ oob) {
    __shared__ uint32_t wcnt[NT / 64];
    const int64_t e0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * RECT_EPT;
    uint32_t rec[RECT_EPT], n_oob;
    const uint32_t bits = rect_thread(H, W, n, e0, xs, ys, packed, rec, n_oob);
    if (e0 + RECT_EPT <= n) {                      // 8 mask bytes in one store (keep is 16-byte aligned, e0 a multiple of 8)
        uint2 m;
        m.x = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
        m.y = ((bits >> 4) & 1u) | (((bits >> 4) & 2u) << 7) | (((bits >> 4) & 4u) << 14) | (((bits >> 4) & 8u) << 21);
        *reinterpret_cast<uint2*>(keep + e0) = m;
    } else {
        for (int j = 0; j < RECT_EPT; ++j)
            if (e0 + j < n) keep[e0 + j] = (uint8_t)((bits >> j) & 1u);
    }
    uint32_t cnt = (uint32_t)__popc(bits);
    uint32_t bad = n_oob;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { cnt += __shfl_xor(cnt, d); bad += __shfl_xor(bad, d); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wcnt[wave] = cnt; if (bad) atomicAdd(oob, (unsigned long long)bad); }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) s += wcnt[k];
        blockcount[blockIdx.x] = s;
    }
}

// One workgroup: blockoff[b] = sum of blockcount[< b] (int64), total[0] = the sum of all.  Walks the counts in pieces of
// RECT_SCAN_NT with a Hillis-Steele scan in LDS; integer sums, so the result does not depend on the scan's shape.
__global__ __launch_bounds__(RECT_SCAN_NT) void k_rect_scan(int nblk, const uint32_t* __restrict__ blockcount,
                                                            int64_t* __restrict__ blockoff, int64_t* __restrict__ total) {
    __shared__ int64_t buf[2][RECT_SCAN_NT];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += RECT_SCAN_NT) {
        const int i = base + (int)threadIdx.x;
        const int64_t own = i < nblk ? (int64_t)blockcount[i] : 0;
        int cur = 0;
        buf[0][threadIdx.x] = own;
        __syncthreads();
        for (int d = 1; d < RECT_SCAN_NT; d <<= 1) {
            const int64_t v = buf[cur][threadIdx.x] + ((int)threadIdx.x >= d ? buf[cur][threadIdx.x - d] : 0);
            buf[cur ^ 1][threadIdx.x] = v;
            cur ^= 1;
            __syncthreads();
        }
        const int64_t incl = buf[cur][threadIdx.x];
        const int64_t c = carry;
        if (i < nblk) blockoff[i] = c + incl - own;
        __syncthreads();
        if (threadIdx.x == RECT_SCAN_NT - 1) carry = c + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// grid as k_rect_count.  The kept events of the block go to rec_x / rec_y [blockoff[block] ...) in event order.
__global__ __launch_bounds__(NT) void k_rect_scatter(int H, int W, int64_t n, const int16_t* __restrict__ xs, const int16_t* __restrict__ ys,
                                                     const uint32_t* __restrict__ packed, const int64_t* __restrict__ blockoff,
                                                     int16_t* __restrict__ rec_x, int16_t* __restrict__ rec_y) {
    __shared__ uint32_t wcnt[NT / 64];
    const int64_t e0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * RECT_EPT;
    uint32_t rec[RECT_EPT], n_oob;
    const uint32_t bits = rect_thread(H, W, n, e0, xs, ys, packed, rec, n_oob);
    const uint32_t cnt = (uint32_t)__popc(bits);                 // 0 .. 8: four bits
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;      // the lanes before this one
    // kept events of the lower lanes: one ballot per bit of the count, popcount of the lower lanes' part, weighted by the bit
    uint32_t before = 0u, wave_total = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __ballot((cnt >> b) & 1u);
        before += (uint32_t)__popcll(m & below) << b;
        wave_total += (uint32_t)__popcll(m) << b;
    }
    if (lane == 0) wcnt[wave] = wave_total;
    __syncthreads();
    int64_t at = blockoff[blockIdx.x] + before;
    for (int k = 0; k < wave; ++k) at += wcnt[k];
#pragma unroll
    for (int j = 0; j < RECT_EPT; ++j) {
        if ((bits >> j) & 1u) {
            rec_x[at] = (int16_t)(rec[j] & 0xffffu);
            rec_y[at] = (int16_t)(rec[j] >> 16);
            ++at;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cv.remap(src, map, None, INTER_CUBIC), 8-bit single channel, constant 0 border, as the contract of DESIGN.md section 16 states it.
// src (n, Hs, Ws) uint8; map (H * W, 2) float32, channel 0 = x; tab (32 * 32, 16) int32: row (fy * 32 + fx), entry (ky * 4 + kx), each
// row summing to 2^15; dst (n, H, W).  Per component: p = map * 32 in float32; NaN -> the pixel is 0; p clamped to +-2^30, rint (half
// to even) -> s; integer part s >> 5 (arithmetic) clamped to int16, fraction s & 31.  Taps (iy - 1 .. iy + 2, ix - 1 .. ix + 2), a tap
// outside the source adds 0; dst = clamp((sum + 2^14) >> 15, 0, 255).  Hs, Ws <= 32766, so a clamped integer part has no tap inside.
__global__ __launch_bounds__(NT) void k_remap_cubic(int n, int Hs, int Ws, int64_t npix, const uint8_t* __restrict__ src,
                                                    const float2* __restrict__ map, const int32_t* __restrict__ tab,
                                                    uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const float2 m = map[p];
    const float px = m.x * 32.0f, py = m.y * 32.0f;
    const bool nan = !(px == px) || !(py == py);
    const float lim = 1073741824.0f;
    const int sx = (int)rintf(fminf(fmaxf(nan ? 0.0f : px, -lim), lim));
    const int sy = (int)rintf(fminf(fmaxf(nan ? 0.0f : py, -lim), lim));
    const int ix = min(max(sx >> 5, -32768), 32767), iy = min(max(sy >> 5, -32768), 32767);
    const int x0 = ix - 1, y0 = iy - 1;
    const bool none = nan || x0 >= Ws || x0 + 3 < 0 || y0 >= Hs || y0 + 3 < 0;
    if (none) {
        for (int k = 0; k < n; ++k) dst[(int64_t)k * npix + p] = 0;
        return;
    }
    int32_t w[16];
    {
        const int4* row = reinterpret_cast<const int4*>(tab + (((sy & 31) << 5) | (sx & 31)) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int4 v = row[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    }
    const bool inside = x0 >= 0 && x0 + 3 < Ws && y0 >= 0 && y0 + 3 < Hs;
    if (!inside) {                                 // fold the border into the weights: a tap outside the source weighs 0 ...
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx)
                if (x0 + kx < 0 || x0 + kx >= Ws || y0 + ky < 0 || y0 + ky >= Hs) w[4 * ky + kx] = 0;
    }
    const int cx0 = min(max(x0, 0), Ws - 1), cx1 = min(max(x0 + 1, 0), Ws - 1), cx2 = min(max(x0 + 2, 0), Ws - 1), cx3 = min(max(x0 + 3, 0), Ws - 1);
    int64_t rowoff[4];                             // ... and reads a clamped address
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) rowoff[ky] = (int64_t)min(max(y0 + ky, 0), Hs - 1) * Ws;
    const int64_t simg = (int64_t)Hs * Ws;
    for (int k = 0; k < n; ++k) {
        const uint8_t* s = src + (int64_t)k * simg;
        int32_t acc = 0;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const uint8_t* r = s + rowoff[ky];
            acc += (int32_t)r[cx0] * w[4 * ky] + (int32_t)r[cx1] * w[4 * ky + 1] + (int32_t)r[cx2] * w[4 * ky + 2] + (int32_t)r[cx3] * w[4 * ky + 3];
        }
        const int32_t v = (acc + (1 << 14)) >> 15;
        dst[(int64_t)k * npix + p] = (uint8_t)min(max(v, 0), 255);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// flow16 (npix_total, 3) uint16 -> flow (npix_total, 2) float64, valid (npix_total) 0 / 1; bad[0] += pixels whose channel 2 is not 0 or 1
__global__ __launch_bounds__(NT) void k_flow_decode(int64_t npix_total, const uint16_t* __restrict__ flow16, double* __restrict__ flow,
                                                    uint8_t* __restrict__ valid, unsigned long long* __restrict__ bad) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix_total) return;
    const uint16_t a = flow16[3 * p], b = flow16[3 * p + 1], v = flow16[3 * p + 2];
    const bool ok = v == 1;
    reinterpret_cast<double2*>(flow)[p] = ok ? make_double2(((double)a - 32768.0) / 128.0, ((double)b - 32768.0) / 128.0) : make_double2(0.0, 0.0);
    valid[p] = ok ? 1 : 0;
    if (v > 1) atomicAdd(bad, 1ull);
}

// theta (B, h, w, 2) float64 -> out (B, H, W, 3) uint16.  Row taps: output row y reads theta rows [rlo[y], rlo[y] + rcnt[y]) with the
// weights rwt[y * rstride ...]; columns likewise (the non-zero runs of the engine's resample matrices).  v = sum_i a_i (sum_j b_j
// theta[i][j]), unfused; code = trunc(v * 128 + 32768) in float64.  Not finite or outside [0, 65536): stored as 0, the pixel counted in bad[0].
// Channel 2: valid[b][y][x] != 0 where a mask is given, else 0.  grid (ceil(H * W / NT), B).
__global__ __launch_bounds__(NT) void k_flow_encode(int H, int W, int h, int w, const double* __restrict__ theta,
                                                    const int32_t* __restrict__ rlo, const int32_t* __restrict__ rcnt,
                                                    const double* __restrict__ rwt, int rstride, const int32_t* __restrict__ clo,
                                                    const int32_t* __restrict__ ccnt, const double* __restrict__ cwt, int cstride,
                                                    const uint8_t* __restrict__ valid, uint16_t* __restrict__ out,
                                                    unsigned long long* __restrict__ bad) {
#pragma clang fp contract(off)
    const int npix = H * W;                        // H, W <= 32767: pixel indices fit 32 bits
    const int p = (int)(blockIdx.x * NT + threadIdx.x);
    if (p >= npix) return;
    const int b = blockIdx.y;
    const int y = p / W, x = p - y * W;
    const int i0 = rlo[y], ni = rcnt[y], j0 = clo[x], nj = ccnt[x];
    const double2* th = reinterpret_cast<const double2*>(theta) + (int64_t)b * h * w;
    double vx = 0.0, vy = 0.0;
    for (int i = 0; i < ni; ++i) {
        double sx = 0.0, sy = 0.0;
        for (int j = 0; j < nj; ++j) {
            const double2 t = th[(int64_t)(i0 + i) * w + (j0 + j)];
            const double bw = cwt[(int64_t)x * cstride + j];
            sx += bw * t.x;
            sy += bw * t.y;
        }
        const double aw = rwt[(int64_t)y * rstride + i];
        vx += aw * sx;
        vy += aw * sy;
    }
    const double cx = vx * 128.0 + 32768.0, cy = vy * 128.0 + 32768.0;
    const bool okx = cx >= 0.0 && cx < 65536.0, oky = cy >= 0.0 && cy < 65536.0;     // false for NaN
    uint16_t* o = out + ((int64_t)b * npix + p) * 3;
    o[0] = okx ? (uint16_t)cx : (uint16_t)0;
    o[1] = oky ? (uint16_t)cy : (uint16_t)0;
    o[2] = (valid && valid[(int64_t)b * npix + p]) ? (uint16_t)1 : (uint16_t)0;
    if (!(okx && oky)) atomicAdd(bad, 1ull);
}

}  // namespace eincm
