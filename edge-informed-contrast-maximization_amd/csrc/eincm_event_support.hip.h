// eincm_event_support.hip.h — the spatiotemporal support filter (background-activity filter) of a raw event stream, one chunk per
// call (the rules themselves are in eincm_event_support.h).  The textbook form is one sequential walk with a
// last-timestamp map; here every event finds each neighbour's most recent earlier event by a binary search in that neighbour's list
// of event indices, which is in stream order:
//
//   k_es_validate   per event: coordinates, finiteness, order against the predecessor (the carried last time for event 0); the first
//                   offender by atomicMax on n - e (zero: none); the pixel key y W + x
//   k_es_hist       } a stable LSD radix sort of (key, index) by key, 8 bits per pass, ceil(bits(H W) / 8) passes.  A wave owns
//   k_es_scan_tiles } ES_SORT_BLOCK consecutive events and walks them 64 at a time in order; a lane's place among the lanes of its
//   k_es_scan       } digit comes from ballots, the digit's cursor from LDS.  The digit-major (digit, block) histogram is scanned in
//   k_es_scatter    } tiles of 4096 entries, the tile sums by one workgroup.  No atomic decides a position: the sorted arrays are a
//                   pure function of the input, and as every pass is stable and the indices start in order, every pixel's run of
//                   indices is ascending.
//   k_es_bounds     per sorted position: where a key's run starts and ends -> lo[pixel], hi[pixel] (zeroed before: an empty list)
//   k_es_support    per event, per neighbour inside the sensor and not masked: binary search of the neighbour's list for the last
//                   index below e, its time or the carried map's, one subtraction and one compare; support and weight by plain
//                   stores in the order handed over.  A list is never walked linearly: one pixel with 10^5 events costs 17 probes.
//   k_es_map        per pixel with a list: last_t[pixel] = the time of the list's last element
//   k_es_fill       the carried map to "no event" (first call, reset)
// Integer counts, one exact compare and one correctly rounded division: the outputs are the same bytes on every run.
//
// k_es_validate to k_es_bounds and k_es_fill are launched by the chunk front end of eincm_api.hip (StreamChunk, DESIGN.md section
// 23), which the refractory filter of eincm_event_filter.hip.h uses too; the sort's geometry (ES_RADIX_BITS, ES_SORT_BLOCK,
// ES_SCAN_TILE, es_sort_plan) is host arithmetic and lives in eincm_event_support.h.  Three pieces are written once for both
// filters' kernels: block_scan (a workgroup's inclusive scan under any operator), block_exclusive_prefix (the body of k_es_scan
// and k_ef_scan) and es_run_lower_bound (the search of k_es_support and k_ef_support).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_event_support.h"
#include "eincm_kernels.hip.h"

namespace eincm {

// grid ceil(n / NT).  err[0] = max(n - e) over the refused events e (zero before the launch: none), key[e] = y W + x.
__global__ __launch_bounds__(NT) void k_es_validate(int H, int W, int64_t n, const int16_t* __restrict__ xs, const int16_t* __restrict__ ys,
                                                    const double* __restrict__ ts, double carried, uint32_t* __restrict__ key,
                                                    uint32_t* __restrict__ err) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    const int x = xs[e], y = ys[e];
    const int fault = es_event_fault(H, W, x, y, ts[e], e > 0 ? ts[e - 1] : carried);
    key[e] = fault == ES_EV_COORD ? 0u : (uint32_t)y * (uint32_t)W + (uint32_t)x;
    if (fault) atomicMax(err, (uint32_t)(n - e));
}

// grid nblk, one wave each.  hist[digit * nblk + block] = events of the block whose key has that digit at `shift`.
__global__ __launch_bounds__(64) void k_es_hist(int64_t n, int nblk, int shift, const uint32_t* __restrict__ key, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[ES_RADIX];
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * ES_SORT_BLOCK;
#pragma unroll
    for (int k = 0; k < ES_RADIX / 64; ++k) h[lane + 64 * k] = 0u;
    __syncthreads();
    for (int trip = 0; trip < ES_SORT_BLOCK / 64; ++trip) {
        const int64_t e = e0 + trip * 64 + lane;
        if (e < n) atomicAdd(&h[(key[e] >> shift) & (ES_RADIX - 1)], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ES_RADIX / 64; ++k) hist[(int64_t)(lane + 64 * k) * nblk + blockIdx.x] = h[lane + 64 * k];
}

// The workgroup's NTH values become their inclusive prefixes under op in part (Hillis-Steele in LDS); returns the calling thread's.
// T{} is op's identity (zero: sums and maxima of unsigned integers).  part is complete and no longer written when the function
// returns.  Every use is an integer sum, an integer maximum or feeds an exact compare: the shape of the scan does not show in a result.
template <int NTH, typename T, typename Op> __device__ __forceinline__ T block_scan(T* part, T own, Op op) {
    const int tid = threadIdx.x;
    part[tid] = own;
    __syncthreads();
    for (int d = 1; d < NTH; d <<= 1) {
        const T v = tid >= d ? part[tid - d] : T{};
        __syncthreads();
        part[tid] = op(part[tid], v);
        __syncthreads();
    }
    return part[tid];
}

// One workgroup of NTH threads: data (len) becomes its exclusive prefix under op, in place.  A thread owns a contiguous piece; the
// pieces' totals are scanned in part (NTH elements of LDS).
template <int NTH, typename T, typename Op> __device__ __forceinline__ void block_exclusive_prefix(T* part, int64_t len, T* data, Op op) {
    const int tid = threadIdx.x;
    const int64_t per = (len + NTH - 1) / NTH;
    const int64_t i0 = (int64_t)tid * per < len ? (int64_t)tid * per : len, i1 = i0 + per < len ? i0 + per : len;
    T own{};
    for (int64_t i = i0; i < i1; ++i) own = op(own, data[i]);
    block_scan<NTH>(part, own, op);
    T run = tid > 0 ? part[tid - 1] : T{};
    for (int64_t i = i0; i < i1; ++i) { const T v = data[i]; data[i] = run; run = op(run, v); }
}

struct EsSum { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };

// grid ceil(len / ES_SCAN_TILE).  Every tile of data (len) becomes its own exclusive prefix sum, in place, and tilesum[tile] its total:
// the exclusive prefix sum of data is then data[i] + (the exclusive prefix sum of tilesum)[i / ES_SCAN_TILE], which k_es_scatter adds
// as it reads.  A thread owns four consecutive values: one 16-byte load and store (data is 16-byte aligned, a tile starts at a multiple
// of four).  Sums stay below 2^30 (they count events).
__global__ __launch_bounds__(ES_SCAN_NT) void k_es_scan_tiles(int64_t len, uint32_t* data, uint32_t* __restrict__ tilesum) {
    __shared__ uint32_t part[ES_SCAN_NT];
    const int64_t i0 = (int64_t)blockIdx.x * ES_SCAN_TILE + (int64_t)threadIdx.x * 4;
    const bool full = i0 + 4 <= len;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (full) {
        const uint4 q = *reinterpret_cast<const uint4*>(data + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < len) v[k] = data[i0 + k];
    }
    const uint32_t own = v[0] + v[1] + v[2] + v[3];
    const uint32_t incl = block_scan<ES_SCAN_NT>(part, own, EsSum{});
    if (threadIdx.x == ES_SCAN_NT - 1) tilesum[blockIdx.x] = incl;
    const uint32_t run = incl - own;
    if (full) {
        *reinterpret_cast<uint4*>(data + i0) = make_uint4(run, run + v[0], run + v[0] + v[1], run + v[0] + v[1] + v[2]);
    } else {
        uint32_t r = run;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < len) { data[i0 + k] = r; r += v[k]; }
    }
}

// One workgroup: data (len) becomes its exclusive prefix sum, in place (the tile sums of k_es_scan_tiles: len / 4096 of the
// histogram).
__global__ __launch_bounds__(ES_SCAN_NT) void k_es_scan(int64_t len, uint32_t* data) {
    __shared__ uint32_t part[ES_SCAN_NT];
    block_exclusive_prefix<ES_SCAN_NT>(part, len, data, EsSum{});
}

// grid nblk, one wave each.  base, tilebase: the scanned histogram as k_es_scan_tiles and k_es_scan leave it.  The block's events go
// to their digit's run in event order.  val_in NULL: the values are the event indices themselves (the first pass).
__global__ __launch_bounds__(64) void k_es_scatter(int64_t n, int nblk, int shift, const uint32_t* __restrict__ key_in,
                                                   const uint32_t* __restrict__ val_in, const uint32_t* __restrict__ base,
                                                   const uint32_t* __restrict__ tilebase, uint32_t* __restrict__ key_out,
                                                   uint32_t* __restrict__ val_out) {
    __shared__ uint32_t cur[ES_RADIX];
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * ES_SORT_BLOCK;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < ES_RADIX / 64; ++k) {
        const int64_t j = (int64_t)(lane + 64 * k) * nblk + blockIdx.x;
        cur[lane + 64 * k] = base[j] + tilebase[j / ES_SCAN_TILE];
    }
    __syncthreads();
    for (int trip = 0; trip < ES_SORT_BLOCK / 64; ++trip) {
        if (e0 + trip * 64 >= n) break;                       // (the same for the whole wave)
        const int64_t e = e0 + trip * 64 + lane;
        const bool live = e < n;
        const uint32_t k = live ? key_in[e] : 0u;
        const uint32_t d = (k >> shift) & (ES_RADIX - 1);
        unsigned long long peers = __ballot(live);            // the live lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < ES_RADIX_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(live && bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t pos = live ? cur[d] + (uint32_t)__popcll(peers & below) : 0u;
        __syncthreads();
        if (live && (peers >> lane) == 1ull) cur[d] = pos + 1u;      // the last lane of the digit moves its cursor on
        __syncthreads();
        if (live && pos < n) {
            key_out[pos] = k;
            val_out[pos] = val_in ? val_in[e] : (uint32_t)e;
        }
    }
}

// grid ceil(n / NT).  key (n) sorted; lo, hi (npix) zero before the launch.  The run of pixel p is [lo[p], hi[p]).
__global__ __launch_bounds__(NT) void k_es_bounds(int64_t n, int64_t npix, const uint32_t* __restrict__ key, uint32_t* __restrict__ lo,
                                                  uint32_t* __restrict__ hi) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = key[i];
    if (k >= npix) return;
    if (i == 0 || key[i - 1] != k) lo[k] = (uint32_t)i;
    if (i == n - 1 || key[i + 1] != k) hi[k] = (uint32_t)(i + 1);
}

// The first position of the run [lo, hi) of idx whose index is not below e (hi: none); the run ascends.  log2(hi - lo) + 1 probes
__device__ __forceinline__ uint32_t es_run_lower_bound(const uint32_t* __restrict__ idx, uint32_t lo, uint32_t hi, uint32_t e) {
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (idx[m] < e) lo = m + 1u; else hi = m;
    }
    return lo;
}

// grid ceil(n / NT).  idx: the sorted event indices (every pixel's run ascending); last_t (npix) the carried map; mask (npix) or NULL.
__global__ __launch_bounds__(NT) void k_es_support(int H, int W, int64_t n, const int16_t* __restrict__ xs, const int16_t* __restrict__ ys,
                                                   const double* __restrict__ ts, double tau, int radius, int full_support,
                                                   const uint8_t* __restrict__ mask, const uint32_t* __restrict__ lo,
                                                   const uint32_t* __restrict__ hi, const uint32_t* __restrict__ idx,
                                                   const double* __restrict__ last_t, float* __restrict__ weights,
                                                   uint8_t* __restrict__ support) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    const int x = xs[e], y = ys[e];
    const double te = ts[e];
    const int p = y * W + x;
    int s = 0;
    if (!(mask && mask[p])) {
        const EsWindow w = es_window(H, W, x, y, radius);
        for (int qy = w.y0; qy <= w.y1; ++qy)
            for (int qx = w.x0; qx <= w.x1; ++qx) {
                const int q = qy * W + qx;
                if (q == p || (mask && mask[q])) continue;
                const uint32_t first = lo[q];
                const uint32_t a = es_run_lower_bound(idx, first, hi[q], (uint32_t)e);
                const uint32_t j = a > first ? idx[a - 1u] : (uint32_t)e;
                const bool in_chunk = j < (uint32_t)e;        // (an index of the run below e: never read past the chunk)
                const double tp = in_chunk ? es_prev_time(true, ts[j], 0.0) : es_prev_time(false, 0.0, last_t[q]);
                s += es_supported(te, tp, tau) ? 1 : 0;
            }
    }
    support[e] = (uint8_t)s;
    weights[e] = es_weight(s, full_support);
}

// grid ceil(npix / NT).  After a chunk the map holds, per pixel, the time of its last event so far.
__global__ __launch_bounds__(NT) void k_es_map(int64_t npix, int64_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                               const uint32_t* __restrict__ idx, const double* __restrict__ ts, double* __restrict__ last_t) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const uint32_t a = lo[p], b = hi[p];
    if (b <= a) return;
    const uint32_t j = idx[b - 1u];
    if (j < n) last_t[p] = ts[j];
}

__global__ __launch_bounds__(NT) void k_es_fill(int64_t npix, double* __restrict__ last_t, double value) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p < npix) last_t[p] = value;
}

}   // namespace eincm
