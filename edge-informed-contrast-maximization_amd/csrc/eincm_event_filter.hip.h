// eincm_event_filter.hip.h — the refractory and polarity-aware event filter of a raw event stream, one chunk per call (DESIGN.md
// section 24; the rules themselves are in eincm_event_filter.h).  The chunk front end of eincm_api.hip (StreamChunk) validates the
// chunk, sorts it by pixel and bounds the runs with the event-support filter's kernels (k_es_validate, k_es_hist, k_es_scan_tiles,
// k_es_scan, k_es_scatter, k_es_bounds of eincm_event_support.hip.h), after which every pixel's events are one ascending run of the
// sorted positions.  The scans below are that header's block_scan and block_exclusive_prefix under EfMax, the search its
// es_run_lower_bound.  What is new:
//
//   k_ef_keep        per sorted position s: the event's predecessor on its pixel is position s - 1 (the carried last_any map for
//                    the first of a run), whatever became of it, so the refractory rule is one subtraction and one compare;
//                    keep[event], and the scan seeds m[s] = (kept and class 0 ? s + 1 : 0, kept and class 1 ? s + 1 : 0)
//   k_ef_scan_tiles  } an inclusive max-scan of the pairs m over the sorted positions: per tile of EF_SCAN_TILE positions in LDS,
//   k_ef_scan        } the tile maxima by one workgroup into their exclusive prefix, which every reader joins to what it reads
//                    (ef_scanned).  No segment flags: positions ascend, so m_c[s] - 1 is the position of the last kept class-c
//                    event at or before s, and it lies in pixel q's run exactly when it is >= lo[q].
//   k_ef_support     per event in stream order, per neighbour: the binary search of k_es_support for the neighbour's last position
//                    below the event, the scan there for its last kept one, that event's time or the carried last_kept maps', one
//                    subtraction and one compare.  A pixel with 10^5 dropped events in a row costs the same probes as any other.
//   k_ef_map         per pixel with a run: last_any and, where the run kept an event of the class, last_kept of that class
// Integer maxima, exact compares and one correctly rounded division: the outputs are the same bytes on every run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_event_filter.h"
#include "eincm_event_support.hip.h"

namespace eincm {

constexpr int EF_SCAN_NT = 1024;
constexpr int EF_SCAN_TILE = EF_SCAN_NT * 4;       // sorted positions per workgroup of the tile scan (the tests name this size)

__device__ __forceinline__ uint2 ef_max(uint2 a, uint2 b) { return make_uint2(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y); }
struct EfMax { __device__ uint2 operator()(uint2 a, uint2 b) const { return ef_max(a, b); } };

// The scanned pair at position j: the tile's own scan joined to the maximum of every tile before it
__device__ __forceinline__ uint2 ef_scanned(const uint2* __restrict__ m, const uint2* __restrict__ tilepre, uint32_t j) {
    return ef_max(m[j], tilepre[j / EF_SCAN_TILE]);
}

// grid ceil(n / NT).  key, val: the sorted (pixel, event index) arrays; lo (npix): where every run starts; last_any (npix) the
// carried map; pol (n, stream order) or NULL: class 0; mask (npix) or NULL.
__global__ __launch_bounds__(NT) void k_ef_keep(int64_t n, const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                const uint32_t* __restrict__ lo, const double* __restrict__ ts,
                                                const int8_t* __restrict__ pol, double rho, const uint8_t* __restrict__ mask,
                                                const double* __restrict__ last_any, uint8_t* __restrict__ keep, uint2* __restrict__ m) {
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (s >= n) return;
    const uint32_t q = key[s], e = val[s];
    const double prev = (uint32_t)s > lo[q] ? ts[val[s - 1]] : last_any[q];
    const bool kept = ef_kept(ts[e], prev, rho, mask && mask[q]);
    const int cls = pol ? ef_class(pol[e]) : 0;
    keep[e] = kept ? 1 : 0;
    const uint32_t seed = kept ? (uint32_t)s + 1u : 0u;
    m[s] = make_uint2(cls == 0 ? seed : 0u, cls == 1 ? seed : 0u);
}

// grid ceil(n / EF_SCAN_TILE).  Every tile of m (n) becomes its own inclusive prefix maximum, in place, and tilemax[tile] its
// maximum.  A thread owns four consecutive pairs: two 16-byte loads and stores (m is 16-byte aligned, a thread starts at a multiple
// of four pairs).
__global__ __launch_bounds__(EF_SCAN_NT) void k_ef_scan_tiles(int64_t n, uint2* m, uint2* __restrict__ tilemax) {
    __shared__ uint2 part[EF_SCAN_NT];
    const int64_t i0 = (int64_t)blockIdx.x * EF_SCAN_TILE + (int64_t)threadIdx.x * 4;
    const bool full = i0 + 4 <= n;
    uint2 v[4] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (full) {
        const uint4 a = *reinterpret_cast<const uint4*>(m + i0), b = *reinterpret_cast<const uint4*>(m + i0 + 2);
        v[0] = make_uint2(a.x, a.y); v[1] = make_uint2(a.z, a.w); v[2] = make_uint2(b.x, b.y); v[3] = make_uint2(b.z, b.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < n) v[k] = m[i0 + k];
    }
    block_scan<EF_SCAN_NT>(part, ef_max(ef_max(v[0], v[1]), ef_max(v[2], v[3])), EfMax{});
    if (threadIdx.x == EF_SCAN_NT - 1) tilemax[blockIdx.x] = part[EF_SCAN_NT - 1];
    uint2 r = threadIdx.x > 0 ? part[threadIdx.x - 1] : make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) { r = ef_max(r, v[k]); v[k] = r; }
    if (full) {
        *reinterpret_cast<uint4*>(m + i0) = make_uint4(v[0].x, v[0].y, v[1].x, v[1].y);
        *reinterpret_cast<uint4*>(m + i0 + 2) = make_uint4(v[2].x, v[2].y, v[3].x, v[3].y);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (i0 + k < n) m[i0 + k] = v[k];
    }
}

// One workgroup: data (len, the tile maxima) becomes its exclusive prefix maximum, in place.
__global__ __launch_bounds__(EF_SCAN_NT) void k_ef_scan(int64_t len, uint2* data) {
    __shared__ uint2 part[EF_SCAN_NT];
    block_exclusive_prefix<EF_SCAN_NT>(part, len, data, EfMax{});
}

// grid ceil(n / NT).  idx: the sorted event indices (every pixel's run ascending); m, tilepre: the scan as k_ef_scan_tiles and
// k_ef_scan leave it; keep (n) as k_ef_keep wrote it; kept0, kept1 (npix) the carried last_kept maps; pol (n) or NULL; mask (npix)
// or NULL.
__global__ __launch_bounds__(NT) void k_ef_support(int H, int W, int64_t n, const int16_t* __restrict__ xs, const int16_t* __restrict__ ys,
                                                   const double* __restrict__ ts, const int8_t* __restrict__ pol, double tau, int radius,
                                                   int full_support, int polarity, const uint8_t* __restrict__ mask,
                                                   const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                   const uint32_t* __restrict__ idx, const uint2* __restrict__ m,
                                                   const uint2* __restrict__ tilepre, const uint8_t* __restrict__ keep,
                                                   const double* __restrict__ kept0, const double* __restrict__ kept1,
                                                   float* __restrict__ weights, uint8_t* __restrict__ support) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= n) return;
    const bool kept = keep[e] != 0;
    int s = 0;
    if (kept && radius > 0) {                                 // (a kept event's pixel is not masked)
        const int x = xs[e], y = ys[e];
        const double te = ts[e];
        const int p = y * W + x;
        const int cls = pol ? ef_class(pol[e]) : 0;
        const EsWindow w = es_window(H, W, x, y, radius);
        for (int qy = w.y0; qy <= w.y1; ++qy)
            for (int qx = w.x0; qx <= w.x1; ++qx) {
                const int q = qy * W + qx;
                if (q == p || (mask && mask[q])) continue;
                const uint32_t first = lo[q];
                const uint32_t a = es_run_lower_bound(idx, first, hi[q], (uint32_t)e);
                uint32_t last = 0u;                           // one past the position of q's last kept event below e that counts
                if (a > first) {
                    const uint2 sc = ef_scanned(m, tilepre, a - 1u);
                    last = polarity ? (cls ? sc.y : sc.x) : (sc.x > sc.y ? sc.x : sc.y);
                }
                // (last > first: a position of q's run, at or before a - 1, so its index is below e: never read past the chunk)
                const double tp = last > first ? ts[idx[last - 1u]] : ef_last_kept(kept0[q], kept1[q], cls, polarity != 0);
                s += es_supported(te, tp, tau) ? 1 : 0;
            }
    }
    support[e] = (uint8_t)s;
    weights[e] = ef_weight(kept, s, radius, full_support);
}

// grid ceil(npix / NT).  After a chunk the maps hold, per pixel, the time of its last event and of its last kept event of each class.
__global__ __launch_bounds__(NT) void k_ef_map(int64_t npix, int64_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                               const uint32_t* __restrict__ idx, const uint2* __restrict__ m,
                                               const uint2* __restrict__ tilepre, const double* __restrict__ ts,
                                               double* __restrict__ last_any, double* __restrict__ kept0, double* __restrict__ kept1) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= npix) return;
    const uint32_t a = lo[p], b = hi[p];
    if (b <= a || b > n) return;
    last_any[p] = ts[idx[b - 1u]];
    const uint2 sc = ef_scanned(m, tilepre, b - 1u);
    if (sc.x > a) kept0[p] = ts[idx[sc.x - 1u]];
    if (sc.y > a) kept1[p] = ts[idx[sc.y - 1u]];
}

}   // namespace eincm
