// eincm_label_prior.hip.h — k_label_prior: the per-pixel label prior of the E-step (eincm_label_prior).  The
// staged batch is G groups of K consecutive windows; k_ml_mass (eincm_motion_layers.hip.h) has left M (G, K, H, W), every model's
// quantised staged weights summed per pixel.  Per (group, pixel) this kernel takes the box sum S_l of every model's M over the
// (2r + 1)^2 window clipped to the sensor and hands the K sums to lp_prior (eincm_label_prior.h), which holds the arithmetic.
//
// The fused form: one workgroup serves one (32x32 tile, group) and walks the K models, one thread per pixel of the tile, the thread's
// K sums in registers (the model loop is unrolled over the template's K, so S[] and P[] are never indexed at run time: no scratch),
// so the normalisation needs no second pass over HBM.  Per model the tile and its halo of r go into LDS once, each cell by one
// predicated load (a cell outside the sensor is 0 and its address is never formed into a load), the row sums into a second LDS array
// as uint64, and every thread adds its column of 2r + 1 row sums.  Everything up to lp_prior's division is integer, every output cell
// has one owner, and there is no atomic: any launch shape gives the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eincm_kernels.hip.h"
#include "eincm_label_prior.h"

namespace eincm {

constexpr int LP_NT = TS * TS;                                       // one thread per pixel of the tile
constexpr int LP_SIDE_MAX = TS + 2 * EINCM_LP_MAX_RADIUS;            // 48: the tile with the widest halo

struct LpGeom {
    int H, W, tilesX, r;
    uint32_t floor_mass;
};

// grid (ntiles, G), LP_NT threads, 9 KiB + 12 KiB of static LDS.
//   mass (G, K, H, W) as k_ml_mass wrote it.  prior (G * K, H, W) and smoothed (G, K, H, W): this workgroup's 32x32 block of every
//   model's image, clipped to the sensor; smoothed may be nullptr.
// Bank conflicts: none.  The row pass reads `side` words apart per row and consecutive words per lane; the column pass reads
// consecutive 8-byte words per lane.
template <int K>
__global__ __launch_bounds__(LP_NT) void k_label_prior(LpGeom g, const uint32_t* __restrict__ mass, float* __restrict__ prior,
                                                       unsigned long long* __restrict__ smoothed)
{
    __shared__ uint32_t cell[LP_SIDE_MAX * LP_SIDE_MAX];
    __shared__ unsigned long long rows[LP_SIDE_MAX * TS];
    const int tile = blockIdx.x, grp = blockIdx.y, r = g.r, side = TS + 2 * r;
    const int x0 = (tile % g.tilesX) * TS, y0 = (tile / g.tilesX) * TS;
    const int tx = threadIdx.x & (TS - 1), ty = threadIdx.x / TS;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < g.W && y < g.H;
    const size_t npix = (size_t)g.H * g.W;
    uint64_t S[K];
#pragma unroll
    for (int l = 0; l < K; ++l) {
        const uint32_t* m = mass + ((size_t)grp * K + l) * npix;
        for (int i = threadIdx.x; i < side * side; i += LP_NT) {
            const int cx = x0 - r + i % side, cy = y0 - r + i / side;
            uint32_t v = 0u;
            if (cx >= 0 && cx < g.W && cy >= 0 && cy < g.H) v = m[(size_t)cy * g.W + cx];
            cell[i] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < side * TS; i += LP_NT) {      // row sums: row i / TS of the halo'd tile, column i % TS of the tile
            const uint32_t* c = cell + (i / TS) * side + (i & (TS - 1));
            unsigned long long s = 0ull;
            for (int d = 0; d <= 2 * r; ++d) s += c[d];
            rows[i] = s;
        }
        __syncthreads();
        unsigned long long s = 0ull;
        for (int d = 0; d <= 2 * r; ++d) s += rows[(ty + d) * TS + tx];
        S[l] = s;
        // (the next model's cells are written while others still add rows[]; its row pass waits at the barrier after the loads)
    }
    if (!inside) return;
    const size_t p = (size_t)y * g.W + x;
    float P[K];
    lp_prior(S, K, g.floor_mass, P);
#pragma unroll
    for (int l = 0; l < K; ++l) {
        prior[((size_t)grp * K + l) * npix + p] = P[l];
        if (smoothed) smoothed[((size_t)grp * K + l) * npix + p] = S[l];
    }
}

// k_label_prior<K> for a call's K (1 .. EINCM_RS_MAX_MODELS, checked by lp_check before)
template <int K = 1> static auto lp_kernel(int n_models) -> decltype(&k_label_prior<1>) {
    if constexpr (K < EINCM_RS_MAX_MODELS) { if (n_models != K) return lp_kernel<K + 1>(n_models); }
    return k_label_prior<K>;
}

}   // namespace eincm
