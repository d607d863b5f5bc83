// eincm_bfgs.hip.h — the linear algebra of B independent BFGS minimisations whose state lives in HBM.
//
// SciPy's BFGS (scipy.optimize._optimize._minimize_bfgs) keeps, per minimisation of n unknowns, the point x, its gradient g, the search
// direction p and the inverse Hessian H; its two line searches see nothing but the scalars phi(a) = f(x + a p) and phi'(a) = grad f . p.
// So the vectors stay here and the host drives the line searches with a few doubles per window and evaluation:
//   k_bfgs_begin    H = I, P = G = 0                                                         (x0 is uploaded by the host)
//   k_bfgs_trial    Xt = X + a P                                                              (the point the engine evaluates next)
//   k_bfgs_reduce   phi' = Gt . P, max|Gt|            (Gt: the engine's gradient at Xt, or whatever the caller wrote there)
//   k_bfgs_hy       s = a P, y = Gt - G, Hy = H y                                             first read of H
//   k_bfgs_update   w = (c / 2) s - r Hy, c = r (1 + r y.Hy), r = 1 / y.s (1000 where y.s == 0); H += s w^T + w s^T; P = -H' Gt;
//                   X <- Xt, G <- Gt                                                          second read and the one write of H
//   k_bfgs_scalars  G.P, max|G|, |P|_2, max|X|, max|P|, |G|_2, y.s, y.Hy -> pinned host memory
// The update is the symmetric rank-two form of SciPy's (I - r s y^T) H (I - r y s^T) + r s s^T that batch_solver._WindowBFGS
// uses above 64 unknowns.  k_bfgs_update holds a whole row of H' in registers when it writes it, so the next direction's row sum
// comes from the same pass: two reads and one write of H per accepted step.
//
// Rules (section 4.1's spirit): float64 throughout; every sum is an ordered sum in a fixed association - a lane adds its elements in
// ascending order, the 64 lanes combine in a fixed butterfly, the waves of a workgroup in wave order - so every result is the same
// bits on every call and in every context; no floating-point atomics; no contraction (s_i w_j + w_i s_j must be the same bits as
// s_j w_i + w_j s_i for H to stay bit-symmetric, which an FMA of one product into the other breaks).
// Work split: one workgroup per BFGS_ROWS rows of one window's H (n = 512, B = 8: 512 workgroups), one per window for the n-vectors.
// A window takes part in a launch iff its bit is set in the launch's mask (as Geom::wmask); the state of the others is not touched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eincm {

constexpr int BFGS_MAX_N = 1024;       // EINCM_BFGS_MAX_N: unknowns per window (the reference's pyramid tops out at 2 * 16 * 16 = 512)
constexpr int BFGS_MAX_B = 64;         // windows (one mask word)
constexpr int BFGS_NT = 256;           // threads per workgroup
constexpr int BFGS_NW = BFGS_NT / 64;  // waves per workgroup
constexpr int BFGS_ROWS = 8;           // rows of H per workgroup: two per wave
constexpr int BFGS_NS = 8;             // EINCM_BFGS_NS: scalars per window (EINCM_BFGS_S_*)

struct BfgsAlpha { double a[BFGS_MAX_B]; };      // the step of every window, in the kernel arguments

__device__ __forceinline__ bool bfgs_on(unsigned long long m, int b) { return ((m >> b) & 1ull) != 0ull; }

__device__ __forceinline__ double bfgs_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // a fixed butterfly: every lane ends with the same bits
    return v;
}

// max that keeps a NaN (numpy's np.abs(g).max() does)
__device__ __forceinline__ double bfgs_nanmax(double acc, double x) { return (x > acc || x != x) ? x : acc; }

__device__ __forceinline__ double bfgs_wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = bfgs_nanmax(v, __shfl_xor(v, o));
    return v;
}

// the workgroup's sum / max of one value per thread; red: BFGS_NW doubles of LDS; every thread gets the result
__device__ __forceinline__ double bfgs_block_sum(double v, double* red) {
    v = bfgs_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int k = 1; k < BFGS_NW; ++k) r += red[k];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double bfgs_block_max(double v, double* red) {
    v = bfgs_wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int k = 1; k < BFGS_NW; ++k) r = bfgs_nanmax(r, red[k]);
    __syncthreads();
    return r;
}

// grid (ceil(n / BFGS_ROWS), B): H = I and P = G = 0 for the windows of the mask
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_begin(int n, unsigned long long mask, double* __restrict__ H, double* __restrict__ P,
                                                        double* __restrict__ G) {
    const int b = blockIdx.y;
    if (!bfgs_on(mask, b)) return;
    const int i0 = blockIdx.x * BFGS_ROWS;
    double* Hb = H + (size_t)b * n * n;
    for (int r = 0; r < BFGS_ROWS && i0 + r < n; ++r) {
        const int i = i0 + r;
        for (int j = threadIdx.x; j < n; j += BFGS_NT) Hb[(size_t)i * n + j] = (i == j) ? 1.0 : 0.0;
    }
    if ((int)threadIdx.x < BFGS_ROWS && i0 + (int)threadIdx.x < n) {
        P[(size_t)b * n + i0 + threadIdx.x] = 0.0;
        G[(size_t)b * n + i0 + threadIdx.x] = 0.0;
    }
}

// grid (ceil(n / BFGS_NT), B): Xt = X + a P, the product rounded before the sum (numpy's xk + stp * pk)
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_trial(int n, unsigned long long mask, BfgsAlpha al, const double* __restrict__ X,
                                                        const double* __restrict__ P, double* __restrict__ Xt) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    if (!bfgs_on(mask, b)) return;
    const int i = blockIdx.x * BFGS_NT + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)b * n + i;
    const double step = al.a[b] * P[at];
    Xt[at] = X[at] + step;
}

// grid (B): Gt <- Gsrc (if given: the engine's gradient block), then out[b] = { Gt . P, max|Gt| } into pinned host memory
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_reduce(int n, unsigned long long mask, const double* __restrict__ Gsrc,
                                                         double* __restrict__ Gt, const double* __restrict__ P, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[BFGS_NW];
    const int b = blockIdx.x;
    if (!bfgs_on(mask, b)) return;
    double dot = 0.0, mx = 0.0;
    for (int i = threadIdx.x; i < n; i += BFGS_NT) {
        const size_t at = (size_t)b * n + i;
        double g;
        if (Gsrc) { g = Gsrc[at]; Gt[at] = g; } else g = Gt[at];
        dot += g * P[at];
        mx = bfgs_nanmax(mx, fabs(g));
    }
    dot = bfgs_block_sum(dot, red);
    mx = bfgs_block_max(mx, red);
    if (threadIdx.x == 0) { out[2 * b] = dot; out[2 * b + 1] = mx; }
}

// dot of row `row` (n doubles) with the LDS vector v, by one wave: lane l takes the pairs (2l, 2l + 1) + 128 k in ascending order
__device__ __forceinline__ double bfgs_row_dot(const double* __restrict__ row, const double* v, int n, int lane) {
#pragma clang fp contract(off)
    double acc = 0.0;
    if ((n & 1) == 0) {               // even n: every row starts 16-byte aligned
        for (int j = 2 * lane; j < n; j += 128) {
            const double2 h = *reinterpret_cast<const double2*>(row + j);
            acc += h.x * v[j];
            acc += h.y * v[j + 1];
        }
    } else {
        for (int j = 2 * lane; j < n; j += 128) {
            acc += row[j] * v[j];
            if (j + 1 < n) acc += row[j + 1] * v[j + 1];
        }
    }
    return bfgs_wave_sum(acc);
}

// grid (ceil(n / BFGS_ROWS), B), LDS n doubles: for the windows of the mask S = a P, Y = Gt - G, Hy = H Y (this workgroup's rows)
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_hy(int n, unsigned long long mask, BfgsAlpha al, const double* __restrict__ H,
                                                     const double* __restrict__ G, const double* __restrict__ Gt,
                                                     const double* __restrict__ P, double* __restrict__ S, double* __restrict__ Y,
                                                     double* __restrict__ Hy) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double bfgs_lds[];
    const int b = blockIdx.y;
    if (!bfgs_on(mask, b)) return;
    double* y = bfgs_lds;
    const size_t vb = (size_t)b * n;
    for (int j = threadIdx.x; j < n; j += BFGS_NT) y[j] = Gt[vb + j] - G[vb + j];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* Hb = H + (size_t)b * n * n;
    for (int r = wave; r < BFGS_ROWS; r += BFGS_NW) {
        const int i = blockIdx.x * BFGS_ROWS + r;
        if (i >= n) break;
        const double hy = bfgs_row_dot(Hb + (size_t)i * n, y, n, lane);
        if (lane == 0) {
            Hy[vb + i] = hy;
            S[vb + i] = al.a[b] * P[vb + i];
            Y[vb + i] = y[i];
        }
    }
}

// grid (ceil(n / BFGS_ROWS), B), LDS 3 n doubles.  Windows of `upd`: w from (S, Y, Hy), this workgroup's rows of H += s w^T + w s^T and of
// P = -H' Gt.  Windows of `act` (a superset of upd): X <- Xt, G <- Gt; those of `init` as well: P = -Gt (H = I: the first direction).
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_update(int n, unsigned long long act, unsigned long long upd, unsigned long long init,
                                                         double* __restrict__ H, const double* __restrict__ S, const double* __restrict__ Y,
                                                         const double* __restrict__ Hy, double* __restrict__ X, const double* __restrict__ Xt,
                                                         double* __restrict__ G, const double* __restrict__ Gt, double* __restrict__ P) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double bfgs_lds[];
    __shared__ double red[BFGS_NW];
    const int b = blockIdx.y;
    if (!bfgs_on(act, b)) return;
    const size_t vb = (size_t)b * n;
    const int i0 = blockIdx.x * BFGS_ROWS;
    if (bfgs_on(upd, b)) {
        double* s = bfgs_lds;
        double* w = bfgs_lds + n;
        double* g = bfgs_lds + 2 * n;
        double ys = 0.0, yhy = 0.0;
        for (int j = threadIdx.x; j < n; j += BFGS_NT) {
            const double sj = S[vb + j], yj = Y[vb + j], hyj = Hy[vb + j];
            s[j] = sj; w[j] = hyj; g[j] = Gt[vb + j];
            ys += yj * sj;
            yhy += yj * hyj;
        }
        ys = bfgs_block_sum(ys, red);            // (the barrier inside also publishes s, w = Hy and g)
        yhy = bfgs_block_sum(yhy, red);
        const double rho = (ys == 0.0) ? 1000.0 : 1.0 / ys;
        const double coef = (0.5 * rho) * (1.0 + rho * yhy);
        for (int j = threadIdx.x; j < n; j += BFGS_NT) w[j] = coef * s[j] - rho * w[j];
        __syncthreads();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        double* Hb = H + (size_t)b * n * n;
        for (int r = wave; r < BFGS_ROWS; r += BFGS_NW) {
            const int i = i0 + r;
            if (i >= n) break;
            double* row = Hb + (size_t)i * n;
            const double si = s[i], wi = w[i];
            double acc = 0.0;
            if ((n & 1) == 0) {
                for (int j = 2 * lane; j < n; j += 128) {
                    double2 h = *reinterpret_cast<const double2*>(row + j);
                    // both products are rounded, then added: the same bits at (i, j) and (j, i)
                    h.x = h.x + (si * w[j] + wi * s[j]);
                    h.y = h.y + (si * w[j + 1] + wi * s[j + 1]);
                    *reinterpret_cast<double2*>(row + j) = h;
                    acc += h.x * g[j];
                    acc += h.y * g[j + 1];
                }
            } else {
                for (int j = 2 * lane; j < n; j += 128) {
                    const double h0 = row[j] + (si * w[j] + wi * s[j]);
                    row[j] = h0;
                    acc += h0 * g[j];
                    if (j + 1 < n) {
                        const double h1 = row[j + 1] + (si * w[j + 1] + wi * s[j + 1]);
                        row[j + 1] = h1;
                        acc += h1 * g[j + 1];
                    }
                }
            }
            acc = bfgs_wave_sum(acc);
            if (lane == 0) P[vb + i] = -acc;
        }
    }
    if ((int)threadIdx.x < BFGS_ROWS && i0 + (int)threadIdx.x < n) {
        const size_t at = vb + i0 + threadIdx.x;
        const double gt = Gt[at];
        X[at] = Xt[at];
        G[at] = gt;
        if (bfgs_on(init, b)) P[at] = -gt;
    }
}

// grid (B): the scalars the host's line search and stopping rules need of the new iterate, into pinned host memory (BFGS_NS per window)
__global__ __launch_bounds__(BFGS_NT) void k_bfgs_scalars(int n, unsigned long long mask, const double* __restrict__ X,
                                                          const double* __restrict__ G, const double* __restrict__ P,
                                                          const double* __restrict__ S, const double* __restrict__ Y,
                                                          const double* __restrict__ Hy, unsigned long long upd, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[BFGS_NW];
    const int b = blockIdx.x;
    if (!bfgs_on(mask, b)) return;
    const bool u = bfgs_on(upd, b);
    double gp = 0.0, gmax = 0.0, pp = 0.0, xmax = 0.0, pmax = 0.0, gg = 0.0, ys = 0.0, yhy = 0.0;
    for (int i = threadIdx.x; i < n; i += BFGS_NT) {
        const size_t at = (size_t)b * n + i;
        const double x = X[at], g = G[at], p = P[at];
        gp += g * p;
        pp += p * p;
        gg += g * g;
        gmax = bfgs_nanmax(gmax, fabs(g));
        xmax = bfgs_nanmax(xmax, fabs(x));
        pmax = bfgs_nanmax(pmax, fabs(p));
        if (u) { const double y = Y[at]; ys += y * S[at]; yhy += y * Hy[at]; }
    }
    gp = bfgs_block_sum(gp, red);
    pp = bfgs_block_sum(pp, red);
    gg = bfgs_block_sum(gg, red);
    ys = bfgs_block_sum(ys, red);
    yhy = bfgs_block_sum(yhy, red);
    gmax = bfgs_block_max(gmax, red);
    xmax = bfgs_block_max(xmax, red);
    pmax = bfgs_block_max(pmax, red);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)b * BFGS_NS;
        o[0] = gp; o[1] = gmax; o[2] = sqrt(pp); o[3] = xmax; o[4] = pmax; o[5] = sqrt(gg); o[6] = ys; o[7] = yhy;
    }
}

}  // namespace eincm
