// eincm_lbfgs.hip.h — the limited-memory form of the BFGS state in HBM: the inverse Hessian of a window is a ring
// of at most m pairs (s, y) instead of an n x n matrix, so n is bounded by memory alone (a dense 480 x 640 theta has 614400 unknowns).
//
// The state machine, the line searches and the scalars are those of eincm_bfgs.hip.h; only what an accept does with the vectors differs.
// Per window: X, G, P, Xt, Gt (n), the ring S, Y (m, n) indexed by RING SLOT (nothing is ever shifted), its head (slot of the oldest
// pair) and count c, the dot matrix D (2m+1, 2m+1) and the coefficients delta (2m+1), both indexed by slot as well: s of slot k at k, y
// of slot k at m + k, g at 2m.  With the basis b = [s_0 .. s_{c-1}, y_0 .. y_{c-1}, g] (oldest pair first) and D[u][v] = b_u . b_v the
// two-loop recursion needs no vector at all ("vector-free" L-BFGS): it runs on D and ends in the coefficients of P = sum_j delta_j b_j.
// An accept is four launches:
//   k_lbfgs_dots    grid (chunk, window)  s = a P, y = Gt - G into the staging rows; per-chunk partials of s, y, Gt against every ring slot
//                                         and against each other (6 m + 6 dots, one ring slot at a time: six accumulators live at once)
//   k_lbfgs_coef    one wave per window   partials summed in chunk order; the pair is kept iff y.s > 2^-52 y.y (the oldest leaves a full
//                                         ring); the rows of D of the new s, y and g; the recursion, sequentially, on D in LDS
//   k_lbfgs_dir     grid (chunk, window)  X <- Xt, G <- Gt, the kept pair from the staging rows into its slot, P = sum_j delta_j b_j in
//                                         basis order with every product rounded; partials of G.P, P.P, G.G, max|P|, max|X|, max|G|
//   k_lbfgs_finish  one wave per window   those partials in chunk order -> the EINCM_BFGS_S_* scalars in pinned host memory
// and the reduction after an evaluation has the same two stages (k_lbfgs_reduce, k_lbfgs_reduce_fin).
//
// Rules: those of eincm_bfgs.hip.h.  float64, no contraction, no floating-point atomics; every sum has an association fixed by (n, m):
// a lane adds its four elements (two 16-byte loads: n = 2 h w is even, every row is 16-byte aligned) in ascending order, the 64 lanes
// combine in the fixed butterfly, the waves in wave order, the chunks in index order.  Windows outside a launch's mask keep every bit.
#pragma once
#include "eincm_bfgs.hip.h"

namespace eincm {

constexpr int LBFGS_MAX_M = 16;                  // EINCM_LBFGS_MAX_HISTORY
constexpr int LBFGS_NT = 128;                    // threads per workgroup of the sweeps
constexpr int LBFGS_NW = LBFGS_NT / 64;
constexpr int LBFGS_CHUNK = 4 * LBFGS_NT;        // elements per workgroup: lane t takes (2t, 2t+1) and (2t, 2t+1) + 2 NT
constexpr int LBFGS_NX = 6;                      // dots among the new vectors: s.s, s.y, y.y, s.g, y.g, g.g
constexpr int LBFGS_NP = 6;                      // partials of the direction sweep: G.P, P.P, G.G, max|P|, max|X|, max|G|
constexpr int LBFGS_MAX_NQ = 6 * LBFGS_MAX_M + LBFGS_NX;
constexpr int LBFGS_MAX_D = 2 * LBFGS_MAX_M + 1;
constexpr double LBFGS_EPS = 2.220446049250313e-16;      // the pair is kept iff y.s > LBFGS_EPS * y.y (SciPy's L-BFGS-B)

__host__ __device__ constexpr int lbfgs_nq(int m) { return 6 * m + LBFGS_NX; }
__host__ __device__ constexpr int lbfgs_chunks(int n) { return (n + LBFGS_CHUNK - 1) / LBFGS_CHUNK; }

struct Lb4 { double2 v[2]; };                    // a lane's four elements of a row

__device__ __forceinline__ Lb4 lb_load(const double* __restrict__ row, int j0, int n) {
    Lb4 r;
    for (int e = 0; e < 2; ++e) {
        const int j = j0 + 2 * LBFGS_NT * e;
        r.v[e] = (j < n) ? *reinterpret_cast<const double2*>(row + j) : make_double2(0.0, 0.0);
    }
    return r;
}

__device__ __forceinline__ void lb_store(double* __restrict__ row, int j0, int n, const Lb4& a) {
    for (int e = 0; e < 2; ++e) {
        const int j = j0 + 2 * LBFGS_NT * e;
        if (j < n) *reinterpret_cast<double2*>(row + j) = a.v[e];
    }
}

// a lane's part of a dot product: its elements in ascending order (elements past n are zeros on both sides)
__device__ __forceinline__ double lb_dot(const Lb4& a, const Lb4& b) {
#pragma clang fp contract(off)
    double r = a.v[0].x * b.v[0].x;
    r += a.v[0].y * b.v[0].y;
    r += a.v[1].x * b.v[1].x;
    r += a.v[1].y * b.v[1].y;
    return r;
}

__device__ __forceinline__ double lb_absmax(const Lb4& a) {
    double r = bfgs_nanmax(0.0, fabs(a.v[0].x));
    r = bfgs_nanmax(r, fabs(a.v[0].y));
    r = bfgs_nanmax(r, fabs(a.v[1].x));
    return bfgs_nanmax(r, fabs(a.v[1].y));
}

// zeros past n (a product with an infinite factor must not leave a NaN where the row has no element)
__device__ __forceinline__ void lb_clip(Lb4& a, int j0, int n) {
    for (int e = 0; e < 2; ++e)
        if (j0 + 2 * LBFGS_NT * e >= n) a.v[e] = make_double2(0.0, 0.0);
}

__device__ __forceinline__ int lb_slot(int head, int i, int m) { const int k = head + i; return k >= m ? k - m : k; }

// grid (chunks, B): P = G = 0 and an empty ring for the windows of the mask
__global__ __launch_bounds__(LBFGS_NT) void k_lbfgs_begin(int n, unsigned long long mask, double* __restrict__ P, double* __restrict__ G,
                                                          int* __restrict__ head, int* __restrict__ count, int* __restrict__ stored) {
    const int b = blockIdx.y;
    if (!bfgs_on(mask, b)) return;
    const int j0 = blockIdx.x * LBFGS_CHUNK + 2 * threadIdx.x;
    Lb4 z;
    z.v[0] = z.v[1] = make_double2(0.0, 0.0);
    lb_store(P + (size_t)b * n, j0, n, z);
    lb_store(G + (size_t)b * n, j0, n, z);
    if (blockIdx.x == 0 && threadIdx.x == 0) { head[b] = 0; count[b] = 0; stored[b] = 0; }
}

// grid (chunks, B): Gt <- Gsrc (if given: the engine's gradient block); part[(b, chunk)] = { Gt . P, max|Gt| } of the chunk
__global__ __launch_bounds__(LBFGS_NT) void k_lbfgs_reduce(int n, unsigned long long mask, const double* __restrict__ Gsrc,
                                                           double* __restrict__ Gt, const double* __restrict__ P, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[LBFGS_NW][2];
    const int b = blockIdx.y;
    if (!bfgs_on(mask, b)) return;
    const size_t vb = (size_t)b * n;
    const int j0 = blockIdx.x * LBFGS_CHUNK + 2 * threadIdx.x;
    Lb4 g;
    if (Gsrc) { g = lb_load(Gsrc + vb, j0, n); lb_store(Gt + vb, j0, n, g); } else g = lb_load(Gt + vb, j0, n);
    const Lb4 p = lb_load(P + vb, j0, n);
    const double dot = bfgs_wave_sum(lb_dot(g, p));
    const double mx = bfgs_wave_max(lb_absmax(g));
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = dot; red[threadIdx.x >> 6][1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double d = red[0][0], x = red[0][1];
        for (int k = 1; k < LBFGS_NW; ++k) { d += red[k][0]; x = bfgs_nanmax(x, red[k][1]); }
        double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        o[0] = d; o[1] = x;
    }
}

// grid (B), one wave: the chunks' partials in index order -> out[b] = { Gt . P, max|Gt| } in pinned host memory
__global__ __launch_bounds__(64) void k_lbfgs_reduce_fin(int chunks, unsigned long long mask, const double* __restrict__ part,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.x;
    if (!bfgs_on(mask, b) || threadIdx.x >= 2) return;
    const double* p = part + (size_t)b * chunks * 2 + threadIdx.x;
    double acc = p[0];
    if (threadIdx.x == 0) for (int k = 1; k < chunks; ++k) acc += p[2 * k];
    else for (int k = 1; k < chunks; ++k) acc = bfgs_nanmax(acc, p[2 * k]);
    out[2 * b + threadIdx.x] = acc;
}

// grid (chunks, B), windows of upd | init.  upd: s = a P (the product rounded: k_bfgs_trial's step) and y = Gt - G into the staging rows
// Sn, Yn, and the chunk's partials part[(b, chunk)][q] of
//   q = 6 k + { 0: s.S_k, 1: s.Y_k, 2: y.S_k, 3: y.Y_k, 4: g.S_k, 5: g.Y_k }    for every filled ring slot k (g = Gt)
//   q = 6 m + { 0: s.s, 1: s.y, 2: y.y, 3: s.g, 4: y.g, 5: g.g }
// init: g.g alone.  One ring slot is in registers at a time.
__global__ __launch_bounds__(LBFGS_NT) void k_lbfgs_dots(int n, int m, unsigned long long upd, unsigned long long init, BfgsAlpha al,
                                                         const double* __restrict__ G, const double* __restrict__ Gt,
                                                         const double* __restrict__ P, const double* __restrict__ S,
                                                         const double* __restrict__ Y, const int* __restrict__ head,
                                                         const int* __restrict__ count, double* __restrict__ Sn, double* __restrict__ Yn,
                                                         double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[LBFGS_NW][LBFGS_MAX_NQ];
    const int b = blockIdx.y;
    const bool u = bfgs_on(upd, b);
    if (!u && !bfgs_on(init, b)) return;
    const int nq = lbfgs_nq(m);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = threadIdx.x; q < nq; q += LBFGS_NT)
        for (int k = 0; k < LBFGS_NW; ++k) red[k][q] = 0.0;
    __syncthreads();
    const size_t vb = (size_t)b * n;
    const int j0 = blockIdx.x * LBFGS_CHUNK + 2 * threadIdx.x;
    const Lb4 g = lb_load(Gt + vb, j0, n);
    Lb4 s, y;
    s.v[0] = s.v[1] = y.v[0] = y.v[1] = make_double2(0.0, 0.0);
    double* rw = red[wave];
    if (u) {
        const Lb4 p = lb_load(P + vb, j0, n), g0 = lb_load(G + vb, j0, n);
        const double a = al.a[b];
        for (int e = 0; e < 2; ++e) {
            s.v[e].x = a * p.v[e].x; s.v[e].y = a * p.v[e].y;
            y.v[e].x = g.v[e].x - g0.v[e].x; y.v[e].y = g.v[e].y - g0.v[e].y;
        }
        lb_clip(s, j0, n);
        lb_store(Sn + vb, j0, n, s);
        lb_store(Yn + vb, j0, n, y);
        const int c = count[b], h = head[b];
        for (int i = 0; i < c; ++i) {
            const int k = lb_slot(h, i, m);
            const size_t rb = ((size_t)b * m + k) * n;
            const Lb4 sk = lb_load(S + rb, j0, n), yk = lb_load(Y + rb, j0, n);
            const double d0 = bfgs_wave_sum(lb_dot(s, sk)), d1 = bfgs_wave_sum(lb_dot(s, yk));
            const double d2 = bfgs_wave_sum(lb_dot(y, sk)), d3 = bfgs_wave_sum(lb_dot(y, yk));
            const double d4 = bfgs_wave_sum(lb_dot(g, sk)), d5 = bfgs_wave_sum(lb_dot(g, yk));
            if (lane == 0) { double* o = rw + 6 * k; o[0] = d0; o[1] = d1; o[2] = d2; o[3] = d3; o[4] = d4; o[5] = d5; }
        }
        const double ss = bfgs_wave_sum(lb_dot(s, s)), sy = bfgs_wave_sum(lb_dot(s, y)), yy = bfgs_wave_sum(lb_dot(y, y));
        const double sg = bfgs_wave_sum(lb_dot(s, g)), yg = bfgs_wave_sum(lb_dot(y, g));
        if (lane == 0) { double* o = rw + 6 * m; o[0] = ss; o[1] = sy; o[2] = yy; o[3] = sg; o[4] = yg; }
    }
    const double gg = bfgs_wave_sum(lb_dot(g, g));
    if (lane == 0) rw[6 * m + 5] = gg;
    __syncthreads();
    double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * nq;
    for (int q = threadIdx.x; q < nq; q += LBFGS_NT) {
        double r = red[0][q];
        for (int k = 1; k < LBFGS_NW; ++k) r += red[k][q];
        o[q] = r;
    }
}

// The recursion on D (slot-indexed, row stride nd = 2m+1) -> delta (slot-indexed); a: m doubles of scratch.  Every sum runs over the
// basis in its order (s oldest .. newest, y oldest .. newest, g), one rounded product added at a time.
__device__ __forceinline__ void lb_recursion(const double* D, double* delta, double* a, int m, int head, int c, int scale) {
#pragma clang fp contract(off)
    const int nd = 2 * m + 1;
    for (int u = 0; u < nd; ++u) delta[u] = 0.0;
    delta[2 * m] = -1.0;
    for (int i = c - 1; i >= 0; --i) {
        const int ki = lb_slot(head, i, m);
        double acc = 0.0;
        for (int j = 0; j < c; ++j) { const int u = lb_slot(head, j, m); acc += delta[u] * D[u * nd + ki]; }
        for (int j = 0; j < c; ++j) { const int u = m + lb_slot(head, j, m); acc += delta[u] * D[u * nd + ki]; }
        acc += delta[2 * m] * D[2 * m * nd + ki];
        a[i] = acc / D[ki * nd + m + ki];
        delta[m + ki] -= a[i];
    }
    if (scale && c > 0) {
        const int kl = lb_slot(head, c - 1, m);
        const double gamma = D[kl * nd + m + kl] / D[(m + kl) * nd + m + kl];
        for (int j = 0; j < c; ++j) delta[lb_slot(head, j, m)] *= gamma;
        for (int j = 0; j < c; ++j) delta[m + lb_slot(head, j, m)] *= gamma;
        delta[2 * m] *= gamma;
    }
    for (int i = 0; i < c; ++i) {
        const int ki = lb_slot(head, i, m);
        double acc = 0.0;
        for (int j = 0; j < c; ++j) { const int u = lb_slot(head, j, m); acc += delta[u] * D[u * nd + m + ki]; }
        for (int j = 0; j < c; ++j) { const int u = m + lb_slot(head, j, m); acc += delta[u] * D[u * nd + m + ki]; }
        acc += delta[2 * m] * D[2 * m * nd + m + ki];
        const double beta = acc / D[ki * nd + m + ki];
        const double t = a[i] - beta;
        delta[ki] += t;
    }
}

// grid (B), one wave, windows of upd | init: the chunks' partials in index order, the ring's bookkeeping, D's new rows, delta.
// ysyy[b] = { y.s, y.y } of an update.
__global__ __launch_bounds__(64) void k_lbfgs_coef(int chunks, int m, int scale, unsigned long long upd, unsigned long long init,
                                                   const double* __restrict__ part, double* __restrict__ Dg, double* __restrict__ deltag,
                                                   int* __restrict__ head, int* __restrict__ count, int* __restrict__ stored,
                                                   double* __restrict__ ysyy) {
#pragma clang fp contract(off)
    __shared__ double D[LBFGS_MAX_D * LBFGS_MAX_D];
    __shared__ double Q[LBFGS_MAX_NQ];
    __shared__ double delta[LBFGS_MAX_D];
    __shared__ double a[LBFGS_MAX_M];
    const int b = blockIdx.x;
    const bool u = bfgs_on(upd, b);
    if (!u && !bfgs_on(init, b)) return;
    const int nq = lbfgs_nq(m), nd = 2 * m + 1, lane = threadIdx.x;
    int h = u ? head[b] : 0, c = u ? count[b] : 0;
    // which partials exist: the filled slots' six (updates) and the cross terms (g.g alone at an init)
    for (int q = lane; q < nq; q += 64) {
        bool live;
        if (q >= 6 * m) live = u || q == 6 * m + 5;
        else { const int k = q / 6; int i = k - h; if (i < 0) i += m; live = u && i < c; }
        double acc = 0.0;
        if (live) {
            const double* p = part + (size_t)b * chunks * nq + q;
            acc = p[0];
            for (int k = 1; k < chunks; ++k) acc += p[(size_t)k * nq];
        }
        Q[q] = acc;
    }
    double* Db = Dg + (size_t)b * nd * nd;
    for (int e = lane; e < nd * nd; e += 64) D[e] = u ? Db[e] : 0.0;
    __syncthreads();
    const double* X = Q + 6 * m;
    int keep = 0, t = 0;
    if (u) {
        keep = X[1] > LBFGS_EPS * X[2];
        if (keep) {
            t = lb_slot(h, c, m);                      // the free slot, or the oldest pair's when the ring is full
            if (c == m) h = lb_slot(h, 1, m); else ++c;
        }
    }
    // rows of the new s and y (a kept pair) and of g against the pairs that stay, one pair per lane
    for (int i = lane; i < c; i += 64) {
        const int k = lb_slot(h, i, m);
        if (keep && k == t) continue;
        const double* q = Q + 6 * k;
        if (keep) {
            D[t * nd + k] = D[k * nd + t] = q[0];
            D[t * nd + m + k] = D[(m + k) * nd + t] = q[1];
            D[(m + t) * nd + k] = D[k * nd + m + t] = q[2];
            D[(m + t) * nd + m + k] = D[(m + k) * nd + m + t] = q[3];
        }
        D[2 * m * nd + k] = D[k * nd + 2 * m] = q[4];
        D[2 * m * nd + m + k] = D[(m + k) * nd + 2 * m] = q[5];
    }
    if (lane == 0) {
        if (keep) {
            D[t * nd + t] = X[0];
            D[t * nd + m + t] = D[(m + t) * nd + t] = X[1];
            D[(m + t) * nd + m + t] = X[2];
            D[t * nd + 2 * m] = D[2 * m * nd + t] = X[3];
            D[(m + t) * nd + 2 * m] = D[2 * m * nd + m + t] = X[4];
        }
        D[2 * m * nd + 2 * m] = X[5];
    }
    __syncthreads();
    if (lane == 0) lb_recursion(D, delta, a, m, h, c, scale);
    __syncthreads();
    for (int e = lane; e < nd * nd; e += 64) Db[e] = D[e];
    for (int e = lane; e < nd; e += 64) deltag[(size_t)b * nd + e] = delta[e];
    if (lane == 0) {
        head[b] = h; count[b] = c; stored[b] = keep;
        ysyy[2 * b] = u ? X[1] : 0.0; ysyy[2 * b + 1] = u ? X[2] : 0.0;
    }
}

// grid (chunks, B), windows of act: X <- Xt, G <- Gt; unless the window only moves (act without upd or init), the pair kept by this
// accept goes from the staging rows into its slot and P = sum_j delta_j b_j over the basis in its order, the first product taken as
// it is and each later one rounded before it is added.  part[(b, chunk)] = { G.P, P.P, G.G, max|P|, max|X|, max|G| } of the chunk.
__global__ __launch_bounds__(LBFGS_NT) void k_lbfgs_dir(int n, int m, unsigned long long act, unsigned long long upd, unsigned long long init,
                                                        double* __restrict__ X, const double* __restrict__ Xt, double* __restrict__ G,
                                                        const double* __restrict__ Gt, double* __restrict__ P, double* __restrict__ S,
                                                        double* __restrict__ Y, const double* __restrict__ Sn, const double* __restrict__ Yn,
                                                        const double* __restrict__ deltag, const int* __restrict__ head,
                                                        const int* __restrict__ count, const int* __restrict__ stored,
                                                        double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[LBFGS_NW][LBFGS_NP];
    __shared__ double delta[LBFGS_MAX_D];
    const int b = blockIdx.y;
    if (!bfgs_on(act, b)) return;
    const bool dir = bfgs_on(upd, b) || bfgs_on(init, b);
    const int nd = 2 * m + 1;
    if (dir) for (int e = threadIdx.x; e < nd; e += LBFGS_NT) delta[e] = deltag[(size_t)b * nd + e];
    __syncthreads();
    const size_t vb = (size_t)b * n;
    const int j0 = blockIdx.x * LBFGS_CHUNK + 2 * threadIdx.x;
    const Lb4 x = lb_load(Xt + vb, j0, n), g = lb_load(Gt + vb, j0, n);
    lb_store(X + vb, j0, n, x);
    lb_store(G + vb, j0, n, g);
    Lb4 p;
    if (dir) {
        const int c = count[b], h = head[b];
        const bool kept = bfgs_on(upd, b) && stored[b] != 0;
        bool first = true;
        for (int half = 0; half < 2; ++half) {                 // the s of every pair, then the y
            const double* ring = half ? Y : S;
            const double* fresh = half ? Yn : Sn;
            for (int i = 0; i < c; ++i) {
                const int k = lb_slot(h, i, m);
                const size_t rb = ((size_t)b * m + k) * n;
                Lb4 v;
                if (kept && i == c - 1) { v = lb_load(fresh + vb, j0, n); lb_store((half ? Y : S) + rb, j0, n, v); }
                else v = lb_load(ring + rb, j0, n);
                const double d = delta[half * m + k];
                for (int e = 0; e < 2; ++e) {
                    const double tx = d * v.v[e].x, ty = d * v.v[e].y;
                    if (first) { p.v[e].x = tx; p.v[e].y = ty; } else { p.v[e].x += tx; p.v[e].y += ty; }
                }
                first = false;
            }
        }
        const double d = delta[2 * m];
        for (int e = 0; e < 2; ++e) {
            const double tx = d * g.v[e].x, ty = d * g.v[e].y;
            if (first) { p.v[e].x = tx; p.v[e].y = ty; } else { p.v[e].x += tx; p.v[e].y += ty; }
        }
        lb_store(P + vb, j0, n, p);
        lb_clip(p, j0, n);
    } else p = lb_load(P + vb, j0, n);
    const double gp = bfgs_wave_sum(lb_dot(g, p)), pp = bfgs_wave_sum(lb_dot(p, p)), gg = bfgs_wave_sum(lb_dot(g, g));
    const double pm = bfgs_wave_max(lb_absmax(p)), xm = bfgs_wave_max(lb_absmax(x)), gm = bfgs_wave_max(lb_absmax(g));
    if ((threadIdx.x & 63) == 0) {
        double* o = red[threadIdx.x >> 6];
        o[0] = gp; o[1] = pp; o[2] = gg; o[3] = pm; o[4] = xm; o[5] = gm;
    }
    __syncthreads();
    if (threadIdx.x < LBFGS_NP) {
        double r = red[0][threadIdx.x];
        for (int k = 1; k < LBFGS_NW; ++k) r = (threadIdx.x < 3) ? r + red[k][threadIdx.x] : bfgs_nanmax(r, red[k][threadIdx.x]);
        part[((size_t)b * gridDim.x + blockIdx.x) * LBFGS_NP + threadIdx.x] = r;
    }
}

// grid (B), one wave, windows of act: the direction sweep's partials in chunk order -> the window's EINCM_BFGS_S_* in pinned host memory
// (slot YHY holds y.y in this form)
__global__ __launch_bounds__(64) void k_lbfgs_finish(int chunks, unsigned long long act, unsigned long long upd, const double* __restrict__ part,
                                                     const double* __restrict__ ysyy, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double fin[LBFGS_NP];
    const int b = blockIdx.x;
    if (!bfgs_on(act, b)) return;
    if (threadIdx.x < LBFGS_NP) {
        const double* p = part + (size_t)b * chunks * LBFGS_NP + threadIdx.x;
        double acc = p[0];
        if (threadIdx.x < 3) for (int k = 1; k < chunks; ++k) acc += p[(size_t)k * LBFGS_NP];
        else for (int k = 1; k < chunks; ++k) acc = bfgs_nanmax(acc, p[(size_t)k * LBFGS_NP]);
        fin[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool u = bfgs_on(upd, b);
        double* o = out + (size_t)b * BFGS_NS;
        o[0] = fin[0]; o[1] = fin[5]; o[2] = sqrt(fin[1]); o[3] = fin[4]; o[4] = fin[3]; o[5] = sqrt(fin[2]);
        o[6] = u ? ysyy[2 * b] : 0.0; o[7] = u ? ysyy[2 * b + 1] : 0.0;
    }
}

}  // namespace eincm
