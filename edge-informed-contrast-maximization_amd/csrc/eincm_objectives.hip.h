// eincm_objectives.hip.h — the selectable contrast / correlation kinds of the differentiable loss (gfx950).
//
// The default kinds (grad-mag contrast, MSE correlation) run the image pass of eincm_kernels.hip.h unchanged.  Any other
// combination replaces k_imgrad by the two kernels here:
//   k_obj_parts  grid (ncells, R, B): per-cell partial sums that do not depend on the image statistics (moments of I and E over the
//                whole cell and over its whole tile, the tile-local and whole-image Scharr energies and the cross terms the joint
//                contrast needs).  A cell is one th x tw tile; the last cell of a tile row / column also owns the ragged remainder,
//                so the cells partition the image.
//   k_obj_grad   grid (ceil(nig / 4), R, B), one k_imgrad strip per wave: reduces the cell partials of its image in a fixed order,
//                forms the objective values and the per-image coefficients, writes dL/dIWE (with the tie terms at the arg-min and
//                arg-max of the normalisation) and the per-strip max |dL/dIWE| that scales the gather's fixed-point accumulators.
//   k_obj_const  grid (B): the zero-warp values of every new kind from k_obj_parts run on the zero-warp IWE (window constants).
// Every sum is a per-thread partial reduced by a fixed wave tree and the waves in index order: results are bit-reproducible and a
// window's bits do not depend on the other windows of the batch.
//
// Sign rule: error-type correlation kinds (mse, adaptive_mse) enter as -K (losses.py:65), similarity-type kinds (hadamard,
// joint_contrast) as +K, so every kind rewards a larger relative correlation.
#pragma once
#include "eincm_kernels.hip.h"

namespace eincm {

// per-cell partials: [0..3] min, #min, max, #max; [4..7] sum I, I^2, E I, E; [8..12] over the whole tile: sum I, I^2, E I, E, E^2;
// [13] tile-local sum |S_t I|^2; [14] sum |S I|^2; [15] sum S I . S E; [16] sum S I . S 1; [17] sum |S E|^2; [18] sum S E . S 1;
// [19] sum |S 1|^2; [20] sum E^2
constexpr int OBJ_NP = 21;

// Scharr of an accessor u(y, x) at (y, x): the convention of scharr_at
template <typename U> __device__ __forceinline__ void obj_scharr(const U& u, int y, int x, double& gx, double& gy) {
    scharr_at(u, y, x, gx, gy);
}

// d/du(p) of 0.5 * sum_q |S u(q)|^2 over the q of a rectangle [y0,y1) x [x0,x1), u zero outside it:
//   sum over q = p + (dy, dx) inside:  gx(q) * kx(p - q) + gy(q) * ky(p - q),  kx(a, b) = b w(a), ky(a, b) = a w(b), w(0) = 10, w(+-1) = 3
template <typename U> __device__ __forceinline__ double obj_adj(const U& u, int y, int x, int y0, int y1, int x0, int x1) {
    double s = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dy == 0 && dx == 0) continue;                 // kx(0, 0) = ky(0, 0) = 0
            const int qy = y + dy, qx = x + dx;
            if (qy < y0 || qy >= y1 || qx < x0 || qx >= x1) continue;
            double gx, gy;
            obj_scharr(u, qy, qx, gx, gy);
            const double wy = (dy == 0) ? 10.0 : 3.0, wx = (dx == 0) ? 10.0 : 3.0;
            s += gx * (-(double)dx * wy) + gy * (-(double)dy * wx);
        }
    return s;
}

__device__ __forceinline__ void obj_cell_rect(const Geom& g, const ObjGeom& og, int cell, int& y0, int& y1, int& x0, int& x1) {
    const int cy = cell / og.ntx, cx = cell % og.ntx;
    y0 = cy * og.th; y1 = (cy == og.nty - 1) ? g.H : y0 + og.th;
    x0 = cx * og.tw; x1 = (cx == og.ntx - 1) ? g.W : x0 + og.tw;
}

// ------------------------------------------------------------------------------------------------
// k_obj_parts: grid (ncells, R, B).  iwe_per_ref = 0: one image per window serves every reference time (the zero-warp IWE).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_obj_parts(Geom g, ObjGeom og, const float* __restrict__ iwe, int iwe_per_ref,
                                                  const float* __restrict__ edges, double* __restrict__ parts)
{
    __shared__ double red[NWAVE][OBJ_NP];
    const int cell = blockIdx.x, r = blockIdx.y, b = blockIdx.z;
    if (!win_active(g, b)) return;
    const size_t HWs = (size_t)g.H * g.W;
    const float* __restrict__ I = iwe + (iwe_per_ref ? ((size_t)b * g.R + r) : (size_t)b) * HWs;
    const float* __restrict__ E = edges + ((size_t)b * g.R + r) * HWs;
    int y0, y1, x0, x1;
    obj_cell_rect(g, og, cell, y0, y1, x0, x1);
    const int ty1 = og.nty * og.th, tx1 = og.ntx * og.tw;       // whole-tile region [0, ty1) x [0, tx1)
    const int cw = x1 - x0, npx = (y1 - y0) * cw;
    double s[OBJ_NP];
#pragma unroll
    for (int j = 0; j < OBJ_NP; ++j) s[j] = 0.0;
    s[0] = INFINITY; s[2] = -INFINITY;
    for (int k = threadIdx.x; k < npx; k += NT) {
        const int y = y0 + k / cw, x = x0 + k % cw;
        const double v = (double)I[(size_t)y * g.W + x], e = (double)E[(size_t)y * g.W + x];
        s[1] = (v < s[0]) ? 1.0 : s[1] + (v == s[0] ? 1.0 : 0.0);
        s[3] = (v > s[2]) ? 1.0 : s[3] + (v == s[2] ? 1.0 : 0.0);
        s[0] = fmin(s[0], v); s[2] = fmax(s[2], v);
        s[4] += v; s[5] += v * v; s[6] += e * v; s[7] += e; s[20] += e * e;
        const bool inT = y < ty1 && x < tx1;
        if (inT) {
            s[8] += v; s[9] += v * v; s[10] += e * v; s[11] += e; s[12] += e * e;
            if (og.need & OBJ_NEED_TILE_GM) {
                const int ry0 = (y / og.th) * og.th, rx0 = (x / og.tw) * og.tw, ry1 = ry0 + og.th, rx1 = rx0 + og.tw;
                auto ut = [&](int yy, int xx) -> double {
                    return (yy >= ry0 && yy < ry1 && xx >= rx0 && xx < rx1) ? (double)I[(size_t)yy * g.W + xx] : 0.0; };
                double gx, gy;
                obj_scharr(ut, y, x, gx, gy);
                s[13] += gx * gx + gy * gy;
            }
        }
        if (og.need & (OBJ_NEED_GM | OBJ_NEED_JOINT)) {
            auto ui = [&](int yy, int xx) -> double {
                return (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) ? (double)I[(size_t)yy * g.W + xx] : 0.0; };
            double ix, iy;
            obj_scharr(ui, y, x, ix, iy);
            s[14] += ix * ix + iy * iy;
            if (og.need & OBJ_NEED_JOINT) {
                auto ue = [&](int yy, int xx) -> double {
                    return (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) ? (double)E[(size_t)yy * g.W + xx] : 0.0; };
                auto u1 = [&](int yy, int xx) -> double { return (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) ? 1.0 : 0.0; };
                double ex, ey, ox, oy;
                obj_scharr(ue, y, x, ex, ey);
                obj_scharr(u1, y, x, ox, oy);
                s[15] += ix * ex + iy * ey; s[16] += ix * ox + iy * oy;
                s[17] += ex * ex + ey * ey; s[18] += ex * ox + ey * oy; s[19] += ox * ox + oy * oy;
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double wmn = __shfl(wave_min(s[0]), 0, 64), wmx = __shfl(wave_max(s[2]), 0, 64);
    const double cmn = wave_sum(s[0] == wmn ? s[1] : 0.0), cmx = wave_sum(s[2] == wmx ? s[3] : 0.0);
    double t[OBJ_NP];
#pragma unroll
    for (int j = 4; j < OBJ_NP; ++j) t[j] = wave_sum(s[j]);
    if (lane == 0) {
        red[wv][0] = wmn; red[wv][1] = cmn; red[wv][2] = wmx; red[wv][3] = cmx;
#pragma unroll
        for (int j = 4; j < OBJ_NP; ++j) red[wv][j] = t[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double o[OBJ_NP];
        for (int j = 0; j < OBJ_NP; ++j) o[j] = red[0][j];
        for (int i = 1; i < NWAVE; ++i) {
            if (red[i][0] < o[0]) { o[0] = red[i][0]; o[1] = red[i][1]; } else if (red[i][0] == o[0]) o[1] += red[i][1];
            if (red[i][2] > o[2]) { o[2] = red[i][2]; o[3] = red[i][3]; } else if (red[i][2] == o[2]) o[3] += red[i][3];
            for (int j = 4; j < OBJ_NP; ++j) o[j] += red[i][j];
        }
        double* dst = parts + (((size_t)b * g.R + r) * og.ncells + cell) * OBJ_NP;
        for (int j = 0; j < OBJ_NP; ++j) dst[j] = o[j];
    }
}

// Reduce the cell partials of one image.  Called by a full wave; results in all lanes.  av: sum over tiles of the population
// variance of the tile.
__device__ __forceinline__ void obj_reduce(const ObjGeom& og, const double* __restrict__ parts, double* S, double& av) {
    const int lane = threadIdx.x & 63;
    const double N = (double)og.th * (double)og.tw;
    double mn = INFINITY, mx = -INFINITY, cmn = 0.0, cmx = 0.0, v = 0.0;
    double s[OBJ_NP];
#pragma unroll
    for (int j = 4; j < OBJ_NP; ++j) s[j] = 0.0;
    for (int i = lane; i < og.ncells; i += 64) {
        const double* p = parts + (size_t)i * OBJ_NP;
        if (p[0] < mn) { mn = p[0]; cmn = p[1]; } else if (p[0] == mn) cmn += p[1];
        if (p[2] > mx) { mx = p[2]; cmx = p[3]; } else if (p[2] == mx) cmx += p[3];
#pragma unroll
        for (int j = 4; j < OBJ_NP; ++j) s[j] += p[j];
        const double mean = p[8] / N;
        v += p[9] / N - mean * mean;
    }
    S[0] = __shfl(wave_min(mn), 0, 64); S[2] = __shfl(wave_max(mx), 0, 64);
    S[1] = __shfl(wave_sum(mn == S[0] ? cmn : 0.0), 0, 64);
    S[3] = __shfl(wave_sum(mx == S[2] ? cmx : 0.0), 0, 64);
#pragma unroll
    for (int j = 4; j < OBJ_NP; ++j) S[j] = __shfl(wave_sum(s[j]), 0, 64);
    av = __shfl(wave_sum(v), 0, 64);
}

// The objective values of one image from its reduced partials, and the two sums the tie terms of the normalisation need:
//   con   contrast value of the kind ck (on the raw IWE)
//   corr  signed correlation value of the kind rk on (E, n):  -K for mse / adaptive_mse, +K for hadamard / joint_contrast
//   sdn   sum_p d corr / d n_p,   sdnn  sum_p n_p d corr / d n_p
struct ObjVals { double m, M, D, cm, cM, con, corr, sdn, sdnn; };
__device__ __forceinline__ ObjVals obj_values(const ObjGeom& og, const double* S, double av, int ck, int rk, double HW) {
    ObjVals q;
    const double N = (double)og.th * (double)og.tw, NT_ = (double)og.ncells * N;
    q.m = S[0]; q.cm = S[1]; q.M = S[2]; q.cM = S[3];
    q.D = q.M - q.m + EPSN;
    const double m = q.m, D = q.D;
    if (ck == 0)      q.con = S[14] / HW;
    else if (ck == 1) { const double mu = S[4] / HW; q.con = S[5] / HW - mu * mu; }
    else if (ck == 2) q.con = S[13] / N;
    else              q.con = av;
    if (rk == 0 || rk == 2) {                  // whole image moments
        const double sn = (S[4] - m * HW) / D;                              // sum n
        const double sEn = (S[6] - m * S[7]) / D;                           // sum E n
        const double snn = (S[5] - 2.0 * m * S[4] + m * m * HW) / (D * D);  // sum n^2
        if (rk == 0) {
            q.corr = -(S[20] - 2.0 * sEn + snn) / HW;
            q.sdn = 2.0 * (S[7] - sn) / HW; q.sdnn = 2.0 * (sEn - snn) / HW;
        } else {
            q.corr = sEn / HW;
            q.sdn = S[7] / HW; q.sdnn = sEn / HW;
        }
    } else if (rk == 1) {                      // the same over the whole tiles, each tile's mean over N pixels
        const double sn = (S[8] - m * NT_) / D;
        const double sEn = (S[10] - m * S[11]) / D;
        const double snn = (S[9] - 2.0 * m * S[8] + m * m * NT_) / (D * D);
        q.corr = -(S[12] - 2.0 * sEn + snn) / N;
        q.sdn = 2.0 * (S[11] - sn) / N; q.sdnn = 2.0 * (sEn - snn) / N;
    } else {                                   // joint contrast: S(E + n) = S E + (S I - m S 1) / D
        const double EI = S[15], I1 = S[16], II = S[14], EE = S[17], E1 = S[18], O = S[19];
        const double pn = (EI - m * E1) / D;                                 // sum S E . S n
        const double nn = (II - 2.0 * m * I1 + m * m * O) / (D * D);         // sum |S n|^2
        const double p1 = E1 + (I1 - m * O) / D;                             // sum S(E + n) . S 1
        q.corr = (EE + 2.0 * pn + nn) / HW;
        q.sdn = 2.0 * p1 / HW; q.sdnn = 2.0 * (pn + nn) / HW;
    }
    return q;
}

// ------------------------------------------------------------------------------------------------
// k_obj_grad: grid (ceil(nig / 4), R, B), IG_NT threads, one IG_COLS x IG_ROWS strip per wave (the strips of k_imgrad, so
// that gmax keeps its layout).  write_g = 0 (forward-only evaluations): only the per-image values, grid (1, R, B).
//   dL/dIWE = a_r * d con / dI + (b_r / D) * d corr / dn + ties [+ the divergence adjoint, delta != 0]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IG_NT) void k_obj_grad(Geom g, EvalParams ep, ObjGeom og,
        const float* __restrict__ iwe, const float* __restrict__ edges, const double* __restrict__ oparts,
        const WinConst* __restrict__ wc, const ObjConst* __restrict__ oc,
        const float* __restrict__ gdiv, const double* __restrict__ dgparts,    // delta != 0 gradients only
        float* __restrict__ G, unsigned* __restrict__ gmax,
        double* __restrict__ vals_out,         // (B,R,2): con, corr of every image (pinned host memory)
        int write_g)
{
    __shared__ double sc[12];
    const int r = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63;
    if (!win_active(g, b)) return;
    const bool use_div = write_g && (ep.delta != 0.0);
    const double HW = (double)g.H * (double)g.W, N = (double)og.th * (double)og.tw;
    const size_t img = ((size_t)b * g.R + r) * g.H * g.W;
    const double* __restrict__ P = oparts + ((size_t)b * g.R + r) * og.ncells * OBJ_NP;
    const int ck = og.ck, rk = og.rk;
    if (threadIdx.x < 64) {
        double S[OBJ_NP], av;
        obj_reduce(og, P, S, av);
        const ObjVals q = obj_values(og, S, av, ck, rk, HW);
        double dAn = 0.0, dA = 0.0;
        if (use_div) {
            const double* dp = dgparts + ((size_t)b * g.R + r) * g.ntiles * 2;
            for (int i = threadIdx.x; i < g.ntiles; i += 64) { dAn += dp[2 * i]; dA += dp[2 * i + 1]; }
            dAn = __shfl(wave_sum(dAn), 0, 64); dA = __shfl(wave_sum(dA), 0, 64);
        }
        if (threadIdx.x == 0) {
            const WinConst& c = wc[b];
            if (blockIdx.x == 0) { vals_out[((size_t)b * g.R + r) * 2] = q.con; vals_out[((size_t)b * g.R + r) * 2 + 1] = q.corr; }
            const double c0 = oc[b].c0[ck], zc = oc[b].zc[rk][r];
            const LossWeights lw = loss_weights(ep, c.mrw[r], (double)g.R, c0, zc, c.d0, HW);
            const double a_r = lw.a, b_r = lw.b, e_hw = use_div ? lw.e : 0.0;
            const double sGn_n = b_r * q.sdnn + e_hw * dAn;          // sum Gn * n   (Gn = dL/dn)
            const double sGn = b_r * q.sdn + e_hw * dA;              // sum Gn
            sc[0] = q.m; sc[1] = q.M; sc[2] = 1.0 / q.D;
            sc[3] = a_r * 2.0 / ((ck <= 1) ? HW : N);               // contrast scale
            sc[4] = b_r / q.D;                                       // scale of d corr / dn
            sc[5] = ((sGn_n - sGn) / q.D) / q.cm;                    // dL/dm per arg-min pixel
            sc[6] = (-sGn_n / q.D) / q.cM;                           // dL/dM per arg-max pixel
            sc[7] = S[4] / HW;                                       // mean I
            sc[8] = e_hw / q.D;                                      // scale of the divergence adjoint image
        }
    }
    __syncthreads();
    if (!write_g) return;
    const int strip = __builtin_amdgcn_readfirstlane(blockIdx.x * (IG_NT / 64) + (threadIdx.x >> 6));
    if (strip >= g.nig) return;                              // (no barrier below)
    const float* __restrict__ I = iwe + img;
    const float* __restrict__ E = edges + img;
    const double m = sc[0], M = sc[1], invD = sc[2], k_c = sc[3], k_n = sc[4], k_m = sc[5], k_M = sc[6], meanI = sc[7], k_d = sc[8];
    const int cx0 = (strip % g.igx) * IG_COLS, cy0 = (strip / g.igx) * IG_ROWS;
    const int x = cx0 + lane;
    const int ty1 = og.nty * og.th, tx1 = og.ntx * og.tw;
    unsigned gm = 0u;
    if (lane < IG_COLS && x < g.W) {
        auto ui = [&](int yy, int xx) -> double {
            return (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W) ? (double)I[(size_t)yy * g.W + xx] : 0.0; };
        for (int y = cy0; y < min(cy0 + IG_ROWS, g.H); ++y) {
            const double v = (double)I[(size_t)y * g.W + x], e = (double)E[(size_t)y * g.W + x];
            const double n = (v - m) * invD;
            const bool inT = y < ty1 && x < tx1;
            const int ry0 = (y / og.th) * og.th, rx0 = (x / og.tw) * og.tw;
            double dc = 0.0;
            if (ck == 0) dc = obj_adj(ui, y, x, 0, g.H, 0, g.W);
            else if (ck == 1) dc = v - meanI;
            else if (ck == 2) {
                if (inT) {
                    auto ut = [&](int yy, int xx) -> double {
                        return (yy >= ry0 && yy < ry0 + og.th && xx >= rx0 && xx < rx0 + og.tw) ? (double)I[(size_t)yy * g.W + xx] : 0.0; };
                    dc = obj_adj(ut, y, x, ry0, ry0 + og.th, rx0, rx0 + og.tw);
                }
            } else if (inT) {
                const double* cp = P + (size_t)((y / og.th) * og.ntx + x / og.tw) * OBJ_NP;
                dc = v - cp[8] / N;
            }
            double dn;
            if (rk == 0) dn = 2.0 * (e - n) / HW;
            else if (rk == 1) dn = inT ? 2.0 * (e - n) / N : 0.0;
            else if (rk == 2) dn = e / HW;
            else {
                auto uj = [&](int yy, int xx) -> double {
                    if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) return 0.0;
                    const size_t o = (size_t)yy * g.W + xx;
                    return (double)E[o] + ((double)I[o] - m) * invD; };
                dn = 2.0 * obj_adj(uj, y, x, 0, g.H, 0, g.W) / HW;
            }
            double gv = k_c * dc + k_n * dn;
            if (use_div) gv += k_d * (double)gdiv[img + (size_t)y * g.W + x];
            if (v == m) gv += k_m;
            if (v == M) gv += k_M;
            const float gf = (float)gv;
            G[img + (size_t)y * g.W + x] = gf;
            gm = max(gm, __float_as_uint(gf) & 0x7fffffffu);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gm = max(gm, (unsigned)__shfl_down((int)gm, o, 64));
    if (lane == 0) gmax[((size_t)b * g.R + r) * g.nig + strip] = gm;
}

// ------------------------------------------------------------------------------------------------
// k_obj_const: grid (B), one wave.  The zero-warp values of the new kinds from k_obj_parts run on (zero-warp IWE, E_r).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_obj_const(Geom g, ObjGeom og, const double* __restrict__ oparts, ObjConst* __restrict__ oc)
{
    const int b = blockIdx.x;
    const double HW = (double)g.H * (double)g.W;
    for (int r = 0; r < g.R; ++r) {
        double S[OBJ_NP], av;
        obj_reduce(og, oparts + ((size_t)b * g.R + r) * og.ncells * OBJ_NP, S, av);
        for (int k = 1; k < 4; ++k) {
            const ObjVals q = obj_values(og, S, av, (k >= 2) ? k : 0, k, HW);
            if (threadIdx.x == 0) {
                oc[b].zc[k][r] = q.corr;
                if (r == 0 && k >= 2) oc[b].c0[k] = q.con;
            }
        }
    }
}

}  // namespace eincm
