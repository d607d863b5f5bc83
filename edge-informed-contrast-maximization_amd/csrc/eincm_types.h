// eincm_types.h — the plain types and constants the kernels (eincm_kernels.hip.h, eincm_objectives.hip.h) share with the host's
// planning (eincm_plan.h).  Plain C++17: no HIP header and no device code, so a compiler that knows no HIP can build what the host
// decides with them.  Layouts, field order and values are the kernels' argument layouts: they do not change here.
#pragma once
#include <stddef.h>
#include <stdint.h>

// The one function both sides run: __host__ __device__ under hipcc, a plain inline function anywhere else.
#if defined(__HIPCC__)
#define EINCM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EINCM_HD inline
#endif

namespace eincm {

constexpr int TS = 32;            // source tile edge (pixels)
constexpr int WIN_CAP_DEFAULT = 2304;   // pixels of LDS for a segment's destination window
constexpr int NXCD = 8;           // XCDs: blocks b and b+8 share an L2 (round-robin dispatch; speed only, never correctness)
constexpr int MAX_SEG = 1 << 20;   // events per segment (one window flush per segment and reference time)
// A tile's c events are cut into ceil(c/seg) segments of EQUAL length (rounded up to whole workgroup trips), not into
// seg, seg, ..., remainder: the event kernels' workgroups then finish together instead of leaving a tail of short ones.
EINCM_HD int balanced_seg_len(int c, int seg) {
    const int nseg = (c + seg - 1) / seg;
    if (nseg <= 1) return seg;
    const int len = (((c + nseg - 1) / nseg + 255) / 256) * 256;
    return len < seg ? len : seg;
}

struct Geom {
    int H, W, R, B;
    int tilesX, tilesY, ntiles;
    int wincap, winmaxw;      // LDS destination-window capacity (pixels) and maximum width: the splat's segment list (items_s, "list b")
    int wincap_a, winmaxw_a;  // the same for the gather's own list (items, "list a"): its segments are longer, so they span more time and move further
    int nparts;               // StatParts per image written by the statistics kernel of this evaluation (ntiles or NSPART)
    int pstride;              // StatPart slots per image: max(ntiles, NSPART)
    int gmax_n;               // words of `gmax` per window: R * nig per-strip maxima of k_imgrad
    unsigned long long wmask; // bit b: window b takes part in this evaluation (eincm_loss_grad_masked: a lockstep solver's converged windows
                              // sit out; their workgroups leave at once and their outputs are not written).  Windows >= 64 always take part.
    int igx, nig;             // k_imgrad strips per image row / per image (IG_COLS x IG_ROWS pixels each): slots of g2parts and gmax
    int pitch_aligned;        // LDS windows of the splat's event copy at a row pitch rounded up to the 32 banks (win_pitch)
};

struct Item {                     // one segment of event work: <= seg events of one source tile of one window
    int32_t win, tile, begin, count;
    double t_lo, t_hi;            // time range of its events
};

struct EvalParams {
    double alpha, beta, gamma, delta;
    int cur_pyr_lvl, contrast_kind;
    int want_div, want_tv, use_tv_grad;
    int h, w, identity;
};

constexpr int THETA_ARG_MAX = 128;    // doubles of theta that ride in the kernel arguments instead of an H2D copy
constexpr int THETA_ARG_BIG = 4096;   // k_theta alone takes up to 32 KiB of theta (16x16 grids of 8 windows) in its arguments: no read of pinned host memory
constexpr int THETA_ARG_MID = 512;    // ... and a 4 KiB form for one window's 16x16 grid: the launch copies its arguments twice on the host (k_theta<TA>)

// ---- what the event kernels' launch forms are made of (eincm_plan.h: SplatForm, GatherForm) ----
constexpr int NT = 256;           // threads per workgroup = 4 waves of 64

// Where an event's velocity Theta[y,x] comes from inside the event kernels.  A per-event global gather costs ~64 L1 cycles per
// wave-instruction (64 lanes, 64 different cache lines) and was 2/3 of k_splat's time; every workgroup works on ONE source tile, so:
constexpr int THETA_CONST = 1;   // theta (1,1,2): Theta is one constant per window (read from the tile bounds, min == max)
constexpr int THETA_TILE = 2;    // otherwise: the tile's 32x32 double2 velocities are staged in LDS once per segment (16 KiB)
constexpr int THETA_POLY = 3;    // a motion model: the tile is formed in LDS from the window's polynomial, no Theta image
// THETA_POLY: LDS beside the Theta tile: u of the tile's 32 columns | v of its 32 rows | 4 bounds of each of up to 8 waves
constexpr int POLY_SCRATCH = 2 * TS + 4 * 8;
constexpr size_t POLY_SCRATCH_BYTES = POLY_SCRATCH * sizeof(double);
// another splat window (eincm_splat_window.hip.h):
constexpr int SW_CAP_TILE = 4608;            // u64 words of k_splat_r's window beside the 16 KiB Theta tile (36 + 16 KiB of LDS)
constexpr int SW_CAP_CONST = 6912;           // ... with nothing beside it (54 KiB)

struct Window { int ox, oy, ww, wh; };

struct TileRange { int ilo, ni, jlo, nj; };     // the coarse cells a tile's pixels have weight on (host: build_resample)

constexpr int NSPART = 32;        // blocks per image of k_stats_stream
constexpr int IG_ROWS = 12, IG_COLS = 60, IG_NT = 256;      // rows: 16.5 / 15.7 / 16.0 us with 16 / 12 / 8 on the 8-window batch, 8.2 / 7.2 / 6.7 on one window (k_final pays for more strips)
constexpr int PG_MAXC = 6;        // coarse rows / columns under one 32x32 tile that k_gather's own projection handles (16x16 theta on 260x346: 4)

// the selectable objective kinds (eincm_objectives.hip.h)
struct ObjGeom {
    int th, tw;          // tile size
    int nty, ntx;        // whole tiles per column / row (>= 1)
    int ncells;          // nty * ntx
    int ck, rk;          // contrast kind (0..3), correlation kind (0..3)
    int need;            // OBJ_NEED_* bits: which stencil sums k_obj_parts forms
};
constexpr int OBJ_NEED_TILE_GM = 1;     // tile-local Scharr energy          (adaptive_grad_mag)
constexpr int OBJ_NEED_GM = 2;          // whole-image Scharr energy of I    (grad_mag, joint_contrast)
constexpr int OBJ_NEED_JOINT = 4;       // cross terms with S E and S 1      (joint_contrast)

constexpr double EPSN = 2.220446049250313e-16;   // sys.float_info.epsilon (losses.py:24)

struct StatPart {                 // per (window, ref, tile) partial of the image reductions
    double mn, mx, cmn, cmx;      // min, max and how many pixels attain them inside the tile
    double sI, sII, sEI, sG2;     // sum I, sum I^2, sum E*I, sum (gx^2+gy^2)
};

struct ImgScal {                  // per (window, ref) reduced scalars
    double m, M, D, cm, cM, sI, sII, sEI, sG2;
};
constexpr int IMGSCAL_N = 9;      // doubles per image handed to the host: m, M, D, cm, cM, sI, sII, sEI, sG2

struct WinConst {                 // theta-independent constants of a window (losses.py:54-55,66,71,80,84)
    double c0_gradmag, c0_var, d0;
    double zc[16];                // zero_corrs[r] = -MSE(E_r, n0)
    double sE[16], sEE[16];       // sum E_r, sum E_r^2
    double eabs[16];              // max |E_r|
    double inv_c0_gradmag, inv_c0_var, inv_zc[16];   // 1 / (c0 + eps), 1 / (zc[r] + eps)
    // (no kernel reads eabs or inv_*: they stay so that the layout, and with it every kernel's code, does not move)
    double mrw[16];               // multi-reference weights (losses.py:39-46)
    double dtmax;                 // max |t_e - tau_r| over the window's events and reference times (bounds a gradient term)
    double nev;                   // events staged in this window of this context
    double cntmax;                // most events on one source pixel (bounds a per-pixel gradient sum)
};

struct OutScal {                  // per-window result block written by k_final
    double value, mean_rel_corr, mean_rel_contrast, mean_rel_div, tv, tv_scale, nonfinite, _pad;
    double corr[16], contrast_gm[16], var[16], div[16];
};

struct F64Scal {                       // per (window, ref) image scalars of the fp64 mode
    double m, M, D, cm, cM, mean, var, g2, mse, div;   // g2 = mean(gx^2 + gy^2), mse = mean((E - n)^2), div = mean |div n|
};

struct ObjConst {                  // zero-warp values per window, indexed by kind: [0] / [1] from WinConst (host), [2] / [3] here
    double c0[4];                  // contrast of the zero-warp IWE
    double zc[4][16];              // correlation (signed) of (E_r, n0)
};

// the kernels' argument and result layouts: a move of one cannot go unnoticed
static_assert(sizeof(StatPart) == 64 && offsetof(StatPart, mn) == 0 && offsetof(StatPart, sG2) == 56, "StatPart layout");
static_assert(sizeof(ImgScal) == IMGSCAL_N * 8 && offsetof(ImgScal, m) == 0 && offsetof(ImgScal, sG2) == 64, "ImgScal layout");
static_assert(sizeof(WinConst) == 104 * 8 && offsetof(WinConst, c0_gradmag) == 0 && offsetof(WinConst, cntmax) == 103 * 8, "WinConst layout");
static_assert(sizeof(OutScal) == 72 * 8 && offsetof(OutScal, value) == 0 && offsetof(OutScal, div) == 56 * 8, "OutScal layout");
static_assert(sizeof(F64Scal) == 80 && offsetof(F64Scal, m) == 0 && offsetof(F64Scal, div) == 72, "F64Scal layout");
static_assert(sizeof(ObjConst) == 68 * 8 && offsetof(ObjConst, c0) == 0 && offsetof(ObjConst, zc) == 32, "ObjConst layout");

}  // namespace eincm
