// eincm_api.hip — host engine behind the C-ABI of include/eincm.h (libeincm_hip.so, gfx950 only).
//
// Host responsibilities (everything else runs in the kernels of eincm_kernels.hip.h):
//   - own the HBM layout of a batch of event windows (see DESIGN.md "Data layout in HBM")
//   - bin events by 32x32 source tile once per window and cut the bins into work items
//   - build the scale_and_translate weight matrices (theta_utils.py:25-35) for the current theta shape
//   - launch the evaluation sequence on one stream and hand (value, grad, aux) back as float64
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "eincm.h"
#include "eincm_plan.h"
#include "eincm_kernels.hip.h"
#include "eincm_kernels_f64.hip.h"
#include "eincm_binning.hip.h"
#include "eincm_edges.hip.h"
#include "eincm_objectives.hip.h"
#include "eincm_splat_window.hip.h"
#include "eincm_canny.hip.h"
#include "eincm_preprocess.hip.h"
#include "eincm_gtflow.hip.h"
#include "eincm_dsec.hip.h"
#include "eincm_floweval.hip.h"
#include "eincm_bfgs.hip.h"
#include "eincm_lbfgs.hip.h"
#include "eincm_motion.hip.h"
#include "eincm_event_support.hip.h"
#include "eincm_event_filter.hip.h"
#include "eincm_event_scores.h"
#include "eincm_event_scores.hip.h"
#include "eincm_responsibilities.h"
#include "eincm_responsibilities.hip.h"
#include "eincm_motion_layers.h"
#include "eincm_motion_layers.hip.h"
#include "eincm_motion_fill.h"
#include "eincm_motion_fill.hip.h"
#include "eincm_label_prior.h"
#include "eincm_label_prior.hip.h"
#include "eincm_label_carry.h"
#include "eincm_label_carry.hip.h"
#include "eincm_theta_advect.h"
#include "eincm_theta_advect.hip.h"
#include "eincm_contrast_landscape.h"
#include "eincm_contrast_landscape.hip.h"

using namespace eincm;

namespace {

thread_local std::string g_create_error;

// The owner of a context's device and pinned host memory: every block is allocated through it and freed by it, one by one (release:
// a buffer that grows) or all at once (release_all: the context ends, or its creation failed).  DESIGN.md section 5.2.
struct Mem {
    struct Block { void* p; size_t bytes; };
    std::vector<Block> dev, pinned;
    size_t dev_bytes = 0, pinned_bytes = 0;

    template <typename T> hipError_t alloc_dev(T*& p, size_t n, bool zero = false) {
        p = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
        if (e == hipSuccess && p && zero) e = hipMemset(p, 0, n * sizeof(T));
        return own(dev, dev_bytes, p, n * sizeof(T), e, hipFree);
    }
    template <typename T> hipError_t alloc_pinned(T*& p, size_t n, bool zero = false) {
        p = nullptr;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess && p && zero) memset(p, 0, n * sizeof(T));
        return own(pinned, pinned_bytes, p, n * sizeof(T), e, hipHostFree);
    }
    void release(void* p) {
        if (!p) return;
        if (!drop(dev, dev_bytes, p, hipFree)) drop(pinned, pinned_bytes, p, hipHostFree);
    }
    void release_all() {
        for (const Block& b : dev) (void)hipFree(b.p);
        for (const Block& b : pinned) (void)hipHostFree(b.p);
        dev.clear(); pinned.clear();
        dev_bytes = pinned_bytes = 0;
    }

private:
    template <typename T> static hipError_t own(std::vector<Block>& v, size_t& total, T*& p, size_t bytes, hipError_t e, hipError_t (*free_fn)(void*)) {
        if (e != hipSuccess) { if (p) (void)free_fn(p); p = nullptr; return e; }       // (the block was allocated, zeroing it failed)
        if (p) { v.push_back(Block{p, bytes}); total += bytes; }
        return hipSuccess;
    }
    static bool drop(std::vector<Block>& v, size_t& total, void* p, hipError_t (*free_fn)(void*)) {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i].p == p) { (void)free_fn(p); total -= v[i].bytes; v.erase(v.begin() + i); return true; }
        return false;
    }
};

// A buffer that is allocated on first use or grows on demand (ensure): n elements at p, in HBM or (PINNED) in pinned host memory.
template <typename T, bool PINNED = false> struct Grow {
    T* p = nullptr;
    size_t n = 0;
};

// The caller's arrays of one staging: one pointer per window (nothing is concatenated on the host)
struct StageArgs {
    int B, R; const int64_t* n_events;
    const int16_t* const* xs; const int16_t* const* ys; const double* const* ts; const double* const* edges; const double* edge_ts;
    uint32_t flags;
    const float* const* weights = nullptr;      // eincm_set_windows_weighted: NULL, or per window its events' weights (NULL: ones)
};

// All host memory an asynchronous copy of a staging reads or writes.  stage_windows constructs it before the guard that drains the
// stream, so every way out of a staging drains first and frees afterwards.
struct StageScratch {
    std::vector<unsigned> cntmax; std::vector<double> dtmax;       // (B) most events on one source pixel, max |t - tau|
    bool edge_ts_uploaded = false;
    std::vector<BinBlock> blks; std::vector<int32_t> win_blk; int32_t misc[4]; std::vector<double> mom;   // device binning
    std::vector<uint32_t> sxy; std::vector<double> st; std::vector<float> ef; std::vector<float> sw; std::vector<uint32_t> sidx;   // host binning
    std::vector<int> ishift;                                                                              // float64 mode
};

// The evaluation in flight: eval_begin enqueues its forward half (FORWARD; the caller may all-reduce the IWE
// stack; a float64 context goes to LAUNCHED at once), eval_end_launch the rest (LAUNCHED), eval_end_collect waits and hands over (IDLE).
// All of it belongs to that one evaluation, as does the window mask, which is g.wmask because the kernels take it from the Geom.
struct Flight {
    enum State { IDLE, FORWARD, LAUNCHED } state = IDLE;
    EvalPlan plan{};                    // (outlives the evaluation: eincm_get_launch_policy)
    DevIo io{};                         // the call's device-resident theta and gradient, if any
    const double* theta_dev = nullptr; ThetaArg targ{};      // where the event kernels find theta
    int copy_mode = 0;                  // 1: the D2H copies of the results are still to be enqueued (device_results)
    int n_pieces = 0;                   // pieces of the gradient download (0: it came with the results / in one copy)
    size_t piece_len = 0;
    std::vector<uint8_t> theta_nan;     // (B) a NaN / Inf somewhere in window b's theta (host-assembled and float64 evaluations)
    bool timed_now = true;              // EINCM_CF_TIMING_DOMINANT: this evaluation carries events (eincm_set_timing_period)
    int ring_cur = 0;                   // ... in this slot of the ring
    bool idle() const { return state == IDLE; }
    bool launched() const { return state == LAUNCHED; }
    void land() { state = IDLE; io = DevIo{}; }          // (the caller's device pointers end with the evaluation)
    // Give the evaluation up: what it enqueued reads the pinned theta buffer and writes the pinned result block, so the stream drains
    // before the context looks idle.  (acc_dirty, set when the forward half starts, already says what the kernels left behind.)
    void abandon(hipStream_t stream) { (void)hipStreamSynchronize(stream); land(); }
};

}  // namespace

// (PlanCtx, eincm_plan.h: the sensor size, the staged batch's geometry, plan and segment lists, and the settings both plans read)
struct eincm_ctx : PlanCtx {
    int device = 0;
    int maxR = 0, maxB = 0;
    int64_t maxN = 0;
    uint32_t cflags = 0;
    hipStream_t stream = nullptr;
    std::string err;
    Mem mem;                       // owns every device and pinned block below

    // staged batch
    bool staged = false;
    std::vector<int64_t> win_events;

    // device buffers
    uint32_t* d_xy = nullptr;      // (maxN) x | y<<16, binned by (window, tile); the splat's copy: time order inside a tile, re-dealt in blocks of 256 (k_spread)
    double* d_t = nullptr;         // (maxN)
    uint32_t* d_xy_g = nullptr;    // (maxN) the gather's copy: the same bins, every segment of the gather list sorted by source pixel and dealt to its threads (k_segsort)
    double* d_t_g = nullptr;       // (maxN)
    // per-event weights of a weighted batch (stage.weighted), one copy per event layout: allocated by the first
    // weighted staging of the context (ensure_weights), not read by an unweighted batch
    float* d_w = nullptr;          // (maxN) in the order of d_xy
    float* d_w_g = nullptr;        // (maxN) in the order of d_xy_g; during a device binning it first holds the weights as handed over
    // a keep-order batch (EINCM_SW_KEEP_ORDER; stage.keep_order): allocated by the first staging that asks for it
    // (ensure_order), not touched by any other
    struct {
        uint32_t* splat = nullptr;     // (maxN) for every slot of d_xy: where its event stood in the batch as handed over (the index into d_raw_*)
        uint32_t* gather = nullptr;    // (maxN) the same for d_xy_g
        float* stream = nullptr;       // (maxN) the staged weights in the order of d_raw_*: what k_bin_scatter and k_reweight read, ones where a window was handed none
        std::vector<uint32_t> h_xy;    // host binning only: the events as handed over, x | y << 16 (the host counts the most events on one pixel)
    } ord;
    std::vector<int32_t> h_tilecount;   // (B, ntiles) events per (window, tile) of the staged batch: what every segment list is cut from
    bool policy_evaluated = false; // an evaluation has chosen capacities since the last staging (eincm_get_launch_policy)
    // device-side staging (eincm_binning.hip.h)
    int16_t* d_raw_x = nullptr; int16_t* d_raw_y = nullptr; double* d_raw_t = nullptr;   // (maxN) events as handed over
    BinBlock* d_binblocks = nullptr; int32_t* d_win_blk = nullptr; uint32_t* d_blockhist = nullptr;
    int32_t* d_tilecount = nullptr; int32_t* d_tilebase = nullptr; int32_t* d_bin_misc = nullptr;
    double* d_edges_raw = nullptr; double* d_edge_moments = nullptr;
    int64_t max_binblocks = 0;
    int64_t max_items = 0;
    float* d_edges = nullptr;      // (B,R,H,W)
    double* d_edge_ts = nullptr;   // (B,R)
    unsigned long long* d_acc = nullptr;   // (B,R,H,W) u64 fixed-point accumulator of the IWE stack (2^30); zero between evaluations (consumer-clears)
    float* d_iwe = nullptr;        // (B,R,H,W) the fp32 IWE stack, written by the statistics pass from d_acc
    float* d_G = nullptr;          // (B,R,H,W)
    float* d_zero_iwe = nullptr;   // (B,H,W)
    double* d_Theta = nullptr;     // (B,H,W,2)
    double* d_theta_in = nullptr;  // (B,H,W,2) capacity (coarse uses a prefix)
    long long* d_gTheta = nullptr; // (B,H,W,2) i64 fixed point, zero between evaluations (k_project / k_final_dense clear it)
    double* d_g11 = nullptr;       // (max_items, R, 2) 2-DoF theta: per-workgroup partials of dL/dtheta (k_gather -> k_final)
    double* d_dtmax = nullptr;     // (B) staging scratch: max |t - tau| per window
    unsigned* d_gmax = nullptr;    // (B,R,nig) per-strip max |dL/dIWE| as float bits (scale of the i64 gradient accumulators)
    unsigned* d_cntmax = nullptr;  // (B) staging scratch: most events on one source pixel
    unsigned* d_gticket = nullptr; // (B) arrival counters of the gather's tail (theta grids), zero between launches
    double* d_tvg = nullptr;       // (B,H,W,2)
    uint8_t* d_mask = nullptr;     // (B,H,W)
    double* d_tmm = nullptr;       // (B,ntiles,4)
    StatPart* d_parts = nullptr;   // (B,R,pstride)
    double* d_divparts = nullptr;  // (B,R,ntiles)
    double* d_g2parts = nullptr;   // (B,R,nig) contrast energy partials written by k_imgrad
    Grow<float> d_gdiv;            // (B,R,H,W) divergence adjoint image, allocated on the first delta != 0 gradient
    Grow<double> d_dgparts;        // (B,R,ntiles,2) ... and its per-tile partials
    double* d_tvparts = nullptr;   // (B,ntiles,3)
    WinConst* d_wc = nullptr;      // (B)
    OutScal* d_outs = nullptr;     // (B) the base of one block [OutScal x B | d_grad]
    Grow<long long> d_gth;         // (2,B,coarse_cap) main | tv i64 accumulators for coarse theta, zero between evaluations (k_final clears); grown by ensure_coarse
    double* d_grad = nullptr;      // (B,H,W,2) capacity, inside d_outs' block
    Grow<double> d_AH, d_AW;       // (H,h) (W,w) for the current theta shape, grown on demand (ensure_resample)
    int2* d_rowtap = nullptr; int2* d_coltap = nullptr;
    TileRange* d_tilerng = nullptr;    // (ntiles) coarse cells under each tile for the current theta shape
    int cur_h = -1, cur_w = -1, cur_method = -1;
    int64_t coarse_cap = 0;        // cells per window in d_gth's halves: the stride the kernels are given (ensure_coarse)

    // selectable objective kinds (eincm_objectives.hip.h): the zero-warp values of every kind
    // (computed on the first evaluation that needs them, dropped by set_windows and by a tile-size change) and the per-cell partials
    bool objc_valid = false;
    std::vector<ObjConst> h_objc;
    Grow<ObjConst> d_objc;         // (maxB), allocated on first use
    Grow<double> d_oparts;         // (B,R,ncells,OBJ_NP), grown on demand
    Grow<double, true> h_ovals;    // (maxB,maxR,2) pinned: contrast and signed correlation of every image (k_obj_grad), allocated on first use

    // The one scratch block of the one-shot operators (edge smoothing, Canny, preprocessing, ground-truth flow, the DSEC data path,
    // warped events, tiled objectives, the transients of the flow-error evaluation).  An operator takes its pieces of it through its call
    // frame (OneShot), which grows the block once and drains the stream on every exit, so nothing in here outlives a call.  What a later
    // call reads has a buffer of its own:
    Grow<char> scratch;
    struct {                           // eincm_preprocess_image
        Grow<int32_t> p_nlm;           // the NL-means weight table, kept for the (template, search, h^2) it was built for
        std::vector<int32_t> h_pre_tab, h_nlm_tab;   // host sides of the per-call tables and of p_nlm (uploads read them)
        float nlm_hh = 0.0f;
        int nlm_tw = 0, nlm_sw = 0;
    } pre;
    struct {                           // eincm_rectify_events
        Grow<uint32_t> r_map;          // the rounded rectify map packed as int16 pairs, kept from the call that handed a map over
        bool rect_map_set = false;
    } rect;
    struct {                           // eincm_event_support: what one chunk of a stream hands to the next
        Grow<double> last_t;           // (H, W) the time of every pixel's last event so far, -inf: none; allocated by the first call
        double last_time = es_no_event();   // the time of the last event of the previous chunk
    } es;
    struct {                           // eincm_event_filter: its own carried state, apart from es
        Grow<double> maps;             // 3 (H, W): last_any | last_kept[0] | last_kept[1], -inf: none; allocated by the first call
        double last_time = es_no_event();   // the time of the last event of the previous chunk
    } ef;
    // the staged flow evaluation of eincm_flow_eval_stage: [GT flow (n, H, W) double2 | flag bytes (n, H, W)],
    // kept from one staging to the next; every eincm_flow_errors reads it
    struct {
        Grow<char> f_eval;
        int fe_n = 0;                  // windows of the staged flow evaluation (0: none)
        std::vector<int64_t> fe_ngt;   // (fe_n) GT-valid pixels of every window
    } fe;

    struct {                           // eincm_label_prior: the staged prior, read in place by the spatial E-step
        Grow<float> prior;             // (B, H, W), allocated by the first call
        bool staged = false;           // it belongs to the staged batch: dropped by the next staging, kept across a re-weighting
    } lp;

    struct {                           // eincm_carry_label_prior: the carried prior, not the staged one
        Grow<float> prior;             // (B, H, W) of the batch it was formed on, allocated by the first call
        LcCarried of{false, 0, 0, 0, 0};       // valid once a call's result is whole; a staging leaves it alone: it is meant for the next batch
    } lc;

    // pinned host staging
    double* h_theta = nullptr;     // (B,H,W,2) capacity
    double* h_grad = nullptr;      // inside h_outs' block, as d_grad is inside d_outs'
    OutScal* h_outs = nullptr;
    WinConst* h_wc = nullptr;
    // host-assembled evaluations (2-DoF theta, no TV / divergence / full aux): the kernels write their partials straight into these
    // and the host adds them in index order after the stream has drained (no k_final, no k_theta_const: two launches fewer per evaluation)
    double* h_g11 = nullptr;       // (max_items + NXCD, R, 2) per-workgroup partials of dL/dtheta (k_gather)
    double* h_g2 = nullptr;        // (B,R,nig) contrast energy per k_imgrad strip
    double* h_img = nullptr;       // (B,R,IMGSCAL_N) reduced image scalars (k_imgrad)
    double* h_tvparts = nullptr;   // (B,ntiles,3) k_tv's per-tile partials (host-assembled evaluations with the TV term)

    // timing.  EINCM_CF_TIMING_DOMINANT keeps a ring of event sets and reads them out later (eincm_get_timings*): asking HIP for
    // elapsed times after every evaluation cost the caller ~15 us per evaluation, which a throughput measurement should not pay.
    static constexpr int EV_RING = 64;
    hipEvent_t ev[EV_RING][EINCM_N_STAGES + 1][2] = {};
    bool ev_used[EV_RING][EINCM_N_STAGES + 1] = {};
    int ring_size = 1;             // EV_RING in the dominant mode, 1 otherwise (read out at once)
    int ring_lo = 0, ring_n = 0;   // finished evaluations whose events have not been read yet: slots ring_lo .. ring_lo + ring_n - 1
    static constexpr int GRAD_PIECES = 4;
    hipEvent_t ev_piece[GRAD_PIECES] = {};   // dense gradients come back in pieces; the host scans piece k while piece k + 1 crosses PCIe
    int attach_stage = -1;         // EINCM_CF_TIMING: the single-kernel stage whose launch takes its events along (StageTimer)
    int time_period = 1; int64_t time_counter = 0;   // EINCM_CF_TIMING_DOMINANT: events on every time_period-th evaluation only (eincm_set_timing_period)
    bool time_splat = true, time_gather = true;   // EINCM_CF_TIMING_DOMINANT: which event kernels carry start / stop events (eincm_set_timed_kernels)
    bool have_events = false;
    eincm_timings last_t{};
    eincm_timings sum_t{};         // running sums since the last reset (eincm_get_timings_total)
    int64_t sum_n = 0;

    // last eval bookkeeping
    bool have_eval = false;
    unsigned long long eval_wmask = ~0ull;   // the window mask the last evaluation was begun with (g.wmask is rewritten by ensure_theta_image)
    bool G_valid = false;          // d_G holds dL/dIWE of the last evaluation (eincm_get_count_images borrows the buffer)
    int last_nparts = 0;           // how many StatParts per image the last evaluation wrote (k_stats vs k_stats_stream)
    Flight fl;                     // the evaluation in flight
    // host-side wall time of the phases of an evaluation (eincm_get_host_profile): a few clock reads per evaluation, always on
    double hp_us[EINCM_N_HOST_PHASES] = {};
    int64_t hp_n = 0;
    bool constants_pending = false;   // staged with EINCM_SW_DEFER_CONSTANTS and not finished yet
    bool sharded_staging = false;     // the staged batch's constants came from EINCM_SW_DEFER_CONSTANTS (summed IUEs of all shards)
    int splat_size = 3;               // eincm_set_splat_window: events_to_pdf_frame's window_size (splat_rad: its radius splat_size / 2)
    bool acc_dirty = false;        // a forward half was launched and its consumers were not: accumulators must be memset before reuse
    bool Theta_valid = false;      // d_Theta holds the upsampled theta of the last evaluation (2-DoF evaluations skip the image)
    std::vector<double> last_theta11;   // (B,2) theta of the last 2-DoF evaluation (to build d_Theta on demand)

    // float64 mode (EINCM_CF_FP64, eincm_kernels_f64.hip.h): its own images and accumulators, sized at create
    struct {
        unsigned long long* acc = nullptr;   // (B,R,H,W) u64 IWE accumulator at 2^ishift[b], zero between evaluations (k64_img_a clears)
        double* iwe = nullptr;               // (B,R,H,W)
        double* zero_iwe = nullptr;          // (B,H,W)
        double* edges = nullptr;             // (B,R,H,W) the edges as handed over
        double* G = nullptr;                 // (B,R,H,W) dL/dIWE
        double* sgn = nullptr;               // (B,R,H,W) sign of the divergence image (delta != 0 gradients)
        unsigned long long* gacc = nullptr;  // (B,H,W,2) x 2 words: i128 dL/dTheta, zero between evaluations (k64_gfin clears)
        double* gTh = nullptr;               // (B,H,W,2) dL/dTheta
        double* T = nullptr;                 // (B,H,W,2) capacity: the half-projected gradient (k64_proj_w)
        double* grad = nullptr;              // (B,H,W,2) capacity: dL/dtheta
        double* partA = nullptr; double* partB = nullptr; double* partC = nullptr;   // per-workgroup partials of the image passes
        F64Scal* scal = nullptr;             // (B,R)
        F64Scal* h_scal = nullptr;           // pinned copy
        unsigned long long* gmax = nullptr;  // (B) max |dL/dIWE| as double bits
        int* ishift = nullptr;               // (B)
        unsigned* bad = nullptr;             // (B) a non-finite dL/dIWE or event term in this evaluation (gradient -> NaN)
        int P = 0;                           // image-pass workgroups per image
    } f64;

    // BFGS state in HBM (eincm_bfgs.hip.h): allocated at the first eincm_bfgs_begin, grown on demand, nothing per call
    struct {
        bool begun = false;                  // eincm_bfgs_begin has run for the staged batch (set_windows clears it)
        int n = 0, h = 0, w = 0, B = 0;
        Grow<double> vec;                    // one block: X, G, P, Xt, Gt, S, Y, Hy, each (B, n) at stride vec.n / 8
        double *X = nullptr, *G = nullptr, *P = nullptr, *Xt = nullptr, *Gt = nullptr, *S = nullptr, *Y = nullptr, *Hy = nullptr;
        Grow<double> H;                      // (B, n, n)
        Grow<double, true> h_scal;           // pinned (maxB, BFGS_NS): k_bfgs_scalars writes it
        Grow<double, true> h_red;            // pinned (maxB, 2): k_bfgs_reduce writes it
        // the limited-memory form (eincm_lbfgs.hip.h, eincm_lbfgs_begin): no H; S and Y above are the staging rows of the newest pair
        int m = 0;                           // pairs kept per window; 0: the dense form
        int scale = 0;                       // EINCM_LBFGS_SCALE_*
        Grow<double> hist;                   // the rings S | Y, each (B, m, n) by ring slot
        Grow<double> dmat;                   // D (B, 2m+1, 2m+1) | delta (B, 2m+1) | y.s, y.y (B, 2)
        Grow<int> ring;                      // head (B) | count (B) | the last accept kept its pair (B)
        Grow<double> part;                   // per-chunk partials: dots (B, chunks, 6m+6) | direction (B, chunks, 6) | reduce (B, chunks, 2)
        double* lS() const { return hist.p; }
        double* lY() const { return hist.p + (size_t)B * m * n; }
        double* lD() const { return dmat.p; }
        double* ldelta() const { return dmat.p + (size_t)B * (2 * m + 1) * (2 * m + 1); }
        double* lysyy() const { return ldelta() + (size_t)B * (2 * m + 1); }
        int* head() const { return ring.p; }
        int* count() const { return ring.p + B; }
        int* stored() const { return ring.p + 2 * B; }
        double* part_dots() const { return part.p; }
        double* part_dir() const { return part.p + (size_t)B * lbfgs_chunks(n) * lbfgs_nq(m); }
        double* part_red() const { return part_dir() + (size_t)B * lbfgs_chunks(n) * LBFGS_NP; }
    } bfgs;

    // parametric motion-field models (eincm_motion.hip.h): nothing is allocated before the first call that needs it
    struct {
        bool set = false;                    // eincm_set_motion_model handed a model over
        eincm_motion_model model{};
        Grow<double> Theta;                  // (maxB, H, W, 2) the expanded field: the device-resident theta of the evaluation
        Grow<double, true> h_part;           // pinned: the moment partials (maxB, MOTION_PARTS, 12) | q of every window (maxB, 12)
        double* h_q(int maxB) const { return h_part.p + (size_t)maxB * MOTION_PARTS * MOTION_NQ; }
        // the fused evaluation
        Grow<double, true> h_fpart;          // pinned: the gather's moment partials, one slot of 12 per (segment, reference time) or per segment
        Grow<double> tmm_zero;               // (maxB, ntiles, 4) zeros: k_final's NaN scan of the velocity bounds (the host has looked at q)
        std::vector<double> last_q;          // (B, 12) q of the last fused evaluation (to build d_Theta on demand, as last_theta11)
        std::vector<int64_t> seg0;           // (B + 1) first segment of every window in the gather's list (motion_slot_offsets); empty: not formed for this staging
    } motion;
};

namespace {

using hp_clock = std::chrono::steady_clock;
struct HostPhase {                 // adds the lifetime of the object to ctx->hp_us[phase]
    eincm_ctx* c; int phase; hp_clock::time_point t0;
    HostPhase(eincm_ctx* c_, int p) : c(c_), phase(p), t0(hp_clock::now()) {}
    ~HostPhase() { c->hp_us[phase] += std::chrono::duration<double, std::micro>(hp_clock::now() - t0).count(); }
};

int fail(eincm_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((c), EINCM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                       \
    } while (0)

// g holds at least n elements afterwards.  Growth drains the stream (work in flight may read the old block), frees the old block and
// allocates the new one, zeroed on request; the old contents are gone.  A failed growth leaves g empty.
template <typename T, bool PINNED> hipError_t ensure(eincm_ctx* c, Grow<T, PINNED>& g, size_t n, bool zero = false) {
    if (n <= g.n) return hipSuccess;
    if (const hipError_t e = hipStreamSynchronize(c->stream)) return e;
    c->mem.release(g.p);
    g.p = nullptr; g.n = 0;
    if (const hipError_t e = PINNED ? c->mem.alloc_pinned(g.p, n, zero) : c->mem.alloc_dev(g.p, n, zero)) return e;
    g.n = n;
    return hipSuccess;
}

// The coarse-theta accumulators for theta of up to `cells` doubles per window, zero as every evaluation expects them.
hipError_t ensure_coarse(eincm_ctx* c, size_t cells) {
    if (const hipError_t e = ensure(c, c->d_gth, (size_t)2 * c->maxB * cells, true)) return e;
    c->coarse_cap = (int64_t)(c->d_gth.n / ((size_t)2 * c->maxB));
    return hipSuccess;
}

// The one-shot operators that must not run beside an evaluation begun and not yet collected (its kernels may be on the stream)
int not_in_flight(eincm_ctx* c, const char* who) {
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "%s: an evaluation is in flight", who);
    return EINCM_OK;
}

// Abandons the evaluation in flight (Flight::abandon: drain, IDLE) on every exit of its scope but the hand-over: keep() says the state
// the flight is left in is meant - FORWARD or LAUNCHED for the next call, IDLE after a collect (who arms one).
struct FlightGuard {
    eincm_ctx* c; bool armed = true;
    explicit FlightGuard(eincm_ctx* c_) : c(c_) {}
    FlightGuard(const FlightGuard&) = delete;
    ~FlightGuard() { if (armed) c->fl.abandon(c->stream); }
    int keep(int rc = EINCM_OK) { armed = false; return rc; }
};

// The call frame of a one-shot operator.  After its argument checks an operator declares the pieces of c->scratch
// it needs (piece) and the host memory its downloads land in (host_buf), grows the block once (begin), and puts every command on the
// stream through the frame.  The destructor drains the stream on every exit that sync() has not drained already, and the members are
// freed after it: no exit leaves work on the block, or a copy in flight on host memory of the call.  Host memory an asynchronous copy
// touches is therefore the caller's, the context's, a host_buf, or (upload sources only) a local declared before the frame.
struct OneShot {
    eincm_ctx* c; size_t total = 0; bool pending = false;
    std::vector<std::vector<char>> host;
    explicit OneShot(eincm_ctx* c_) : c(c_) {}
    OneShot(const OneShot&) = delete;
    ~OneShot() { if (pending) (void)hipStreamSynchronize(c->stream); }
    // A piece resolves its pointer when it is used, so the block cannot be read before begin() has grown it
    template <typename T> struct Piece {
        const OneShot* op; size_t off; bool on;
        operator T*() const { return on ? reinterpret_cast<T*>(op->c->scratch.p + off) : nullptr; }
    };
    // n elements at the next 256-byte-aligned offset; a piece that is not wanted takes no bytes and is null
    template <typename T> Piece<T> piece(size_t n, bool wanted = true) {
        const size_t off = total;
        if (wanted) total += (n * sizeof(T) + 255) & ~(size_t)255;
        return {this, off, wanted};
    }
    template <typename T> T* host_buf(size_t n) { host.emplace_back(n * sizeof(T), 0); return reinterpret_cast<T*>(host.back().data()); }
    hipError_t begin() { if (const hipError_t e = hipSetDevice(c->device)) return e; return ensure(c, c->scratch, total); }
    hipError_t up(void* dst, const void* src, size_t bytes) { pending = true; return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream); }
    hipError_t down(void* dst, const void* src, size_t bytes) { pending = true; return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream); }
    hipError_t zero(void* dst, size_t bytes) { pending = true; return hipMemsetAsync(dst, 0, bytes, c->stream); }
    // every argument is cast to the kernel's own parameter type (a Piece<T> to T* or const T*, a void* to any object pointer)
    template <typename... P, typename... A> hipError_t launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds, A&&... a) {
        pending = true;
        hipLaunchKernelGGL(k, grid, block, lds, c->stream, static_cast<P>(a)...);
        return hipGetLastError();
    }
    hipError_t sync() { pending = false; return hipStreamSynchronize(c->stream); }
};

// The front end of the operators on one chunk of a raw event stream (eincm_event_support, eincm_event_filter; DESIGN.md
// sections 5.2 and 23): what they share before their own kernels.  Constructed on the call's OneShot before begin(), it declares the shared pieces;
// then, in the operator's order of calls, validate() refuses a bad chunk, carried_maps() readies the operator's own carried state,
// and sort_and_bound() leaves every pixel's events as one ascending run [lo()[pixel], hi()[pixel]) of key() (sorted pixel keys) and
// idx() (the event indices in that order).  It touches no carried state but what carried_maps() is handed.
struct StreamChunk {
    eincm_ctx* const c; OneShot& op;
    const int16_t* const x; const int16_t* const y; const double* const t; const int64_t n; const uint8_t* const pixel_mask;
    const int H, W; const int64_t npix; const EsSortPlan plan;
    const unsigned gn, gp;                                               // grids of NT threads over the events, over the pixels
    const OneShot::Piece<int16_t> d_x, d_y; const OneShot::Piece<double> d_t;
    const OneShot::Piece<uint32_t> d_key[2], d_val[2], d_hist, d_tiles, d_lohi;      // (lo | hi)
    const OneShot::Piece<uint8_t> d_mask; const OneShot::Piece<uint32_t> d_err;
    uint32_t* const h_err;                                               // d_err comes down here
    int cur = 0;                                                         // the sorted (key, index) arrays so far: d_key[cur], d_val[cur]
    StreamChunk(OneShot& op_, const int16_t* x_, const int16_t* y_, const double* t_, int64_t n_, const uint8_t* pixel_mask_)
        : c(op_.c), op(op_), x(x_), y(y_), t(t_), n(n_), pixel_mask(pixel_mask_), H(c->H), W(c->W), npix((int64_t)H * W),
          plan(es_sort_plan(n, npix)), gn((unsigned)((n + NT - 1) / NT)), gp((unsigned)((npix + NT - 1) / NT)),
          d_x(op.piece<int16_t>((size_t)n)), d_y(op.piece<int16_t>((size_t)n)), d_t(op.piece<double>((size_t)n)),
          d_key{op.piece<uint32_t>((size_t)n), op.piece<uint32_t>((size_t)n)},
          d_val{op.piece<uint32_t>((size_t)n), op.piece<uint32_t>((size_t)n)}, d_hist(op.piece<uint32_t>((size_t)plan.nhist)),
          d_tiles(op.piece<uint32_t>((size_t)plan.ntiles)), d_lohi(op.piece<uint32_t>((size_t)npix * 2)),
          d_mask(op.piece<uint8_t>((size_t)npix, pixel_mask != nullptr)), d_err(op.piece<uint32_t>(1)), h_err(op.host_buf<uint32_t>(1)) {}

    // The argument faults that every stream operator words alike
    static int bad_n(eincm_ctx* c, int64_t n) {
        return fail(c, EINCM_ERR_ARG, "n = %lld outside [0, 2^30] (walk a recording in chunks)", (long long)n);
    }
    static int bad_tau(eincm_ctx* c, double tau) { return fail(c, EINCM_ERR_ARG, "tau = %g (finite and >= 0)", tau); }

    // x, y, t go up and are checked against `carried`, the time of the last event before the chunk; the pixel keys are left in key().
    // A refusal names the first offender.
    int validate(double carried) {
        if (n == 0) return EINCM_OK;
        HIPCHK(c, op.up(d_x, x, (size_t)n * 2));                         // (host memory: the caller's, as every copy below but h_err's)
        HIPCHK(c, op.up(d_y, y, (size_t)n * 2));
        HIPCHK(c, op.up(d_t, t, (size_t)n * 8));
        HIPCHK(c, op.zero(d_err, sizeof(uint32_t)));
        HIPCHK(c, op.launch(k_es_validate, dim3(gn), dim3(NT), 0, H, W, n, d_x, d_y, d_t, carried, d_key[0], d_err));
        HIPCHK(c, op.down(h_err, d_err, sizeof(uint32_t)));
        HIPCHK(c, op.sync());
        if (!*h_err) return EINCM_OK;
        const int64_t e = n - (int64_t)*h_err;
        if (e < 0 || e >= n) return fail(c, EINCM_ERR_HIP, "first refused event %lld of %lld", (long long)e, (long long)n);
        switch (es_event_fault(H, W, x[e], y[e], t[e], e > 0 ? t[e - 1] : carried)) {
            case ES_EV_COORD: return fail(c, EINCM_ERR_ARG, "event %lld: (%d, %d) outside the %dx%d sensor", (long long)e, x[e], y[e], H, W);
            case ES_EV_TIME: return fail(c, EINCM_ERR_ARG, "event %lld: time %g is not finite", (long long)e, t[e]);
            default:
                return fail(c, EINCM_ERR_ARG, "event %lld: time %.17g is smaller than %.17g, %s", (long long)e, t[e],
                            e > 0 ? t[e - 1] : carried, e > 0 ? "its predecessor's" : "the last time of the previous chunk");
        }
    }

    // An operator's carried maps (count doubles) exist afterwards; on the first call and on a reset they, and last_time, say "no event"
    int carried_maps(Grow<double>& maps, size_t count, int reset, double& last_time) {
        const bool fresh = maps.n < count;
        HIPCHK(c, ensure(c, maps, count));
        if (fresh || reset) {
            HIPCHK(c, op.launch(k_es_fill, dim3((unsigned)((count + NT - 1) / NT)), dim3(NT), 0, (int64_t)count, maps.p, es_no_event()));
            last_time = es_no_event();
        }
        return EINCM_OK;
    }

    // n > 0, after validate(): the mask goes up, (key, index) are sorted by key and every pixel's run is bounded
    int sort_and_bound() {
        if (pixel_mask) HIPCHK(c, op.up(d_mask, pixel_mask, (size_t)npix));
        HIPCHK(c, op.zero(d_lohi, (size_t)npix * 2 * sizeof(uint32_t)));
        const unsigned nblk = (unsigned)plan.nblk, ntiles = (unsigned)plan.ntiles;
        for (int pass = 0; pass < plan.passes; ++pass, cur ^= 1) {
            const int shift = pass * ES_RADIX_BITS;
            const uint32_t* const vin = pass ? (const uint32_t*)d_val[cur] : nullptr;      // (pass 0: the indices themselves)
            HIPCHK(c, op.launch(k_es_hist, dim3(nblk), dim3(64), 0, n, plan.nblk, shift, d_key[cur], d_hist));
            HIPCHK(c, op.launch(k_es_scan_tiles, dim3(ntiles), dim3(ES_SCAN_NT), 0, plan.nhist, d_hist, d_tiles));
            HIPCHK(c, op.launch(k_es_scan, dim3(1), dim3(ES_SCAN_NT), 0, plan.ntiles, d_tiles));
            HIPCHK(c, op.launch(k_es_scatter, dim3(nblk), dim3(64), 0, n, plan.nblk, shift, d_key[cur], vin, d_hist, d_tiles,
                                d_key[cur ^ 1], d_val[cur ^ 1]));
        }
        HIPCHK(c, op.launch(k_es_bounds, dim3(gn), dim3(NT), 0, n, npix, d_key[cur], lo(), hi()));
        return EINCM_OK;
    }
    uint32_t* lo() const { return d_lohi; }
    uint32_t* hi() const { return lo() + npix; }
    const uint32_t* key() const { return d_key[cur]; }
    const uint32_t* idx() const { return d_val[cur]; }
};

// Where window b's events start in the stream order (the batch as handed over: d_raw_*, ord.stream, every per-event array of an operator)
inline int64_t stream_offset(const int64_t* n_events, int b) { return sc_block_offset(n_events, b, 1, true); }

// The front of the per-event operators on the staged raw events (eincm_event_scores, eincm_event_responsibilities,
// eincm_contrast_landscape).  Constructed on the call's OneShot after the operator's checks and before begin(), it declares the (B + 1)
// offset table of the kernels, the frame's first piece, and fills it by the layout function of the operator's contract (the stream order).
struct RawEvents {
    OneShot& op; const int B; const int64_t* const ne;                   // the staged windows' event counts
    const OneShot::Piece<int64_t> d_off; int64_t* const h_off;           // d_off goes up from h_off (upload)
    int64_t n_max = 0;                                                   // the most events of one window
    explicit RawEvents(OneShot& op_, int64_t (*offset)(const int64_t* n_events, int b) = stream_offset)
        : op(op_), B(op.c->g.B), ne(op.c->win_events.data()), d_off(op.piece<int64_t>((size_t)B + 1)), h_off(op.host_buf<int64_t>((size_t)B + 1)) {
        for (int b = 0; b <= B; ++b) h_off[b] = offset(ne, b);
        for (int b = 0; b < B; ++b) n_max = std::max(n_max, ne[b]);
    }
    int64_t total() const { return h_off[B]; }
    // Did the last evaluation leave a window of the staged batch out (eincm_loss_grad_masked)?  Its Theta and IWEs are not that window's.
    static bool masked(const eincm_ctx* c) {
        for (int b = 0; c->staged && b < c->g.B && b < 64; ++b) if (!((c->eval_wmask >> b) & 1ull)) return true;
        return false;
    }
    hipError_t upload() { return op.up(d_off, h_off, ((size_t)B + 1) * sizeof(int64_t)); }
    // One optional host array per window (the caller's: NULL, or per window NULL or its events' values) as one packed device array in
    // the stream order plus a `has` byte per window.  any(): some window with events has one - what the two pieces are wanted for.
    template <typename T> bool any(const T* const* arrays) const {
        for (int b = 0; arrays && b < B; ++b) if (arrays[b] && ne[b] > 0) return true;
        return false;
    }
    template <typename T> hipError_t upload_per_window(const T* const* arrays, T* piece, uint8_t* has_piece) {
        uint8_t* h_has = op.host_buf<uint8_t>((size_t)B);
        for (int b = 0; b < B; ++b) h_has[b] = arrays[b] && ne[b] > 0;
        if (const hipError_t e = op.up(has_piece, h_has, (size_t)B)) return e;
        for (int b = 0; b < B; ++b)
            if (h_has[b]) if (const hipError_t e = op.up(piece + h_off[b], arrays[b], (size_t)ne[b] * sizeof(T))) return e;
        return hipSuccess;
    }
};

// ---- the environment: every read, one function per lifetime ----
const EvalKnobs& process_knobs() {     // once per process, at the first evaluation of a context that is not float64
    static const EvalKnobs k{getenv("EINCM_NO_BIG_THETA_ARG") != nullptr, getenv("EINCM_NO_HOST_ASM") != nullptr,
                             getenv("EINCM_GATHER_ALL_R") ? atoi(getenv("EINCM_GATHER_ALL_R")) : -1};
    return k;
}
struct CreateKnobs { int seg = 0, seg_s = 0, wincap = 0; bool host_binning = false; };      // (0: not set)
CreateKnobs create_knobs() {           // when a context is created
    CreateKnobs k;
    if (const char* s = getenv("EINCM_SEG")) k.seg = atoi(s);
    if (const char* s = getenv("EINCM_SEG_SPLAT")) k.seg_s = atoi(s);
    if (const char* s = getenv("EINCM_WINCAP")) k.wincap = atoi(s);
    k.host_binning = getenv("EINCM_HOST_BINNING") != nullptr;
    return k;
}
struct LiveKnobs { StageKnobs stage; bool no_proj_in_gather = false; };
LiveKnobs live_knobs() {               // where they are used: `stage` at every staging, the other whenever the resample tables are rebuilt
    LiveKnobs k;
    if (const char* e = getenv("EINCM_SEG_2DOF")) k.stage.seg_2 = atoi(e);
    if (const char* e = getenv("EINCM_PITCH_ALIGNED")) { k.stage.has_pitch = true; k.stage.pitch = atoi(e); }
    k.stage.no_segsort = getenv("EINCM_NO_SEGSORT") != nullptr;
    k.stage.no_spread = getenv("EINCM_NO_SPREAD") != nullptr;
    k.no_proj_in_gather = getenv("EINCM_NO_PROJ_IN_GATHER") != nullptr;
    return k;
}

void free_all(eincm_ctx* c) {
    if (c->have_events) {
        for (int k = 0; k < eincm_ctx::EV_RING; ++k)
            for (int i = 0; i <= EINCM_N_STAGES; ++i)
                for (int e = 0; e < 2; ++e)
                    if (c->ev[k][i][e]) { (void)hipEventDestroy(c->ev[k][i][e]); c->ev[k][i][e] = nullptr; }
        for (int k = 0; k < eincm_ctx::GRAD_PIECES; ++k) if (c->ev_piece[k]) { (void)hipEventDestroy(c->ev_piece[k]); c->ev_piece[k] = nullptr; }
        c->have_events = false;
    }
    if (c->stream) { (void)hipStreamDestroy(c->stream); c->stream = nullptr; }
    c->mem.release_all();
}

// EINCM_CF_TIMING: a stage made of ONE kernel launch (single = true) gets its start / stop events attached to that launch
// (launch_timed: the dispatch's own timestamps, no packets on the stream); any other stage is bracketed by marker events, whose
// barrier packets add a few microseconds to the interval they measure and to the evaluation.
struct StageTimer {
    eincm_ctx* c; int stage; bool on, single;
    StageTimer(eincm_ctx* c_, int s, bool single_ = false) : c(c_), stage(s), on((c_->cflags & EINCM_CF_TIMING) != 0), single(single_) {
        if (on && single) c->attach_stage = stage;
        else if (on) { (void)hipEventRecord(c->ev[c->fl.ring_cur][stage][0], c->stream); }
    }
    ~StageTimer() {
        if (on && single) c->attach_stage = -1;
        else if (on) { (void)hipEventRecord(c->ev[c->fl.ring_cur][stage][1], c->stream); c->ev_used[c->fl.ring_cur][stage] = true; }
    }
};

// EINCM_CF_TIMING_DOMINANT: the two event kernels are launched with their own start / stop events (hipExtLaunchKernelGGL: the
// dispatch's completion signal carries the timestamps).  Marker events around them (hipEventRecord) cost 25 us per evaluation in
// barrier packets and lost launch overlap; attached events cost ~6 us per timed kernel.
static inline bool timing_on(const eincm_ctx* c) {
    return (c->cflags & EINCM_CF_TIMING) != 0 || ((c->cflags & EINCM_CF_TIMING_DOMINANT) != 0 && c->fl.timed_now);
}

template <typename K, typename... Args>
void launch_timed(eincm_ctx* c, int stage, K kernel, dim3 grid, dim3 block, size_t lds, Args... args) {
    const bool attach = (c->cflags & EINCM_CF_TIMING) ? c->attach_stage == stage
                      : ((c->cflags & EINCM_CF_TIMING_DOMINANT) && c->fl.timed_now) ? (stage == EINCM_STAGE_SPLAT ? c->time_splat : stage == EINCM_STAGE_GATHER && c->time_gather)
                      : false;
    if (attach) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, c->stream, c->ev[c->fl.ring_cur][stage][0], c->ev[c->fl.ring_cur][stage][1], 0,
                              args...);
        c->ev_used[c->fl.ring_cur][stage] = true;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, args...);
    }
}

int ensure_resample(eincm_ctx* c, int h, int w, int method) {
    if (c->cur_h == h && c->cur_w == w && c->cur_method == method) return EINCM_OK;
    static_assert(sizeof(Int2) == sizeof(int2) && sizeof(TileRange) == 4 * sizeof(int), "the tap tables go up as they are");
    ResampleTables t;
    build_resample(h, w, c->H, c->W, method, t);
    HIPCHK(c, ensure(c, c->d_AH, t.AH.size()));
    HIPCHK(c, ensure(c, c->d_AW, t.AW.size()));
    HIPCHK(c, hipMemcpyAsync(c->d_AH.p, t.AH.data(), t.AH.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_AW.p, t.AW.data(), t.AW.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_rowtap, t.rowtap.data(), t.rowtap.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_coltap, t.coltap.data(), t.coltap.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_tilerng, t.tilerng.data(), t.tilerng.size() * sizeof(TileRange), hipMemcpyHostToDevice, c->stream));
    c->proj_in_gather = t.fits && !live_knobs().no_proj_in_gather;
    HIPCHK(c, hipStreamSynchronize(c->stream));     // host vectors go out of scope
    c->cur_h = h; c->cur_w = w; c->cur_method = method;
    return EINCM_OK;
}

// Every cross-workgroup accumulator (u64 IWE stack, i64 dL/dTheta, i64 coarse cells) is zero between evaluations because its
// consumer clears it.  If a forward half was launched and never consumed (error between the two halves), clear them here.
int clear_accumulators(eincm_ctx* c) {
    const size_t img = (size_t)c->H * c->W;
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, (size_t)c->maxB * c->maxR * img * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_gTheta, 0, (size_t)c->maxB * img * 2 * sizeof(long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_gth.p, 0, (size_t)2 * c->maxB * c->coarse_cap * sizeof(long long), c->stream));
    c->acc_dirty = false;
    return EINCM_OK;
}

// theta -> Theta image (+ per-tile velocity bounds) for every window.  theta_dev: (B,h,w,2) on the device or in mapped host memory.
// with_windows: k_theta also fills the window tables of both segment lists (every theta but the 2-DoF one, whose k_theta_const does)
void launch_theta_image(eincm_ctx* c, int h, int w, bool identity, bool use_arg, const ThetaArgBig& targ, const double* theta_dev,
                        bool with_windows) {
    const Geom& g = c->g;
    const bool ww = with_windows && c->itembase_valid;
    auto go = [&](auto kernel, const auto& ta) {
        launch_timed(c, EINCM_STAGE_THETA, kernel, dim3(g.ntiles, g.B), dim3(NT), 0, g, h, w, identity ? 1 : 0, use_arg ? 1 : 0, ta,
                     theta_dev, c->d_AH.p, c->d_AW.p, c->d_rowtap, c->d_coltap, c->d_tilerng, c->d_Theta, c->d_tmm, c->d_edge_ts,
                     c->gather.n, c->gather.d_items, ww ? c->gather.d_itembase : nullptr, c->gather.d_wins,
                     c->splat.n, c->splat.d_items, ww ? c->splat.d_itembase : nullptr, c->splat.d_wins);
    };
    // the argument block is copied by value into the launch and again into the kernarg buffer: 4 KiB where theta fits (one window at 16x16)
    if (!use_arg || (size_t)g.B * h * w * 2 <= (size_t)THETA_ARG_MID) {
        ThetaArgMid mid;
        if (use_arg) memcpy(mid.v, targ.v, (size_t)g.B * h * w * 2 * sizeof(double));
        go(k_theta<ThetaArgMid>, mid);
    } else {
        go(k_theta<ThetaArgBig>, targ);
    }
    c->Theta_valid = true;
}

// The event kernels the library contains: every row of eincm_plan.h's four form lists bound to its instantiation, in the lists' order,
// so a plan's row (SplatForm.row, GatherForm.row) is the kernel to launch.  No other place names an instantiation of the four.
template <size_t... I> constexpr auto bind_splat(std::index_sequence<I...>) {
    return std::array{&k_splat<SPLAT_FORMS[I].mode, SPLAT_FORMS[I].threads, SPLAT_FORMS[I].weighted>...};
}
template <size_t... I> constexpr auto bind_splat_r(std::index_sequence<I...>) {
    return std::array{&k_splat_r<SPLAT_R_FORMS[I].mode, SPLAT_R_FORMS[I].rad>...};
}
template <size_t... I> constexpr auto bind_gather(std::index_sequence<I...>) {
    return std::array{&k_gather<GATHER_FORMS[I].mode, GATHER_FORMS[I].wide, GATHER_FORMS[I].threads, GATHER_FORMS[I].proj, GATHER_FORMS[I].all_r,
                                GATHER_FORMS[I].weighted>...};
}
template <size_t... I> constexpr auto bind_gather_r(std::index_sequence<I...>) {
    return std::array{&k_gather_r<GATHER_R_FORMS[I].mode, GATHER_R_FORMS[I].rad>...};
}
const auto SPLAT_KERNELS = bind_splat(std::make_index_sequence<std::size(SPLAT_FORMS)>{});
const auto SPLAT_R_KERNELS = bind_splat_r(std::make_index_sequence<std::size(SPLAT_R_FORMS)>{});
const auto GATHER_KERNELS = bind_gather(std::make_index_sequence<std::size(GATHER_FORMS)>{});
const auto GATHER_R_KERNELS = bind_gather_r(std::make_index_sequence<std::size(GATHER_R_FORMS)>{});
// k_splat_r and k_gather_r take the mode and the radius alone: their rows hold what the kernels are written for in every other field
constexpr bool other_window_rows_plain() {
    for (const SplatKey& k : SPLAT_R_FORMS) if (k.threads != NT || k.weighted) return false;
    for (const GatherKey& k : GATHER_R_FORMS) if (k.threads != NT || k.wide || k.proj || k.all_r || k.weighted) return false;
    return true;
}
static_assert(other_window_rows_plain(), "a row of SPLAT_R_FORMS / GATHER_R_FORMS names a kernel that k_splat_r / k_gather_r are not");

// a plan whose form is no row: what the entry points refuse (plan_forms), had it come this far
int no_such_form(eincm_ctx* c, const char* kernel, const GatherKey& k) {
    return fail(c, EINCM_ERR_UNSUPPORTED, "internal: the library holds no %s kernel for theta mode %d, splat radius %d, wide %d, %d threads, "
                "proj %d, all_r %d, weighted %d (eincm_plan.h)", kernel, k.mode, k.rad, k.wide, k.threads, k.proj, k.all_r, k.weighted);
}

// The splat of the planned evaluation as its form says (fl.plan.splat), and with it the end of the forward half
int launch_splat(eincm_ctx* c, const double* theta_dev, const ThetaArg& targ) {
    const EvalPlan& P = c->fl.plan;
    const SplatForm& F = P.splat;
    {
        StageTimer t(c, EINCM_STAGE_SPLAT, true);
        if (c->splat.n > 0) {
            if (F.row < 0) return no_such_form(c, "splat", GatherKey{F.key.mode, F.key.rad, 0, F.key.threads, 0, 0, F.key.weighted});
            const SegList& L = seg_list(*c, F.list);
            Geom gs = c->g;
            gs.wincap = F.wincap; gs.winmaxw = F.winmaxw;
            const dim3 grid(L.grid(gs.R)), block(F.key.threads);
            const int use_arg = P.use_arg ? 1 : 0;
            if (F.key.rad == 1)
                launch_timed(c, EINCM_STAGE_SPLAT, SPLAT_KERNELS[F.row], grid, block, F.lds, gs, L.n, L.d_items, c->d_xy, c->d_t, c->d_Theta,
                             c->d_edge_ts, c->splat.d_wins, c->d_acc, L.d_order, use_arg, theta_dev, targ,
                             (const float*)(F.key.weighted ? c->d_w : nullptr));
            else
                launch_timed(c, EINCM_STAGE_SPLAT, SPLAT_R_KERNELS[F.row], grid, block, F.lds, gs, L.n, L.d_items, c->d_xy, c->d_t, c->d_Theta,
                             c->d_tmm, c->d_edge_ts, c->d_acc, L.d_order, use_arg, theta_dev, targ);
        }
    }
    HIPCHK(c, hipGetLastError());
    c->fl.theta_dev = theta_dev; c->fl.targ = targ;
    return EINCM_OK;
}

// Launch the forward half of the planned evaluation (fl.plan): theta -> Theta -> u64 IWE accumulator.
int launch_forward(eincm_ctx* c, const double* theta_host) {
    const EvalPlan& P = c->fl.plan;
    const Geom& g = c->g;
    const bool two_dof = P.shape == EvalPlan::TWO_DOF;
    const size_t nall = (size_t)g.B * P.nth;
    c->acc_dirty = true;               // from the first command on: an exit below leaves accumulators half-written
    if (P.shape == EvalPlan::MOTION) {
        // theta_host is q (B, 12): it rides in the event kernels' arguments behind (cx, cy, s), or is read from the pinned block; the
        // splat forms its tiles and derives its windows itself, so nothing runs in front of it
        auto& mo = c->motion;
        ThetaArg ta{};
        ta.v[0] = mo.model.cx; ta.v[1] = mo.model.cy; ta.v[2] = mo.model.scale;
        const size_t nq = (size_t)g.B * MOTION_NQ;
        if (P.use_arg) memcpy(ta.v + POLY_ARG_Q0, theta_host, nq * sizeof(double));
        else memcpy(mo.h_q(c->maxB), theta_host, nq * sizeof(double));
        mo.last_q.assign(theta_host, theta_host + nq);
        c->last_theta11.clear();
        c->Theta_valid = false;
        return launch_splat(c, mo.h_q(c->maxB), ta);
    }
    ThetaArg targ;
    static thread_local ThetaArgBig targ_big;
    if (P.use_arg_big) memcpy(targ_big.v, theta_host, nall * sizeof(double));
    if (P.use_arg) memcpy(targ.v, theta_host, nall * sizeof(double));      // theta rides in the kernel arguments
    const double* theta_dev = P.use_arg ? c->d_theta_in : c->h_theta;      // (not read where every kernel has theta in its arguments)
    if (P.theta_src == EvalPlan::THETA_DEVICE) {            // the kernels read the caller's buffer, nothing crosses PCIe
        theta_dev = c->fl.io.theta;
    } else if (P.theta_src == EvalPlan::THETA_PINNED) {     // read straight from the pinned, GPU-mapped staging buffer (no copy command)
        memcpy(c->h_theta, theta_host, nall * sizeof(double));
        theta_dev = c->h_theta;
    } else if (P.theta_src == EvalPlan::THETA_PIECES) {
        // dense theta (4.9 MB at 480x640): staged through pinned memory in a few pieces, so that the DMA of one piece runs while the
        // host copies the next (one memcpy + one DMA back to back: 131 + 187 us)
        StageTimer t(c, EINCM_STAGE_COPY);
        const size_t piece = std::max<size_t>((nall + 5) / 6, (size_t)32768);
        for (size_t off = 0; off < nall; off += piece) {
            const size_t n = std::min(piece, nall - off);
            memcpy(c->h_theta + off, theta_host + off, n * sizeof(double));
            HIPCHK(c, hipMemcpyAsync(c->d_theta_in + off, c->h_theta + off, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        theta_dev = c->d_theta_in;
    }
    {
        StageTimer t(c, EINCM_STAGE_THETA, two_dof ? !P.need_theta_image : c->itembase_valid);       // one kernel in either case
        const SegList &ga = c->gather, &sp = c->splat;
        const int nwin_threads = (ga.n + sp.n) * g.R;
        if (two_dof) {
            if (theta_host) c->last_theta11.assign(theta_host, theta_host + (size_t)g.B * 2); else c->last_theta11.clear();
            c->motion.last_q.clear();
            c->Theta_valid = false;
            if (P.need_theta_image) launch_theta_image(c, P.h, P.w, false, P.use_arg_big, targ_big, theta_dev, false);
            // the event kernels derive their windows from theta themselves; the velocity bounds (tmm) only feed k_final's NaN scan,
            // which a host-assembled evaluation does on the host
            if (!P.host_asm)
                launch_timed(c, EINCM_STAGE_THETA, k_theta_const, dim3((std::max(g.B * g.ntiles, nwin_threads) + NT - 1) / NT), dim3(NT), 0, g,
                                   P.use_arg ? 1 : 0, targ, theta_dev, c->d_tmm, c->d_edge_ts, ga.n, ga.d_items, ga.d_wins,
                                   sp.n, sp.d_items, sp.d_wins);
        } else {
            launch_theta_image(c, P.h, P.w, P.shape == EvalPlan::IDENTITY, P.use_arg_big, targ_big, theta_dev, true);
            if (nwin_threads > 0 && !c->itembase_valid)
                hipLaunchKernelGGL(k_windows, dim3((nwin_threads + NT - 1) / NT), dim3(NT), 0, c->stream, g, c->d_tmm, c->d_edge_ts,
                                   ga.n, ga.d_items, ga.d_wins, sp.n, sp.d_items, sp.d_wins);
        }
    }
    return launch_splat(c, theta_dev, targ);
}

// Read one finished evaluation's events (its stream work has been waited for) into last_t and the running sums.
int read_event_slot(eincm_ctx* c, int k) {
    memset(&c->last_t, 0, sizeof c->last_t);
    for (int s = 0; s <= EINCM_N_STAGES; ++s) {
        if (!c->ev_used[k][s]) continue;
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[k][s][0], c->ev[k][s][1]));
        if (s < EINCM_N_STAGES) c->last_t.ms[s] = ms; else c->last_t.total_ms = ms;
    }
    for (int s = 0; s < EINCM_N_STAGES; ++s) c->sum_t.ms[s] += c->last_t.ms[s];
    c->sum_t.total_ms += c->last_t.total_ms;
    ++c->sum_n;
    return EINCM_OK;
}
int drain_event_ring(eincm_ctx* c, int keep) {          // read the oldest finished evaluations until at most `keep` are left
    while (c->ring_n > keep) {
        const int rc = read_event_slot(c, c->ring_lo);
        c->ring_lo = (c->ring_lo + 1) % c->ring_size; --c->ring_n;
        if (rc) return rc;
    }
    return EINCM_OK;
}
// The evaluation in flight has finished (stream waited for): its events join the ring; read at once unless the mode defers it.
int collect_timings(eincm_ctx* c) {
    if (!timing_on(c)) return EINCM_OK;
    ++c->ring_n;
    return (c->ring_size == 1) ? drain_event_ring(c, 0) : EINCM_OK;
}

// The view eincm_loss.h's assemblies take of the evaluation that has landed: the plan's parameters and the pinned memory its kernels wrote
LossView loss_view(eincm_ctx* c) {
    const EvalPlan& P = c->fl.plan;
    return LossView{&c->g, &P.ep, P.shape == EvalPlan::TWO_DOF, P.nth, c->h_wc, c->h_outs, c->h_grad, c->fl.theta_nan.data(), c->h_tvparts,
                    c->h_img, c->h_g2, c->h_g11, c->gather_2.h_win_item0.data(), c->win_events.data(), c->f64.h_scal,
                    c->h_objc.data(), c->h_ovals.p, P.og.ck, P.og.rk, P.host_asm};
}

// The whole evaluation of a float64 context (EINCM_CF_FP64), enqueued at once: theta -> Theta (k_theta) -> k64_splat -> image passes
// [-> k_tv] [-> dL/dIWE -> k64_gather -> k64_gfin -> projection] -> results into pinned memory.  eval_end_collect waits and f64_assemble
// adds the scalars up on the host in index order.  None of the fp32 path's launch policy applies: one segment list, one launch form.
int f64_launch(eincm_ctx* c, const double* theta_host) {
    const EvalPlan& P = c->fl.plan;
    const EvalParams& ep = P.ep;
    const Geom& g = c->g;
    const int h = P.h, w = P.w;
    const size_t img = (size_t)g.H * g.W, nth = P.nth;
    memcpy(c->h_theta, theta_host, (size_t)g.B * nth * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(c->d_theta_in, c->h_theta, (size_t)g.B * nth * sizeof(double), hipMemcpyHostToDevice, c->stream));
    static const ThetaArgBig targ{};
    launch_theta_image(c, h, w, P.shape == EvalPlan::IDENTITY, false, targ, c->d_theta_in, false);
    if (P.shape == EvalPlan::TWO_DOF) c->last_theta11.assign(theta_host, theta_host + (size_t)g.B * 2);
    HIPCHK(c, hipMemsetAsync(c->f64.gmax, 0, (size_t)g.B * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipMemsetAsync(c->f64.bad, 0, (size_t)g.B * sizeof(unsigned), c->stream));
    // both event kernels walk the gather's list and copy of the events (sorted by source pixel; the splat's spread copy measured
    // slower with these global atomics: 13.6 vs 10.9 ms of k64_splat on the bench batch, profiles/r04/fp64_mode.txt)
    const SegList& L = c->gather;
    if (L.n > 0)
        hipLaunchKernelGGL(k64_splat, dim3(L.grid(g.R)), dim3(NT), 0, c->stream, g, L.n, L.d_items, c->d_xy_g, c->d_t_g, c->d_Theta,
                           c->d_edge_ts, c->f64.ishift, c->f64.acc);
    const dim3 gimg(c->f64.P, g.R, g.B);
    hipLaunchKernelGGL(k64_img_a, gimg, dim3(NT), 0, c->stream, g, c->f64.ishift, c->f64.acc, c->f64.iwe, c->f64.partA);
    hipLaunchKernelGGL(k64_img_b, gimg, dim3(NT), 0, c->stream, g, c->f64.iwe, c->f64.edges, c->f64.partA, c->f64.partB, ep.want_div,
                       P.div_grad ? c->f64.sgn : nullptr);
    hipLaunchKernelGGL(k64_scal, dim3(g.R, g.B), dim3(NT), 0, c->stream, g, c->f64.P, c->f64.partA, c->f64.partB, c->f64.scal);
    HIPCHK(c, hipMemcpyAsync(c->f64.h_scal, c->f64.scal, (size_t)g.B * g.R * sizeof(F64Scal), hipMemcpyDeviceToHost, c->stream));
    if (ep.want_tv)            // shared with the fp32 path: k_tv is fp64 throughout; its partials also land in pinned memory for f64_assemble
        hipLaunchKernelGGL(k_tv<0>, dim3(g.ntiles, g.B), dim3(NT), 0, c->stream, g, c->d_Theta, c->d_mask, c->d_tvg, c->d_tvparts,
                           P.full_aux ? 1 : 0, h, w, c->d_AH.p, c->d_AW.p, c->d_tilerng, c->d_gth.p + (size_t)c->maxB * c->coarse_cap,
                           (int)c->coarse_cap, c->h_tvparts);
    if (P.want_grad) {
        hipLaunchKernelGGL(k64_grad1, gimg, dim3(NT), 0, c->stream, g, ep, c->f64.iwe, c->f64.edges, c->f64.scal, c->d_wc,
                           P.div_grad ? c->f64.sgn : nullptr, c->f64.G, c->f64.partC);
        hipLaunchKernelGGL(k64_grad2, gimg, dim3(NT), 0, c->stream, g, c->f64.iwe, c->f64.scal, c->f64.partC, c->f64.G, c->f64.gmax,
                           c->f64.bad);
        if (L.n > 0)
            hipLaunchKernelGGL(k64_gather, dim3(L.n), dim3(NT), 0, c->stream, g, L.n, L.d_items, c->d_xy_g, c->d_t_g,
                               c->d_Theta, c->d_edge_ts, c->f64.G, c->d_wc, c->f64.gmax, c->f64.gacc, c->f64.bad);
        const unsigned nblk = (unsigned)std::min<size_t>((img * 2 + NT - 1) / NT, 512);
        hipLaunchKernelGGL(k64_gfin, dim3(nblk, g.B), dim3(NT), 0, c->stream, g, ep.use_tv_grad, ep.gamma, c->d_tvparts, c->d_tvg, c->d_wc,
                           c->f64.gmax, c->f64.gacc, c->f64.bad, c->f64.gTh);
        const double* out = c->f64.gTh;
        if (P.shape != EvalPlan::IDENTITY) {
            // the intermediate goes through T, of capacity (B,H,W,2): columns first, (B,H,w,2), unless theta is wider than the sensor;
            // then h < H (h * w <= H * W) and the rows go first, (B,h,W,2)
            const size_t nO = (size_t)g.B * nth;
            if (w <= g.W) {
                const size_t nT = (size_t)g.B * g.H * w * 2;
                hipLaunchKernelGGL(k64_proj_w, dim3((unsigned)std::min<size_t>((nT + NT - 1) / NT, 4096)), dim3(NT), 0, c->stream, g, w, c->d_AW.p,
                                   c->f64.gTh, c->f64.T);
                hipLaunchKernelGGL(k64_proj_h, dim3((unsigned)std::min<size_t>((nO + NT - 1) / NT, 4096)), dim3(NT), 0, c->stream, g, h, w,
                                   c->d_AH.p, c->f64.T, c->f64.grad);
            } else {
                const size_t nT = (size_t)g.B * h * g.W * 2;
                hipLaunchKernelGGL(k64_proj_h_first, dim3((unsigned)std::min<size_t>((nT + NT - 1) / NT, 4096)), dim3(NT), 0, c->stream, g, h,
                                   c->d_AH.p, c->f64.gTh, c->f64.T);
                hipLaunchKernelGGL(k64_proj_w_second, dim3((unsigned)std::min<size_t>((nO + NT - 1) / NT, 4096)), dim3(NT), 0, c->stream, g, h,
                                   w, c->d_AW.p, c->f64.T, c->f64.grad);
            }
            out = c->f64.grad;
        }
        HIPCHK(c, hipMemcpyAsync(c->h_grad, out, (size_t)g.B * nth * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipGetLastError());
    c->fl.n_pieces = 0; c->fl.copy_mode = 0;
    return EINCM_OK;
}

// ---- selectable objective kinds (eincm_objectives.hip.h) ----
int obj_buffers(eincm_ctx* c, const ObjGeom& og) {
    const size_t n = (size_t)c->g.B * c->g.R * og.ncells * OBJ_NP;
    HIPCHK(c, ensure(c, c->d_oparts, n));
    HIPCHK(c, ensure(c, c->d_objc, (size_t)c->maxB));
    HIPCHK(c, ensure(c, c->h_ovals, (size_t)c->maxB * c->maxR * 2));
    return EINCM_OK;
}

// The zero-warp values of every kind for the staged windows and the current tile size: k_obj_parts on (zero-warp IWE, E_r),
// k_obj_const; the default kinds' values come from the window constants of staging.  Synchronous (once per staging / tile size).
int obj_constants(eincm_ctx* c) {
    if (c->objc_valid) return EINCM_OK;
    const ObjGeom og = obj_geom(*c, 0, 0, OBJ_NEED_TILE_GM | OBJ_NEED_GM | OBJ_NEED_JOINT);
    int rc = obj_buffers(c, og);
    if (rc) return rc;
    Geom g = c->g;
    g.wmask = ~0ull;
    hipLaunchKernelGGL(k_obj_parts, dim3(og.ncells, g.R, g.B), dim3(NT), 0, c->stream, g, og, c->d_zero_iwe, 0, c->d_edges, c->d_oparts.p);
    hipLaunchKernelGGL(k_obj_const, dim3(g.B), dim3(64), 0, c->stream, g, og, c->d_oparts.p, c->d_objc.p);
    HIPCHK(c, hipGetLastError());
    c->h_objc.assign((size_t)c->maxB, ObjConst{});
    HIPCHK(c, hipMemcpyAsync(c->h_objc.data(), c->d_objc.p, (size_t)g.B * sizeof(ObjConst), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < g.B; ++b) {
        ObjConst& o = c->h_objc[b];
        const WinConst& wc = c->h_wc[b];
        o.c0[0] = wc.c0_gradmag; o.c0[1] = wc.c0_var;
        for (int r = 0; r < g.R; ++r) o.zc[0][r] = wc.zc[r];
    }
    HIPCHK(c, hipMemcpyAsync(c->d_objc.p, c->h_objc.data(), (size_t)g.B * sizeof(ObjConst), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->objc_valid = true;
    return EINCM_OK;
}

void scan_theta(eincm_ctx* c, const double* theta_host, size_t nth) {
    c->fl.theta_nan.assign((size_t)c->g.B, 0);
    eincm::scan_theta(theta_host, c->g.B, nth, c->fl.theta_nan.data());
}

// First half of an evaluation: checks, side effects, plan_eval, then theta -> Theta -> IWE stack (launch_forward; a float64 context
// enqueues the whole evaluation, f64_launch).  theta_host: (B,h,w,2) doubles, or io.theta in HBM.  Leaves the flight FORWARD (float64:
// LAUNCHED); any other exit abandons it.  A forward half that was never finished is discarded.
// motion: the fused evaluation of a motion model (plan_motion): theta_host is q (B, 12) and io carries the bound of the field alone.
int eval_begin(eincm_ctx* c, const double* theta_host, int h, int w, const eincm_params* p, bool want_grad, const uint8_t* active = nullptr,
               const DevIo& io = DevIo{}, bool motion = false) {
    HostPhase hp(c, EINCM_HP_BEGIN);
    // (checked before the flight is touched: the evaluation in flight reads the mask and its plan again when it is collected)
    if (c->fl.launched())
        return fail(c, EINCM_ERR_STATE, "an asynchronous evaluation is in flight: call eincm_loss_grad_wait first");
    FlightGuard guard(c);
    c->fl.land(); c->fl.io = io;
    {   // which windows take part (eincm_loss_grad_masked); the others' workgroups leave at once, their outputs are not written
        unsigned long long m = ~0ull;
        if (active) { m = 0ull; for (int b = 0; b < c->g.B && b < 64; ++b) if (active[b]) m |= 1ull << b; }
        c->g.wmask = m;
        c->eval_wmask = m;
    }
    const Geom& g = c->g;
    const size_t img = (size_t)g.H * g.W;
    const size_t nth = (size_t)h * w * 2;
    if (p->delta != 0.0 && want_grad && !c->fp64) {      // rare path (the reference keeps delta = 0, configs/main.yaml:19): allocated on first use
        HIPCHK(c, ensure(c, c->d_gdiv, (size_t)c->maxB * c->maxR * img));
        HIPCHK(c, ensure(c, c->d_dgparts, (size_t)c->maxB * c->maxR * g.ntiles * 2));
    }
    if (p->contrast_kind < EINCM_CONTRAST_GRAD_MAG || p->contrast_kind > EINCM_CONTRAST_ADAPTIVE_VARIANCE)
        return fail(c, EINCM_ERR_ARG, "contrast_kind %d unknown", p->contrast_kind);
    const int corr_kind = correlation_kind(p);
    if (corr_kind > EINCM_CORRELATION_JOINT_CONTRAST) return fail(c, EINCM_ERR_ARG, "correlation kind %d unknown", corr_kind);
    if (other_kinds(p)) {
        if (c->fp64)
            return fail(c, EINCM_ERR_UNSUPPORTED, "contrast kind %d / correlation kind %d: not supported in fp64 mode (EINCM_CF_FP64)",
                        p->contrast_kind, corr_kind);
        if (c->constants_pending) return fail(c, EINCM_ERR_STATE, "window constants pending (eincm_finish_constants)");
        const int rco = obj_constants(c);
        if (rco) return rco;
    }
    if (theta_shape(g, h, w) != EvalPlan::IDENTITY) {
        if ((int64_t)h * w > (int64_t)g.H * g.W)
            return fail(c, EINCM_ERR_ARG, "theta (%d,%d,2) has more cells than the %dx%d sensor has pixels: not supported", h, w, g.H, g.W);
        HIPCHK(c, ensure_coarse(c, nth));            // grows for theta beyond 64x64 only (the pyramid tops out at 16x16)
        int rc = ensure_resample(c, h, w, p->method);
        if (rc) return rc;
    }
    static const EvalKnobs no_knobs;               // (a float64 evaluation has no launch policy and reads none)
    const EvalPlan P = motion ? plan_motion(*c, process_knobs(), io.vmax, p, want_grad)
                              : plan_eval(*c, c->fl.io, c->fp64 ? no_knobs : process_knobs(), theta_host, h, w, p, want_grad);
    if (c->fp64) {
        c->fl.plan = P; scan_theta(c, theta_host, nth);
        if (const int rc = f64_launch(c, theta_host)) return rc;
        c->fl.state = Flight::LAUNCHED;
        return guard.keep();
    }
    if (c->acc_dirty) { const int rcd = clear_accumulators(c); if (rcd) return rcd; }
    if (c->cflags & EINCM_CF_TIMING_DOMINANT) c->fl.timed_now = (c->time_counter++ % c->time_period) == 0;
    if (timing_on(c)) {
        if (c->ring_n == c->ring_size) { const int rcr = drain_event_ring(c, c->ring_size - 1); if (rcr) return rcr; }   // ring full: read the oldest
        c->fl.ring_cur = (c->ring_lo + c->ring_n) % c->ring_size;
        for (int s = 0; s <= EINCM_N_STAGES; ++s) c->ev_used[c->fl.ring_cur][s] = false;
        if (c->ring_size == 1) (void)hipEventRecord(c->ev[c->fl.ring_cur][EINCM_N_STAGES][0], c->stream);    // EINCM_CF_TIMING only
    }
    c->fl.plan = P;
    c->policy_evaluated = true;
    c->g.wincap = P.wincap; c->g.winmaxw = P.winmaxw; c->g.pitch_aligned = P.pitch_aligned; c->g.wincap_a = P.wincap_a; c->g.winmaxw_a = P.winmaxw_a;
    if (P.host_asm) scan_theta(c, theta_host, nth);
    if (const int rc = launch_forward(c, theta_host)) return rc;
    c->fl.state = Flight::FORWARD;
    return guard.keep();
}

// The D2H copies of an evaluation whose results k_final left in HBM (d_outs, d_grad).  Enqueued right behind the kernels, or - with
// eincm_set_device_results - only by eincm_finish_collect, after the caller has all-reduced the gradient in HBM.
int enqueue_result_copies(eincm_ctx* c) {
    const Geom& g = c->g;
    const bool want_grad = c->fl.plan.want_grad;
    const size_t nth = c->fl.plan.nth;
    c->fl.n_pieces = 0;
    if (c->fl.io.theta) {                           // eincm_loss_grad_device: scalars to the host, the gradient device to device
        HIPCHK(c, hipMemcpyAsync(c->h_outs, c->d_outs, (size_t)g.B * sizeof(OutScal), hipMemcpyDeviceToHost, c->stream));
        if (want_grad && c->fl.io.grad)
            HIPCHK(c, hipMemcpyAsync(c->fl.io.grad, c->d_grad, (size_t)g.B * nth * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return EINCM_OK;
    }
    if (want_grad && (size_t)g.B * nth >= ((size_t)1 << 17)) {
        // a dense gradient (4.9 MB at 480x640): in pieces, an event behind each, so that eval_end_collect hands piece k over
        // (copy + finite scan on the host) while piece k + 1 is still crossing PCIe
        HIPCHK(c, hipMemcpyAsync(c->h_outs, c->d_outs, (size_t)g.B * sizeof(OutScal), hipMemcpyDeviceToHost, c->stream));
        // the rows of windows that sat this evaluation out were not written: clear them, so that they come back as 0 and pass the
        // host's finite scan (eval_end_collect zeroes them on the host only when the gradient comes in one piece)
        for (int b = 0; b < g.B; ) {
            if (!window_sat_out(g, b)) { ++b; continue; }
            int e = b + 1;
            while (e < g.B && window_sat_out(g, e)) ++e;
            HIPCHK(c, hipMemsetAsync(c->d_grad + (size_t)b * nth, 0, (size_t)(e - b) * nth * sizeof(double), c->stream));
            b = e;
        }
        const size_t total = (size_t)g.B * nth;
        c->fl.piece_len = (total + eincm_ctx::GRAD_PIECES - 1) / eincm_ctx::GRAD_PIECES;
        for (int k = 0; k < eincm_ctx::GRAD_PIECES; ++k) {
            const size_t off = (size_t)k * c->fl.piece_len;
            if (off >= total) break;
            const size_t n = std::min(c->fl.piece_len, total - off);
            HIPCHK(c, hipMemcpyAsync(c->h_grad + off, c->d_grad + off, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->ev_piece[k], c->stream));
            c->fl.n_pieces = k + 1;
        }
    } else if (want_grad && g.B == c->maxB) {      // outs and grad are contiguous: one copy
        HIPCHK(c, hipMemcpyAsync(c->h_outs, c->d_outs, (size_t)g.B * sizeof(OutScal) + (size_t)g.B * nth * sizeof(double),
                                 hipMemcpyDeviceToHost, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->h_outs, c->d_outs, (size_t)g.B * sizeof(OutScal), hipMemcpyDeviceToHost, c->stream));
        if (want_grad)
            HIPCHK(c, hipMemcpyAsync(c->h_grad, c->d_grad, (size_t)g.B * nth * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return EINCM_OK;
}

// Second half, part 1: enqueue image statistics, dL/dIWE, gather, projection, scalar assembly (on whatever is in the IWE
// stack now) and the copy back to pinned memory, as planned (fl.plan).  Returns without synchronising: FORWARD -> LAUNCHED; any
// other exit abandons the flight.
int eval_end_launch(eincm_ctx* c) {
    if (c->fl.idle()) return fail(c, EINCM_ERR_STATE, "no evaluation in flight");
    if (c->fl.launched()) return EINCM_OK;
    FlightGuard guard(c);
    HostPhase hp(c, EINCM_HP_LAUNCH);
    const EvalPlan& P = c->fl.plan;
    const EvalParams& ep = P.ep;
    Geom g = c->g;
    const bool identity = P.shape == EvalPlan::IDENTITY, want_grad = P.want_grad, host_asm = P.host_asm;
    const bool timing = timing_on(c);
    const int n_imwg = (g.nig + IG_NT / 64 - 1) / (IG_NT / 64);
    g.gmax_n = g.R * g.nig;
    {
        StageTimer t(c, EINCM_STAGE_STATS, P.stream_stats);
        // Either way the statistics pass is the consumer of the u64 accumulator: it leaves the fp32 IWE stack in d_iwe and clears
        // the accumulator.
        if (P.stream_stats) {
            g.nparts = NSPART;
            launch_timed(c, EINCM_STAGE_STATS, k_stats_stream, dim3(NSPART, g.R, g.B), dim3(NT), 0, g, c->d_acc, c->d_iwe, c->d_edges,
                         c->d_parts);
        } else {
            g.nparts = g.ntiles;
            const size_t ntot = (size_t)g.B * g.R * g.H * g.W;
            hipLaunchKernelGGL(k_iwe_finish, dim3((unsigned)std::min<size_t>((ntot + NT - 1) / NT, 2048)), dim3(NT), 0, c->stream, g,
                               c->d_acc, c->d_iwe);
            hipLaunchKernelGGL(k_stats, dim3(g.ntiles, g.R, g.B), dim3(NT), 0, c->stream, g, c->d_iwe, c->d_edges, c->d_parts,
                               P.g2_from_imgrad ? 0 : 1);
        }
        c->last_nparts = g.nparts;
    }

    if (ep.want_div) {
        hipLaunchKernelGGL(k_div, dim3(g.ntiles, g.R, g.B), dim3(NT), 0, c->stream, g, c->d_iwe, c->d_parts, c->d_divparts);
    }
    if (ep.want_tv) {
        StageTimer t(c, EINCM_STAGE_TV, true);
        auto go = [&](auto kernel) {
            launch_timed(c, EINCM_STAGE_TV, kernel, dim3(g.ntiles, g.B), dim3(NT), 0, g, c->d_Theta, c->d_mask, c->d_tvg, c->d_tvparts,
                         P.full_aux ? 1 : 0, P.h, P.w, c->d_AH.p, c->d_AW.p, c->d_tilerng, c->d_gth.p + (size_t)c->maxB * c->coarse_cap,
                         (int)c->coarse_cap, host_asm ? c->h_tvparts : nullptr);
        };
        P.tv_proj ? go(k_tv<1>) : go(k_tv<0>);
    }
    if (P.obj && !want_grad) {          // forward only: the per-image values alone
        const ObjGeom& og = P.og;
        hipLaunchKernelGGL(k_obj_parts, dim3(og.ncells, g.R, g.B), dim3(NT), 0, c->stream, g, og, c->d_iwe, 1, c->d_edges, c->d_oparts.p);
        hipLaunchKernelGGL(k_obj_grad, dim3(1, g.R, g.B), dim3(IG_NT), 0, c->stream, g, ep, og, c->d_iwe, c->d_edges, c->d_oparts.p,
                           c->d_wc, c->d_objc.p, c->d_gdiv.p, c->d_dgparts.p, c->d_G, c->d_gmax, c->h_ovals.p, 0);
    }
    if (want_grad) {
        {
            StageTimer t(c, EINCM_STAGE_IMGRAD, !P.div_grad && !P.obj);
            if (P.div_grad)
                hipLaunchKernelGGL(k_divgrad, dim3(g.ntiles, g.R, g.B), dim3(NT), 0, c->stream, g, c->d_iwe, c->d_parts,
                                   c->d_gdiv.p, c->d_dgparts.p);
            if (P.obj) {
                const ObjGeom& og = P.og;
                hipLaunchKernelGGL(k_obj_parts, dim3(og.ncells, g.R, g.B), dim3(NT), 0, c->stream, g, og, c->d_iwe, 1, c->d_edges, c->d_oparts.p);
                hipLaunchKernelGGL(k_obj_grad, dim3(n_imwg, g.R, g.B), dim3(IG_NT), 0, c->stream, g, ep, og, c->d_iwe, c->d_edges, c->d_oparts.p,
                                   c->d_wc, c->d_objc.p, c->d_gdiv.p, c->d_dgparts.p, c->d_G, c->d_gmax, c->h_ovals.p, 1);
            } else {
                launch_timed(c, EINCM_STAGE_IMGRAD, k_imgrad, dim3(n_imwg, g.R, g.B), dim3(IG_NT), 0, g, ep, c->d_iwe, c->d_edges,
                                   c->d_parts, c->d_wc, c->d_gdiv.p, c->d_dgparts.p, host_asm ? c->h_g2 : c->d_g2parts, c->d_G, c->d_gmax,
                                   host_asm ? c->h_img : nullptr, host_asm ? 1 : 0);
            }
        }
        {
            StageTimer t(c, EINCM_STAGE_GATHER, true);
            if (c->gather.n > 0) {
                // as the plan's form says (P.gather): the list, the copy of the events and weights, the window geometry, the kernel
                const GatherForm& F = P.gather;
                if (F.row < 0) return no_such_form(c, "gather", F.key);
                const SegList& L = seg_list(*c, F.list);
                const bool own_copy = F.copy == EventCopy::GATHER;
                const uint32_t* xy_g = own_copy ? c->d_xy_g : c->d_xy;
                const double* t_g = own_copy ? c->d_t_g : c->d_t;
                Geom gg = g;
                gg.pitch_aligned = F.pitch_aligned; gg.wincap_a = F.wincap; gg.winmaxw_a = F.winmaxw;
                const dim3 grid(L.grid(F.wg_per_seg)), block(F.key.threads);
                // the polynomial mode: the moments go to their pinned slots
                double* g11 = P.shape == EvalPlan::MOTION ? c->motion.h_fpart.p : host_asm ? c->h_g11 : c->d_g11;
                const int use_arg = P.use_arg ? 1 : 0;
                if (F.key.rad == 1)
                    launch_timed(c, EINCM_STAGE_GATHER, GATHER_KERNELS[F.row], grid, block, F.lds, gg, L.n, L.d_items, xy_g, t_g, c->d_Theta,
                                 c->d_edge_ts, c->d_G, c->gather.d_wins, c->d_gTheta, g11, c->d_wc, c->d_gmax, L.d_order, use_arg,
                                 c->fl.theta_dev, c->fl.targ, P.h, P.w, c->d_AH.p, c->d_AW.p, c->d_tilerng, c->d_gth.p, (int)c->coarse_cap,
                                 P.grid_tail ? 1 : 0, c->d_gticket, c->gather.d_win_item0, c->h_grad,
                                 (P.grid_tail && ep.use_tv_grad) ? ep.gamma : 0.0, c->d_tvparts, c->d_gth.p + (size_t)c->maxB * c->coarse_cap,
                                 (const float*)(F.key.weighted ? (own_copy ? c->d_w_g : c->d_w) : nullptr));
                else    // another splat window (eincm_splat_window.hip.h): per-workgroup partials (2-DoF) or the dL/dTheta image for k_project
                    launch_timed(c, EINCM_STAGE_GATHER, GATHER_R_KERNELS[F.row], grid, block, F.lds, gg, L.n, L.d_items, xy_g, t_g, c->d_Theta,
                                 c->d_tmm, c->d_edge_ts, c->d_G, c->d_gTheta, g11, c->d_wc, c->d_gmax, c->stage.wide ? 1 : 0, use_arg,
                                 c->fl.theta_dev, c->fl.targ);
            }
        }
        // accumulators: two halves (event gradient | TV gradient), each (maxB, coarse_cap) i64, zero on entry (k_final clears them)
        if (P.nsrc > 0) {
            StageTimer t(c, EINCM_STAGE_PROJECT, true);
            launch_timed(c, EINCM_STAGE_PROJECT, k_project, dim3(g.ntiles, g.B, P.nsrc), dim3(NT), 0, g, P.h, P.w,
                               (int)c->coarse_cap, P.events_projected ? 1 : 0, c->stage.wide ? 1 : 0, c->d_AH.p, c->d_AW.p, c->d_rowtap, c->d_coltap, c->d_gTheta, c->d_tvg,
                               c->d_wc, c->d_gmax, c->d_gth.p, c->d_gth.p + (size_t)c->maxB * c->coarse_cap);
        }
    }
    if (!host_asm) {
        StageTimer t(c, EINCM_STAGE_FINAL, !(want_grad && identity));
        launch_timed(c, EINCM_STAGE_FINAL, k_final, dim3(g.B), dim3(FT), 0, g, ep, c->d_parts, c->d_divparts, c->d_tvparts,
                           P.shape == EvalPlan::MOTION ? c->motion.tmm_zero.p : c->d_tmm, c->d_wc, P.g2_from_imgrad ? c->d_g2parts : nullptr, c->d_gth.p, c->d_gth.p + (size_t)c->maxB * c->coarse_cap, (int)c->coarse_cap,
                           c->d_g11, c->gather_2.d_win_item0, c->gather_2.n, c->d_gmax,
                           P.zero_copy_out ? c->h_outs : c->d_outs, P.zero_copy_out ? c->h_grad : c->d_grad, want_grad ? 1 : 0);
        if (want_grad && identity) {
            hipLaunchKernelGGL(k_final_dense, dim3(256, g.B), dim3(NT), 0, c->stream, g, ep.use_tv_grad, c->stage.wide ? 1 : 0, c->d_gTheta,
                               c->d_tvg, c->d_wc, c->d_gmax, c->d_outs, c->d_grad);
        }
    }
    HIPCHK(c, hipGetLastError());
    c->fl.n_pieces = 0;
    c->fl.copy_mode = (P.zero_copy_out || host_asm) ? 0 : 1;
    if (c->fl.copy_mode && !c->device_results) { const int rcc = enqueue_result_copies(c); if (rcc) return rcc; c->fl.copy_mode = 0; }
    if (timing && c->ring_size == 1) { (void)hipEventRecord(c->ev[c->fl.ring_cur][EINCM_N_STAGES][1], c->stream); c->ev_used[c->fl.ring_cur][EINCM_N_STAGES] = true; }
    c->fl.state = Flight::LAUNCHED;
    c->acc_dirty = false;          // every accumulator this evaluation touched has been consumed (and cleared) by the kernels above
    return guard.keep();
}

// Second half, part 2: wait for the stream and hand the results over.  LAUNCHED -> IDLE once the stream has drained; an exit before
// that abandons the flight (the kernels in flight read the pinned theta staging buffer and write the pinned result block, so the
// context must not look idle, and accept the next theta, while they run).
int eval_end_collect(eincm_ctx* c, double* value, double* grad, eincm_aux* aux) {
    if (!c->fl.launched()) return fail(c, EINCM_ERR_STATE, "no evaluation in flight");
    FlightGuard guard(c);
    Flight& fl = c->fl;
    const Geom& g = c->g;
    const bool want_grad = fl.plan.want_grad;
    const size_t nth = fl.plan.nth, total = (size_t)g.B * nth;
    if (fl.copy_mode) { fl.copy_mode = 0; if (const int rcc = enqueue_result_copies(c)) return rcc; }
    bool nonfinite = false;
    if (fl.n_pieces > 0 && want_grad && grad) {
        for (int k = 0; k < fl.n_pieces; ++k) {
            if (hipEventSynchronize(c->ev_piece[k]) != hipSuccess) break;      // the stream sync below reports the error
            const size_t off = (size_t)k * fl.piece_len;
            if (copy_scan_finite(grad + off, c->h_grad + off, std::min(fl.piece_len, total - off))) nonfinite = true;
        }
    }
    {
        HostPhase hp(c, EINCM_HP_WAIT);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // the gradient went device to device (enqueue_result_copies), or as the moments of a motion model (eincm_loss_grad_motion_fused)
    const bool dev_io = fl.io.theta != nullptr || fl.plan.shape == EvalPlan::MOTION;
    fl.land();
    guard.keep();
    ++c->hp_n;
    const bool whole_grad = want_grad && fl.n_pieces == 0 && !dev_io;        // in pinned memory, in one piece
    if (want_grad && !grad && !dev_io) return fail(c, EINCM_ERR_ARG, "the evaluation was begun with a gradient but grad is NULL");
    HostPhase hp(c, EINCM_HP_COLLECT);
    const LossView v = loss_view(c);
    if (fl.plan.host_asm) host_assemble(v);
    else if (c->fp64) f64_assemble(v);
    if (fl.plan.obj) obj_assemble(v);
    if (const int rc = collect_timings(c)) return rc;
    c->have_eval = true;
    c->G_valid = want_grad;

    if (hand_over(v, whole_grad, value, aux)) nonfinite = true;
    if (whole_grad && copy_scan_finite(grad, c->h_grad, total)) nonfinite = true;      // copy out and look for NaN / Inf in the same pass
    if (nonfinite) return fail(c, EINCM_ERR_NONFINITE, "loss or gradient is not finite");
    return EINCM_OK;
}

int eval_end(eincm_ctx* c, double* value, double* grad, eincm_aux* aux) {
    if (!c->fl.idle() && c->fl.plan.want_grad && !grad) {
        c->fl.abandon(c->stream);                    // the forward half is in flight and reads the pinned theta buffer
        return fail(c, EINCM_ERR_ARG, "the evaluation was begun with a gradient but grad is NULL");
    }
    if (const int rc = eval_end_launch(c)) return rc;
    return eval_end_collect(c, value, grad, aux);
}

// The whole evaluation.  theta_host: (B,h,w,2) doubles (already validated).
int evaluate(eincm_ctx* c, const double* theta_host, int h, int w, const eincm_params* p,
             double* value, double* grad, eincm_aux* aux, const uint8_t* active = nullptr) {
    if (const int rc = eval_begin(c, theta_host, h, w, p, grad != nullptr, active)) return rc;
    return eval_end(c, value, grad, aux);
}

// theta = 0 pass parameters used to obtain the window constants (every IWE_r then equals the IUE)
eincm_params zero_pass_params() {
    eincm_params p{};
    p.alpha = 1.0; p.beta = 1.0; p.cur_pyr_lvl = 1; p.method = EINCM_METHOD_BILINEAR; p.flags = EINCM_PF_FULL_AUX;
    return p;
}

// After the theta = 0 pass has been finished (rc_pass: what its eval_end returned): fill the window constants from its outputs.
int store_constants(eincm_ctx* c, int rc_pass) {
    if (rc_pass != EINCM_OK && rc_pass != EINCM_ERR_NONFINITE) return rc_pass;
    const Geom& g = c->g;
    const size_t img = (size_t)g.H * g.W;
    for (int b = 0; b < g.B; ++b) constants_from_zero_pass(c->h_outs[b], g.R, c->h_wc[b]);
    HIPCHK(c, hipMemcpyAsync(c->d_wc, c->h_wc, (size_t)g.B * sizeof(WinConst), hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < g.B && c->fp64; ++b)
        HIPCHK(c, hipMemcpyAsync(c->f64.zero_iwe + (size_t)b * img, c->f64.iwe + (size_t)b * g.R * img, img * sizeof(double),
                                 hipMemcpyDeviceToDevice, c->stream));
    for (int b = 0; b < g.B && !c->fp64; ++b)      // keep the IUE of every window (first reference image of the theta = 0 pass)
        HIPCHK(c, hipMemcpyAsync(c->d_zero_iwe + (size_t)b * img, c->d_iwe + (size_t)b * g.R * img, img * sizeof(float),
                                 hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_eval = false;
    c->constants_pending = false;
    c->err.clear();
    return EINCM_OK;
}

// What an evaluation entry point asks of the context first: a staged batch, with its window constants unless the call forms them.
int eval_ready(eincm_ctx* c, const char* who, bool need_constants = true) {
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "%s called before eincm_set_windows", who);
    if (need_constants && c->constants_pending) return fail(c, EINCM_ERR_STATE, "window constants pending (eincm_finish_constants)");
    return EINCM_OK;
}

// The argument checks of an evaluation entry point; the call names what differs from eincm_loss_grad's
enum : unsigned { THETA_MAY_BE_NULL = 1, NO_VALUE = 2, CONSTANTS_MAY_PEND = 4, NOT_IN_FP64 = 8 };
int eval_entry(eincm_ctx* c, const char* who, const void* theta, int h, int w, const eincm_params* p, const void* value, unsigned except = 0) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64 && (except & NOT_IN_FP64)) return fail(c, EINCM_ERR_UNSUPPORTED, "%s is not supported in fp64 mode (EINCM_CF_FP64)", who);
    if (const int rc = eval_ready(c, who, !(except & CONSTANTS_MAY_PEND))) return rc;
    if ((!theta && !(except & THETA_MAY_BE_NULL)) || !p || (!value && !(except & NO_VALUE))) return fail(c, EINCM_ERR_ARG, "%s: null pointer argument", who);
    if (h < 1 || w < 1) return fail(c, EINCM_ERR_ARG, "%s: theta shape (%d,%d,2) invalid", who, h, w);
    if (p->method < 0 || p->method > EINCM_METHOD_CUBIC) return fail(c, EINCM_ERR_ARG, "%s: method %d unknown", who, p->method);
    HIPCHK(c, hipSetDevice(c->device));
    return EINCM_OK;
}

// c0, zc[r], d0 are 1 while the theta = 0 pass runs, so that it is well defined; store_constants overwrites them.
int preset_constants(eincm_ctx* c) {
    for (int b = 0; b < c->g.B; ++b) {
        WinConst& wc = c->h_wc[b];
        wc.c0_gradmag = 1.0; wc.c0_var = 1.0; wc.d0 = 1.0;
        for (int r = 0; r < c->g.R; ++r) wc.zc[r] = 1.0;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_wc, c->h_wc, (size_t)c->g.B * sizeof(WinConst), hipMemcpyHostToDevice, c->stream));
    return EINCM_OK;
}

// The zero-warp constants of the staged windows: one forward pass at theta = 0 (then IWE_r == IUE for every r).
int window_constants(eincm_ctx* c) {
    if (const int rc = preset_constants(c)) return rc;
    const std::vector<double> zero((size_t)c->g.B * 2, 0.0);
    std::vector<double> val((size_t)c->g.B);
    const eincm_params p = zero_pass_params();
    const int rc = evaluate(c, zero.data(), 1, 1, &p, val.data(), nullptr, nullptr);
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) c->staged = false;
    return store_constants(c, rc);
}

}  // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

int eincm_abi_version(void) { return EINCM_ABI_VERSION; }

const char* eincm_last_error(const eincm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int eincm_multi_ref_weights(int n_refs, double* w) {
    if (n_refs < 1 || n_refs > EINCM_MAX_REFS || !w) return EINCM_ERR_ARG;
    multi_ref_weights(n_refs, w);
    return EINCM_OK;
}

int eincm_resample_matrix(int n_in, int n_out, int method, double* A) {
    if (n_in < 1 || n_out < 1 || !A || method < 0 || method > EINCM_METHOD_CUBIC) return EINCM_ERR_ARG;
    std::vector<double> M;
    resample_matrix(n_in, n_out, method, M);
    memcpy(A, M.data(), M.size() * sizeof(double));
    return EINCM_OK;
}

eincm_ctx* eincm_create(int device, int H, int W, int max_refs, int max_windows, int64_t max_events_total, uint32_t flags) {
    if (H < 3 || W < 3 || H > 32767 || W > 32767 || max_refs < 1 || max_refs > EINCM_MAX_REFS || max_windows < 1 ||
        max_events_total < 1 || max_events_total > (int64_t)2000000000) {
        fail(nullptr, EINCM_ERR_ARG, "eincm_create: bad argument (H=%d W=%d max_refs=%d max_windows=%d max_events=%lld)",
             H, W, max_refs, max_windows, (long long)max_events_total);
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        fail(nullptr, EINCM_ERR_HIP, "eincm_create: no HIP device visible (%s); this engine has no CPU fallback",
             hipGetErrorString(e));
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        fail(nullptr, EINCM_ERR_ARG, "eincm_create: device %d out of range (0..%d)", device, ndev - 1);
        return nullptr;
    }
    if ((flags & EINCM_CF_FP64) && (flags & (EINCM_CF_TIMING | EINCM_CF_TIMING_DOMINANT))) {
        fail(nullptr, EINCM_ERR_UNSUPPORTED, "eincm_create: the timing flags are not supported with EINCM_CF_FP64");
        return nullptr;
    }
    eincm_ctx* c = new eincm_ctx();
    c->fp64 = (flags & EINCM_CF_FP64) != 0;
    c->device = device; c->H = H; c->W = W; c->maxR = max_refs; c->maxB = max_windows; c->maxN = max_events_total;
    c->cflags = flags;
    auto bail = [&](const char* what, hipError_t err) -> eincm_ctx* {
        fail(nullptr, EINCM_ERR_HIP, "eincm_create: %s failed: %s", what, hipGetErrorString(err));
        free_all(c);
        delete c;
        return nullptr;
    };
#define TRY(expr) do { hipError_t e2_ = (expr); if (e2_ != hipSuccess) return bail(#expr, e2_); } while (0)
    TRY(hipSetDevice(device));
    TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const int tilesX = (W + TS - 1) / TS, tilesY = (H + TS - 1) / TS, ntiles = tilesX * tilesY;
    const size_t B = max_windows, R = max_refs, img = (size_t)H * W;
    // the switches a context reads when it is created, all of them (a staging reads its own: live_knobs)
    const CreateKnobs k = create_knobs();
    if (k.seg >= MIN_SEG && k.seg <= MAX_SEG) c->seg = k.seg;
    if (k.seg_s >= MIN_SEG && k.seg_s <= MAX_CHUNK) c->seg_s = k.seg_s;   // k_splat's u32 sums bound a segment
    if (k.wincap >= 1024 && k.wincap <= 6912) { c->wincap = (k.wincap / 4) * 4; c->wincap_fixed = true; }
    c->host_binning = (ntiles > BIN_MAX_TILES) || k.host_binning;
    c->max_items = (int64_t)B * ntiles + max_events_total / MIN_SEG + 1;   // a tile of n events is cut into ceil(n / seg) segments, seg >= MIN_SEG
    TRY(c->mem.alloc_dev(c->d_xy, (size_t)max_events_total));
    TRY(c->mem.alloc_dev(c->d_t, (size_t)max_events_total));
    TRY(c->mem.alloc_dev(c->d_xy_g, (size_t)max_events_total));
    TRY(c->mem.alloc_dev(c->d_t_g, (size_t)max_events_total));
    for (SegList* L : {&c->gather, &c->splat, &c->splat_sh, &c->gather_2}) {
        TRY(c->mem.alloc_dev(L->d_items, (size_t)c->max_items));
        TRY(c->mem.alloc_dev(L->d_order, (size_t)c->max_items));
    }
    for (SegList* L : {&c->gather, &c->gather_2}) TRY(c->mem.alloc_dev(L->d_win_item0, B + 1));
    for (SegList* L : {&c->gather, &c->splat}) {
        TRY(c->mem.alloc_dev(L->d_wins, (size_t)c->max_items * max_refs));
        if (!c->host_binning) TRY(c->mem.alloc_dev(L->d_itembase, B * ntiles));
    }
    TRY(c->mem.alloc_dev(c->d_raw_x, (size_t)max_events_total));          // kept after staging: eincm_get_warped_events walks them
    TRY(c->mem.alloc_dev(c->d_raw_y, (size_t)max_events_total));
    TRY(c->mem.alloc_dev(c->d_raw_t, (size_t)max_events_total));
    if (!c->host_binning) {
        c->max_binblocks = max_events_total / BIN_CHUNK + (int64_t)B + 1;
        TRY(c->mem.alloc_dev(c->d_binblocks, (size_t)c->max_binblocks));
        TRY(c->mem.alloc_dev(c->d_win_blk, B + 1));
        TRY(c->mem.alloc_dev(c->d_blockhist, (size_t)c->max_binblocks * ntiles));
        TRY(c->mem.alloc_dev(c->d_tilecount, B * ntiles));
        TRY(c->mem.alloc_dev(c->d_tilebase, B * ntiles));
        TRY(c->mem.alloc_dev(c->d_bin_misc, (size_t)8));
        TRY(c->mem.alloc_dev(c->d_edges_raw, B * R * img));
        TRY(c->mem.alloc_dev(c->d_edge_moments, B * R * EDGE_PARTS * EDGE_MOM));
    }
    TRY(c->mem.alloc_dev(c->d_edges, B * R * img));
    TRY(c->mem.alloc_dev(c->d_edge_ts, B * R));
    TRY(c->mem.alloc_dev(c->d_acc, B * R * img, true));
    TRY(c->mem.alloc_dev(c->d_iwe, B * R * img));
    TRY(c->mem.alloc_dev(c->d_G, B * R * img));
    TRY(c->mem.alloc_dev(c->d_g11, (size_t)(c->max_items + NXCD) * R * 2));
    TRY(c->mem.alloc_dev(c->d_dtmax, B));
    TRY(c->mem.alloc_dev(c->d_cntmax, B));
    const size_t nig = (size_t)((W + IG_COLS - 1) / IG_COLS) * ((H + IG_ROWS - 1) / IG_ROWS);   // k_imgrad strips per image
    TRY(c->mem.alloc_dev(c->d_gmax, B * R * nig, true));
    TRY(c->mem.alloc_dev(c->d_zero_iwe, B * img));
    TRY(c->mem.alloc_dev(c->d_Theta, B * img * 2));
    TRY(c->mem.alloc_dev(c->d_theta_in, B * img * 2));
    TRY(c->mem.alloc_dev(c->d_gTheta, B * img * 2, true));
    TRY(c->mem.alloc_dev(c->d_tvg, B * img * 2));
    TRY(c->mem.alloc_dev(c->d_mask, B * img));
    TRY(c->mem.alloc_dev(c->d_tmm, B * ntiles * 4));
    const size_t pstride = (size_t)std::max(ntiles, NSPART);
    TRY(c->mem.alloc_dev(c->d_parts, B * R * pstride));
    TRY(c->mem.alloc_dev(c->d_gticket, B, true));
    TRY(c->mem.alloc_dev(c->d_divparts, B * R * ntiles));
    TRY(c->mem.alloc_dev(c->d_g2parts, B * R * nig));
    TRY(c->mem.alloc_dev(c->d_tvparts, B * ntiles * 3));
    TRY(c->mem.alloc_dev(c->d_wc, B));
    {   // one device block and one pinned block: [OutScal x B | grad (B,H,W,2)] -> a single D2H copy per evaluation
        char* blk = nullptr;
        TRY(c->mem.alloc_dev(blk, B * sizeof(OutScal) + B * img * 2 * sizeof(double)));
        c->d_outs = reinterpret_cast<OutScal*>(blk);
        c->d_grad = reinterpret_cast<double*>(blk + B * sizeof(OutScal));
        char* hblk = nullptr;
        TRY(c->mem.alloc_pinned(hblk, B * sizeof(OutScal) + B * img * 2 * sizeof(double)));
        c->h_outs = reinterpret_cast<OutScal*>(hblk);
        c->h_grad = reinterpret_cast<double*>(hblk + B * sizeof(OutScal));
    }
    TRY(ensure_coarse(c, 64 * 64 * 2));   // coarse theta up to 64x64 (the pyramid tops out at 16x16); grown on demand
    TRY(c->mem.alloc_dev(c->d_rowtap, (size_t)H));
    TRY(c->mem.alloc_dev(c->d_coltap, (size_t)W));
    TRY(c->mem.alloc_dev(c->d_tilerng, (size_t)ntiles));
    TRY(c->mem.alloc_pinned(c->h_theta, B * img * 2));
    TRY(c->mem.alloc_pinned(c->h_wc, B));
    TRY(c->mem.alloc_pinned(c->h_g11, (size_t)(c->max_items + NXCD) * R * 2));
    TRY(c->mem.alloc_pinned(c->h_g2, B * R * nig));
    TRY(c->mem.alloc_pinned(c->h_img, B * R * IMGSCAL_N));
    TRY(c->mem.alloc_pinned(c->h_tvparts, B * ntiles * 3));
    c->have_events = true;
    for (int k = 0; k < eincm_ctx::GRAD_PIECES; ++k) TRY(hipEventCreateWithFlags(&c->ev_piece[k], hipEventDisableTiming));
    c->ring_size = (flags & EINCM_CF_TIMING_DOMINANT) && !(flags & EINCM_CF_TIMING) ? eincm_ctx::EV_RING : 1;
    if (flags & (EINCM_CF_TIMING | EINCM_CF_TIMING_DOMINANT))
        for (int k = 0; k < c->ring_size; ++k)
            for (int i = 0; i <= EINCM_N_STAGES; ++i) {
                const bool needed = (flags & EINCM_CF_TIMING) || i == EINCM_STAGE_SPLAT || i == EINCM_STAGE_GATHER || i == EINCM_N_STAGES;
                if (needed) { TRY(hipEventCreate(&c->ev[k][i][0])); TRY(hipEventCreate(&c->ev[k][i][1])); }
            }
    if (c->fp64) {             // the float64 mode's own buffers (eincm_kernels_f64.hip.h): nothing is allocated per evaluation
        const int P = (int)((img + F64_PIX - 1) / F64_PIX);
        c->f64.P = P;
        TRY(c->mem.alloc_dev(c->f64.acc, B * R * img, true));
        TRY(c->mem.alloc_dev(c->f64.iwe, B * R * img));
        TRY(c->mem.alloc_dev(c->f64.zero_iwe, B * img));
        TRY(c->mem.alloc_dev(c->f64.edges, B * R * img));
        TRY(c->mem.alloc_dev(c->f64.G, B * R * img));
        TRY(c->mem.alloc_dev(c->f64.sgn, B * R * img));
        TRY(c->mem.alloc_dev(c->f64.gacc, B * img * 4, true));
        TRY(c->mem.alloc_dev(c->f64.gTh, B * img * 2));
        TRY(c->mem.alloc_dev(c->f64.T, B * img * 2));
        TRY(c->mem.alloc_dev(c->f64.grad, B * img * 2));
        TRY(c->mem.alloc_dev(c->f64.partA, B * R * P * F64_PA));
        TRY(c->mem.alloc_dev(c->f64.partB, B * R * P * F64_PB));
        TRY(c->mem.alloc_dev(c->f64.partC, B * R * P * F64_PC));
        TRY(c->mem.alloc_dev(c->f64.scal, B * R));
        TRY(c->mem.alloc_pinned(c->f64.h_scal, B * R));
        TRY(c->mem.alloc_dev(c->f64.gmax, B));
        TRY(c->mem.alloc_dev(c->f64.ishift, B));
        TRY(c->mem.alloc_dev(c->f64.bad, B));
    }
    // both event kernels need > 32 KiB... (<= 64 KiB default limit is fine on gfx950, no attribute needed)
#undef TRY
    return c;
}

void eincm_destroy(eincm_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_all(ctx);
    delete ctx;
}

// Segment list L of the staged bins (h_tilecount) at `seg` events per segment (cut_segments).  on_host: the host cuts the segments
// (with the first one of every window) and uploads them; otherwise k_items has already written the L.n the caller counted.  Then
// the longest-first order goes up and k_seg_minmax takes every segment's time range from ev_t, the copy of the events the list's
// walkers read.
static int build_list(eincm_ctx* c, SegList& L, int seg, bool on_host, int ntiles, const double* ev_t, int64_t N)
{
    std::vector<int32_t> lens;
    cut_segments(c->h_tilecount.data(), c->h_tilecount.size(), ntiles, seg, N, on_host, L, lens);
    if ((int64_t)lens.size() > c->max_items) return fail(c, EINCM_ERR_ARG, "internal: %zu segments exceed capacity", lens.size());
    if (on_host) L.n = (int)lens.size();
    else if ((int)lens.size() != L.n) return fail(c, EINCM_ERR_ARG, "internal: segment lists disagree (%zu, %d)", lens.size(), L.n);
    if (on_host) {
        if (L.d_win_item0)
            HIPCHK(c, hipMemcpyAsync(L.d_win_item0, L.h_win_item0.data(), L.h_win_item0.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        if (L.n > 0) HIPCHK(c, hipMemcpyAsync(L.d_items, L.h_items.data(), (size_t)L.n * sizeof(Item), hipMemcpyHostToDevice, c->stream));
    }
    if (L.n == 0) return EINCM_OK;
    HIPCHK(c, hipMemcpyAsync(L.d_order, L.h_order.data(), (size_t)L.n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_seg_minmax, dim3(std::min(L.n, 4096)), dim3(NT), 0, c->stream, L.n, L.d_items, ev_t);
    HIPCHK(c, hipGetLastError());
    return EINCM_OK;
}

// ---- staging (eincm_set_windows*): check_staging -> plan_staging -> the phases, each reading the plan ----

// Everything a staging refuses from its arguments alone, before it touches the context or enqueues work.
static int check_staging(eincm_ctx* c, const StageArgs& a) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fl.launched())
        return fail(c, EINCM_ERR_STATE, "an asynchronous evaluation is in flight: call eincm_loss_grad_wait first");
    if (a.B < 1 || a.B > c->maxB) return fail(c, EINCM_ERR_ARG, "n_windows %d outside 1..%d", a.B, c->maxB);
    if (a.R < 1 || a.R > c->maxR) return fail(c, EINCM_ERR_ARG, "n_refs %d outside 1..%d", a.R, c->maxR);
    if (!a.n_events || !a.xs || !a.ys || !a.ts || !a.edges || !a.edge_ts) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    for (int b = 0; b < a.B; ++b)
        if (!a.edges[b] || (a.n_events[b] > 0 && (!a.xs[b] || !a.ys[b] || !a.ts[b]))) return fail(c, EINCM_ERR_ARG, "null pointer argument (window %d)", b);
    int64_t N = 0;
    for (int b = 0; b < a.B; ++b) {
        if (a.n_events[b] < 0) return fail(c, EINCM_ERR_ARG, "n_events[%d] negative", b);
        N += a.n_events[b];
    }
    if (N > c->maxN) return fail(c, EINCM_ERR_ARG, "total events %lld exceed capacity %lld", (long long)N, (long long)c->maxN);
    for (int b = 0; b < a.B; ++b)
        for (int r = 0; r < a.R; ++r)
            if (!std::isfinite(a.edge_ts[b * a.R + r])) return fail(c, EINCM_ERR_ARG, "edge_ts[%d,%d] is not finite", b, r);
    if (c->fp64) {
        if (a.flags & EINCM_SW_DEFER_CONSTANTS) return fail(c, EINCM_ERR_UNSUPPORTED, "event-sharded staging is not supported in fp64 mode");
        for (int b = 0; b < a.B; ++b)
            if (f64_ishift(a.n_events[b]) < 40)
                return fail(c, EINCM_ERR_UNSUPPORTED, "window %d: %lld events exceed the fp64 mode's IWE scale (2^-40 per tap)", b, (long long)a.n_events[b]);
    }
    // per-event weights: the values first, on the host arrays; then what has no weighted form
    if (const WeightRefusal r = check_weights(a.B, a.n_events, a.weights))
        return fail(c, EINCM_ERR_ARG, "weight %lld of window %d is %g: weights are finite and within [0, 1]", (long long)r.index, r.win, (double)r.value);
    if (batch_weighted(a.B, a.n_events, a.weights)) {
        if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "per-event weights are not supported in fp64 mode (EINCM_CF_FP64)");
        if (c->splat_size != 3)
            return fail(c, EINCM_ERR_UNSUPPORTED, "per-event weights have the 3x3 splat window only, the context has %d (eincm_set_splat_window)", c->splat_size);
        if (a.flags & EINCM_SW_DEFER_CONSTANTS) return fail(c, EINCM_ERR_UNSUPPORTED, "per-event weights are not supported in an event-sharded staging");
    }
    // a keep-order batch is a weighted one whatever it was handed: the same three, in its own words
    if (a.flags & EINCM_SW_KEEP_ORDER) {
        if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "EINCM_SW_KEEP_ORDER is not supported in fp64 mode (EINCM_CF_FP64)");
        if (c->splat_size != 3)
            return fail(c, EINCM_ERR_UNSUPPORTED, "EINCM_SW_KEEP_ORDER has the 3x3 splat window only, the context has %d (eincm_set_splat_window)", c->splat_size);
        if (a.flags & EINCM_SW_DEFER_CONSTANTS) return fail(c, EINCM_ERR_UNSUPPORTED, "EINCM_SW_KEEP_ORDER is not supported in an event-sharded staging");
    }
    return EINCM_OK;
}

// The two weight buffers of a weighted batch, allocated by the first weighted staging of the context and kept from then on
static int ensure_weights(eincm_ctx* c) {
    if (!c->d_w) HIPCHK(c, c->mem.alloc_dev(c->d_w, (size_t)c->maxN));
    if (!c->d_w_g) HIPCHK(c, c->mem.alloc_dev(c->d_w_g, (size_t)c->maxN));
    return EINCM_OK;
}

// The two indices and the stream-order weights of a keep-order batch, allocated by the first such staging of the context and kept
static int ensure_order(eincm_ctx* c) {
    if (!c->ord.splat) HIPCHK(c, c->mem.alloc_dev(c->ord.splat, (size_t)c->maxN));
    if (!c->ord.gather) HIPCHK(c, c->mem.alloc_dev(c->ord.gather, (size_t)c->maxN));
    if (!c->ord.stream) HIPCHK(c, c->mem.alloc_dev(c->ord.stream, (size_t)c->maxN));
    return EINCM_OK;
}

// The refusal of event i of window b: outside the sensor (bad_xy), or with a non-finite timestamp.  refuse_event_at: of the event at
// index e of the whole batch (what k_bin_hist reports).
static int refuse_event(eincm_ctx* c, const StageArgs& a, int b, int64_t i, bool bad_xy) {
    if (!bad_xy) return fail(c, EINCM_ERR_ARG, "event %lld of window %d has a non-finite timestamp", (long long)i, b);
    return fail(c, EINCM_ERR_ARG, "event %lld of window %d at (x=%d, y=%d) outside the %dx%d sensor", (long long)i, b, (int)a.xs[b][i],
                (int)a.ys[b][i], c->H, c->W);
}
static int refuse_event_at(eincm_ctx* c, const StageArgs& a, int64_t e, bool bad_xy) {
    int b = 0;
    while (b < a.B - 1 && e >= a.n_events[b]) { e -= a.n_events[b]; ++b; }
    return refuse_event(c, a, b, e, bad_xy);
}

// The events as handed over, window after window: what the device path bins, and what eincm_get_warped_events walks on either path.
static int upload_raw_events(eincm_ctx* c, const StageArgs& a) {
    int64_t off = 0;
    for (int b = 0; b < a.B; ++b) {
        const size_t nb = (size_t)a.n_events[b];
        if (nb > 0) {
            HIPCHK(c, hipMemcpyAsync(c->d_raw_x + off, a.xs[b], nb * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->d_raw_y + off, a.ys[b], nb * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->d_raw_t + off, a.ts[b], nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
        off += (int64_t)nb;
    }
    return EINCM_OK;
}

// The weights as handed over, window after window like the events, ones for a window without (weights NULL: for every window), into
// dst.  A weighted batch on the device path sends them to d_w_g, which k_bin_scatter reads and k_segsort overwrites afterwards with the
// gather's order; a keep-order batch, and eincm_set_weights, to ord.stream, where they stay.
static int upload_raw_weights(eincm_ctx* c, int B, const int64_t* n_events, const float* const* weights, float* dst) {
    for (int b = 0; b < B; ++b) {
        const size_t nb = (size_t)n_events[b];
        float* const d = dst + stream_offset(n_events, b);
        if (nb > 0 && weights && weights[b]) HIPCHK(c, hipMemcpyAsync(d, weights[b], nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
        else if (nb > 0) HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d), 0x3f800000 /* 1.0f */, nb, c->stream));
    }
    return EINCM_OK;
}

// The staged batch's payload beside one event layout (StagePlan.payload): its device arrays, null where the payload has none.  raw: where
// k_bin_scatter reads the weights as handed over - ord.stream, where a keep-order batch keeps them, or d_w_g, which k_segsort overwrites.
struct Payload { float* w = nullptr; uint32_t* idx = nullptr; float* raw = nullptr; };
enum Layout { SPLAT_LAYOUT, GATHER_LAYOUT };
static Payload payload(const eincm_ctx* c, Layout l) {
    Payload p;
    if (c->stage.payload != PAYLOAD_NONE) { p.w = l == SPLAT_LAYOUT ? c->d_w : c->d_w_g; p.raw = c->d_w_g; }
    if (c->stage.payload == PAYLOAD_WEIGHTS_ORDER) { p.idx = l == SPLAT_LAYOUT ? c->ord.splat : c->ord.gather; p.raw = c->ord.stream; }
    return p;
}

// Staging's three kernels that carry the payload, every StagePayload state (in the enum's order) bound to its instantiation:
// StagePlan.payload is the kernel to launch.  No other place names an instantiation of the three.
const std::array BIN_SCATTER_KERNELS{&k_bin_scatter<0>, &k_bin_scatter<1>, &k_bin_scatter<1, 1>};
const std::array SPREAD_KERNELS{&k_spread<0>, &k_spread<1>, &k_spread<1, 1>};
const std::array SEGSORT_KERNELS{&k_segsort<0>, &k_segsort<1>, &k_segsort<1, 1>};

// The gather's copy of the binned events: every segment of its list sorted by source pixel and dealt to the threads that walk it
// (k_segsort, from the binned time order, before the splat's copy is re-dealt in place); EINCM_NO_SEGSORT: a plain copy.
static int copy_for_gather(eincm_ctx* c) {
    if (c->gather.n == 0) return EINCM_OK;
    const Payload src = payload(c, SPLAT_LAYOUT), dst = payload(c, GATHER_LAYOUT);      // the payload takes the same way as the events
    if (c->stage.sort_segments) {
        hipLaunchKernelGGL(SEGSORT_KERNELS[c->stage.payload], dim3(std::min(c->gather.n, 8192)), dim3(SORT_NT), 0, c->stream, c->gather.n,
                           c->gather.d_items, c->d_xy, c->d_t, c->d_xy_g, c->d_t_g, (const float*)src.w, dst.w, (const uint32_t*)src.idx, dst.idx);
        return EINCM_OK;
    }
    if (src.idx) HIPCHK(c, hipMemcpyAsync(dst.idx, src.idx, (size_t)c->stage.N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    if (src.w) HIPCHK(c, hipMemcpyAsync(dst.w, src.w, (size_t)c->stage.N * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_xy_g, c->d_xy, (size_t)c->stage.N * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_t_g, c->d_t, (size_t)c->stage.N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return EINCM_OK;
}

// Device binning: counting sort by (window, source tile) on the GPU (eincm_binning.hip.h), the edges to fp32 with their moments, the
// gather's and the splat's lists cut by k_items.  One synchronisation, for the tile populations and the kernels' verdict on the events.
static int bin_on_device(eincm_ctx* c, const StageArgs& a, StageScratch& sc) {
    const StagePlan& P = c->stage;
    const Geom& g = P.g;
    const size_t img = (size_t)g.H * g.W;
    int rc = EINCM_OK;
    sc.win_blk.resize((size_t)a.B + 1);
    int64_t base = 0;
    for (int b = 0; b < a.B; ++b) {
        sc.win_blk[b] = (int32_t)sc.blks.size();
        for (int64_t s0 = 0; s0 < a.n_events[b]; s0 += BIN_CHUNK) {
            BinBlock bb; bb.win = b; bb.start = (int32_t)(base + s0); bb.count = (int32_t)std::min<int64_t>(BIN_CHUNK, a.n_events[b] - s0);
            bb.first_blk = sc.win_blk[b];
            sc.blks.push_back(bb);
        }
        base += a.n_events[b];
    }
    sc.win_blk[a.B] = (int32_t)sc.blks.size();
    const int nblk = (int)sc.blks.size();
    if (nblk > c->max_binblocks) return fail(c, EINCM_ERR_ARG, "internal: %d staging blocks exceed capacity", nblk);
    static const int32_t misc_init[4] = {0, 0, 0x7fffffff, 0x7fffffff};               // totals[2], err[2]
    HIPCHK(c, hipMemcpyAsync(c->d_bin_misc, misc_init, sizeof misc_init, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_win_blk, sc.win_blk.data(), sc.win_blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < a.B; ++b)
        HIPCHK(c, hipMemcpyAsync(c->d_edges_raw + (size_t)b * a.R * img, a.edges[b], (size_t)a.R * img * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_edges, dim3(EDGE_PARTS, a.R, a.B), dim3(NT), 0, c->stream, g, c->d_edges_raw, c->d_edges, c->d_edge_moments);
    if (nblk > 0) {
        HIPCHK(c, hipMemcpyAsync(c->d_binblocks, sc.blks.data(), sc.blks.size() * sizeof(BinBlock), hipMemcpyHostToDevice, c->stream));
        if ((rc = upload_raw_events(c, a))) return rc;
        hipLaunchKernelGGL(k_bin_hist, dim3(nblk), dim3(BIN_NT), g.ntiles * sizeof(uint32_t), c->stream, g, c->d_binblocks, c->d_raw_x, c->d_raw_y,
                           c->d_raw_t, c->d_blockhist, c->d_bin_misc + 2);
    } else {
        HIPCHK(c, hipMemsetAsync(c->d_blockhist, 0, sizeof(uint32_t), c->stream));
    }
    const int M = a.B * g.ntiles;
    hipLaunchKernelGGL(k_bin_scan, dim3((M + 255) / 256), dim3(256), 0, c->stream, g, c->d_win_blk, c->d_blockhist, c->d_tilecount);
    hipLaunchKernelGGL(k_bin_tilescan, dim3(1), dim3(1024), 0, c->stream, M, P.seg, c->d_tilecount, c->d_tilebase, c->gather.d_itembase, c->d_bin_misc);
    HIPCHK(c, hipGetLastError());
    sc.mom.resize((size_t)a.B * a.R * EDGE_PARTS * EDGE_MOM);
    HIPCHK(c, hipMemcpyAsync(sc.misc, c->d_bin_misc, sizeof sc.misc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sc.mom.data(), c->d_edge_moments, sc.mom.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    c->h_tilecount.resize((size_t)M);
    HIPCHK(c, hipMemcpyAsync(c->h_tilecount.data(), c->d_tilecount, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sc.misc[2] != 0x7fffffff) return refuse_event_at(c, a, sc.misc[2], true);
    if (sc.misc[3] != 0x7fffffff) return refuse_event_at(c, a, sc.misc[3], false);
    c->gather.n = sc.misc[1];
    if (c->gather.n > c->max_items) return fail(c, EINCM_ERR_ARG, "internal: %d segments exceed capacity", c->gather.n);
    for (int b = 0; b < a.B; ++b)
        for (int r = 0; r < a.R; ++r) {          // the blocks' partials, added in index order
            double sE = 0.0, sEE = 0.0, eabs = 0.0;
            for (int k = 0; k < EDGE_PARTS; ++k) {
                const double* m = &sc.mom[(((size_t)b * a.R + r) * EDGE_PARTS + k) * EDGE_MOM];
                sE += m[0]; sEE += m[1]; eabs = std::max(eabs, m[2]);
            }
            c->h_wc[b].sE[r] = sE; c->h_wc[b].sEE[r] = sEE; c->h_wc[b].eabs[r] = eabs;
        }
    const Payload pl = payload(c, SPLAT_LAYOUT);
    if (nblk > 0) {
        if (pl.raw && (rc = upload_raw_weights(c, a.B, a.n_events, a.weights, pl.raw))) return rc;
        hipLaunchKernelGGL(BIN_SCATTER_KERNELS[P.payload], dim3(nblk), dim3(BIN_NT), g.ntiles * sizeof(uint32_t), c->stream, g, c->d_binblocks,
                           c->d_raw_x, c->d_raw_y, c->d_raw_t, c->d_blockhist, c->d_tilebase, c->d_xy, c->d_t, (const float*)pl.raw, pl.w, pl.idx);
        hipLaunchKernelGGL(k_items, dim3((M + 255) / 256), dim3(256), 0, c->stream, g, P.seg, c->d_tilecount, c->d_tilebase, c->gather.d_itembase,
                           c->gather.d_items);
        if ((rc = copy_for_gather(c))) return rc;
    }
    if ((rc = build_list(c, c->gather, P.seg, false, g.ntiles, c->d_t_g, P.N))) return rc;
    c->splat.n = 0;
    if (nblk > 0) {
        if (P.spread)
            hipLaunchKernelGGL(SPREAD_KERNELS[P.payload], dim3(M, SPREAD_Y), dim3(256), 0, c->stream, g, c->d_tilecount, c->d_tilebase, c->d_xy, c->d_t,
                               pl.w, pl.idx);
        // per window: first segment and max |t - tau| (needs the segment time ranges and the FIRST segmentation's itembase)
        HIPCHK(c, hipMemcpyAsync(c->d_edge_ts, a.edge_ts, (size_t)a.B * a.R * sizeof(double), hipMemcpyHostToDevice, c->stream));
        sc.edge_ts_uploaded = true;
        hipLaunchKernelGGL(k_win_consts, dim3(a.B), dim3(NT), 0, c->stream, g, c->gather.n, c->gather.d_items, c->gather.d_itembase,
                           c->d_edge_ts, c->gather.d_win_item0, c->d_dtmax);
        HIPCHK(c, hipMemcpyAsync(sc.dtmax.data(), c->d_dtmax, (size_t)a.B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        // second segmentation of the same binned events for k_splat; its total is not read back (a synchronisation per staging):
        // the host repeats the arithmetic on the tile populations it holds
        hipLaunchKernelGGL(k_bin_tilescan, dim3(1), dim3(1024), 0, c->stream, M, P.seg_s, c->d_tilecount, c->d_tilebase, c->splat.d_itembase, c->d_bin_misc);
        for (const int32_t cnt : c->h_tilecount) c->splat.n += (cnt + P.seg_s - 1) / P.seg_s;
        if (c->splat.n > c->max_items) return fail(c, EINCM_ERR_ARG, "internal: %d splat segments exceed capacity", c->splat.n);
        hipLaunchKernelGGL(k_items, dim3((M + 255) / 256), dim3(256), 0, c->stream, g, P.seg_s, c->d_tilecount, c->d_tilebase, c->splat.d_itembase,
                           c->splat.d_items);
    } else {
        HIPCHK(c, hipMemsetAsync(c->gather.d_win_item0, 0, (size_t)(a.B + 1) * sizeof(int32_t), c->stream));
    }
    return build_list(c, c->splat, P.seg_s, false, g.ntiles, c->d_t, P.N);
}

// Host binning (sensors with more tiles than the LDS histogram holds, or EINCM_HOST_BINNING=1): a stable counting sort, the edges to
// fp32 with their moments, the gather's and the splat's lists cut on the host like the two others.
static int bin_on_host(eincm_ctx* c, const StageArgs& a, StageScratch& sc) {
    const StagePlan& P = c->stage;
    const Geom& g = P.g;
    const size_t img = (size_t)g.H * g.W;
    int rc = EINCM_OK;
    const Payload pl = payload(c, SPLAT_LAYOUT);
    if (const EventRefusal r = bin_events(g, a.n_events, a.xs, a.ys, a.ts, a.edge_ts, P.N, c->h_tilecount, sc.sxy, sc.st, sc.cntmax, sc.dtmax,
                                          a.weights, pl.w ? &sc.sw : nullptr, pl.idx ? &sc.sidx : nullptr))
        return refuse_event(c, a, r.win, r.index, r.bad_xy);
    sc.ef.resize((size_t)a.B * a.R * img);
    for (int b = 0; b < a.B; ++b) {
        WinConst& wc = c->h_wc[b];
        for (int r = 0; r < a.R; ++r)
            edge_moments(a.edges[b] + (size_t)r * img, img, sc.ef.data() + ((size_t)b * a.R + r) * img, wc.sE[r], wc.sEE[r], wc.eabs[r]);
    }
    if (P.N > 0) {
        HIPCHK(c, hipMemcpyAsync(c->d_xy, sc.sxy.data(), (size_t)P.N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_t, sc.st.data(), (size_t)P.N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (pl.w) HIPCHK(c, hipMemcpyAsync(pl.w, sc.sw.data(), (size_t)P.N * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (pl.idx) {            // the index beside the splat's copy, the weights in stream order, and the host's copy of the pixels (weight_state counts on them)
            HIPCHK(c, hipMemcpyAsync(pl.idx, sc.sidx.data(), (size_t)P.N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            if ((rc = upload_raw_weights(c, a.B, a.n_events, a.weights, pl.raw))) return rc;
            c->ord.h_xy.resize((size_t)P.N);
            size_t e = 0;
            for (int b = 0; b < a.B; ++b)
                for (int64_t i = 0; i < a.n_events[b]; ++i) c->ord.h_xy[e++] = (uint32_t)(uint16_t)a.xs[b][i] | ((uint32_t)(uint16_t)a.ys[b][i] << 16);
        }
        if ((rc = upload_raw_events(c, a))) return rc;
    }
    // (the gather's copy is a permutation inside the gather list's segments: their time ranges come from either copy)
    if ((rc = build_list(c, c->gather, P.seg, true, g.ntiles, c->d_t, P.N))) return rc;
    if ((rc = copy_for_gather(c))) return rc;
    if ((rc = build_list(c, c->splat, P.seg_s, true, g.ntiles, c->d_t, P.N))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_edges, sc.ef.data(), sc.ef.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return EINCM_OK;
}

// What depends on the weights of the batch in c->stage, once its lists exist and both layouts hold their weights: the event mask, and
// per window the most events of weight > 0 on one source pixel into h_cnt (B) and, with its floor of 1, into WinConst.cntmax.  The
// device path takes both from k_tile_counts, per tile from its LDS histogram; a host-binned batch takes the mask from k_mask and the
// count from the host: h_cnt as bin_events filled it, or, with h_w (N floats: a re-weighting), counted here on ord.stream.  One
// synchronisation, which whatever the caller enqueued before rides on; the call ends on it.
static int weight_state(eincm_ctx* c, unsigned* h_cnt, float* h_w = nullptr) {
    const StagePlan& P = c->stage;
    const Geom& g = P.g;
    const float* const w = payload(c, SPLAT_LAYOUT).w;
    HIPCHK(c, hipMemsetAsync(c->d_mask, 0, (size_t)g.B * g.H * g.W, c->stream));
    if (c->gather.n > 0 && !P.host_binning) {
        HIPCHK(c, hipMemsetAsync(c->d_cntmax, 0, (size_t)g.B * sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(k_tile_counts, dim3(g.ntiles, g.B), dim3(NT), 0, c->stream, g, c->d_tilebase, c->d_tilecount, c->d_xy, c->d_mask, c->d_cntmax, w);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_cnt, c->d_cntmax, (size_t)g.B * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    } else if (c->gather.n > 0) {
        hipLaunchKernelGGL(k_mask, dim3(std::min(c->gather.n, 2048)), dim3(NT), 0, c->stream, g, c->gather.d_items, c->gather.n, c->d_xy, c->d_mask, w);
        HIPCHK(c, hipGetLastError());
        if (h_w) HIPCHK(c, hipMemcpyAsync(h_w, c->ord.stream, (size_t)P.N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < g.B; ++b) {
        const int64_t off = stream_offset(c->win_events.data(), b), nb = c->win_events[b];
        if (h_w && nb > 0) h_cnt[b] = most_on_one_pixel(g.H, g.W, nb, c->ord.h_xy.data() + off, h_w + off);
        c->h_wc[b].cntmax = (double)std::max(h_cnt[b], 1u);     // a bound behind the scale of the i64 gradient accumulators (grad_shift)
    }
    return EINCM_OK;
}

// What a new batch, and new weights for the staged one, drop: the objective kinds' zero-warp values, the Theta image, a fused evaluation's q
// and segment ranges, the BFGS state, the chosen capacities, the last evaluation and error.  A cache tied to the staged batch goes here.
static void drop_batch_state(eincm_ctx* c) {
    c->objc_valid = false; c->Theta_valid = false;
    c->motion.last_q.clear(); c->motion.seg0.clear();
    c->bfgs.begun = false; c->policy_evaluated = false;
    c->have_eval = false; c->err.clear();
}

// What both paths share: the 2-DoF gather's list (on the splat's copy of the events) and the splat's short one, both cut on the host
// from the tile populations; what depends on the weights (weight_state, with this phase's one synchronisation); then the batch is the context's.
static int finish_lists(eincm_ctx* c, const StageArgs& a, StageScratch& sc) {
    const StagePlan& P = c->stage;
    const Geom& g = P.g;
    int rc = EINCM_OK;
    if (!sc.edge_ts_uploaded)
        HIPCHK(c, hipMemcpyAsync(c->d_edge_ts, a.edge_ts, (size_t)a.B * a.R * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = build_list(c, c->gather_2, P.seg_2, true, g.ntiles, c->d_t, P.N))) return rc;
    c->splat_sh.n = 0;
    if (P.splat_short && (rc = build_list(c, c->splat_sh, SEG_SHORT, true, g.ntiles, c->d_t, P.N))) return rc;
    c->win_events.assign(a.n_events, a.n_events + a.B);
    if ((rc = weight_state(c, sc.cntmax.data()))) return rc;
    c->g = g;
    c->itembase_valid = !P.host_binning && c->gather.n > 0 && c->splat.n > 0;      // both tile scans ran on the device
    return EINCM_OK;
}

// float64 mode: the edges as handed over, and the scale of each window's u64 IWE accumulator
static int stage_fp64(eincm_ctx* c, const StageArgs& a, StageScratch& sc) {
    const size_t img = (size_t)c->H * c->W;
    for (int b = 0; b < a.B; ++b) sc.ishift.push_back(f64_ishift(a.n_events[b]));
    HIPCHK(c, hipMemcpyAsync(c->f64.ishift, sc.ishift.data(), sc.ishift.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    for (int b = 0; b < a.B; ++b)
        HIPCHK(c, hipMemcpyAsync(c->f64.edges + (size_t)b * a.R * img, a.edges[b], (size_t)a.R * img * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return EINCM_OK;
}

// One staging.  The scratch is constructed before the guard, so whatever path leaves this function (an error return included) drains
// the stream first and frees the host memory its copies read from / write into afterwards; the caller's arrays live longer still.
static int stage_windows(eincm_ctx* c, const StageArgs& a) {
    int rc = check_staging(c, a);
    if (rc) return rc;
    c->staged = false;               // (every reader of what drop_batch_state drops asks for a staged batch first)
    c->lp.staged = false;            // the staged prior belonged to the batch that goes (a re-weighting keeps it: it is not a staging)
    c->stage = plan_staging(*c, a.B, a.R, a.n_events, a.flags, live_knobs().stage, a.weights);    // (an unweighted staging drops the weighted state with the plan)
    const StagePlan& P = c->stage;
    HIPCHK(c, hipSetDevice(c->device));
    if (P.weighted && (rc = ensure_weights(c))) return rc;
    if (P.keep_order && (rc = ensure_order(c))) return rc;
    StageScratch sc;
    struct DrainOnExit { hipStream_t s; ~DrainOnExit() { (void)hipStreamSynchronize(s); } } drain_on_exit{c->stream};
    if (c->acc_dirty && (rc = clear_accumulators(c))) return rc;
    for (int b = 0; b < a.B; ++b) {
        memset(&c->h_wc[b], 0, sizeof(WinConst));
        multi_ref_weights(a.R, c->h_wc[b].mrw);
    }
    sc.cntmax.assign((size_t)a.B, 0u);
    sc.dtmax.assign((size_t)a.B, 0.0);
    if ((rc = P.host_binning ? bin_on_host(c, a, sc) : bin_on_device(c, a, sc))) return rc;
    if ((rc = finish_lists(c, a, sc))) return rc;
    if (c->fp64 && (rc = stage_fp64(c, a, sc))) return rc;
    for (int b = 0; b < a.B; ++b) {      // bounds behind the scale of the i64 gradient accumulators (grad_shift), beside weight_state's cntmax
        WinConst& wc = c->h_wc[b];
        wc.nev = (double)std::max<int64_t>(a.n_events[b], 1);
        wc.dtmax = sc.dtmax[b];
    }
    drop_batch_state(c);
    c->staged = true;
    c->sharded_staging = P.defer_constants;
    if (!P.defer_constants) return window_constants(c);
    // event-sharded mode: the caller sums the shards' IUEs first (eincm_forward_iwe(NULL theta), eincm_finish_constants)
    if ((rc = preset_constants(c))) return rc;
    c->constants_pending = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EINCM_OK;
}

// The concatenated forms: per-window pointers into the caller's arrays (arguments stage_windows would refuse go through as they are).
int eincm_set_windows_ex(eincm_ctx* c, int n_windows, int n_refs, const int64_t* n_events, const int16_t* xs, const int16_t* ys,
                         const double* ts, const double* edges, const double* edge_ts, uint32_t flags) {
    const bool sane = c && n_events && xs && ys && ts && edges && n_windows >= 1 && n_windows <= c->maxB;
    const size_t nb = sane ? (size_t)n_windows : 0, img = c ? (size_t)c->H * c->W : 0;
    std::vector<const int16_t*> xw(nb), yw(nb);
    std::vector<const double*> tw(nb), ew(nb);
    int64_t base = 0;
    for (size_t b = 0; b < nb; ++b) {
        xw[b] = xs + base; yw[b] = ys + base; tw[b] = ts + base; ew[b] = edges + b * (size_t)std::max(n_refs, 0) * img;
        base += std::max<int64_t>(n_events[b], 0);
    }
    return stage_windows(c, StageArgs{n_windows, n_refs, n_events, sane ? xw.data() : nullptr, sane ? yw.data() : nullptr,
                                      sane ? tw.data() : nullptr, sane ? ew.data() : nullptr, edge_ts, flags});
}

int eincm_set_windows(eincm_ctx* c, int n_windows, int n_refs, const int64_t* n_events, const int16_t* xs, const int16_t* ys,
                      const double* ts, const double* edges, const double* edge_ts) {
    return eincm_set_windows_ex(c, n_windows, n_refs, n_events, xs, ys, ts, edges, edge_ts, 0u);
}

int eincm_set_windows_ptrs(eincm_ctx* c, int n_windows, int n_refs, const int64_t* n_events, const int16_t* const* xs,
                           const int16_t* const* ys, const double* const* ts, const double* const* edges, const double* edge_ts,
                           uint32_t flags) {
    return stage_windows(c, StageArgs{n_windows, n_refs, n_events, xs, ys, ts, edges, edge_ts, flags});
}

int eincm_set_windows_weighted(eincm_ctx* c, int n_windows, int n_refs, const int64_t* n_events, const int16_t* const* xs,
                               const int16_t* const* ys, const double* const* ts, const double* const* edges, const double* edge_ts,
                               const float* const* weights, uint32_t flags) {
    return stage_windows(c, StageArgs{n_windows, n_refs, n_events, xs, ys, ts, edges, edge_ts, flags, weights});
}

// ---- a keep-order batch takes new weights in place ----

// Why a call that needs the indices of a keep-order staging cannot run, or EINCM_OK
static int keep_order_ready(eincm_ctx* c, const char* who) {
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "%s called before eincm_set_windows", who);
    if (!c->stage.keep_order)
        return fail(c, EINCM_ERR_STATE, "%s: the batch was staged without EINCM_SW_KEEP_ORDER (keep_order=True), so staging kept no index back to "
                    "the order of its events", who);
    return EINCM_OK;
}

// The weights in ord.stream (enqueued on the stream by the caller, through its frame) become the staged batch's: the gather through the
// two indices into both layouts, then what a staging derives from the weights (weight_state), what it drops (drop_batch_state) and the
// zero-warp constants.  The edges and their moments, the four lists, dtmax and the raw events do not depend on the weights and stay.
static int reweight_staged(eincm_ctx* c, OneShot& op) {
    const StagePlan& P = c->stage;
    const size_t N = (size_t)P.N;
    unsigned* h_cnt = op.host_buf<unsigned>((size_t)P.g.B);              // d_cntmax comes down here (zeros: a window without events)
    float* h_w = P.host_binning ? op.host_buf<float>(N) : nullptr;       // host binning: ord.stream comes down here
    if (N > 0)
        HIPCHK(c, op.launch(k_reweight, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, (int64_t)N, c->ord.stream, c->ord.splat, c->ord.gather,
                            c->d_w, c->d_w_g));
    op.pending = true;                              // weight_state enqueues on the stream itself: the frame drains that too, until ...
    if (const int rc = weight_state(c, h_cnt, h_w)) return rc;
    op.pending = false;                             // ... the call has ended on its synchronisation
    drop_batch_state(c);
    return window_constants(c);
}

int eincm_set_weights(eincm_ctx* c, const float* const* weights) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = keep_order_ready(c, "eincm_set_weights")) return rc;
    if (const int rc = not_in_flight(c, "eincm_set_weights")) return rc;
    const int B = c->g.B;
    const int64_t* ne = c->win_events.data();
    if (const WeightRefusal r = check_weights(B, ne, weights))
        return fail(c, EINCM_ERR_ARG, "weight %lld of window %d is %g: weights are finite and within [0, 1]", (long long)r.index, r.win, (double)r.value);
    OneShot op(c);                                  // no piece of the scratch: the frame is here for its drain
    HIPCHK(c, op.begin());
    op.pending = true;                              // staging's own upload enqueues below, not through the frame: the frame drains it all the same
    if (const int rc = upload_raw_weights(c, B, ne, weights, c->ord.stream)) return rc;       // (host memory: the caller's)
    return reweight_staged(c, op);
}

int eincm_get_stage_order(eincm_ctx* c, uint32_t* order_splat, uint32_t* order_gather) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = keep_order_ready(c, "eincm_get_stage_order")) return rc;
    const size_t bytes = (size_t)c->stage.N * sizeof(uint32_t);
    if (bytes == 0) return EINCM_OK;
    OneShot op(c);
    HIPCHK(c, op.begin());
    if (order_splat) HIPCHK(c, op.down(order_splat, c->ord.splat, bytes));       // (host memory: the caller's, both)
    if (order_gather) HIPCHK(c, op.down(order_gather, c->ord.gather, bytes));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

int eincm_get_staged_weights(eincm_ctx* c, float* weights) {
    if (!c) return EINCM_ERR_ARG;
    if (!weights) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (const int rc = keep_order_ready(c, "eincm_get_staged_weights")) return rc;
    if (c->stage.N == 0) return EINCM_OK;
    OneShot op(c);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.down(weights, c->ord.stream, (size_t)c->stage.N * sizeof(float)));      // (host memory: the caller's)
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// ---- event-sharded evaluation: forward half / [caller all-reduces the IWE stack] / finishing half ----
int eincm_forward_iwe(eincm_ctx* c, const double* theta, int h, int w, const eincm_params* p, int want_grad) {
    if (const int rc = eval_entry(c, "eincm_forward_iwe", theta, h, w, p, nullptr,
                                  THETA_MAY_BE_NULL | NO_VALUE | CONSTANTS_MAY_PEND | NOT_IN_FP64)) return rc;
    std::vector<double> zero;
    eincm_params pz;
    if (!theta) {                                    // NULL theta = the theta = 0 pass that yields the window constants
        zero.assign((size_t)c->g.B * 2, 0.0);
        theta = zero.data(); h = 1; w = 1; pz = zero_pass_params(); p = &pz; want_grad = 0;
    } else if (c->constants_pending) {
        return fail(c, EINCM_ERR_STATE, "window constants pending: run eincm_forward_iwe(NULL theta), sum the IWE stacks, eincm_finish_constants");
    }
    if (const int rc = eval_begin(c, theta, h, w, p, want_grad != 0)) return rc;
    FlightGuard guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));     // the IWE stack is complete: safe to reduce on any stream
    return guard.keep();
}

int eincm_finish_loss_grad(eincm_ctx* c, double* value, double* grad, eincm_aux* aux) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_finish_loss_grad (event-sharded mode) is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!value) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (c->constants_pending) return fail(c, EINCM_ERR_STATE, "window constants pending (eincm_finish_constants)");
    HIPCHK(c, hipSetDevice(c->device));
    return eval_end(c, value, grad, aux);
}

// theta and gradient resident in HBM (a caller whose optimiser lives on the GPU): nothing but the scalars crosses PCIe.
int eincm_loss_grad_device(eincm_ctx* c, const double* theta_dev, int h, int w, const eincm_params* p, double theta_abs_max,
                           double* value, double* grad_dev, eincm_aux* aux) {
    if (const int rc = eval_entry(c, "eincm_loss_grad_device", theta_dev, h, w, p, value, NOT_IN_FP64)) return rc;
    if (c->device_results) return fail(c, EINCM_ERR_STATE, "eincm_set_device_results is on: use the split finishing half");
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, theta_dev) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->device) {
        (void)hipGetLastError();
        return fail(c, EINCM_ERR_ARG, "theta_dev is not memory of device %d", c->device);
    }
    if (grad_dev && (hipPointerGetAttributes(&at, grad_dev) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->device)) {
        (void)hipGetLastError();
        return fail(c, EINCM_ERR_ARG, "grad_dev is not memory of device %d", c->device);
    }
    if (const int rc = eval_begin(c, nullptr, h, w, p, grad_dev != nullptr, nullptr, DevIo{theta_dev, grad_dev, theta_abs_max})) return rc;
    if (const int rc = eval_end_launch(c)) return rc;
    return eval_end_collect(c, value, nullptr, aux);
}

int eincm_set_device_results(eincm_ctx* c, int on) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_set_device_results is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "an evaluation is in flight");
    c->device_results = on != 0;
    return EINCM_OK;
}

int eincm_finish_launch(eincm_ctx* c) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_finish_launch is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!c->device_results) return fail(c, EINCM_ERR_STATE, "eincm_finish_launch needs eincm_set_device_results(ctx, 1)");
    if (c->constants_pending) return fail(c, EINCM_ERR_STATE, "window constants pending (eincm_finish_constants)");
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = eval_end_launch(c)) return rc;
    FlightGuard guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));     // the gradient is complete in HBM: safe to reduce on any stream
    return guard.keep();
}

int eincm_grad_device_ptr(eincm_ctx* c, void** dptr, int64_t* n_doubles) {
    if (!c || !dptr || !n_doubles) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_grad_device_ptr is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!c->fl.launched() || !c->fl.plan.want_grad) return fail(c, EINCM_ERR_STATE, "no launched gradient evaluation (eincm_finish_launch)");
    *dptr = c->d_grad; *n_doubles = (int64_t)c->g.B * (int64_t)c->fl.plan.nth;
    return EINCM_OK;
}

int eincm_finish_collect(eincm_ctx* c, double* value, double* grad, eincm_aux* aux) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_finish_collect is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!value) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->fl.launched()) return fail(c, EINCM_ERR_STATE, "eincm_finish_collect without eincm_finish_launch");
    HIPCHK(c, hipSetDevice(c->device));
    return eval_end_collect(c, value, grad, aux);
}

int eincm_finish_constants(eincm_ctx* c) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_finish_constants (event-sharded mode) is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!c->constants_pending) return fail(c, EINCM_ERR_STATE, "no deferred window constants");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> val((size_t)c->g.B);
    return store_constants(c, eval_end(c, val.data(), nullptr, nullptr));
}

int eincm_iwe_device_ptr(eincm_ctx* c, void** dptr, int64_t* n_words) {
    if (!c || !dptr || !n_words) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_iwe_device_ptr is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "no staged windows");
    *dptr = c->d_acc; *n_words = (int64_t)c->g.B * c->g.R * c->g.H * c->g.W;
    return EINCM_OK;
}


int eincm_mask_device_ptr(eincm_ctx* c, void** dptr, int64_t* n_bytes) {
    if (!c || !dptr || !n_bytes) return EINCM_ERR_ARG;
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "no staged windows");
    *dptr = c->d_mask; *n_bytes = (int64_t)c->g.B * c->g.H * c->g.W;
    return EINCM_OK;
}

int eincm_loss_grad_async(eincm_ctx* c, const double* theta, int h, int w, const eincm_params* p, int want_grad) {
    return eincm_loss_grad_masked_async(c, theta, h, w, p, nullptr, want_grad);
}

int eincm_loss_grad_masked_async(eincm_ctx* c, const double* theta, int h, int w, const eincm_params* p, const uint8_t* active, int want_grad) {
    if (const int rc = eval_entry(c, "eincm_loss_grad_async", theta, h, w, p, nullptr, NO_VALUE)) return rc;
    if (const int rc = eval_begin(c, theta, h, w, p, want_grad != 0, active)) return rc;
    return eval_end_launch(c);
}

int eincm_loss_grad_wait(eincm_ctx* c, double* value, double* grad, eincm_aux* aux) {
    if (!c) return EINCM_ERR_ARG;
    if (!c->fl.launched()) return fail(c, EINCM_ERR_STATE, "eincm_loss_grad_wait without eincm_loss_grad_async");
    HIPCHK(c, hipSetDevice(c->device));
    return eval_end_collect(c, value, grad, aux);      // drains the stream and clears the pending state on every path
}

int eincm_loss_grad(eincm_ctx* c, const double* theta, int h, int w, const eincm_params* p, double* value, double* grad, eincm_aux* aux) {
    if (const int rc = eval_entry(c, "eincm_loss_grad", theta, h, w, p, value)) return rc;
    return evaluate(c, theta, h, w, p, value, grad, aux);
}

int eincm_loss_grad_masked(eincm_ctx* c, const double* theta, int h, int w, const eincm_params* p, const uint8_t* active,
                           double* value, double* grad, eincm_aux* aux) {
    if (const int rc = eval_entry(c, "eincm_loss_grad_masked", theta, h, w, p, value)) return rc;
    return evaluate(c, theta, h, w, p, value, grad, aux, active);
}

int eincm_handover_loss_grad(eincm_ctx* c, const double* a, const double* prev_theta, const double* theta, int h, int w,
                             const eincm_params* p, double* value, double* dvalue_da) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = eval_ready(c, "eincm_handover_loss_grad", false)) return rc;
    if (!a || !prev_theta || !theta || !p || !value) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (h < 1 || w < 1) return fail(c, EINCM_ERR_ARG, "theta shape (%d,%d,2) invalid", h, w);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nth = (size_t)h * w * 2, B = c->g.B;
    std::vector<double> tho(B * nth), grad;
    handover_blend(a, prev_theta, theta, B, nth, tho.data());
    if (dvalue_da) grad.resize(B * nth);
    const int rc = evaluate(c, tho.data(), h, w, p, value, dvalue_da ? grad.data() : nullptr, nullptr);
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) return rc;
    if (dvalue_da) handover_chain(grad.data(), prev_theta, theta, B, nth, dvalue_da);
    return rc;
}

int eincm_objectives(eincm_ctx* c, const double* Theta, eincm_objectives_out* out) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = eval_ready(c, "eincm_objectives", false)) return rc;
    if (!Theta || !out) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const Geom& g = c->g;
    eincm_params p{};
    p.alpha = 1.0; p.beta = 1.0; p.gamma = 0.0; p.delta = 0.0; p.cur_pyr_lvl = 0; p.method = EINCM_METHOD_BILINEAR;
    p.flags = EINCM_PF_FULL_AUX;
    std::vector<double> val((size_t)g.B);
    const int rc = evaluate(c, Theta, g.H, g.W, &p, val.data(), nullptr, nullptr);
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) return rc;
    std::vector<double> tvp((size_t)g.B * g.ntiles * 3);
    HIPCHK(c, hipMemcpy(tvp.data(), c->d_tvparts, tvp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int b = 0; b < g.B; ++b) fill_objectives(g, c->h_outs[b], c->h_wc[b], tvp.data() + (size_t)b * g.ntiles * 3, out[b]);
    return rc;
}

static int copy_out(eincm_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c) return EINCM_ERR_ARG;
    if (!dst) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "no staged windows");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return EINCM_OK;
}

// The images of a float64 context in either width, and those of an fp32 context widened (the _f64 accessors work in both modes)
static int copy_image(eincm_ctx* c, const float* src32, const double* src64, size_t n, float* dst32, double* dst64) {
    if (!c) return EINCM_ERR_ARG;
    if (!dst32 && !dst64) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->staged) return fail(c, EINCM_ERR_STATE, "no staged windows");
    if (c->fp64 ? (dst64 != nullptr) : (dst32 != nullptr))
        return c->fp64 ? copy_out(c, dst64, src64, n * sizeof(double)) : copy_out(c, dst32, src32, n * sizeof(float));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fp64) {
        std::vector<double> tmp(n);
        HIPCHK(c, hipMemcpy(tmp.data(), src64, n * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) dst32[i] = (float)tmp[i];
    } else {
        std::vector<float> tmp(n);
        HIPCHK(c, hipMemcpy(tmp.data(), src32, n * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) dst64[i] = (double)tmp[i];
    }
    return EINCM_OK;
}
int eincm_get_iwes_f64(eincm_ctx* c, double* iwes) {
    if (c && !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    return c ? copy_image(c, c->d_iwe, c->f64.iwe, (size_t)c->g.B * c->g.R * c->g.H * c->g.W, nullptr, iwes) : EINCM_ERR_ARG;
}
int eincm_get_zero_iwe_f64(eincm_ctx* c, double* z) {
    return c ? copy_image(c, c->d_zero_iwe, c->f64.zero_iwe, (size_t)c->g.B * c->g.H * c->g.W, nullptr, z) : EINCM_ERR_ARG;
}
int eincm_get_image_grad_f64(eincm_ctx* c, double* G) {
    if (!c) return EINCM_ERR_ARG;
    if (!c->fp64) {
        std::vector<float> tmp((size_t)c->g.B * c->g.R * c->g.H * c->g.W);
        const int rc = eincm_get_image_grad(c, tmp.data());
        if (rc) return rc;
        if (!G) return fail(c, EINCM_ERR_ARG, "null pointer argument");
        for (size_t i = 0; i < tmp.size(); ++i) G[i] = (double)tmp[i];
        return EINCM_OK;
    }
    if (!c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    if (!c->G_valid) return fail(c, EINCM_ERR_STATE, "no dL/dIWE image: the last evaluation had no gradient");
    return copy_image(c, nullptr, c->f64.G, (size_t)c->g.B * c->g.R * c->g.H * c->g.W, nullptr, G);
}

int eincm_get_iwes(eincm_ctx* c, float* iwes) {
    if (c && !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    if (c && c->fp64) return copy_image(c, nullptr, c->f64.iwe, (size_t)c->g.B * c->g.R * c->g.H * c->g.W, iwes, nullptr);
    return copy_out(c, iwes, c ? c->d_iwe : nullptr, c ? (size_t)c->g.B * c->g.R * c->g.H * c->g.W * sizeof(float) : 0);
}
int eincm_get_zero_iwe(eincm_ctx* c, float* z) {
    if (c && c->fp64) return copy_image(c, nullptr, c->f64.zero_iwe, (size_t)c->g.B * c->g.H * c->g.W, z, nullptr);
    return copy_out(c, z, c ? c->d_zero_iwe : nullptr, c ? (size_t)c->g.B * c->g.H * c->g.W * sizeof(float) : 0);
}
int eincm_get_image_grad(eincm_ctx* c, float* G) {
    if (c && !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    if (c && !c->G_valid) return fail(c, EINCM_ERR_STATE, "no dL/dIWE image: the last evaluation had no gradient, or eincm_get_count_images reused the buffer");
    if (c && c->fp64) return copy_image(c, nullptr, c->f64.G, (size_t)c->g.B * c->g.R * c->g.H * c->g.W, G, nullptr);
    return copy_out(c, G, c ? c->d_G : nullptr, c ? (size_t)c->g.B * c->g.R * c->g.H * c->g.W * sizeof(float) : 0);
}
static int motion_theta_image(eincm_ctx* c);
// 2-DoF evaluations and fused motion-model evaluations skip the Theta image; build it when somebody asks for it
static int ensure_theta_image(eincm_ctx* c) {
    if (c->Theta_valid) return EINCM_OK;
    if (c->motion.last_q.size() == (size_t)c->g.B * MOTION_NQ && c->motion.set) return motion_theta_image(c);
    if (c->last_theta11.size() != (size_t)c->g.B * 2) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = ensure_resample(c, 1, 1, EINCM_METHOD_BILINEAR);      // a (1,1,2) theta upsamples to a constant with every method
    if (rc) return rc;
    memcpy(c->h_theta, c->last_theta11.data(), c->last_theta11.size() * sizeof(double));
    c->g.wmask = ~0ull;                              // every window's image, whatever the last evaluation masked
    static const ThetaArgBig targ{};
    launch_theta_image(c, 1, 1, false, false, targ, c->h_theta, false);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EINCM_OK;
}

int eincm_get_scaled_theta(eincm_ctx* c, double* T) {
    if (c && !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    if (c && c->staged) { const int rc = ensure_theta_image(c); if (rc) return rc; }
    return copy_out(c, T, c ? c->d_Theta : nullptr, c ? (size_t)c->g.B * c->g.H * c->g.W * 2 * sizeof(double) : 0);
}

int eincm_get_count_images(eincm_ctx* c, uint32_t* counts) {
    if (!c) return EINCM_ERR_ARG;
    if (!counts) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->staged || !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    { const int rc = ensure_theta_image(c); if (rc) return rc; }
    const Geom& g = c->g;
    const size_t n = (size_t)g.B * g.R * g.H * g.W;
    // the dL/dIWE buffer is free between evaluations and has exactly this many 4-byte cells
    uint32_t* d = reinterpret_cast<uint32_t*>(c->d_G);
    OneShot op(c);                                  // no piece of the scratch: the frame is here for its drain
    HIPCHK(c, op.begin());
    if (!c->fp64) c->G_valid = false;               // (an fp64 context keeps dL/dIWE in its own buffer)
    HIPCHK(c, op.zero(d, n * sizeof(uint32_t)));
    const SegList& L = c->gather;
    if (L.n > 0)
        HIPCHK(c, op.launch(k_count, dim3(L.grid(g.R)), dim3(NT), 0, g, L.n, L.d_items, c->d_xy, c->d_t, c->d_Theta, c->d_edge_ts, d,
                             (const float*)(c->stage.weighted ? c->d_w : nullptr)));
    HIPCHK(c, op.down(counts, d, n * sizeof(uint32_t)));          // (host memory: the caller's)
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// ---------------------------------------------------------------------------------------------
// SURVEY row f-4 (eincm_edges.hip.h, eincm_canny.hip.h)
// ---------------------------------------------------------------------------------------------
// The one-shot operators below share c->scratch through one call frame each (OneShot): state and argument checks first; then the frame,
// its pieces and host buffers; begin() grows the block once, before the first command; every command goes onto the stream through the
// frame, which drains it on every way out, failures included, so no call finds another's work on the block still enqueued.  Before the
// frame only a return that had reached its last synchronisation drained.  Each copy says whose host memory it touches.

// 'warped_xs' / 'warped_ys' of compute_loss_objectives (losses.py:58,90-91) for one window under the last evaluation's theta
int eincm_get_warped_events(eincm_ctx* c, int window, double* warped_xs, double* warped_ys) {
    if (!c) return EINCM_ERR_ARG;
    if (!warped_xs || !warped_ys) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->staged || !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    const Geom& g = c->g;
    if (window < 0 || window >= g.B) return fail(c, EINCM_ERR_ARG, "window %d of %d", window, g.B);
    { const int rc = ensure_theta_image(c); if (rc) return rc; }
    const int64_t n = c->win_events[window];
    if (n == 0) return EINCM_OK;
    const int64_t off = stream_offset(c->win_events.data(), window);
    const size_t cells = (size_t)g.R * (size_t)n;
    OneShot op(c);
    const auto dx = op.piece<double>(cells), dy = op.piece<double>(cells);
    HIPCHK(c, op.begin());
    const int grid = (int)std::min<int64_t>((n + NT - 1) / NT, 8192);
    HIPCHK(c, op.launch(k_warp_events, dim3(grid), dim3(NT), 0, g, window, n, c->d_raw_x + off, c->d_raw_y + off, c->d_raw_t + off,
                        c->d_Theta, c->d_edge_ts, dx, dy));
    HIPCHK(c, op.down(warped_xs, dx, cells * sizeof(double)));    // (host memory: the caller's, both)
    HIPCHK(c, op.down(warped_ys, dy, cells * sizeof(double)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}


// Per-event scores of the whole staged batch under the last evaluation's Theta (eincm_event_scores.hip.h): the
// checks and the layout are eincm_event_scores.h's.  images == NULL reads the IWE stack where the evaluation left it.
int eincm_event_scores(eincm_ctx* c, const float* images, const double* ref_weights, float* scores, float* selfs) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const ScState st{!c->fl.idle(), scores != nullptr, c->staged, c->have_eval, c->fp64, c->splat_size,
                     c->sharded_staging || c->constants_pending, images != nullptr, RawEvents::masked(c)};
    if (const ScFault f = sc_check(st, ref_weights, g.R)) return fail(c, sc_code(f), "eincm_event_scores: %s", sc_why(f));
    { const int rc = ensure_theta_image(c); if (rc) return rc; }
    const int B = g.B, R = g.R;
    const bool combined = ref_weights != nullptr;
    OneShot op(c);
    RawEvents ev(op, [](const int64_t* n, int b) { return sc_block_offset(n, b, 1, true); });
    const int64_t n_out = sc_total(ev.ne, B, R, combined);
    if (ev.total() == 0) return EINCM_OK;
    const size_t stack = (size_t)B * R * g.H * g.W;
    const auto d_img = op.piece<float>(stack, images != nullptr);
    const auto d_rw = op.piece<float>((size_t)R, combined);
    const auto d_s = op.piece<float>((size_t)n_out);
    const auto d_q = op.piece<float>((size_t)n_out, selfs != nullptr);
    float* h_rw = op.host_buf<float>((size_t)R);                         // d_rw goes up from here
    for (int r = 0; combined && r < R; ++r) h_rw[r] = (float)ref_weights[r];
    HIPCHK(c, op.begin());
    HIPCHK(c, ev.upload());
    if (images) HIPCHK(c, op.up(d_img, images, stack * sizeof(float)));  // (host memory: the caller's, as scores and selfs)
    if (combined) HIPCHK(c, op.up(d_rw, h_rw, (size_t)R * sizeof(float)));
    const float* F = images ? (const float*)d_img : (const float*)c->d_iwe;
    const dim3 grid((unsigned)((ev.n_max + NT - 1) / NT), (unsigned)B);
    HIPCHK(c, op.launch(k_event_scores, grid, dim3(NT), 0, g, ev.d_off, c->d_raw_x, c->d_raw_y, c->d_raw_t, c->d_Theta, c->d_edge_ts, F, d_rw,
                        d_s, d_q));
    HIPCHK(c, op.down(scores, d_s, (size_t)n_out * sizeof(float)));
    if (selfs) HIPCHK(c, op.down(selfs, d_q, (size_t)n_out * sizeof(float)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// The E-step of a segmentation into n_models motions (eincm_responsibilities.hip.h): the scores of
// eincm_event_scores' combined form, normalised over the models of a group on the device.  The checks and the layout are
// eincm_responsibilities.h's.
int eincm_event_responsibilities(eincm_ctx* c, int n_models, const float* images, const double* ref_weights, const float* const* weights_in,
                                 const double* prior, uint32_t flags, float* weights_out, uint8_t* labels, double* mass,
                                 int64_t* n_unsupported) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const bool apply = (flags & EINCM_RS_APPLY) != 0, own_w = (flags & EINCM_RS_STAGED_WEIGHTS) != 0;    // a keep-order batch's two
    const RsState st{{!c->fl.idle(), weights_out || labels || mass || n_unsupported || apply, c->staged, c->have_eval, c->fp64, c->splat_size,
                      c->sharded_staging || c->constants_pending, images != nullptr, RawEvents::masked(c)},
                     c->staged ? g.B : 0, c->win_events.data()};
    if (const RsFault f = rs_check(st, n_models, ref_weights, g.R, prior))
        return fail(c, rs_code(f), "eincm_event_responsibilities: %s", rs_why(f));
    if (apply || own_w) {
        if (const int rc = keep_order_ready(c, apply ? "eincm_event_responsibilities (EINCM_RS_APPLY)" : "eincm_event_responsibilities (EINCM_RS_STAGED_WEIGHTS)")) return rc;
        if (own_w && weights_in) return fail(c, EINCM_ERR_ARG, "eincm_event_responsibilities: weights_in must be NULL with EINCM_RS_STAGED_WEIGHTS");
    }
    { const int rc = ensure_theta_image(c); if (rc) return rc; }
    const int B = g.B, R = g.R, K = n_models, G = B / K;
    OneShot op(c);
    RawEvents ev(op, [](const int64_t* n, int b) { return rs_weights_offset(n, b); });
    const int64_t n_events = rs_weights_total(ev.ne, B), n_labels = rs_labels_total(ev.ne, B, K);
    if (n_events == 0) return EINCM_OK;
    const size_t n_blk = (size_t)((ev.n_max + NT - 1) / NT), stack = (size_t)B * R * g.H * g.W;
    const bool any_w = (flags & EINCM_RS_EXCLUDE_SELF) && ev.any(weights_in);
    const bool self_own = own_w && (flags & EINCM_RS_EXCLUDE_SELF);       // w_l is read where staging left it: every window has its weights there
    const auto d_img = op.piece<float>(stack, images != nullptr);
    const auto d_rw = op.piece<float>((size_t)R);
    const auto d_pi = op.piece<float>((size_t)B);
    const auto d_win = op.piece<float>((size_t)n_events, any_w);
    const auto d_has = op.piece<uint8_t>((size_t)B, any_w || self_own);
    const auto d_wout = op.piece<float>((size_t)n_events, weights_out != nullptr || apply);
    const auto d_lab = op.piece<uint8_t>((size_t)n_labels, labels != nullptr);
    const auto d_part = op.piece<double>((size_t)B * n_blk, mass != nullptr);
    const auto d_mass = op.piece<double>((size_t)B, mass != nullptr);
    const auto d_uns = op.piece<unsigned long long>((size_t)G, n_unsupported != nullptr);
    float* h_rw = op.host_buf<float>((size_t)R);                         // d_rw, d_pi and (self_own) d_has go up from these
    float* h_pi = op.host_buf<float>((size_t)B);
    uint8_t* h_all = op.host_buf<uint8_t>((size_t)B);
    for (int r = 0; r < R; ++r) h_rw[r] = (float)ref_weights[r];
    for (int b = 0; b < B; ++b) h_pi[b] = prior ? (float)prior[b] : 1.0f;
    for (int b = 0; b < B; ++b) h_all[b] = 1;
    HIPCHK(c, op.begin());
    HIPCHK(c, ev.upload());
    if (images) HIPCHK(c, op.up(d_img, images, stack * sizeof(float)));  // (host memory: the caller's, as weights_in and the outputs)
    HIPCHK(c, op.up(d_rw, h_rw, (size_t)R * sizeof(float)));
    HIPCHK(c, op.up(d_pi, h_pi, (size_t)B * sizeof(float)));
    if (any_w) HIPCHK(c, ev.upload_per_window(weights_in, (float*)d_win, d_has));
    if (self_own) HIPCHK(c, op.up(d_has, h_all, (size_t)B));
    const float* w_self = self_own ? (const float*)c->ord.stream : (const float*)d_win;     // (the stream order is the layout of weights_in)
    if (n_unsupported) HIPCHK(c, op.zero(d_uns, (size_t)G * sizeof(unsigned long long)));
    const float* F = images ? (const float*)d_img : (const float*)c->d_iwe;
    const dim3 grid((unsigned)n_blk, (unsigned)G);
    HIPCHK(c, op.launch(rs_kernel(K), grid, dim3(NT), 0, g, ev.d_off, c->d_raw_x, c->d_raw_y, c->d_raw_t, c->d_Theta, c->d_edge_ts, F, d_rw,
                        w_self, d_has, d_pi, flags, d_wout, d_lab, d_part, d_uns));
    if (mass) {
        HIPCHK(c, op.launch(k_rs_mass, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, B, ev.d_off, d_part, (int64_t)n_blk, d_mass));
        HIPCHK(c, op.down(mass, d_mass, (size_t)B * sizeof(double)));
    }
    if (weights_out) HIPCHK(c, op.down(weights_out, d_wout, (size_t)n_events * sizeof(float)));
    if (labels) HIPCHK(c, op.down(labels, d_lab, (size_t)n_labels));
    if (n_unsupported) HIPCHK(c, op.down(n_unsupported, d_uns, (size_t)G * sizeof(int64_t)));
    if (apply) {                                    // w' is in the stream order already: it becomes the staged weights without leaving the device
        HIPCHK(c, hipMemcpyAsync(c->ord.stream, (const float*)d_wout, (size_t)n_events * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        return reweight_staged(c, op);
    }
    HIPCHK(c, op.sync());
    return EINCM_OK;
}


// The contrast landscape over motion coefficients (eincm_contrast_landscape.hip.h): per window and candidate the
// integer sum of squared cell counts of the warped events, and how many events stayed inside the sensor.  The checks, their order and
// the band plan are eincm_contrast_landscape.h's; q = M c is motion_q, as eincm_loss_grad_motion forms it.
int eincm_contrast_landscape(eincm_ctx* c, int n_candidates, const double* coeffs, const double* t_ref, int cell, const uint8_t* const* keep,
                             uint64_t* sumsq, uint32_t* n_in) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const auto& mo = c->motion;
    const ClState st{!c->fl.idle(), sumsq || n_in, c->staged, mo.set, c->sharded_staging || c->constants_pending, c->staged ? g.B : 0,
                     mo.set ? mo.model.n_coeffs : 0};
    int bad_b = 0; int64_t bad_i = 0;
    if (const ClFault f = cl_check(st, n_candidates, cell, coeffs, t_ref, &bad_b, &bad_i)) {
        if (f == CL_NONFINITE && bad_i < 0) return fail(c, cl_code(f), "eincm_contrast_landscape: %s: t_ref of window %d", cl_why(f), bad_b);
        if (f == CL_NONFINITE)
            return fail(c, cl_code(f), "eincm_contrast_landscape: %s: window %d, candidate %lld, coefficient %d", cl_why(f), bad_b,
                        (long long)(bad_i / mo.model.n_coeffs), (int)(bad_i % mo.model.n_coeffs));
        return fail(c, cl_code(f), "eincm_contrast_landscape: %s", cl_why(f));
    }
    const int B = g.B, V = n_candidates, K = mo.model.n_coeffs;
    const ClBands plan = cl_bands(g.H, g.W, cell);
    const size_t BV = (size_t)B * V, n_bands = (size_t)plan.n_bands();
    OneShot op(c);
    RawEvents ev(op);
    const bool any_keep = ev.any(keep);
    const auto d_q = op.piece<double>(BV * MOTION_NQ);
    const auto d_tref = op.piece<double>((size_t)B);
    const auto d_keep = op.piece<uint8_t>((size_t)ev.total(), any_keep);
    const auto d_has = op.piece<uint8_t>((size_t)B, any_keep);
    const auto d_part = op.piece<unsigned long long>(BV * n_bands * 2);
    const auto d_sumsq = op.piece<unsigned long long>(BV, sumsq != nullptr);
    const auto d_nin = op.piece<uint32_t>(BV, n_in != nullptr);
    double* h_q = op.host_buf<double>(BV * MOTION_NQ);                   // d_q goes up from here; d_tref from the caller's
    for (size_t i = 0; i < BV; ++i) motion_q(mo.model, coeffs + i * K, h_q + i * MOTION_NQ);
    HIPCHK(c, op.begin());
    HIPCHK(c, ev.upload());
    HIPCHK(c, op.up(d_q, h_q, BV * MOTION_NQ * sizeof(double)));
    HIPCHK(c, op.up(d_tref, t_ref, (size_t)B * sizeof(double)));         // (host memory: the caller's, as keep and the outputs)
    if (any_keep) HIPCHK(c, ev.upload_per_window(keep, (uint8_t*)d_keep, d_has));
    const ClGeom cg{g.H, g.W, V, cl_log2_cell(cell), plan.rows, plan.cols, plan.n_col_bands, plan.Hc, plan.Wc, plan.table,
                    mo.model.cx, mo.model.cy, mo.model.scale};
    HIPCHK(c, op.launch(k_contrast_landscape, dim3((unsigned)n_bands, (unsigned)V, (unsigned)B), dim3(CL_NT), (size_t)plan.lds_bytes(), cg, ev.d_off,
                        c->d_raw_x, c->d_raw_y, c->d_raw_t, d_q, d_tref, d_keep, d_has, d_part));
    HIPCHK(c, op.launch(k_cl_sum_bands, dim3((unsigned)((BV + NT - 1) / NT)), dim3(NT), 0, (int)BV, (int)n_bands, d_part, d_sumsq, d_nin));
    if (sumsq) HIPCHK(c, op.down(sumsq, d_sumsq, BV * sizeof(uint64_t)));
    if (n_in) HIPCHK(c, op.down(n_in, d_nin, BV * sizeof(uint32_t)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// A motion segmentation composed into one flow field and a label image (eincm_motion_layers.hip.h): per pixel the
// quantised staged weights of the events that fired there, summed per model; the label is the model of the largest sum and Theta that
// model's field, or the blend.  The checks, their order and the layout are eincm_motion_layers.h's; q = M c is motion_q.  Only the
// gather's copy of the staged events and its weights are read; the mass images, the largest piece, live in the call frame's scratch,
// which grows on the first call.
int eincm_compose_motions(eincm_ctx* c, int n_models, const double* coeffs, unsigned flags, double* theta, uint8_t* labels, uint32_t* mass,
                          uint64_t* total) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const auto& mo = c->motion;
    const MlState st{!c->fl.idle(), theta || labels || mass || total, c->staged, mo.set, c->fp64, c->sharded_staging || c->constants_pending,
                     c->staged ? g.B : 0, c->win_events.data(), mo.set ? mo.model.n_coeffs : 0, c->h_tilecount.data(),
                     c->staged ? (int64_t)c->h_tilecount.size() : 0};
    int bad_b = 0; int64_t bad_i = 0;
    if (const MlFault f = ml_check(st, n_models, coeffs, flags, &bad_b, &bad_i)) {
        if (f == ML_COEFFS && bad_b >= 0)
            return fail(c, ml_code(f), "eincm_compose_motions: %s: window %d, coefficient %d", ml_why(f), bad_b, (int)bad_i);
        if (f == ML_CROWDED)
            return fail(c, ml_code(f), "eincm_compose_motions: %s: window %d, tile %lld holds %d", ml_why(f), bad_b, (long long)bad_i,
                        (int)c->h_tilecount[(size_t)bad_b * g.ntiles + (size_t)bad_i]);
        return fail(c, ml_code(f), "eincm_compose_motions: %s", ml_why(f));
    }
    const int B = g.B, K = n_models, G = B / K, Kc = mo.model.n_coeffs;
    const size_t npix = (size_t)g.H * g.W, bins = (size_t)B * g.ntiles, GK = (size_t)G * K;
    OneShot op(c);
    const auto d_off = op.piece<int32_t>(bins + 1);
    const auto d_q = op.piece<double>((size_t)B * MOTION_NQ);
    const auto d_mass = op.piece<uint32_t>(GK * npix);
    const auto d_part = op.piece<unsigned long long>(GK * g.ntiles);
    const auto d_total = op.piece<unsigned long long>(GK);
    const auto d_theta = op.piece<double2>((size_t)G * npix, theta != nullptr);
    const auto d_lab = op.piece<uint8_t>((size_t)G * npix, labels != nullptr);
    int32_t* h_off = op.host_buf<int32_t>(bins + 1);                     // d_off and d_q go up from these
    double* h_q = op.host_buf<double>((size_t)B * MOTION_NQ);
    int64_t run = 0;                                                     // (the bins lie one after another in (window, tile) order: eincm_binning.hip.h)
    for (size_t i = 0; i < bins; ++i) { h_off[i] = (int32_t)run; run += c->h_tilecount[i]; }
    h_off[bins] = (int32_t)run;
    if (run != c->stage.N) return fail(c, EINCM_ERR_STATE, "eincm_compose_motions: internal: the tile populations do not add up to the staged events");
    for (int b = 0; b < B; ++b) motion_q(mo.model, coeffs + (size_t)b * Kc, h_q + (size_t)b * MOTION_NQ);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_off, h_off, (bins + 1) * sizeof(int32_t)));
    HIPCHK(c, op.up(d_q, h_q, (size_t)B * MOTION_NQ * sizeof(double)));
    const MlGeom mg{g.H, g.W, g.tilesX, g.ntiles, K, flags, mo.model.cx, mo.model.cy, mo.model.scale};
    const float* w = c->stage.weighted ? (const float*)c->d_w_g : nullptr;          // (an unweighted batch has no ev_w: q = 4096)
    HIPCHK(c, op.launch(k_ml_mass, dim3((unsigned)g.ntiles, (unsigned)G), dim3(ML_NT), (size_t)K * ML_TILE_PIX * sizeof(uint32_t), mg, d_off,
                        c->d_xy_g, w, d_mass, d_part));
    HIPCHK(c, op.launch(k_ml_total, dim3((unsigned)GK), dim3(64), 0, g.ntiles, d_part, d_total));
    if (theta || labels)
        HIPCHK(c, op.launch(k_ml_compose, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)G), dim3(NT), 0, mg, d_mass, d_total, d_q, d_theta,
                            d_lab));
    if (theta) HIPCHK(c, op.down(theta, d_theta, (size_t)G * npix * sizeof(double2)));   // (host memory: the caller's, all four)
    if (labels) HIPCHK(c, op.down(labels, d_lab, (size_t)G * npix));
    if (mass) HIPCHK(c, op.down(mass, d_mass, GK * npix * sizeof(uint32_t)));
    if (total) HIPCHK(c, op.down(total, d_total, GK * sizeof(uint64_t)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// That composition made dense (eincm_motion_fill.hip.h): the masses and totals by the same two kernels, then the
// sites, the feature transform (columns, rows) and the composition at every pixel's nearest site.  The checks, their order and the
// layout are eincm_motion_fill.h's.  Only what an output asked for needs is allocated, launched and downloaded.
int eincm_densify_motions(eincm_ctx* c, int n_models, const double* coeffs, unsigned flags, uint32_t min_site_mass, uint32_t max_dist2,
                          double* theta, uint8_t* labels, uint32_t* dist2, int32_t* nearest, uint32_t* n_sites) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const auto& mo = c->motion;
    const MlState st{!c->fl.idle(), theta || labels || dist2 || nearest || n_sites, c->staged, mo.set, c->fp64,
                     c->sharded_staging || c->constants_pending, c->staged ? g.B : 0, c->win_events.data(), mo.set ? mo.model.n_coeffs : 0,
                     c->h_tilecount.data(), c->staged ? (int64_t)c->h_tilecount.size() : 0};
    int bad_b = 0; int64_t bad_i = 0;
    if (const int f = mf_check(st, g.W, n_models, coeffs, flags, min_site_mass, &bad_b, &bad_i)) {
        if (f == ML_COEFFS && bad_b >= 0)
            return fail(c, mf_code(f), "eincm_densify_motions: %s: window %d, coefficient %d", mf_why(f), bad_b, (int)bad_i);
        if (f == ML_CROWDED)
            return fail(c, mf_code(f), "eincm_densify_motions: %s: window %d, tile %lld holds %d", mf_why(f), bad_b, (long long)bad_i,
                        (int)c->h_tilecount[(size_t)bad_b * g.ntiles + (size_t)bad_i]);
        return fail(c, mf_code(f), "eincm_densify_motions: %s", mf_why(f));
    }
    const int B = g.B, K = n_models, G = B / K, Kc = mo.model.n_coeffs;
    const size_t npix = (size_t)g.H * g.W, bins = (size_t)B * g.ntiles, GK = (size_t)G * K, nblk = (npix + NT - 1) / NT;
    const bool composed = theta || labels, transformed = composed || dist2 || nearest;
    OneShot op(c);
    const auto d_off = op.piece<int32_t>(bins + 1);
    const auto d_q = op.piece<double>((size_t)B * MOTION_NQ, composed);
    const auto d_mass = op.piece<uint32_t>(GK * npix);
    const auto d_part = op.piece<unsigned long long>(GK * g.ntiles);
    const auto d_total = op.piece<unsigned long long>(GK);
    const auto d_site = op.piece<uint8_t>((size_t)G * npix);
    const auto d_cnt = op.piece<uint32_t>((size_t)G * nblk);
    const auto d_nsites = op.piece<uint32_t>((size_t)G, n_sites != nullptr);
    const auto d_rec = op.piece<uint32_t>((size_t)G * npix, transformed);
    const auto d_near = op.piece<int32_t>((size_t)G * npix, composed || nearest);
    const auto d_d2 = op.piece<uint32_t>((size_t)G * npix, composed || dist2);
    const auto d_theta = op.piece<double2>((size_t)G * npix, theta != nullptr);
    const auto d_lab = op.piece<uint8_t>((size_t)G * npix, labels != nullptr);
    int32_t* h_off = op.host_buf<int32_t>(bins + 1);                     // d_off and d_q go up from these
    double* h_q = op.host_buf<double>((size_t)B * MOTION_NQ);
    int64_t run = 0;                                                     // (as eincm_compose_motions: the bins lie in (window, tile) order)
    for (size_t i = 0; i < bins; ++i) { h_off[i] = (int32_t)run; run += c->h_tilecount[i]; }
    h_off[bins] = (int32_t)run;
    if (run != c->stage.N) return fail(c, EINCM_ERR_STATE, "eincm_densify_motions: internal: the tile populations do not add up to the staged events");
    for (int b = 0; b < B; ++b) motion_q(mo.model, coeffs + (size_t)b * Kc, h_q + (size_t)b * MOTION_NQ);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_off, h_off, (bins + 1) * sizeof(int32_t)));
    if (composed) HIPCHK(c, op.up(d_q, h_q, (size_t)B * MOTION_NQ * sizeof(double)));
    const MlGeom mg{g.H, g.W, g.tilesX, g.ntiles, K, flags, mo.model.cx, mo.model.cy, mo.model.scale};
    const float* w = c->stage.weighted ? (const float*)c->d_w_g : nullptr;          // (an unweighted batch has no ev_w: q = 4096)
    HIPCHK(c, op.launch(k_ml_mass, dim3((unsigned)g.ntiles, (unsigned)G), dim3(ML_NT), (size_t)K * ML_TILE_PIX * sizeof(uint32_t), mg, d_off,
                        c->d_xy_g, w, d_mass, d_part));
    if (composed) HIPCHK(c, op.launch(k_ml_total, dim3((unsigned)GK), dim3(64), 0, g.ntiles, d_part, d_total));
    HIPCHK(c, op.launch(k_mf_sites, dim3((unsigned)nblk, (unsigned)G), dim3(NT), 0, (int)npix, K, min_site_mass, d_mass, d_site, d_cnt));
    if (n_sites) HIPCHK(c, op.launch(k_mf_count, dim3((unsigned)G), dim3(64), 0, (int)nblk, d_cnt, d_nsites));
    if (transformed) {
        HIPCHK(c, op.launch(k_mf_cols, dim3((unsigned)((g.W + NT - 1) / NT), (unsigned)G), dim3(NT), 0, g.H, g.W, d_site, d_rec));
        HIPCHK(c, op.launch(k_mf_rows, dim3((unsigned)g.H, (unsigned)G), dim3(NT), (size_t)g.W * sizeof(uint32_t), g.H, g.W, d_rec, d_near, d_d2));
    }
    if (composed)
        HIPCHK(c, op.launch(k_mf_compose, dim3((unsigned)nblk, (unsigned)G), dim3(NT), 0, mg, max_dist2, d_mass, d_total, d_q, d_near, d_d2,
                            d_theta, d_lab));
    if (theta) HIPCHK(c, op.down(theta, d_theta, (size_t)G * npix * sizeof(double2)));   // (host memory: the caller's, all five)
    if (labels) HIPCHK(c, op.down(labels, d_lab, (size_t)G * npix));
    if (dist2) HIPCHK(c, op.down(dist2, d_d2, (size_t)G * npix * sizeof(uint32_t)));
    if (nearest) HIPCHK(c, op.down(nearest, d_near, (size_t)G * npix * sizeof(int32_t)));
    if (n_sites) HIPCHK(c, op.down(n_sites, d_nsites, (size_t)G * sizeof(uint32_t)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// The per-pixel label prior (eincm_label_prior.hip.h): the mass images by k_ml_mass, as eincm_compose_motions
// forms them, then every (tile, group)'s box sums and shares by one workgroup.  The checks, their order and the layout are
// eincm_label_prior.h's.  The prior stack is written where it stays, c->lp.prior (grown before the frame begins: a growth drains the
// stream and nothing of this call is on it yet), and marked staged once the call has ended on its synchronisation.
int eincm_label_prior(eincm_ctx* c, int n_models, int radius, uint32_t floor_mass, unsigned flags, float* prior, uint64_t* smoothed) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const LpState st{!c->fl.idle(), c->staged, c->fp64, c->sharded_staging || c->constants_pending, c->staged ? g.B : 0, c->win_events.data(),
                     c->h_tilecount.data(), c->staged ? (int64_t)c->h_tilecount.size() : 0};
    int bad_b = 0; int64_t bad_i = 0;
    if (const LpFault f = lp_check(st, n_models, radius, flags, &bad_b, &bad_i)) {
        if (f == LP_CROWDED)
            return fail(c, lp_code(f), "eincm_label_prior: %s: window %d, tile %lld holds %d", lp_why(f), bad_b, (long long)bad_i,
                        (int)c->h_tilecount[(size_t)bad_b * g.ntiles + (size_t)bad_i]);
        return fail(c, lp_code(f), "eincm_label_prior: %s", lp_why(f));
    }
    const int B = g.B, K = n_models, G = B / K;
    const size_t npix = (size_t)g.H * g.W, bins = (size_t)B * g.ntiles, GK = (size_t)G * K;
    OneShot op(c);
    const auto d_off = op.piece<int32_t>(bins + 1);
    const auto d_mass = op.piece<uint32_t>(GK * npix);
    const auto d_part = op.piece<unsigned long long>(GK * g.ntiles);
    const auto d_smooth = op.piece<unsigned long long>(GK * npix, smoothed != nullptr);
    int32_t* h_off = op.host_buf<int32_t>(bins + 1);                     // d_off goes up from here
    int64_t run = 0;                                                     // (as eincm_compose_motions: the bins lie in (window, tile) order)
    for (size_t i = 0; i < bins; ++i) { h_off[i] = (int32_t)run; run += c->h_tilecount[i]; }
    h_off[bins] = (int32_t)run;
    if (run != c->stage.N) return fail(c, EINCM_ERR_STATE, "eincm_label_prior: internal: the tile populations do not add up to the staged events");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, ensure(c, c->lp.prior, (size_t)B * npix));
    c->lp.staged = false;                                                // (until this call's prior is whole)
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_off, h_off, (bins + 1) * sizeof(int32_t)));
    const MlGeom mg{g.H, g.W, g.tilesX, g.ntiles, K, 0u, 0.0, 0.0, 1.0};                   // (k_ml_mass reads no flag and no model)
    const float* w = c->stage.weighted ? (const float*)c->d_w_g : nullptr;          // (an unweighted batch has no ev_w: q = 4096)
    HIPCHK(c, op.launch(k_ml_mass, dim3((unsigned)g.ntiles, (unsigned)G), dim3(ML_NT), (size_t)K * ML_TILE_PIX * sizeof(uint32_t), mg, d_off,
                        c->d_xy_g, w, d_mass, d_part));
    const LpGeom lg{g.H, g.W, g.tilesX, radius, floor_mass};
    HIPCHK(c, op.launch(lp_kernel(K), dim3((unsigned)g.ntiles, (unsigned)G), dim3(LP_NT), 0, lg, d_mass, c->lp.prior.p, d_smooth));
    if (prior) HIPCHK(c, op.down(prior, c->lp.prior.p, (size_t)B * npix * sizeof(float)));       // (host memory: the caller's, both)
    if (smoothed) HIPCHK(c, op.down(smoothed, d_smooth, GK * npix * sizeof(uint64_t)));
    HIPCHK(c, op.sync());
    c->lp.staged = true;
    return EINCM_OK;
}

int eincm_get_staged_prior(eincm_ctx* c, float* prior) {
    if (!c) return EINCM_ERR_ARG;
    if (!prior) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (const int rc = not_in_flight(c, "eincm_get_staged_prior")) return rc;
    if (!c->staged || !c->lp.staged)
        return fail(c, EINCM_ERR_STATE, "eincm_get_staged_prior: no staged prior (eincm_label_prior since the last eincm_set_windows)");
    OneShot op(c);                                  // no piece of the scratch: the frame is here for its drain
    HIPCHK(c, op.begin());
    HIPCHK(c, op.down(prior, c->lp.prior.p, (size_t)c->g.B * c->g.H * c->g.W * sizeof(float)));          // (host memory: the caller's)
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// The label prior carried to the next window (eincm_label_carry.hip.h): the mass images by k_ml_mass, as
// eincm_label_prior forms them; every model's image pushed along that model's own field into u64 accumulators (k_lc_splat), resolved to
// uint32 masses (k_lc_resolve), and k_label_prior, unchanged, on those.  The checks, their order and the layout are
// eincm_label_carry.h's.  The result is written where it stays, c->lc.prior (grown before the frame begins), and marked valid once the
// call has ended on its synchronisation; c->lp, the staged prior of the batch that is staged now, is not touched.
int eincm_carry_label_prior(eincm_ctx* c, int n_models, const double* coeffs, int n_coeffs, const double* tau, int radius, uint32_t floor_mass,
                            unsigned flags, float* prior, uint32_t* carried, uint64_t* accum, uint64_t* dropped) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    const auto& mo = c->motion;
    const LpState st{!c->fl.idle(), c->staged, c->fp64, c->sharded_staging || c->constants_pending, c->staged ? g.B : 0, c->win_events.data(),
                     c->h_tilecount.data(), c->staged ? (int64_t)c->h_tilecount.size() : 0};
    const LcArgs la{coeffs != nullptr, tau != nullptr, mo.set, n_coeffs, mo.set ? mo.model.n_coeffs : 0, tau, flags};
    int bad_b = 0; int64_t bad_i = 0;
    if (const int f = lc_check(st, la, n_models, radius, &bad_b, &bad_i)) {
        if (f == LP_CROWDED)
            return fail(c, lc_code(f), "eincm_carry_label_prior: %s: window %d, tile %lld holds %d", lc_why(f), bad_b, (long long)bad_i,
                        (int)c->h_tilecount[(size_t)bad_b * g.ntiles + (size_t)bad_i]);
        if (f == LC_TAU) return fail(c, lc_code(f), "eincm_carry_label_prior: %s: group %d", lc_why(f), bad_b);
        if (f == LC_WIDTH) return fail(c, lc_code(f), "eincm_carry_label_prior: %s: %d, the model has %d", lc_why(f), n_coeffs, mo.model.n_coeffs);
        if (f == LC_EVENTS) return fail(c, lc_code(f), "eincm_carry_label_prior: %s: window %d", lc_why(f), bad_b);
        return fail(c, lc_code(f), "eincm_carry_label_prior: %s", lc_why(f));
    }
    const int B = g.B, K = n_models, G = B / K, Kc = mo.model.n_coeffs;
    const size_t npix = (size_t)g.H * g.W, bins = (size_t)B * g.ntiles, GK = (size_t)G * K;
    OneShot op(c);
    const auto d_off = op.piece<int32_t>(bins + 1);
    const auto d_q = op.piece<double>((size_t)B * MOTION_NQ);
    const auto d_tau = op.piece<double>((size_t)G);
    const auto d_mass = op.piece<uint32_t>(GK * npix);
    const auto d_part = op.piece<unsigned long long>(GK * g.ntiles);
    const auto d_acc = op.piece<unsigned long long>(GK * npix + GK);    // A (G, K, H W) | dropped (G K): one clear for both
    const auto d_car = op.piece<uint32_t>(GK * npix);
    int32_t* h_off = op.host_buf<int32_t>(bins + 1);                     // d_off and d_q go up from these
    double* h_q = op.host_buf<double>((size_t)B * MOTION_NQ);
    int64_t run = 0;                                                     // (as eincm_compose_motions: the bins lie in (window, tile) order)
    for (size_t i = 0; i < bins; ++i) { h_off[i] = (int32_t)run; run += c->h_tilecount[i]; }
    h_off[bins] = (int32_t)run;
    if (run != c->stage.N) return fail(c, EINCM_ERR_STATE, "eincm_carry_label_prior: internal: the tile populations do not add up to the staged events");
    for (int b = 0; b < B; ++b) motion_q(mo.model, coeffs + (size_t)b * Kc, h_q + (size_t)b * MOTION_NQ);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, ensure(c, c->lc.prior, (size_t)B * npix));
    c->lc.of.valid = false;                                              // (until this call's prior is whole)
    HIPCHK(c, op.begin());
    unsigned long long* const d_drop = (unsigned long long*)d_acc + GK * npix;
    HIPCHK(c, op.up(d_off, h_off, (bins + 1) * sizeof(int32_t)));
    HIPCHK(c, op.up(d_q, h_q, (size_t)B * MOTION_NQ * sizeof(double)));
    HIPCHK(c, op.up(d_tau, tau, (size_t)G * sizeof(double)));           // (host memory: the caller's, as the outputs)
    HIPCHK(c, op.zero(d_acc, (GK * npix + GK) * sizeof(unsigned long long)));
    const MlGeom mg{g.H, g.W, g.tilesX, g.ntiles, K, 0u, 0.0, 0.0, 1.0};                   // (k_ml_mass reads no flag and no model)
    const float* w = c->stage.weighted ? (const float*)c->d_w_g : nullptr;          // (an unweighted batch has no ev_w: q = 4096)
    HIPCHK(c, op.launch(k_ml_mass, dim3((unsigned)g.ntiles, (unsigned)G), dim3(ML_NT), (size_t)K * ML_TILE_PIX * sizeof(uint32_t), mg, d_off,
                        c->d_xy_g, w, d_mass, d_part));
    const LcGeom cg{g.H, g.W, K, mo.model.cx, mo.model.cy, mo.model.scale};
    HIPCHK(c, op.launch(k_lc_splat, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)GK), dim3(NT), 0, cg, d_mass, d_q, d_tau, d_acc, d_drop));
    HIPCHK(c, op.launch(k_lc_resolve, dim3((unsigned)((GK * npix + NT - 1) / NT)), dim3(NT), 0, GK * npix, d_acc, d_car));
    const LpGeom lg{g.H, g.W, g.tilesX, radius, floor_mass};
    HIPCHK(c, op.launch(lp_kernel(K), dim3((unsigned)g.ntiles, (unsigned)G), dim3(LP_NT), 0, lg, d_car, c->lc.prior.p, nullptr));
    if (prior) HIPCHK(c, op.down(prior, c->lc.prior.p, (size_t)B * npix * sizeof(float)));
    if (carried) HIPCHK(c, op.down(carried, d_car, GK * npix * sizeof(uint32_t)));
    if (accum) HIPCHK(c, op.down(accum, d_acc, GK * npix * sizeof(uint64_t)));
    if (dropped) HIPCHK(c, op.down(dropped, d_drop, GK * sizeof(uint64_t)));
    HIPCHK(c, op.sync());
    c->lc.of = LcCarried{true, K, B, g.H, g.W};
    return EINCM_OK;
}

// The carried prior becomes the staged prior of the batch staged now: one copy on the device, and c->lp is as eincm_label_prior would
// have left it, so the EINCM_RS_PRIOR_STAGED path of the spatial E-step reads it with no change.  The carried prior stays valid.
int eincm_adopt_carried_prior(eincm_ctx* c, int n_models) {
    if (!c) return EINCM_ERR_ARG;
    const Geom& g = c->g;
    if (const LcAdoptFault f = lc_adopt_check(!c->fl.idle(), c->staged, c->lc.of, n_models, c->staged ? g.B : 0, c->staged ? g.H : 0, c->staged ? g.W : 0))
        return fail(c, lc_adopt_code(f), "eincm_adopt_carried_prior: %s", lc_adopt_why(f));
    const size_t n = (size_t)g.B * g.H * g.W;
    OneShot op(c);                                  // no piece of the scratch: the frame is here for its drain
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, ensure(c, c->lp.prior, n));
    c->lp.staged = false;                           // (until the copy is whole)
    HIPCHK(c, op.begin());
    op.pending = true;
    HIPCHK(c, hipMemcpyAsync(c->lp.prior.p, c->lc.prior.p, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, op.sync());
    c->lp.staged = true;
    return EINCM_OK;
}

int eincm_get_carried_prior(eincm_ctx* c, float* prior) {
    if (!c) return EINCM_ERR_ARG;
    if (!prior) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (const int rc = not_in_flight(c, "eincm_get_carried_prior")) return rc;
    if (!c->lc.of.valid) return fail(c, EINCM_ERR_STATE, "eincm_get_carried_prior: %s", lc_adopt_why(LCA_NONE));
    OneShot op(c);                                  // no piece of the scratch: the frame is here for its drain
    HIPCHK(c, op.begin());
    HIPCHK(c, op.down(prior, c->lc.prior.p, (size_t)c->lc.of.n_windows * c->lc.of.H * c->lc.of.W * sizeof(float)));  // (host memory: the caller's)
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// The E-step with a prior image.  eincm_event_responsibilities' body is pinned by its tests, so this one follows
// it line by line instead of sharing it: the same checks first (rs_check, then the keep-order flags), then rs_spatial_check; the same
// frame with one piece more, the prior stack, uploaded or (EINCM_RS_PRIOR_STAGED) read where eincm_label_prior left it; the SP = 1
// instantiation of the same kernel; k_rs_mass, the downloads and EINCM_RS_APPLY as there.
int eincm_event_responsibilities_spatial(eincm_ctx* c, int n_models, const float* images, const double* ref_weights,
                                         const float* const* weights_in, const double* prior, const float* prior_images, uint32_t flags,
                                         float* weights_out, uint8_t* labels, double* mass, int64_t* n_unsupported) {
    if (!c) return EINCM_ERR_ARG;
    static const char who[] = "eincm_event_responsibilities_spatial";
    const Geom& g = c->g;
    const bool apply = (flags & EINCM_RS_APPLY) != 0, own_w = (flags & EINCM_RS_STAGED_WEIGHTS) != 0;
    const RsState st{{!c->fl.idle(), weights_out || labels || mass || n_unsupported || apply, c->staged, c->have_eval, c->fp64, c->splat_size,
                      c->sharded_staging || c->constants_pending, images != nullptr, RawEvents::masked(c)},
                     c->staged ? g.B : 0, c->win_events.data()};
    if (const RsFault f = rs_check(st, n_models, ref_weights, g.R, prior)) return fail(c, rs_code(f), "%s: %s", who, rs_why(f));
    if (apply || own_w) {
        if (const int rc = keep_order_ready(c, apply ? "eincm_event_responsibilities_spatial (EINCM_RS_APPLY)" : "eincm_event_responsibilities_spatial (EINCM_RS_STAGED_WEIGHTS)")) return rc;
        if (own_w && weights_in) return fail(c, EINCM_ERR_ARG, "%s: weights_in must be NULL with EINCM_RS_STAGED_WEIGHTS", who);
    }
    const size_t npix = (size_t)g.H * g.W;
    int bad_b = 0; int64_t bad_p = 0;
    if (const RsSpatialFault f = rs_spatial_check(prior_images, flags, c->lp.staged, g.B, (int64_t)npix, &bad_b, &bad_p)) {
        if (f == RSS_VALUE)
            return fail(c, rs_spatial_code(f), "%s: %s: window %d, pixel (x %d, y %d) holds %g", who, rs_spatial_why(f), bad_b, (int)(bad_p % g.W),
                        (int)(bad_p / g.W), (double)prior_images[(size_t)bad_b * npix + (size_t)bad_p]);
        return fail(c, rs_spatial_code(f), "%s: %s", who, rs_spatial_why(f));
    }
    { const int rc = ensure_theta_image(c); if (rc) return rc; }
    const int B = g.B, R = g.R, K = n_models, G = B / K;
    OneShot op(c);
    RawEvents ev(op, [](const int64_t* n, int b) { return rs_weights_offset(n, b); });
    const int64_t n_events = rs_weights_total(ev.ne, B), n_labels = rs_labels_total(ev.ne, B, K);
    if (n_events == 0) return EINCM_OK;
    const size_t n_blk = (size_t)((ev.n_max + NT - 1) / NT), stack = (size_t)B * R * npix;
    const bool any_w = (flags & EINCM_RS_EXCLUDE_SELF) && ev.any(weights_in);
    const bool self_own = own_w && (flags & EINCM_RS_EXCLUDE_SELF);
    const auto d_img = op.piece<float>(stack, images != nullptr);
    const auto d_pimg = op.piece<float>((size_t)B * npix, prior_images != nullptr);
    const auto d_rw = op.piece<float>((size_t)R);
    const auto d_pi = op.piece<float>((size_t)B);
    const auto d_win = op.piece<float>((size_t)n_events, any_w);
    const auto d_has = op.piece<uint8_t>((size_t)B, any_w || self_own);
    const auto d_wout = op.piece<float>((size_t)n_events, weights_out != nullptr || apply);
    const auto d_lab = op.piece<uint8_t>((size_t)n_labels, labels != nullptr);
    const auto d_part = op.piece<double>((size_t)B * n_blk, mass != nullptr);
    const auto d_mass = op.piece<double>((size_t)B, mass != nullptr);
    const auto d_uns = op.piece<unsigned long long>((size_t)G, n_unsupported != nullptr);
    float* h_rw = op.host_buf<float>((size_t)R);                         // d_rw, d_pi and (self_own) d_has go up from these
    float* h_pi = op.host_buf<float>((size_t)B);
    uint8_t* h_all = op.host_buf<uint8_t>((size_t)B);
    for (int r = 0; r < R; ++r) h_rw[r] = (float)ref_weights[r];
    for (int b = 0; b < B; ++b) h_pi[b] = prior ? (float)prior[b] : 1.0f;
    for (int b = 0; b < B; ++b) h_all[b] = 1;
    HIPCHK(c, op.begin());
    HIPCHK(c, ev.upload());
    if (images) HIPCHK(c, op.up(d_img, images, stack * sizeof(float)));  // (host memory: the caller's, as prior_images, weights_in and the outputs)
    if (prior_images) HIPCHK(c, op.up(d_pimg, prior_images, (size_t)B * npix * sizeof(float)));
    HIPCHK(c, op.up(d_rw, h_rw, (size_t)R * sizeof(float)));
    HIPCHK(c, op.up(d_pi, h_pi, (size_t)B * sizeof(float)));
    if (any_w) HIPCHK(c, ev.upload_per_window(weights_in, (float*)d_win, d_has));
    if (self_own) HIPCHK(c, op.up(d_has, h_all, (size_t)B));
    const float* w_self = self_own ? (const float*)c->ord.stream : (const float*)d_win;
    if (n_unsupported) HIPCHK(c, op.zero(d_uns, (size_t)G * sizeof(unsigned long long)));
    const float* F = images ? (const float*)d_img : (const float*)c->d_iwe;
    const float* P = prior_images ? (const float*)d_pimg : (const float*)c->lp.prior.p;
    const dim3 grid((unsigned)n_blk, (unsigned)G);
    HIPCHK(c, op.launch(rs_spatial_kernel(K), grid, dim3(NT), 0, g, ev.d_off, c->d_raw_x, c->d_raw_y, c->d_raw_t, c->d_Theta, c->d_edge_ts, F,
                        d_rw, w_self, d_has, d_pi, flags, d_wout, d_lab, d_part, d_uns, P));
    if (mass) {
        HIPCHK(c, op.launch(k_rs_mass, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, B, ev.d_off, d_part, (int64_t)n_blk, d_mass));
        HIPCHK(c, op.down(mass, d_mass, (size_t)B * sizeof(double)));
    }
    if (weights_out) HIPCHK(c, op.down(weights_out, d_wout, (size_t)n_events * sizeof(float)));
    if (labels) HIPCHK(c, op.down(labels, d_lab, (size_t)n_labels));
    if (n_unsupported) HIPCHK(c, op.down(n_unsupported, d_uns, (size_t)G * sizeof(int64_t)));
    if (apply) {
        HIPCHK(c, hipMemcpyAsync(c->ord.stream, (const float*)d_wout, (size_t)n_events * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        return reweight_staged(c, op);
    }
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

int eincm_inv_dist_transform(eincm_ctx* c, const uint8_t* edge_img, int n, int formulation, double alpha, double d_sat,
                             double* out, int32_t* sqdist) {
    if (!c) return EINCM_ERR_ARG;
    if (!edge_img || (!out && !sqdist)) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1) return fail(c, EINCM_ERR_ARG, "n = %d images", n);
    if (formulation < EINCM_EDT_EXPONENTIAL || formulation > EINCM_EDT_LOGARITHMIC)
        return fail(c, EINCM_ERR_ARG, "unknown formulation %d", formulation);
    if (out && formulation == EINCM_EDT_EXPONENTIAL && !(alpha > 0.0)) return fail(c, EINCM_ERR_ARG, "alpha = %g must be positive", alpha);
    if (out && formulation == EINCM_EDT_LINEAR_BOUND && !(d_sat > 0.0)) return fail(c, EINCM_ERR_ARG, "d_sat = %g must be positive", d_sat);
    const int H = c->H, W = c->W;
    const size_t npix = (size_t)H * W, tot = npix * n;
    OneShot op(c);
    const auto d_img = op.piece<uint8_t>(tot);
    const auto d_g = op.piece<uint32_t>(tot);
    const auto d_sq = op.piece<int32_t>(tot);
    const auto d_misc = op.piece<uint32_t>((size_t)n * 2);            // [n] edge pixel count | [n] max squared distance
    const auto d_out = op.piece<double>(tot, out != nullptr);         // (only where out is asked for)
    uint32_t* misc = op.host_buf<uint32_t>((size_t)n * 2);            // d_misc comes down here
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_img, edge_img, tot));                           // (host memory: the caller's, as sqdist and out below)
    HIPCHK(c, op.zero(d_misc, (size_t)n * 8));
    const int gx = (W + NT - 1) / NT;
    HIPCHK(c, op.launch(k_edt_cols, dim3(gx, n), dim3(NT), 0, H, W, d_img, d_g, d_misc));
    HIPCHK(c, op.launch(k_edt_rows, dim3(gx, H, n), dim3(NT), 0, H, W, d_g, d_sq, d_misc + n));
    HIPCHK(c, op.down(misc, d_misc, (size_t)n * 8));
    HIPCHK(c, op.sync());
    for (int i = 0; i < n; ++i)
        if (misc[i] == 0) return fail(c, EINCM_ERR_ARG, "edge image %d has no edge pixel: its distance transform is undefined", i);
    if (sqdist) HIPCHK(c, op.down(sqdist, d_sq, tot * 4));
    if (out) {
        const int nb = (int)std::min<size_t>((npix + NT - 1) / NT, 1024);
        HIPCHK(c, op.launch(k_edt_finish, dim3(nb, n), dim3(NT), 0, npix, d_sq, d_misc + n, formulation, alpha, d_sat, d_out));
        HIPCHK(c, op.down(out, d_out, tot * 8));
    }
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

int eincm_gaussian_blur(eincm_ctx* c, const double* src, int n, double sigma, double* dst) {
    if (!c) return EINCM_ERR_ARG;
    if (!src || !dst) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1) return fail(c, EINCM_ERR_ARG, "n = %d images", n);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(c, EINCM_ERR_ARG, "sigma = %g must be positive", sigma);
    // cv::GaussianBlur on CV_64F with ksize = Size(): ksize = cvRound(sigma*4*2 + 1) | 1; cv::getGaussianKernel (sigma > 0 branch)
    const int taps = (int)std::nearbyint(sigma * 4 * 2 + 1) | 1;
    const int radius = taps / 2;
    if (taps > BLUR_MAX_TAPS) return fail(c, EINCM_ERR_UNSUPPORTED, "sigma = %g needs %d taps (> %d)", sigma, taps, BLUR_MAX_TAPS);
    if (radius >= c->W || radius >= c->H)
        return fail(c, EINCM_ERR_ARG, "kernel radius %d does not fit the %d x %d sensor (BORDER_REFLECT_101)", radius, c->H, c->W);
    std::vector<double> k((size_t)taps);
    double sum = 0.0;
    for (int i = 0; i < taps; ++i) { const double x = i - (taps - 1) * 0.5; k[i] = std::exp(-0.5 / (sigma * sigma) * x * x); sum += k[i]; }
    for (double& v : k) v /= sum;
    const int H = c->H, W = c->W;
    const size_t tot = (size_t)H * W * n;
    OneShot op(c);
    const auto d_a = op.piece<double>(tot);                // the source, then the result
    const auto d_b = op.piece<double>(tot);                // the row pass
    const auto d_kern = op.piece<double>(BLUR_MAX_TAPS);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_kern, k.data(), k.size() * 8));      // (host memory: k, a local older than the frame)
    HIPCHK(c, op.up(d_a, src, tot * 8));                   // (the caller's, as dst)
    const dim3 grid((W + NT - 1) / NT, H, n);
    HIPCHK(c, op.launch(k_blur, grid, dim3(NT), 0, H, W, 0, radius, d_kern, d_a, d_b));
    HIPCHK(c, op.launch(k_blur, grid, dim3(NT), 0, H, W, 1, radius, d_kern, d_b, d_a));
    HIPCHK(c, op.down(dst, d_a, tot * 8));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

int eincm_canny(eincm_ctx* c, const uint8_t* src, int n, double threshold1, double threshold2, int aperture_size, int l2_gradient,
                uint8_t* dst) {
    if (!c) return EINCM_ERR_ARG;
    if (!src || !dst) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1 || n > 65535) return fail(c, EINCM_ERR_ARG, "n = %d images (1..65535)", n);
    if (!std::isfinite(threshold1) || !std::isfinite(threshold2) || threshold1 < 0.0 || threshold2 < 0.0)
        return fail(c, EINCM_ERR_ARG, "thresholds %g, %g must be finite and non-negative", threshold1, threshold2);
    if (aperture_size != 3) return fail(c, EINCM_ERR_UNSUPPORTED, "aperture_size %d: only 3 is implemented", aperture_size);
    // cv::Canny: swap, then for L2 clamp to 32767 and square the positive ones; low/high = cvFloor.  For L1 |dx| + |dy| <= 2040, so
    // the same clamp changes no decision and keeps the floor inside int.
    if (threshold1 > threshold2) std::swap(threshold1, threshold2);
    threshold1 = std::min(threshold1, 32767.0);
    threshold2 = std::min(threshold2, 32767.0);
    if (l2_gradient) {
        if (threshold1 > 0) threshold1 *= threshold1;
        if (threshold2 > 0) threshold2 *= threshold2;
    }
    const int low = (int)std::floor(threshold1), high = (int)std::floor(threshold2);
    const int H = c->H, W = c->W;
    const size_t npix = (size_t)H * W, tot = npix * n;
    OneShot op(c);
    const auto d_img = op.piece<uint8_t>(tot);                     // the source, then the edge image
    const auto d_parent = op.piece<int32_t>(tot);
    const auto d_state = op.piece<uint8_t>(tot);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_img, src, tot));                             // (host memory: the caller's, as dst)
    HIPCHK(c, op.launch(k_canny_nms, dim3((W + CANNY_TW - 1) / CANNY_TW, (H + CANNY_TH - 1) / CANNY_TH, n), dim3(NT), 0, H, W, low, high,
                        l2_gradient ? 1 : 0, d_img, d_state, d_parent));
    const dim3 grid((unsigned)std::min<size_t>((npix + NT - 1) / NT, 1024), n);
    HIPCHK(c, op.launch(k_canny_merge, grid, dim3(NT), 0, H, W, d_state, d_parent));
    HIPCHK(c, op.launch(k_canny_resolve, grid, dim3(NT), 0, H, W, d_state, d_parent));
    HIPCHK(c, op.launch(k_canny_output, grid, dim3(NT), 0, H, W, d_state, d_parent, d_img));
    HIPCHK(c, op.down(dst, d_img, tot));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// preprocess_image (img_utils.py:131-189): host tables of the contract, then the selected stages back to back.

int eincm_preprocess_image(eincm_ctx* c, const uint8_t* src, int n, const eincm_preprocess_params* p, uint8_t* dst) {
#pragma clang fp contract(off)
    if (!c) return EINCM_ERR_ARG;
    if (!src || !dst || !p) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1 || n > 65535) return fail(c, EINCM_ERR_ARG, "n = %d images (1..65535)", n);
    const int st = p->stages;
    if (st < 1 || (st & ~EINCM_PRE_ALL)) return fail(c, EINCM_ERR_ARG, "stages = %d: a non-empty set of EINCM_PRE_* bits", st);
    const int H = c->H, W = c->W;
    const int tw = p->denoise_template_win, sw = p->denoise_search_win;
    if (st & EINCM_PRE_NLMEANS) {
        if (!(p->denoise_h > 0.0) || !std::isfinite(p->denoise_h))
            return fail(c, EINCM_ERR_ARG, "denoise_h = %g must be positive and finite", p->denoise_h);
        if (tw < 1 || sw < 1 || !(tw & 1) || !(sw & 1))
            return fail(c, EINCM_ERR_ARG, "NL-means windows %d, %d must be odd and positive", tw, sw);
        if (tw > NLM_MAX_TEMPLATE || sw > NLM_MAX_SEARCH)
            return fail(c, EINCM_ERR_UNSUPPORTED, "NL-means windows %d, %d (template <= %d, search <= %d)", tw, sw, NLM_MAX_TEMPLATE,
                        NLM_MAX_SEARCH);
    }
    const int tx = p->clahe_tiles_x, ty = p->clahe_tiles_y;
    if (st & EINCM_PRE_CLAHE) {
        if (tx < 1 || ty < 1 || tx > W || ty > H)
            return fail(c, EINCM_ERR_ARG, "CLAHE grid %d x %d (x splits the width) does not fit the %d x %d sensor", tx, ty, H, W);
        if (std::isnan(p->clahe_clip_limit) || std::isinf(p->clahe_clip_limit))
            return fail(c, EINCM_ERR_ARG, "clahe_clip_limit = %g must be finite", p->clahe_clip_limit);
    }
    double taps_d = 0.0;
    if (st & EINCM_PRE_UNSHARP) {
        if (!(p->sharpen_sigma > 0.0) || !std::isfinite(p->sharpen_sigma))
            return fail(c, EINCM_ERR_ARG, "sharpen_sigma = %g must be positive and finite", p->sharpen_sigma);
        if (!std::isfinite(p->sharpen_alpha) || !std::isfinite(p->sharpen_beta))
            return fail(c, EINCM_ERR_ARG, "sharpen weights %g, %g must be finite", p->sharpen_alpha, p->sharpen_beta);
        taps_d = std::nearbyint(p->sharpen_sigma * 3 * 2 + 1);
        if (taps_d > UNSHARP_MAX_TAPS)
            return fail(c, EINCM_ERR_UNSUPPORTED, "sharpen_sigma = %g needs %g taps (> %d)", p->sharpen_sigma, taps_d, UNSHARP_MAX_TAPS);
    }
    int bil_r = 0;
    double sc = 1.0, ss = 1.0;
    if (st & EINCM_PRE_BILATERAL) {
        if (!std::isfinite(p->bilateral_sigma_color) || !std::isfinite(p->bilateral_sigma_space))
            return fail(c, EINCM_ERR_ARG, "bilateral sigmas %g, %g must be finite", p->bilateral_sigma_color, p->bilateral_sigma_space);
        sc = p->bilateral_sigma_color <= 0 ? 1.0 : p->bilateral_sigma_color;
        ss = p->bilateral_sigma_space <= 0 ? 1.0 : p->bilateral_sigma_space;
        const double rd = p->bilateral_d > 0 ? (double)(p->bilateral_d / 2) : std::nearbyint(ss * 1.5);
        if (rd > BIL_MAX_RADIUS) return fail(c, EINCM_ERR_UNSUPPORTED, "bilateral radius %g (> %d)", rd, BIL_MAX_RADIUS);
        bil_r = std::max((int)rd, 1);
    }

    // ---- host tables (in h_pre_tab: unsharp taps, then bilateral colour weights, tap offsets and tap weights as float bits)
    std::vector<int32_t>& T = c->pre.h_pre_tab;
    T.clear();
    int un_r = 0, bil_n = 0;
    size_t off_cw = 0, off_ofs = 0, off_w = 0;
    if (st & EINCM_PRE_UNSHARP) {
        // cv::GaussianBlur, 8-bit: getGaussianKernelBitExact (fp64 here) and error-diffusion rounding to 8 fraction bits
        const double sigma = p->sharpen_sigma;
        const int taps = (int)taps_d | 1, half = taps / 2;
        const double scale2 = -0.125 / (sigma * sigma);
        std::vector<double> v((size_t)half);
        double sum = 0.0;
        for (int i = 0, x = 1 - taps; i < half; ++i, x += 2) { v[i] = std::exp((double)(x * x) * scale2); sum += v[i]; }
        const double mul = 1.0 / (sum * 2.0 + 1.0);
        T.assign((size_t)taps, 0);
        double err = 0.0;
        int acc = 0;
        for (int i = 0; i < half; ++i) {
            const double g = v[i] * mul;
            const double adj = g * 256.0 + err;
            const double v0 = std::nearbyint(adj);
            err = adj - v0;
            T[i] = T[taps - 1 - i] = (int32_t)v0;
            acc += (int32_t)v0;
        }
        T[half] = 256 - 2 * acc;
        un_r = half;
    }
    if (st & EINCM_PRE_BILATERAL) {
        const double cc = -0.5 / (sc * sc), sc2 = -0.5 / (ss * ss);
        off_cw = T.size();
        for (int i = 0; i < 256; ++i) { const float w = (float)std::exp(i * i * cc); int32_t b; std::memcpy(&b, &w, 4); T.push_back(b); }
        std::vector<int32_t> ofs;
        std::vector<int32_t> wts;
        for (int i = -bil_r; i <= bil_r; ++i)
            for (int j = -bil_r; j <= bil_r; ++j) {
                const double r = std::sqrt((double)i * i + (double)j * j);
                if (r > bil_r) continue;
                const float w = (float)std::exp(r * r * sc2);
                int32_t b; std::memcpy(&b, &w, 4);
                ofs.push_back(i); ofs.push_back(j); wts.push_back(b);
            }
        bil_n = (int)wts.size();
        off_ofs = T.size(); T.insert(T.end(), ofs.begin(), ofs.end());
        off_w = T.size(); T.insert(T.end(), wts.begin(), wts.end());
    }
    int clahe_th = 0, clahe_tw = 0, clahe_limit = 0;
    if (st & EINCM_PRE_CLAHE) {
        // OpenCV pads bottom and right by a full remainder-to-tile unless both sides divide
        const bool divides = W % tx == 0 && H % ty == 0;
        const int Hp = divides ? H : H + ty - H % ty, Wp = divides ? W : W + tx - W % tx;
        clahe_th = Hp / ty; clahe_tw = Wp / tx;
        const int total = clahe_th * clahe_tw;
        if (p->clahe_clip_limit > 0.0) {
            const double l = p->clahe_clip_limit * total / CLAHE_BINS;
            clahe_limit = l >= total ? total : std::max((int)l, 1);
        }
    }

    const size_t npix = (size_t)H * W, tot = npix * n;
    // two uint8 stacks, and per stage: the per-call tables, the CLAHE LUTs, the unsharp mask's row pass
    OneShot op(c);
    const OneShot::Piece<uint8_t> img[2] = {op.piece<uint8_t>(tot), op.piece<uint8_t>(tot)};
    const auto d_tab = op.piece<int32_t>(T.size());
    const auto lut = op.piece<uint8_t>((size_t)n * tx * ty * CLAHE_BINS, (st & EINCM_PRE_CLAHE) != 0);
    const auto rows = op.piece<uint16_t>(tot, (st & EINCM_PRE_UNSHARP) != 0);
    HIPCHK(c, op.begin());
    if (!T.empty()) HIPCHK(c, op.up(d_tab, T.data(), T.size() * 4));        // (host memory: the context's, as the NL-means table)
    if (st & EINCM_PRE_NLMEANS) {
        const float hf = (float)p->denoise_h;
        const float hh = hf * hf;
        if (c->pre.nlm_tw != tw || c->pre.nlm_sw != sw || c->pre.nlm_hh != hh) {
            // fastNlMeansDenoising's almost_dist2weight: fixed-point weights indexed by the template distance >> shift
            const int s = nlm_shift(tw);
            const int fpm = INT32_MAX / (sw * sw * 255);
            const double mult = (double)(1 << s) / (tw * tw);
            const int size = (int)(65025 / mult + 1);
            std::vector<int32_t>& N = c->pre.h_nlm_tab;
            N.assign((size_t)size, 0);
            for (int a = 0; a < size; ++a) {
                const double dist = a * mult;
                const double w = std::exp(-dist / (double)hh);
                const double wi = std::nearbyint(fpm * w);
                N[a] = wi < 0.001 * fpm ? 0 : (int32_t)wi;
            }
            c->pre.nlm_tw = 0;                               // invalid until the upload is queued
            HIPCHK(c, ensure(c, c->pre.p_nlm, N.size()));
            HIPCHK(c, op.up(c->pre.p_nlm.p, N.data(), N.size() * 4));
            c->pre.nlm_tw = tw; c->pre.nlm_sw = sw; c->pre.nlm_hh = hh;
        }
    }

    int cur = 0;
    HIPCHK(c, op.up(img[0], src, tot));                                      // (the caller's, as dst)
    const dim3 rows_grid((W + NT - 1) / NT, H, n);
    if (st & EINCM_PRE_NLMEANS) {
        const int b = sw / 2 + tw / 2;
        const size_t lds = (size_t)(NLM_TH + 2 * b) * (NLM_TW + 2 * b) * 4;
        const dim3 grid((W + NLM_TW - 1) / NLM_TW, (H + NLM_TH - 1) / NLM_TH, n);
        static_assert(NLM_MAX_TEMPLATE == 7, "one k_nlm per odd template window");
        decltype(&k_nlm<1>) const k[] = {k_nlm<1>, k_nlm<3>, k_nlm<5>, k_nlm<7>};
        HIPCHK(c, op.launch(k[tw / 2], grid, dim3(NT), lds, H, W, sw / 2, c->pre.p_nlm.p, img[cur], img[cur ^ 1]));
        cur ^= 1;
    }
    if (st & EINCM_PRE_CLAHE) {
        HIPCHK(c, op.launch(k_clahe_lut, dim3(tx, ty, n), dim3(NT), 0, H, W, clahe_th, clahe_tw, clahe_limit, img[cur], lut));
        HIPCHK(c, op.launch(k_clahe_interp, rows_grid, dim3(NT), 0, H, W, clahe_th, clahe_tw, tx, ty, lut, img[cur], img[cur ^ 1]));
        cur ^= 1;
    }
    if (st & EINCM_PRE_UNSHARP) {
        HIPCHK(c, op.launch(k_unsharp_rows, rows_grid, dim3(NT), 0, H, W, un_r, d_tab, img[cur], rows));
        HIPCHK(c, op.launch(k_unsharp_cols, rows_grid, dim3(NT), 0, H, W, un_r, d_tab, p->sharpen_alpha, p->sharpen_beta, rows, img[cur],
                            img[cur ^ 1]));
        cur ^= 1;
    }
    if (st & EINCM_PRE_BILATERAL) {
        const size_t lds = (size_t)(BIL_TH + 2 * bil_r) * (BIL_TW + 2 * bil_r) * 4;
        const dim3 grid((W + BIL_TW - 1) / BIL_TW, (H + BIL_TH - 1) / BIL_TH, n);
        HIPCHK(c, op.launch(k_bilateral, grid, dim3(NT), lds, H, W, bil_r, bil_n, d_tab + off_ofs,
                            reinterpret_cast<const float*>(d_tab + off_w), reinterpret_cast<const float*>(d_tab + off_cw), img[cur],
                            img[cur ^ 1]));
        cur ^= 1;
    }
    HIPCHK(c, op.down(dst, img[cur], tot));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// estimate_gt_flow (mvsec_loader.py:322-433) for a batch of windows: the frames and the step lists go up once, k_gt_flow walks every
// (pixel, window), the (n_windows, H, W, 2) result comes down.
int eincm_gt_flow(eincm_ctx* c, const void* gt_x, const void* gt_y, int elem_bytes, int n_frames, int n_windows, const int32_t* mode,
                  const int32_t* step_off, const int32_t* step_frame, const double* step_num, const double* step_den, double* out) {
    if (!c) return EINCM_ERR_ARG;
    if (!gt_x || !gt_y || !mode || !step_off || !step_frame || !step_num || !step_den || !out)
        return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n_frames < 1 || n_windows < 1) return fail(c, EINCM_ERR_ARG, "n_frames = %d, n_windows = %d (both >= 1)", n_frames, n_windows);
    if (elem_bytes != 4 && elem_bytes != 8) return fail(c, EINCM_ERR_ARG, "elem_bytes = %d (4: float, 8: double)", elem_bytes);
    if (step_off[0] != 0) return fail(c, EINCM_ERR_ARG, "step_off[0] = %d (must be 0)", step_off[0]);
    for (int b = 0; b < n_windows; ++b) {
        const int s0 = step_off[b], s1 = step_off[b + 1];
        if (mode[b] != EINCM_GTF_DIRECT && mode[b] != EINCM_GTF_PROPAGATE) return fail(c, EINCM_ERR_ARG, "window %d: mode %d unknown", b, mode[b]);
        if (s1 <= s0) return fail(c, EINCM_ERR_ARG, "window %d has no steps", b);
        if (mode[b] == EINCM_GTF_DIRECT && s1 - s0 != 1) return fail(c, EINCM_ERR_ARG, "window %d: a direct window has %d steps (1)", b, s1 - s0);
        for (int k = s0; k < s1; ++k) {
            if (step_frame[k] < 0 || step_frame[k] >= n_frames)
                return fail(c, EINCM_ERR_ARG, "window %d step %d: frame %d outside [0, %d)", b, k - s0, step_frame[k], n_frames);
            if (!std::isfinite(step_num[k])) return fail(c, EINCM_ERR_ARG, "window %d step %d: scale %g is not finite", b, k - s0, step_num[k]);
            if (mode[b] == EINCM_GTF_DIRECT && (!(step_den[k] != 0.0) || !std::isfinite(step_den[k])))
                return fail(c, EINCM_ERR_ARG, "window %d: den %g must be finite and non-zero", b, step_den[k]);
        }
    }
    const int H = c->H, W = c->W;
    const size_t npix = (size_t)H * W, stack = (size_t)n_frames * npix * elem_bytes, n_steps = (size_t)step_off[n_windows];
    Packer tab;      // one upload for the step lists: mode | step_off | step_frame | (8-byte aligned) step_num | step_den
    tab.add(mode, (size_t)n_windows * 4);
    const size_t o_off = tab.add(step_off, ((size_t)n_windows + 1) * 4), o_frame = tab.add(step_frame, n_steps * 4);
    const size_t o_num = tab.add(step_num, n_steps * 8, 8), o_den = tab.add(step_den, n_steps * 8);
    OneShot op(c);                                        // the x and y frame stacks, the step lists, the output
    const auto d_frames = op.piece<char>(2 * stack), d_tab = op.piece<char>(tab.buf.size());
    const auto d_out = op.piece<double>((size_t)n_windows * npix * 2);
    HIPCHK(c, op.begin());
    const void* const d_x = d_frames;                     // (launch casts them to the kernel's element type)
    const void* const d_y = d_frames + stack;
    HIPCHK(c, op.up(d_frames, gt_x, stack));              // (host memory: the caller's, as out)
    HIPCHK(c, op.up(d_frames + stack, gt_y, stack));
    HIPCHK(c, op.up(d_tab, tab.buf.data(), tab.buf.size()));     // (tab, a local older than the frame)
    const unsigned gx = (unsigned)((npix + NT - 1) / NT);
    for (int w0 = 0; w0 < n_windows; w0 += GTF_MAX_WINDOWS_PER_LAUNCH) {
        const dim3 grid(gx, (unsigned)std::min(n_windows - w0, GTF_MAX_WINDOWS_PER_LAUNCH));
        if (elem_bytes == 4)
            HIPCHK(c, op.launch(k_gt_flow<float>, grid, dim3(NT), 0, H, W, w0, d_x, d_y, tab.i32(d_tab, 0), tab.i32(d_tab, o_off),
                                tab.i32(d_tab, o_frame), tab.f64(d_tab, o_num), tab.f64(d_tab, o_den), d_out));
        else
            HIPCHK(c, op.launch(k_gt_flow<double>, grid, dim3(NT), 0, H, W, w0, d_x, d_y, tab.i32(d_tab, 0), tab.i32(d_tab, o_off),
                                tab.i32(d_tab, o_frame), tab.f64(d_tab, o_num), tab.f64(d_tab, o_den), d_out));
    }
    HIPCHK(c, op.down(out, d_out, (size_t)n_windows * npix * 16));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// DSECDataLoader.rectify_events (dsec_loader.py:145-171) for one chunk of a recording.
int eincm_rectify_events(eincm_ctx* c, const float* rectify_map, const int16_t* x, const int16_t* y, int64_t n, int16_t* rec_x,
                         int16_t* rec_y, uint8_t* keep, int64_t* n_kept) {
    if (!c) return EINCM_ERR_ARG;
    if (!n_kept) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 0 || n > (int64_t)1 << 30) return fail(c, EINCM_ERR_ARG, "n = %lld outside [0, 2^30] (walk a recording in chunks)", (long long)n);
    if (n > 0 && (!x || !y || !rec_x || !rec_y || !keep)) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!rectify_map && !c->rect.rect_map_set) return fail(c, EINCM_ERR_STATE, "no rectify map: the first call must hand one over");
    const int H = c->H, W = c->W;
    const int64_t npix = (int64_t)H * W;
    // both phases are laid out before the block is grown, so it cannot move between them: the counters and, where a map comes along,
    // its float staging; then the chunk's coordinates in and out, the keep bytes, the block counts and offsets
    const int64_t nblk = (n + RECT_BLOCK - 1) / RECT_BLOCK;
    OneShot op(c);
    const auto d_cnt = op.piece<unsigned long long>(4);               // [0] refused map entries, [1] events outside the sensor, [2] kept
    const auto d_fmap = op.piece<float2>((size_t)npix, rectify_map != nullptr);
    const auto d_x = op.piece<int16_t>((size_t)n), d_y = op.piece<int16_t>((size_t)n);
    const auto d_rx = op.piece<int16_t>((size_t)n), d_ry = op.piece<int16_t>((size_t)n);
    const auto d_keep = op.piece<uint8_t>((size_t)n);
    const auto d_bcnt = op.piece<uint32_t>((size_t)nblk);
    const auto d_boff = op.piece<int64_t>((size_t)nblk);
    unsigned long long* h_cnt = op.host_buf<unsigned long long>(4);   // d_cnt comes down here, in either phase
    if (rectify_map) c->rect.rect_map_set = false;
    HIPCHK(c, op.begin());
    HIPCHK(c, op.zero(d_cnt, 4 * sizeof(unsigned long long)));
    if (rectify_map) {
        HIPCHK(c, ensure(c, c->rect.r_map, (size_t)npix));
        HIPCHK(c, op.up(d_fmap, rectify_map, (size_t)npix * 8));      // (host memory: the caller's, as every copy below but h_cnt's)
        HIPCHK(c, op.launch(k_rect_map, dim3((unsigned)((npix + NT - 1) / NT)), dim3(NT), 0, npix, d_fmap, c->rect.r_map.p, d_cnt));
        HIPCHK(c, op.down(h_cnt, d_cnt, sizeof(unsigned long long)));
        HIPCHK(c, op.sync());
        if (h_cnt[0]) return fail(c, EINCM_ERR_ARG, "rectify map: %llu of %lld entries are not finite or do not round into int16", h_cnt[0], (long long)npix);
        c->rect.rect_map_set = true;
    }
    *n_kept = 0;
    if (n == 0) { HIPCHK(c, op.sync()); return EINCM_OK; }
    const uint32_t* d_map = c->rect.r_map.p;
    HIPCHK(c, op.up(d_x, x, (size_t)n * 2));
    HIPCHK(c, op.up(d_y, y, (size_t)n * 2));
    HIPCHK(c, op.launch(k_rect_count, dim3((unsigned)nblk), dim3(NT), 0, H, W, n, d_x, d_y, d_map, d_keep, d_bcnt, d_cnt + 1));
    HIPCHK(c, op.launch(k_rect_scan, dim3(1), dim3(RECT_SCAN_NT), 0, nblk, d_bcnt, d_boff, reinterpret_cast<int64_t*>(d_cnt + 2)));
    HIPCHK(c, op.launch(k_rect_scatter, dim3((unsigned)nblk), dim3(NT), 0, H, W, n, d_x, d_y, d_map, d_boff, d_rx, d_ry));
    HIPCHK(c, op.down(h_cnt, d_cnt, 4 * sizeof(unsigned long long)));
    HIPCHK(c, op.sync());
    if (h_cnt[1]) return fail(c, EINCM_ERR_ARG, "%llu of %lld events have a coordinate outside the %dx%d sensor", h_cnt[1], (long long)n, H, W);
    const int64_t kept = (int64_t)h_cnt[2];
    if (kept < 0 || kept > n) return fail(c, EINCM_ERR_HIP, "kept count %lld of %lld events", (long long)kept, (long long)n);
    HIPCHK(c, op.down(keep, d_keep, (size_t)n));
    if (kept) {                                     // only the kept prefix comes back
        HIPCHK(c, op.down(rec_x, d_rx, (size_t)kept * 2));
        HIPCHK(c, op.down(rec_y, d_ry, (size_t)kept * 2));
    }
    HIPCHK(c, op.sync());
    *n_kept = kept;
    return EINCM_OK;
}

// The spatiotemporal support filter for one chunk of a stream (eincm_event_support.hip.h): the front end
// validates, sorts the event indices by pixel and bounds the runs; then search every neighbour's run, update the carried map.  A
// refused chunk leaves the carried state as it was: validate() returns before carried_maps() is reached.
int eincm_event_support(eincm_ctx* c, const int16_t* x, const int16_t* y, const double* t, int64_t n, double tau, int radius,
                        int full_support, const uint8_t* pixel_mask, int reset, float* weights, uint8_t* support) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = not_in_flight(c, "eincm_event_support")) return rc;
    switch (es_check_args(n, tau, radius, full_support)) {
        case ES_ARG_N: return StreamChunk::bad_n(c, n);
        case ES_ARG_TAU: return StreamChunk::bad_tau(c, tau);
        case ES_ARG_RADIUS: return fail(c, EINCM_ERR_ARG, "radius = %d outside [1, %d]", radius, ES_MAX_RADIUS);
        case ES_ARG_FULL_SUPPORT:
            return fail(c, EINCM_ERR_ARG, "full_support = %d outside [1, %d] for radius %d", full_support, es_max_support(radius), radius);
        case ES_ARG_OK: break;
    }
    if (n > 0 && (!x || !y || !t || !weights)) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    OneShot op(c);
    StreamChunk sc(op, x, y, t, n, pixel_mask);
    const auto d_w = op.piece<float>((size_t)n);
    const auto d_s = op.piece<uint8_t>((size_t)n);
    HIPCHK(c, op.begin());
    if (const int rc = sc.validate(reset ? es_no_event() : c->es.last_time)) return rc;
    if (const int rc = sc.carried_maps(c->es.last_t, (size_t)sc.npix, reset, c->es.last_time)) return rc;
    if (n == 0) { HIPCHK(c, op.sync()); return EINCM_OK; }
    if (const int rc = sc.sort_and_bound()) return rc;
    HIPCHK(c, op.launch(k_es_support, dim3(sc.gn), dim3(NT), 0, sc.H, sc.W, n, sc.d_x, sc.d_y, sc.d_t, tau, radius, full_support, sc.d_mask,
                        sc.lo(), sc.hi(), sc.idx(), c->es.last_t.p, d_w, d_s));
    HIPCHK(c, op.launch(k_es_map, dim3(sc.gp), dim3(NT), 0, sc.npix, n, sc.lo(), sc.hi(), sc.idx(), sc.d_t, c->es.last_t.p));
    HIPCHK(c, op.down(weights, d_w, (size_t)n * sizeof(float)));
    if (support) HIPCHK(c, op.down(support, d_s, (size_t)n));
    HIPCHK(c, op.sync());
    c->es.last_time = t[n - 1];
    return EINCM_OK;
}

// The refractory and polarity-aware filter for one chunk of a stream (eincm_event_filter.hip.h): the same
// front end; then decide per sorted position which events survive, max-scan the survivors' positions, count every kept event's
// neighbours from kept events alone, update the three carried maps.  A refused chunk leaves the carried state as it was.
int eincm_event_filter(eincm_ctx* c, const int16_t* x, const int16_t* y, const double* t, const int8_t* p, int64_t n, double refractory,
                       double tau, int radius, int full_support, int flags, const uint8_t* pixel_mask, int reset, uint8_t* keep,
                       float* weights, uint8_t* support) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = not_in_flight(c, "eincm_event_filter")) return rc;
    switch (ef_check_args(n, refractory, tau, radius, full_support, flags, p != nullptr)) {
        case EF_ARG_N: return StreamChunk::bad_n(c, n);
        case EF_ARG_REFRACTORY: return fail(c, EINCM_ERR_ARG, "refractory = %g (finite and >= 0)", refractory);
        case EF_ARG_TAU: return StreamChunk::bad_tau(c, tau);
        case EF_ARG_RADIUS: return fail(c, EINCM_ERR_ARG, "radius = %d outside [0, %d]", radius, ES_MAX_RADIUS);
        case EF_ARG_FULL_SUPPORT:
            return fail(c, EINCM_ERR_ARG, "full_support = %d outside [1, %d] for radius %d", full_support,
                        radius == 0 ? 1 : es_max_support(radius), radius);
        case EF_ARG_FLAGS:
            return fail(c, EINCM_ERR_ARG, "flags = %d (%s)", flags,
                        (flags & ~EF_KNOWN_FLAGS) ? "EINCM_EF_POLARITY is the only flag" : "EINCM_EF_POLARITY needs p");
        case EF_ARG_OK: break;
    }
    if (n > 0 && (!x || !y || !t || !keep || !weights)) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    OneShot op(c);
    StreamChunk sc(op, x, y, t, n, pixel_mask);
    const auto d_p = op.piece<int8_t>((size_t)n, p != nullptr);
    const auto d_m = op.piece<uint2>((size_t)n);                         // the scan seeds, then the scan
    const size_t nmt = ((size_t)n + EF_SCAN_TILE - 1) / EF_SCAN_TILE;
    const auto d_mt = op.piece<uint2>(nmt);
    const auto d_k = op.piece<uint8_t>((size_t)n);
    const auto d_w = op.piece<float>((size_t)n);
    const auto d_s = op.piece<uint8_t>((size_t)n);
    HIPCHK(c, op.begin());
    if (const int rc = sc.validate(reset ? es_no_event() : c->ef.last_time)) return rc;
    if (const int rc = sc.carried_maps(c->ef.maps, (size_t)sc.npix * 3, reset, c->ef.last_time)) return rc;
    if (n == 0) { HIPCHK(c, op.sync()); return EINCM_OK; }
    double* const last_any = c->ef.maps.p;
    double* const kept0 = last_any + sc.npix;
    double* const kept1 = kept0 + sc.npix;
    if (p) HIPCHK(c, op.up(d_p, p, (size_t)n));
    if (const int rc = sc.sort_and_bound()) return rc;
    HIPCHK(c, op.launch(k_ef_keep, dim3(sc.gn), dim3(NT), 0, n, sc.key(), sc.idx(), sc.lo(), sc.d_t, d_p, refractory, sc.d_mask, last_any,
                        d_k, d_m));
    HIPCHK(c, op.launch(k_ef_scan_tiles, dim3((unsigned)nmt), dim3(EF_SCAN_NT), 0, n, d_m, d_mt));
    HIPCHK(c, op.launch(k_ef_scan, dim3(1), dim3(EF_SCAN_NT), 0, (int64_t)nmt, d_mt));
    HIPCHK(c, op.launch(k_ef_support, dim3(sc.gn), dim3(NT), 0, sc.H, sc.W, n, sc.d_x, sc.d_y, sc.d_t, d_p, tau, radius, full_support,
                        (flags & EF_POLARITY) ? 1 : 0, sc.d_mask, sc.lo(), sc.hi(), sc.idx(), d_m, d_mt, d_k, kept0, kept1, d_w, d_s));
    HIPCHK(c, op.launch(k_ef_map, dim3(sc.gp), dim3(NT), 0, sc.npix, n, sc.lo(), sc.hi(), sc.idx(), d_m, d_mt, sc.d_t, last_any, kept0, kept1));
    HIPCHK(c, op.down(keep, d_k, (size_t)n));
    HIPCHK(c, op.down(weights, d_w, (size_t)n * sizeof(float)));
    if (support) HIPCHK(c, op.down(support, d_s, (size_t)n));
    HIPCHK(c, op.sync());
    c->ef.last_time = t[n - 1];
    return EINCM_OK;
}

// cv.remap(img, map, None, INTER_CUBIC) for a stack of 8-bit images under the contract of DESIGN.md section 16.
int eincm_remap_cubic(eincm_ctx* c, const uint8_t* src, int n, int src_h, int src_w, const float* map, const int32_t* table, uint8_t* dst) {
    if (!c) return EINCM_ERR_ARG;
    if (!src || !map || !table || !dst) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1 || src_h < 1 || src_w < 1 || src_h > 32766 || src_w > 32766)
        return fail(c, EINCM_ERR_ARG, "n = %d images of %dx%d (n >= 1, 1 <= size <= 32766)", n, src_h, src_w);
    for (int r = 0; r < 1024; ++r) {
        int64_t s = 0;
        for (int k = 0; k < 16; ++k) { const int32_t w = table[r * 16 + k]; if (w < -32768 || w > 32768) s = INT64_MIN / 2; s += w; }
        if (s != 32768) return fail(c, EINCM_ERR_ARG, "weight table row %d: weights within +-32768 that sum to 32768", r);
    }
    const int64_t npix = (int64_t)c->H * c->W;
    const size_t sbytes = (size_t)n * src_h * src_w, dbytes = (size_t)n * npix;
    OneShot op(c);             // (the float map is only staged here: the rounded rectify map lives in r_map and stays)
    const auto d_in = op.piece<uint8_t>(sbytes), d_out = op.piece<uint8_t>(dbytes);
    const auto d_map = op.piece<float2>((size_t)npix);
    const auto d_tab = op.piece<int32_t>(1024 * 16);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.up(d_in, src, sbytes));                              // (host memory: the caller's, all four)
    HIPCHK(c, op.up(d_map, map, (size_t)npix * 8));
    HIPCHK(c, op.up(d_tab, table, 1024 * 16 * 4));
    HIPCHK(c, op.launch(k_remap_cubic, dim3((unsigned)((npix + NT - 1) / NT)), dim3(NT), 0, n, src_h, src_w, npix, d_in, d_map, d_tab, d_out));
    HIPCHK(c, op.down(dst, d_out, dbytes));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// DSECDataLoader.flow_16bit_to_float (dsec_loader.py:247-266) for a stack of n flow images.
int eincm_flow_decode(eincm_ctx* c, const uint16_t* flow16, int n, double* flow, uint8_t* valid, int64_t* n_bad) {
    if (!c) return EINCM_ERR_ARG;
    if (!flow16 || !flow || !valid || !n_bad) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1) return fail(c, EINCM_ERR_ARG, "n = %d (>= 1)", n);
    const int64_t tot = (int64_t)n * c->H * c->W;
    OneShot op(c);
    const auto d_in = op.piece<uint16_t>((size_t)tot * 3);
    const auto d_flow = op.piece<double>((size_t)tot * 2);
    const auto d_valid = op.piece<uint8_t>((size_t)tot);
    const auto d_cnt = op.piece<unsigned long long>(1);
    unsigned long long* bad = op.host_buf<unsigned long long>(1);     // d_cnt comes down here
    HIPCHK(c, op.begin());
    HIPCHK(c, op.zero(d_cnt, sizeof(unsigned long long)));
    HIPCHK(c, op.up(d_in, flow16, (size_t)tot * 6));                  // (host memory: the caller's, as flow and valid)
    HIPCHK(c, op.launch(k_flow_decode, dim3((unsigned)((tot + NT - 1) / NT)), dim3(NT), 0, tot, d_in, d_flow, d_valid, d_cnt));
    HIPCHK(c, op.down(bad, d_cnt, sizeof *bad));
    HIPCHK(c, op.down(flow, d_flow, (size_t)tot * 16));
    HIPCHK(c, op.down(valid, d_valid, (size_t)tot));
    HIPCHK(c, op.sync());
    *n_bad = (int64_t)*bad;
    if (*bad) return fail(c, EINCM_ERR_ARG, "%llu pixels have a third channel that is neither 0 nor 1", *bad);
    return EINCM_OK;
}

// dsec_npz_to_png.py:84-96 for a batch of theta: bilinear scale_and_translate to the sensor and the 16-bit code, in one kernel.
int eincm_flow_encode(eincm_ctx* c, const double* theta, int n, int h, int w, const uint8_t* valid, uint16_t* out, int64_t* n_bad) {
    if (!c) return EINCM_ERR_ARG;
    if (!theta || !out || !n_bad) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n < 1 || n > 65535 || h < 1 || w < 1 || h > 32767 || w > 32767) return fail(c, EINCM_ERR_ARG, "n = %d theta of %dx%d (1 <= n <= 65535)", n, h, w);
    const int H = c->H, W = c->W;
    const int64_t npix = (int64_t)H * W;
    TapTables T;
    build_taps(h, w, H, W, EINCM_METHOD_BILINEAR, T);
    const Packer& tab = T.tab;
    const size_t thbytes = (size_t)n * h * w * 16, vbytes = valid ? (size_t)n * npix : 0, vofs = (thbytes + 15) & ~(size_t)15;
    OneShot op(c);
    const auto d_in = op.piece<char>(vofs + vbytes);                  // theta | (16-byte aligned) valid
    const auto d_out = op.piece<uint16_t>((size_t)n * npix * 3);
    const auto d_tab = op.piece<char>(tab.buf.size());
    const auto d_cnt = op.piece<unsigned long long>(1);
    unsigned long long* bad = op.host_buf<unsigned long long>(1);     // d_cnt comes down here
    HIPCHK(c, op.begin());
    const void* const d_theta = d_in;                                 // (launch casts them to the kernel's types)
    const void* const d_valid = valid ? d_in + vofs : nullptr;
    HIPCHK(c, op.zero(d_cnt, sizeof(unsigned long long)));
    HIPCHK(c, op.up(d_in, theta, thbytes));                           // (host memory: the caller's, as valid and out)
    if (valid) HIPCHK(c, op.up(d_in + vofs, valid, vbytes));
    HIPCHK(c, op.up(d_tab, tab.buf.data(), tab.buf.size()));          // (T, a local older than the frame)
    HIPCHK(c, op.launch(k_flow_encode, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)n), dim3(NT), 0, H, W, h, w, d_theta,
                        tab.i32(d_tab, T.o_rlo), tab.i32(d_tab, T.o_rcnt), tab.f64(d_tab, 0), T.rstride, tab.i32(d_tab, T.o_clo),
                        tab.i32(d_tab, T.o_ccnt), tab.f64(d_tab, T.o_cw), T.cstride, d_valid, d_out, d_cnt));
    HIPCHK(c, op.down(bad, d_cnt, sizeof *bad));
    HIPCHK(c, op.down(out, d_out, (size_t)n * npix * 6));
    HIPCHK(c, op.sync());
    *n_bad = (int64_t)*bad;
    if (*bad) return fail(c, EINCM_ERR_ARG, "%llu pixels have a flow that is not finite or encodes outside [0, 65536)", *bad);
    return EINCM_OK;
}

// ---- a solved theta carried along its own flow to the next window (eincm_theta_advect.hip.h) ----
// The checks, their order and the fixed-point scales are eincm_theta_advect.h's.  Everything is a piece of the shared scratch; a piece
// that is not wanted (the difference image and the column sums for a dense theta, the dense field, the coverage) takes none of it.
int eincm_theta_advect(eincm_ctx* c, const double* theta, int n, int h, int w, int method, const double* tau, const double* gain, int fill,
                       double min_coverage, double* out_theta, double* out_dense, float* out_coverage) {
    if (!c) return EINCM_ERR_ARG;
    const int H = c->H, W = c->W;
    const TaArgs args{theta != nullptr, tau != nullptr, gain != nullptr, out_theta != nullptr, n, h, w, H, W, method, fill, tau, gain, min_coverage};
    if (const TaFault f = ta_check(args))
        return fail(c, ta_code(f), "eincm_theta_advect: %s (n = %d, theta %dx%d, sensor %dx%d, method %d, fill %d, min_coverage %g)", ta_why(f), n, h,
                    w, H, W, method, fill, min_coverage);
    if (const int rc = not_in_flight(c, "eincm_theta_advect")) return rc;
    const bool full = h == H && w == W;
    TapTables up, dn;                                     // (h, w) -> (H, W) of the expansion; (H, W) -> (h, w) of the reduction
    if (!full) { build_taps(h, w, H, W, method, up); build_taps(H, W, h, w, method, dn); }
    if (!ta_range_ok(theta, (size_t)n * h * w * 2, full ? 1.0 : ta_tap_gain(up, H, W)))
        return fail(c, ta_code(TA_RANGE), "eincm_theta_advect: %s", ta_why(TA_RANGE));
    const size_t npix = (size_t)H * W, plane = (size_t)n * npix, cells = (size_t)n * h * w;
    std::vector<double> tg((size_t)2 * n);                // tau | gain: one upload
    std::copy(tau, tau + n, tg.begin());
    std::copy(gain, gain + n, tg.begin() + n);
    OneShot op(c);
    const auto d_th = op.piece<double2>(cells);
    const auto d_tg = op.piece<double>(tg.size());
    const auto d_up = op.piece<char>(up.tab.buf.size(), !full), d_dn = op.piece<char>(dn.tab.buf.size(), !full);
    const auto d_acc = op.piece<int64_t>(plane * 3);
    const auto d_D = op.piece<double2>(plane, !full);
    const auto d_S = op.piece<double2>((size_t)n * H * w, !full);
    const auto d_dense = op.piece<double2>(plane, out_dense != nullptr);
    const auto d_cov = op.piece<float>(plane, out_coverage != nullptr);
    const auto d_out = op.piece<double2>(cells);
    HIPCHK(c, op.begin());
    HIPCHK(c, op.zero(d_acc, plane * 3 * sizeof(int64_t)));
    HIPCHK(c, op.up(d_th, theta, cells * 16));            // (host memory: the caller's, as the three outputs)
    HIPCHK(c, op.up(d_tg, tg.data(), tg.size() * 8));     // (tg, up and dn: locals older than the frame)
    TaTaps taps{};
    if (!full) {
        HIPCHK(c, op.up(d_up, up.tab.buf.data(), up.tab.buf.size()));
        HIPCHK(c, op.up(d_dn, dn.tab.buf.data(), dn.tab.buf.size()));
        const char* const t = d_up;
        taps = TaTaps{Packer::i32(t, up.o_rlo), Packer::i32(t, up.o_rcnt), Packer::f64(t, 0), up.rstride,
                      Packer::i32(t, up.o_clo), Packer::i32(t, up.o_ccnt), Packer::f64(t, up.o_cw), up.cstride};
    }
    const double* const d_tau = d_tg;
    const double* const d_gain = d_tau + n;
    const dim3 pix((unsigned)((npix + NT - 1) / NT), (unsigned)n);
    HIPCHK(c, op.launch(k_ta_splat, pix, dim3(NT), 0, H, W, h, w, full ? 1 : 0, d_th, taps, d_tau, d_acc));
    HIPCHK(c, op.launch(k_ta_resolve, pix, dim3(NT), 0, H, W, h, w, full ? 1 : 0, d_th, taps, d_gain, d_acc, fill == EINCM_TA_FILL_ZERO ? 1 : 0,
                        min_coverage, d_D, d_dense, d_cov, full ? (double2*)d_out : nullptr));
    if (!full) {
        const char* const t = d_dn;
        HIPCHK(c, op.launch(k_ta_reduce_cols, dim3((unsigned)(((size_t)H * w + NT - 1) / NT), (unsigned)n), dim3(NT), 0, H, W, w, d_D,
                            Packer::i32(t, dn.o_clo), Packer::i32(t, dn.o_ccnt), Packer::f64(t, dn.o_cw), dn.cstride, d_S));
        HIPCHK(c, op.launch(k_ta_reduce_rows, dim3((unsigned)(((size_t)h * w + NT - 1) / NT), (unsigned)n), dim3(NT), 0, H, h, w, d_S,
                            Packer::i32(t, dn.o_rlo), Packer::i32(t, dn.o_rcnt), Packer::f64(t, 0), dn.rstride, d_th, d_gain, d_out));
    }
    HIPCHK(c, op.down(out_theta, d_out, cells * 16));
    if (out_dense) HIPCHK(c, op.down(out_dense, d_dense, plane * 16));
    if (out_coverage) HIPCHK(c, op.down(out_coverage, d_cov, plane * 4));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

// ---- flow errors of a batch of thetas against staged ground truth (eincm_floweval.hip.h) ----
// Stage once: the GT flow goes straight into the context's f_eval block, the evaluation events mark their pixels, k_fe_flags folds the
// event plane, the optional error mask and the GT mask into one flag byte per pixel.  The events, the mask and the counters are
// transients of the shared scratch.
int eincm_flow_eval_stage(eincm_ctx* c, int n_windows, const double* gt_flow, const int64_t* n_events, const int16_t* xs, const int16_t* ys,
                          const uint8_t* eval_mask) {
    if (!c) return EINCM_ERR_ARG;
    if (!gt_flow || !n_events || !xs || !ys) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (n_windows < 1 || n_windows > 65535) return fail(c, EINCM_ERR_ARG, "n_windows = %d (1..65535)", n_windows);
    int64_t tot = 0, most = 0;
    for (int b = 0; b < n_windows; ++b) {
        if (n_events[b] < 0 || n_events[b] > (int64_t)1 << 36) return fail(c, EINCM_ERR_ARG, "window %d: n_events = %lld", b, (long long)n_events[b]);
        tot += n_events[b];
        most = std::max(most, n_events[b]);
    }
    if (const int rc = not_in_flight(c, "eincm_flow_eval_stage")) return rc;
    const int H = c->H, W = c->W, n = n_windows;
    const size_t npix = (size_t)H * W, plane = (size_t)n * npix;
    c->fe.fe_n = 0;                                       // whatever was staged is gone from here on
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int b = 0; b < n; ++b) off[b + 1] = off[b] + n_events[b];
    OneShot op(c);
    const auto d_off = op.piece<int64_t>(off.size());
    const auto d_x = op.piece<int16_t>((size_t)tot), d_y = op.piece<int16_t>((size_t)tot);
    const auto d_mask = op.piece<uint8_t>(plane, eval_mask != nullptr);
    const auto d_cnt = op.piece<unsigned long long>((size_t)n + 1);   // [n] GT-valid pixels per window | [1] events outside the sensor
    unsigned long long* cnt = op.host_buf<unsigned long long>((size_t)n + 1);   // d_cnt comes down here
    HIPCHK(c, op.begin());
    HIPCHK(c, ensure(c, c->fe.f_eval, plane * 17));
    double2* d_gt = reinterpret_cast<double2*>(c->fe.f_eval.p);
    uint8_t* d_flags = reinterpret_cast<uint8_t*>(c->fe.f_eval.p + plane * 16);
    HIPCHK(c, op.zero(d_cnt, ((size_t)n + 1) * 8));
    HIPCHK(c, op.zero(d_flags, plane));
    HIPCHK(c, op.up(d_gt, gt_flow, plane * 16));          // (host memory: the caller's, as eval_mask, xs and ys)
    if (eval_mask) HIPCHK(c, op.up(d_mask, eval_mask, plane));
    if (tot > 0) {
        HIPCHK(c, op.up(d_off, off.data(), off.size() * 8));          // (off, a local older than the frame)
        HIPCHK(c, op.up(d_x, xs, (size_t)tot * 2));
        HIPCHK(c, op.up(d_y, ys, (size_t)tot * 2));
        HIPCHK(c, op.launch(k_fe_events, dim3((unsigned)((most + NT - 1) / NT), (unsigned)n), dim3(NT), 0, H, W, d_off, d_x, d_y, d_flags,
                            d_cnt + n));
    }
    HIPCHK(c, op.launch(k_fe_flags, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)n), dim3(NT), 0, npix, d_gt, d_mask, d_flags, d_cnt));
    HIPCHK(c, op.down(cnt, d_cnt, ((size_t)n + 1) * 8));
    HIPCHK(c, op.sync());
    if (cnt[n]) return fail(c, EINCM_ERR_ARG, "%llu of %lld evaluation events have a coordinate outside the %dx%d sensor", cnt[n], (long long)tot, H, W);
    c->fe.fe_ngt.assign(cnt, cnt + n);
    c->fe.fe_n = n;
    return EINCM_OK;
}

// Evaluate many: only theta goes up.  One launch of k_flow_error, FE_PARTS partials per window come down and are added in index order.
int eincm_flow_errors(eincm_ctx* c, const double* theta, int h, int w, int method, eincm_flow_error_out* out, double* ee_map) {
    if (!c) return EINCM_ERR_ARG;
    if (!theta || !out) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (method < 0 || method > EINCM_METHOD_CUBIC) return fail(c, EINCM_ERR_ARG, "method %d unknown", method);
    if (h < 1 || w < 1) return fail(c, EINCM_ERR_ARG, "theta shape (%d,%d,2) invalid", h, w);
    if (h > c->H || w > c->W) return fail(c, EINCM_ERR_ARG, "theta (%d,%d,2) is finer than the %dx%d sensor", h, w, c->H, c->W);
    if (const int rc = not_in_flight(c, "eincm_flow_errors")) return rc;
    if (c->fe.fe_n < 1) return fail(c, EINCM_ERR_STATE, "eincm_flow_errors called before a successful eincm_flow_eval_stage");
    const int H = c->H, W = c->W, n = c->fe.fe_n;
    const size_t npix = (size_t)H * W, plane = (size_t)n * npix;
    const bool full = h == H && w == W;
    TapTables T;
    if (!full) build_taps(h, w, H, W, method, T);
    const Packer& tab = T.tab;
    const size_t thbytes = (size_t)n * h * w * 16, pbytes = (size_t)n * FE_PARTS * sizeof(FlowErrPart);
    OneShot op(c);
    const auto d_th = op.piece<double2>((size_t)n * h * w);
    const auto d_tab = op.piece<char>(tab.buf.size());
    const auto d_parts = op.piece<FlowErrPart>((size_t)n * FE_PARTS);
    const auto d_map = op.piece<double>(plane, ee_map != nullptr);
    FlowErrPart* parts = op.host_buf<FlowErrPart>((size_t)n * FE_PARTS);   // d_parts comes down here
    HIPCHK(c, op.begin());
    const void* const d_gt = c->fe.f_eval.p;              // (launch casts them to the kernel's types)
    const void* const d_flags = c->fe.f_eval.p + plane * 16;
    HIPCHK(c, op.up(d_th, theta, thbytes));               // (host memory: the caller's, as ee_map)
    if (!full) HIPCHK(c, op.up(d_tab, tab.buf.data(), tab.buf.size()));           // (T, a local older than the frame)
    HIPCHK(c, op.launch(k_flow_error, dim3(FE_PARTS, (unsigned)n), dim3(NT), 0, H, W, h, w, full ? 1 : 0, d_gt, d_flags, d_th,
                        tab.i32(d_tab, T.o_rlo), tab.i32(d_tab, T.o_rcnt), tab.f64(d_tab, 0), T.rstride, tab.i32(d_tab, T.o_clo),
                        tab.i32(d_tab, T.o_ccnt), tab.f64(d_tab, T.o_cw), T.cstride, d_parts, d_map));
    HIPCHK(c, op.down(parts, d_parts, pbytes));
    if (ee_map) HIPCHK(c, op.down(ee_map, d_map, plane * 8));
    HIPCHK(c, op.sync());
    for (int b = 0; b < n; ++b) {
        eincm_flow_error_out o{};
        for (int g = 0; g < FE_PARTS; ++g) {              // the partials of a window in index order
            const FlowErrPart& q = parts[(size_t)b * FE_PARTS + g];
            o.sum_ee += q.sum_ee; o.sum_ree += q.sum_ree;
            o.n_ee += q.n_ee; o.n_pred += q.n_pred;
            for (int k = 0; k < FE_NOVER; ++k) o.n_over[k] += q.n_over[k];
        }
        o.n_gt = c->fe.fe_ngt[b];
        // flow_eval.py:60-76: means over the intersection (NaN where it is empty), percentages over n_ee + eps
        o.aee = o.n_ee ? o.sum_ee / (double)o.n_ee : std::nan("");
        o.aree = o.n_ee ? o.sum_ree / (double)o.n_ee : std::nan("");
        for (int k = 0; k < FE_NOVER; ++k) o.anpe[k] = (double)(o.n_over[k] * 100) / ((double)o.n_ee + EPSN);
        out[b] = o;
    }
    return EINCM_OK;
}

int eincm_set_objective_tiles(eincm_ctx* c, int tile_h, int tile_w) {
    if (!c) return EINCM_ERR_ARG;
    if (tile_h < 1 || tile_w < 1 || tile_h > c->H || tile_w > c->W)
        return fail(c, EINCM_ERR_ARG, "objective tile %dx%d outside 1x1 .. %dx%d (the sensor)", tile_h, tile_w, c->H, c->W);
    if (c->fl.launched()) return fail(c, EINCM_ERR_STATE, "an asynchronous evaluation is in flight: call eincm_loss_grad_wait first");
    if (tile_h != c->obj_th || tile_w != c->obj_tw) { c->obj_th = tile_h; c->obj_tw = tile_w; c->objc_valid = false; }
    return EINCM_OK;
}

int eincm_set_splat_window(eincm_ctx* c, int window_size) {
    if (!c) return EINCM_ERR_ARG;
    if (window_size < 1 || window_size > EINCM_SPLAT_WINDOW_MAX)
        return fail(c, EINCM_ERR_ARG, "splat window size %d outside 1..%d", window_size, EINCM_SPLAT_WINDOW_MAX);
    if (c->fl.launched()) return fail(c, EINCM_ERR_STATE, "an asynchronous evaluation is in flight: call eincm_loss_grad_wait first");
    if (c->fp64 && window_size != 3)
        return fail(c, EINCM_ERR_UNSUPPORTED, "splat window size %d: fp64 mode (EINCM_CF_FP64) supports size 3 only", window_size);
    if (window_size == c->splat_size) return EINCM_OK;
    if (c->staged && c->stage.weighted && window_size != 3)
        return fail(c, EINCM_ERR_UNSUPPORTED, "splat window size %d: the staged batch carries per-event weights, which have the 3x3 splat window only",
                    window_size);
    if (c->staged && (c->sharded_staging || c->constants_pending))
        return fail(c, EINCM_ERR_STATE, "the staged batch's window constants come from an event-sharded staging: set the splat window "
                                        "before eincm_set_windows");
    HIPCHK(c, hipSetDevice(c->device));
    c->splat_size = window_size;
    c->splat_rad = window_size / 2;
    c->objc_valid = false;                           // the objective kinds' zero-warp values come from the zero-warp IWE
    if (!c->staged) return EINCM_OK;
    return window_constants(c);      // of the staged batch with the new splat: the theta = 0 pass of staging again
}

int eincm_tiled_objectives(eincm_ctx* c, int tile_h, int tile_w, eincm_tiled_out* out) {
    if (!c) return EINCM_ERR_ARG;
    if (c->fp64) return fail(c, EINCM_ERR_UNSUPPORTED, "eincm_tiled_objectives is not supported in fp64 mode (EINCM_CF_FP64)");
    if (!out) return fail(c, EINCM_ERR_ARG, "null pointer argument");
    if (!c->staged || !c->have_eval) return fail(c, EINCM_ERR_STATE, "no evaluation yet");
    Geom g = c->g;
    g.nparts = c->last_nparts;
    if (tile_h < 1 || tile_w < 1 || tile_h > g.H || tile_w > g.W)
        return fail(c, EINCM_ERR_ARG, "tile %d x %d does not fit the %d x %d sensor", tile_h, tile_w, g.H, g.W);
    const int ntx = g.W / tile_w, nty = g.H / tile_h, ntl = ntx * nty;
    const int nb = std::min((g.H * g.W + NT - 1) / NT, 256);
    const size_t n_t = (size_t)g.B * g.R * ntl * 3, n_p = (size_t)g.B * g.R * nb * 3;
    OneShot op(c);
    const auto d_v = op.piece<double>(n_t + n_p);         // the tiles' values | the workgroups' partials: one piece, one download
    double* hv = op.host_buf<double>(n_t + n_p);          // ... which lands here
    HIPCHK(c, op.begin());
    g.wmask = ~0ull;
    HIPCHK(c, op.launch(k_tiled, dim3(ntl, g.R, g.B), dim3(NT), 0, g, tile_h, tile_w, ntx, c->d_iwe, c->d_edges, c->d_parts, d_v));
    HIPCHK(c, op.launch(k_pair_objectives, dim3(nb, g.R, g.B), dim3(NT), 0, g, c->d_iwe, c->d_edges, c->d_parts, d_v + n_t));
    HIPCHK(c, op.down(hv, d_v, (n_t + n_p) * 8));
    HIPCHK(c, op.sync());
    const double HW = (double)g.H * g.W;
    for (int b = 0; b < g.B; ++b) {
        eincm_tiled_out& o = out[b];
        memset(&o, 0, sizeof o);
        o.n_refs = g.R; o.n_tiles = ntl;
        for (int r = 0; r < g.R; ++r) {
            const double* t = hv + ((size_t)b * g.R + r) * ntl * 3;
            for (int k = 0; k < ntl; ++k) {
                o.adaptive_mean_gradient_magnitude[r] += t[k * 3];
                o.adaptive_variance[r] += t[k * 3 + 1];
                o.adaptive_mean_squared_error[r] += t[k * 3 + 2];
            }
            double q[3] = {0.0, 0.0, 0.0};                       // the workgroups' partials, added in index order
            for (int k = 0; k < nb; ++k) {
                const double* pk = hv + n_t + (((size_t)b * g.R + r) * nb + k) * 3;
                q[0] += pk[0]; q[1] += pk[1]; q[2] += pk[2];
            }
            o.sum_squared_error[r] = q[0];
            o.sum_hadamard_product[r] = q[1];
            o.mean_hadamard_product[r] = q[1] / HW;
            o.joint_contrast[r] = q[2] / HW;
        }
    }
    return EINCM_OK;
}

int eincm_get_timings_total(eincm_ctx* c, eincm_timings* t, int64_t* n_evals, int reset) {
    if (!c || !t || !n_evals) return EINCM_ERR_ARG;
    if (!(c->cflags & (EINCM_CF_TIMING | EINCM_CF_TIMING_DOMINANT)))
        return fail(c, EINCM_ERR_STATE, "context was created without EINCM_CF_TIMING / EINCM_CF_TIMING_DOMINANT");
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "an evaluation is in flight");
    const int rc = drain_event_ring(c, 0);
    if (rc) return rc;
    *t = c->sum_t; *n_evals = c->sum_n;
    if (reset) { c->sum_t = eincm_timings{}; c->sum_n = 0; }
    return EINCM_OK;
}

int eincm_get_host_profile(eincm_ctx* c, double* us, int64_t* n_evals, int reset) {
    if (!c || !us || !n_evals) return EINCM_ERR_ARG;
    for (int i = 0; i < EINCM_N_HOST_PHASES; ++i) us[i] = c->hp_us[i];
    *n_evals = c->hp_n;
    if (reset) { for (double& v : c->hp_us) v = 0.0; c->hp_n = 0; }
    return EINCM_OK;
}

int eincm_get_memory(eincm_ctx* c, int64_t out[4]) {
    if (!c || !out) return EINCM_ERR_ARG;
    out[0] = (int64_t)c->mem.dev_bytes; out[1] = (int64_t)c->mem.pinned_bytes;
    out[2] = (int64_t)(c->mem.dev.size() + c->mem.pinned.size()); out[3] = (int64_t)c->scratch.n;
    return EINCM_OK;
}

int eincm_get_launch_policy(eincm_ctx* c, double* out) {
    if (!c || !out) return EINCM_ERR_ARG;
    launch_policy(*c, c->fl.plan, c->policy_evaluated, out);
    return EINCM_OK;
}

int eincm_set_timed_kernels(eincm_ctx* c, int splat, int gather) {
    if (!c) return EINCM_ERR_ARG;
    if (!(c->cflags & EINCM_CF_TIMING_DOMINANT)) return fail(c, EINCM_ERR_STATE, "context was created without EINCM_CF_TIMING_DOMINANT");
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "an evaluation is in flight");
    c->time_splat = splat != 0; c->time_gather = gather != 0;
    return EINCM_OK;
}

int eincm_set_timing_period(eincm_ctx* c, int period) {
    if (!c) return EINCM_ERR_ARG;
    if (!(c->cflags & EINCM_CF_TIMING_DOMINANT)) return fail(c, EINCM_ERR_STATE, "context was created without EINCM_CF_TIMING_DOMINANT");
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "an evaluation is in flight");
    if (period < 1) return fail(c, EINCM_ERR_ARG, "period %d", period);
    c->time_period = period; c->time_counter = 0;
    return EINCM_OK;
}

int eincm_get_timings(eincm_ctx* c, eincm_timings* t) {
    if (!c || !t) return EINCM_ERR_ARG;
    if (!(c->cflags & (EINCM_CF_TIMING | EINCM_CF_TIMING_DOMINANT)))
        return fail(c, EINCM_ERR_STATE, "context was created without EINCM_CF_TIMING / EINCM_CF_TIMING_DOMINANT");
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "an evaluation is in flight");
    const int rc = drain_event_ring(c, 0);
    if (rc) return rc;
    *t = c->last_t;
    return EINCM_OK;
}

// ---- BFGS with its state in HBM (eincm_bfgs.hip.h) ----
static int bfgs_ready(eincm_ctx* c, const char* who, bool need_begun) {
    if (c->fp64)
        return fail(c, EINCM_ERR_UNSUPPORTED, "%s is not supported in fp64 mode (EINCM_CF_FP64): the device-resident evaluation does not exist there", who);
    if (const int rc = eval_ready(c, who)) return rc;
    if (c->device_results) return fail(c, EINCM_ERR_STATE, "%s: eincm_set_device_results is on (the split finishing half owns the results)", who);
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "%s: an evaluation is in flight", who);
    if (c->g.B > BFGS_MAX_B) return fail(c, EINCM_ERR_ARG, "%s: %d windows exceed EINCM_BFGS_MAX_WINDOWS = %d", who, c->g.B, BFGS_MAX_B);
    if (need_begun && (!c->bfgs.begun || c->bfgs.B != c->g.B))
        return fail(c, EINCM_ERR_STATE, "%s called before eincm_bfgs_begin (for the staged windows)", who);
    return EINCM_OK;
}

static unsigned long long bfgs_mask(const eincm_ctx* c, const uint8_t* active) {
    unsigned long long m = 0ull;
    for (int b = 0; b < c->g.B; ++b) if (!active || active[b]) m |= 1ull << b;
    return m;
}

static BfgsAlpha bfgs_alpha(const eincm_ctx* c, unsigned long long m, const double* alpha) {
    BfgsAlpha al{};
    for (int b = 0; b < c->g.B; ++b) if ((m >> b) & 1ull) al.a[b] = alpha[b];
    return al;
}

static int bfgs_launch_reduce(eincm_ctx* c, unsigned long long m, const double* gsrc) {
    auto& s = c->bfgs;
    if (s.m) {          // the limited form has no bound on n: per-chunk partials, then one wave per window in chunk order
        const int chunks = lbfgs_chunks(s.n);
        hipLaunchKernelGGL(k_lbfgs_reduce, dim3((unsigned)chunks, (unsigned)s.B), dim3(LBFGS_NT), 0, c->stream, s.n, m, gsrc, s.Gt,
                           (const double*)s.P, s.part_red());
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_lbfgs_reduce_fin, dim3((unsigned)s.B), dim3(64), 0, c->stream, chunks, m, (const double*)s.part_red(), s.h_red.p);
        HIPCHK(c, hipGetLastError());
        return EINCM_OK;
    }
    hipLaunchKernelGGL(k_bfgs_reduce, dim3((unsigned)s.B), dim3(BFGS_NT), 0, c->stream, s.n, m, gsrc, s.Gt, (const double*)s.P, s.h_red.p);
    HIPCHK(c, hipGetLastError());
    return EINCM_OK;
}

// Both forms' begin: history = 0 is the dense form (H = I), history = m > 0 the limited one (an empty ring of m slots)
static int bfgs_begin_form(eincm_ctx* c, const char* who, const double* x0_host, int h, int w, const uint8_t* active, int history, int scale) {
    if (const int rc = bfgs_ready(c, who, false)) return rc;
    if (!x0_host || h < 1 || w < 1) return fail(c, EINCM_ERR_ARG, "%s: bad argument", who);
    const int64_t n64 = (int64_t)2 * h * w;
    if (!history && n64 > BFGS_MAX_N)
        return fail(c, EINCM_ERR_ARG, "eincm_bfgs_begin: theta (%d,%d,2) has %lld unknowns, more than EINCM_BFGS_MAX_N = %d", h, w, (long long)n64, BFGS_MAX_N);
    if (n64 > (int64_t)1 << 30) return fail(c, EINCM_ERR_ARG, "%s: theta (%d,%d,2) has %lld unknowns, more than 2^30", who, h, w, (long long)n64);
    HIPCHK(c, hipSetDevice(c->device));
    auto& s = c->bfgs;
    const int n = (int)n64, B = c->g.B;
    s.begun = false;
    HIPCHK(c, ensure(c, s.h_scal, (size_t)c->maxB * BFGS_NS, true));
    HIPCHK(c, ensure(c, s.h_red, (size_t)c->maxB * 2, true));
    const size_t need_vec = (size_t)B * n, need_H = need_vec * n;
    const bool reshaped = n != s.n || B != s.B || history != s.m;
    HIPCHK(c, ensure(c, s.vec, 8 * need_vec));
    double** v[8] = {&s.X, &s.G, &s.P, &s.Xt, &s.Gt, &s.S, &s.Y, &s.Hy};
    for (int k = 0; k < 8; ++k) *v[k] = s.vec.p + (size_t)k * (s.vec.n / 8);
    const int nd = 2 * history + 1, chunks = lbfgs_chunks(n);
    if (history) {
        HIPCHK(c, ensure(c, s.hist, 2 * need_vec * history));
        HIPCHK(c, ensure(c, s.dmat, (size_t)B * (nd * nd + nd + 2)));
        HIPCHK(c, ensure(c, s.ring, (size_t)3 * B));
        HIPCHK(c, ensure(c, s.part, (size_t)B * chunks * (lbfgs_nq(history) + LBFGS_NP + 2)));
    } else HIPCHK(c, ensure(c, s.H, need_H));
    if (reshaped) {          // the rows of windows outside this call's mask must hold finite numbers in the new layout
        HIPCHK(c, hipMemsetAsync(s.vec.p, 0, s.vec.n * sizeof(double), c->stream));
        if (history) {
            HIPCHK(c, hipMemsetAsync(s.hist.p, 0, s.hist.n * sizeof(double), c->stream));
            HIPCHK(c, hipMemsetAsync(s.dmat.p, 0, s.dmat.n * sizeof(double), c->stream));
            HIPCHK(c, hipMemsetAsync(s.ring.p, 0, s.ring.n * sizeof(int), c->stream));
        } else HIPCHK(c, hipMemsetAsync(s.H.p, 0, s.H.n * sizeof(double), c->stream));
        memset(s.h_scal.p, 0, s.h_scal.n * sizeof(double));
    }
    s.n = n; s.h = h; s.w = w; s.B = B; s.m = history; s.scale = scale;
    const unsigned long long m = bfgs_mask(c, active);
    if (history)
        hipLaunchKernelGGL(k_lbfgs_begin, dim3((unsigned)chunks, (unsigned)B), dim3(LBFGS_NT), 0, c->stream, n, m, s.P, s.G, s.head(), s.count(), s.stored());
    else
        hipLaunchKernelGGL(k_bfgs_begin, dim3((unsigned)((n + BFGS_ROWS - 1) / BFGS_ROWS), (unsigned)B), dim3(BFGS_NT), 0, c->stream, n, m, s.H.p, s.P, s.G);
    HIPCHK(c, hipGetLastError());
    for (int b = 0; b < B; ) {                        // x0 of the mask's windows, one copy per run of them
        if (!((m >> b) & 1ull)) { ++b; continue; }
        int e = b + 1;
        while (e < B && ((m >> e) & 1ull)) ++e;
        HIPCHK(c, hipMemcpyAsync(s.X + (size_t)b * n, x0_host + (size_t)b * n, (size_t)(e - b) * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        for (int k = b; k < e; ++k) {                  // max|x0| bounds |theta| of the first evaluation
            double xm = 0.0;
            for (int i = 0; i < n; ++i) { const double a = std::fabs(x0_host[(size_t)k * n + i]); if (a > xm || a != a) xm = a; }
            double* o = s.h_scal.p + (size_t)k * BFGS_NS;
            for (int q = 0; q < BFGS_NS; ++q) o[q] = 0.0;
            o[EINCM_BFGS_S_XMAX] = xm;
        }
        b = e;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.begun = true;
    return EINCM_OK;
}

int eincm_bfgs_begin(eincm_ctx* c, const double* x0_host, int h, int w, const uint8_t* active) {
    if (!c) return EINCM_ERR_ARG;
    return bfgs_begin_form(c, "eincm_bfgs_begin", x0_host, h, w, active, 0, 0);
}

int eincm_lbfgs_begin(eincm_ctx* c, const double* x0_host, int h, int w, const uint8_t* active, int history, int initial_scale) {
    if (!c) return EINCM_ERR_ARG;
    if (history < 1 || history > LBFGS_MAX_M)
        return fail(c, EINCM_ERR_ARG, "eincm_lbfgs_begin: history %d outside 1 .. EINCM_LBFGS_MAX_HISTORY = %d", history, LBFGS_MAX_M);
    if (initial_scale != EINCM_LBFGS_SCALE_IDENTITY && initial_scale != EINCM_LBFGS_SCALE_LAST_PAIR)
        return fail(c, EINCM_ERR_ARG, "eincm_lbfgs_begin: initial_scale %d unknown", initial_scale);
    return bfgs_begin_form(c, "eincm_lbfgs_begin", x0_host, h, w, active, history, initial_scale);
}

int eincm_lbfgs_history_ptrs(eincm_ctx* c, void** s_dptr, void** y_dptr, void** d_dptr, void** delta_dptr, void** head_dptr, void** count_dptr,
                             int* history) {
    if (!c || !s_dptr || !y_dptr || !d_dptr || !delta_dptr || !head_dptr || !count_dptr || !history) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_lbfgs_history_ptrs", true)) return rc;
    auto& s = c->bfgs;
    if (!s.m) return fail(c, EINCM_ERR_STATE, "eincm_lbfgs_history_ptrs: the state is in the dense form (eincm_bfgs_begin)");
    *s_dptr = s.lS(); *y_dptr = s.lY(); *d_dptr = s.lD(); *delta_dptr = s.ldelta(); *head_dptr = s.head(); *count_dptr = s.count();
    *history = s.m;
    return EINCM_OK;
}

int eincm_bfgs_trial(eincm_ctx* c, const double* alpha, const uint8_t* active) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_trial", true)) return rc;
    if (!alpha) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_trial: null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    auto& s = c->bfgs;
    const unsigned long long m = bfgs_mask(c, active);
    hipLaunchKernelGGL(k_bfgs_trial, dim3((unsigned)((s.n + BFGS_NT - 1) / BFGS_NT), (unsigned)s.B), dim3(BFGS_NT), 0, c->stream, s.n, m,
                       bfgs_alpha(c, m, alpha), (const double*)s.X, (const double*)s.P, s.Xt);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EINCM_OK;
}

int eincm_bfgs_reduce(eincm_ctx* c, const uint8_t* active, double* dphi, double* gmax) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_reduce", true)) return rc;
    if (!dphi || !gmax) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_reduce: null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const unsigned long long m = bfgs_mask(c, active);
    if (const int rc = bfgs_launch_reduce(c, m, nullptr)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->bfgs.B; ++b) if ((m >> b) & 1ull) { dphi[b] = c->bfgs.h_red.p[2 * b]; gmax[b] = c->bfgs.h_red.p[2 * b + 1]; }
    return EINCM_OK;
}

int eincm_bfgs_eval(eincm_ctx* c, const eincm_params* p, const double* alpha, const uint8_t* active, double* value, double* dphi, double* gmax) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_eval", true)) return rc;
    if (!p || !alpha || !value || !dphi || !gmax) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_eval: null pointer argument");
    if (p->method < 0 || p->method > EINCM_METHOD_CUBIC) return fail(c, EINCM_ERR_ARG, "method %d unknown", p->method);
    HIPCHK(c, hipSetDevice(c->device));
    auto& s = c->bfgs;
    const unsigned long long m = bfgs_mask(c, active);
    double vmax = 0.0;                             // max|X| + |a| max|P| bounds |theta| at the trial point: selects the LDS window capacity
    for (int b = 0; b < s.B; ++b) if ((m >> b) & 1ull) {
        const double* o = s.h_scal.p + (size_t)b * BFGS_NS;
        const double v = o[EINCM_BFGS_S_XMAX] + std::fabs(alpha[b]) * o[EINCM_BFGS_S_PMAX];
        if (!(v <= vmax)) vmax = v;                // (a NaN ends up in vmax: unknown)
    }
    hipLaunchKernelGGL(k_bfgs_trial, dim3((unsigned)((s.n + BFGS_NT - 1) / BFGS_NT), (unsigned)s.B), dim3(BFGS_NT), 0, c->stream, s.n, m,
                       bfgs_alpha(c, m, alpha), (const double*)s.X, (const double*)s.P, s.Xt);
    HIPCHK(c, hipGetLastError());
    // the masked evaluation with theta = Xt in HBM; its gradient stays in the engine's block, k_bfgs_reduce moves the mask's rows to Gt
    std::vector<uint8_t> act((size_t)s.B);
    for (int b = 0; b < s.B; ++b) act[b] = (uint8_t)((m >> b) & 1ull);
    int rc = eval_begin(c, nullptr, s.h, s.w, p, true, act.data(), DevIo{s.Xt, nullptr, std::isfinite(vmax) ? vmax : -1.0});
    if (!rc) rc = eval_end_launch(c);
    if (rc) return rc;
    FlightGuard guard(c);
    if ((rc = bfgs_launch_reduce(c, m, c->d_grad))) return rc;
    rc = guard.keep(eval_end_collect(c, value, nullptr, nullptr));             // the one synchronisation
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) return rc;
    for (int b = 0; b < s.B; ++b) if ((m >> b) & 1ull) { dphi[b] = s.h_red.p[2 * b]; gmax[b] = s.h_red.p[2 * b + 1]; }
    return rc;
}

int eincm_bfgs_trial_ptrs(eincm_ctx* c, void** xt_dptr, void** gt_dptr, int64_t* n_doubles) {
    if (!c || !xt_dptr || !gt_dptr || !n_doubles) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_trial_ptrs", true)) return rc;
    *xt_dptr = c->bfgs.Xt; *gt_dptr = c->bfgs.Gt; *n_doubles = (int64_t)c->bfgs.B * c->bfgs.n;
    return EINCM_OK;
}

int eincm_bfgs_state_ptrs(eincm_ctx* c, void** x_dptr, void** g_dptr, void** p_dptr, void** hess_inv_dptr, int* n_windows, int* n) {
    if (!c || !x_dptr || !g_dptr || !p_dptr || !hess_inv_dptr || !n_windows || !n) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_state_ptrs", true)) return rc;
    *x_dptr = c->bfgs.X; *g_dptr = c->bfgs.G; *p_dptr = c->bfgs.P; *hess_inv_dptr = c->bfgs.m ? nullptr : c->bfgs.H.p; *n_windows = c->bfgs.B; *n = c->bfgs.n;
    return EINCM_OK;
}

int eincm_bfgs_accept(eincm_ctx* c, const double* alpha, const uint8_t* accept_mode, double* scalars_out) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_accept", true)) return rc;
    if (!alpha || !accept_mode || !scalars_out) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_accept: null pointer argument");
    auto& s = c->bfgs;
    unsigned long long act = 0ull, upd = 0ull, init = 0ull;
    for (int b = 0; b < s.B; ++b) {
        const int mode = accept_mode[b];
        if (mode > EINCM_BFGS_INIT) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_accept: accept_mode[%d] = %d unknown", b, mode);
        if (mode != EINCM_BFGS_SKIP) act |= 1ull << b;
        if (mode == EINCM_BFGS_UPDATE) upd |= 1ull << b;
        if (mode == EINCM_BFGS_INIT) init |= 1ull << b;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (act && s.m) {
        const int chunks = lbfgs_chunks(s.n);
        const dim3 grid((unsigned)chunks, (unsigned)s.B);
        if (upd | init) {
            hipLaunchKernelGGL(k_lbfgs_dots, grid, dim3(LBFGS_NT), 0, c->stream, s.n, s.m, upd, init, bfgs_alpha(c, upd, alpha), (const double*)s.G,
                               (const double*)s.Gt, (const double*)s.P, (const double*)s.lS(), (const double*)s.lY(), (const int*)s.head(),
                               (const int*)s.count(), s.S, s.Y, s.part_dots());
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL(k_lbfgs_coef, dim3((unsigned)s.B), dim3(64), 0, c->stream, chunks, s.m, s.scale, upd, init, (const double*)s.part_dots(),
                               s.lD(), s.ldelta(), s.head(), s.count(), s.stored(), s.lysyy());
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k_lbfgs_dir, grid, dim3(LBFGS_NT), 0, c->stream, s.n, s.m, act, upd, init, s.X, (const double*)s.Xt, s.G, (const double*)s.Gt,
                           s.P, s.lS(), s.lY(), (const double*)s.S, (const double*)s.Y, (const double*)s.ldelta(), (const int*)s.head(),
                           (const int*)s.count(), (const int*)s.stored(), s.part_dir());
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_lbfgs_finish, dim3((unsigned)s.B), dim3(64), 0, c->stream, chunks, act, upd, (const double*)s.part_dir(),
                           (const double*)s.lysyy(), s.h_scal.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if (act) {
        const dim3 grid((unsigned)((s.n + BFGS_ROWS - 1) / BFGS_ROWS), (unsigned)s.B);
        if (upd) {
            hipLaunchKernelGGL(k_bfgs_hy, grid, dim3(BFGS_NT), (size_t)s.n * sizeof(double), c->stream, s.n, upd, bfgs_alpha(c, upd, alpha),
                               (const double*)s.H.p, (const double*)s.G, (const double*)s.Gt, (const double*)s.P, s.S, s.Y, s.Hy);
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k_bfgs_update, grid, dim3(BFGS_NT), (size_t)3 * s.n * sizeof(double), c->stream, s.n, act, upd, init, s.H.p,
                           (const double*)s.S, (const double*)s.Y, (const double*)s.Hy, s.X, (const double*)s.Xt, s.G, (const double*)s.Gt, s.P);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_bfgs_scalars, dim3((unsigned)s.B), dim3(BFGS_NT), 0, c->stream, s.n, act, (const double*)s.X, (const double*)s.G,
                           (const double*)s.P, (const double*)s.S, (const double*)s.Y, (const double*)s.Hy, upd, s.h_scal.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    memcpy(scalars_out, s.h_scal.p, (size_t)s.B * BFGS_NS * sizeof(double));
    return EINCM_OK;
}

int eincm_bfgs_fetch(eincm_ctx* c, double* x, double* g, double* hess_inv) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = bfgs_ready(c, "eincm_bfgs_fetch", true)) return rc;
    auto& s = c->bfgs;
    if (s.m && hess_inv) return fail(c, EINCM_ERR_ARG, "eincm_bfgs_fetch: the limited form (eincm_lbfgs_begin) keeps no inverse Hessian: hess_inv must be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nv = (size_t)s.B * s.n * sizeof(double);
    if (x) HIPCHK(c, hipMemcpyAsync(x, s.X, nv, hipMemcpyDeviceToHost, c->stream));
    if (g) HIPCHK(c, hipMemcpyAsync(g, s.G, nv, hipMemcpyDeviceToHost, c->stream));
    if (hess_inv) HIPCHK(c, hipMemcpyAsync(hess_inv, s.H.p, nv * s.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return EINCM_OK;
}

// ---- parametric motion-field models ----
static int motion_ready(eincm_ctx* c, const char* who, const double* coeffs) {
    if (c->fp64)
        return fail(c, EINCM_ERR_UNSUPPORTED, "%s is not supported in fp64 mode (EINCM_CF_FP64): the device-resident evaluation does not exist there", who);
    if (!c->motion.set) return fail(c, EINCM_ERR_STATE, "%s: no motion model set (eincm_set_motion_model)", who);
    if (const int rc = eval_ready(c, who)) return rc;
    if (c->device_results) return fail(c, EINCM_ERR_STATE, "%s: eincm_set_device_results is on (the split finishing half owns the results)", who);
    if (!c->fl.idle()) return fail(c, EINCM_ERR_STATE, "%s: an evaluation is in flight", who);
    if (!coeffs) return fail(c, EINCM_ERR_ARG, "%s: null pointer argument", who);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, ensure(c, c->motion.Theta, (size_t)c->maxB * c->H * c->W * 2));
    HIPCHK(c, ensure(c, c->motion.h_part, (size_t)c->maxB * (MOTION_PARTS + 1) * MOTION_NQ, true));
    return EINCM_OK;
}

// q = M c of the mask's windows and the launch of k_motion_expand; returns the bound of |Theta| over those windows (NaN: unknown).
// The caller's frame drains the stream: with more than MOTION_ARG_WINDOWS windows the kernel reads q from the pinned block.
static double motion_expand(eincm_ctx* c, const double* coeffs, unsigned long long wmask, MotionGeom& mg) {
    auto& mo = c->motion;
    const Geom& g = c->g;
    const int K = mo.model.n_coeffs;
    mg = MotionGeom{g.H, g.W, g.B, wmask, mo.model.cx, mo.model.cy, mo.model.scale};
    double mm[MOTION_NM];
    motion_monomial_bounds(mo.model, g.H, g.W, mm);
    const bool use_arg = g.B <= MOTION_ARG_WINDOWS;
    static thread_local MotionQArg qarg;
    double* qs = use_arg ? qarg.q : mo.h_q(c->maxB);
    double vmax = 0.0;
    for (int b = 0; b < g.B; ++b) {
        double* q = qs + (size_t)b * MOTION_NQ;
        if (b < 64 && !((wmask >> b) & 1ull)) { for (int j = 0; j < MOTION_NQ; ++j) q[j] = 0.0; continue; }
        motion_q(mo.model, coeffs + (size_t)b * K, q);
        const double v = motion_abs_bound(q, mm);
        if (!(v <= vmax)) vmax = v;                // (a NaN ends up in vmax: unknown)
    }
    const int npix = g.H * g.W;
    hipLaunchKernelGGL(k_motion_expand, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)g.B), dim3(NT), 0, c->stream, mg, use_arg ? 1 : 0, qarg,
                       (const double*)mo.h_q(c->maxB), reinterpret_cast<double2*>(mo.Theta.p));
    return vmax;
}

int eincm_set_motion_model(eincm_ctx* c, const eincm_motion_model* model) {
    if (!c) return EINCM_ERR_ARG;
    if (!model) { c->motion.set = false; c->motion.last_q.clear(); return EINCM_OK; }
    if (const char* what = motion_model_error(*model)) return fail(c, EINCM_ERR_ARG, "eincm_set_motion_model: %s", what);
    c->motion.model = *model;
    c->motion.set = true;
    c->motion.last_q.clear();                       // (a fused evaluation's q belongs to the model it was formed with)
    return EINCM_OK;
}

int eincm_motion_field(eincm_ctx* c, const double* coeffs, double* Theta) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = motion_ready(c, "eincm_motion_field", coeffs)) return rc;
    if (!Theta) return fail(c, EINCM_ERR_ARG, "eincm_motion_field: null pointer argument");
    OneShot op(c);
    op.pending = true;                             // (motion_expand launches on the stream itself)
    MotionGeom mg;
    (void)motion_expand(c, coeffs, ~0ull, mg);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, op.down(Theta, c->motion.Theta.p, (size_t)c->g.B * c->g.H * c->g.W * 2 * sizeof(double)));
    HIPCHK(c, op.sync());
    return EINCM_OK;
}

int eincm_loss_grad_motion(eincm_ctx* c, const double* coeffs, const eincm_params* p, const uint8_t* active, double* value, double* grad,
                           eincm_aux* aux) {
    if (!c) return EINCM_ERR_ARG;
    if (const int rc = motion_ready(c, "eincm_loss_grad_motion", coeffs)) return rc;
    if (!p || !value) return fail(c, EINCM_ERR_ARG, "eincm_loss_grad_motion: null pointer argument");
    auto& mo = c->motion;
    const Geom& g = c->g;
    const int K = mo.model.n_coeffs;
    unsigned long long wmask = ~0ull;
    if (active) { wmask = 0ull; for (int b = 0; b < g.B && b < 64; ++b) if (active[b]) wmask |= 1ull << b; }
    // the dense evaluation needs no resampling method: the field is at sensor size
    eincm_params pe = *p;
    pe.method = EINCM_METHOD_BILINEAR;
    FlightGuard guard(c);                          // from the first launch on, every exit drains the stream
    MotionGeom mg;
    const double vmax = motion_expand(c, coeffs, wmask, mg);
    HIPCHK(c, hipGetLastError());
    // the masked dense evaluation with theta = the field in HBM; its gradient stays in the engine's block for k_motion_moments
    int rc = eval_begin(c, nullptr, g.H, g.W, &pe, grad != nullptr, active, DevIo{mo.Theta.p, nullptr, std::isfinite(vmax) ? vmax : -1.0});
    if (!rc) rc = eval_end_launch(c);
    if (rc) return rc;
    if (grad) {
        hipLaunchKernelGGL(k_motion_moments, dim3((unsigned)MOTION_PARTS, (unsigned)g.B), dim3(NT), 0, c->stream, mg,
                           reinterpret_cast<const double2*>(c->d_grad), mo.h_part.p);
        HIPCHK(c, hipGetLastError());
    }
    rc = guard.keep(eval_end_collect(c, value, nullptr, aux));                 // the one synchronisation
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) return rc;
    if (grad) {
        bool nonfinite = false;
        for (int b = 0; b < g.B; ++b) {
            double* gb = grad + (size_t)b * K;
            if (window_sat_out(g, b)) { for (int k = 0; k < K; ++k) gb[k] = 0.0; continue; }
            double mu[MOTION_NQ];
            motion_sum_partials(mo.h_part.p + (size_t)b * MOTION_PARTS * MOTION_NQ, MOTION_PARTS, mu);
            motion_project(mo.model, mu, gb);
            if (copy_scan_finite(nullptr, gb, (size_t)K)) nonfinite = true;
        }
        if (nonfinite && rc == EINCM_OK) rc = fail(c, EINCM_ERR_NONFINITE, "loss or gradient is not finite");
    }
    return rc;
}

// The field of the last fused evaluation's q into d_Theta, for the accessors that read the image (ensure_theta_image): every window,
// whatever the evaluation masked (a window that sat out has q = 0).
static int motion_theta_image(eincm_ctx* c) {
    auto& mo = c->motion;
    const Geom& g = c->g;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, ensure(c, mo.h_part, (size_t)c->maxB * (MOTION_PARTS + 1) * MOTION_NQ, true));
    OneShot op(c);                                  // (the frame is here for its drain: the kernel reads the pinned q)
    op.pending = true;
    memcpy(mo.h_q(c->maxB), mo.last_q.data(), mo.last_q.size() * sizeof(double));
    const MotionGeom mg{g.H, g.W, g.B, ~0ull, mo.model.cx, mo.model.cy, mo.model.scale};
    static const MotionQArg none{};
    const int npix = g.H * g.W;
    hipLaunchKernelGGL(k_motion_expand, dim3((unsigned)((npix + NT - 1) / NT), (unsigned)g.B), dim3(NT), 0, c->stream, mg, 0, none,
                       (const double*)mo.h_q(c->maxB), reinterpret_cast<double2*>(c->d_Theta));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, op.sync());
    c->Theta_valid = true;
    return EINCM_OK;
}

int eincm_loss_grad_motion_fused(eincm_ctx* c, const double* coeffs, const eincm_params* p, const uint8_t* active, double* value, double* grad,
                                 eincm_aux* aux) {
    if (!c) return EINCM_ERR_ARG;
    static const char* who = "eincm_loss_grad_motion_fused";
    const MotionCtxState st{c->fp64, c->motion.set, c->staged, c->constants_pending, c->device_results, !c->fl.idle(), c->splat_size,
                            c->staged && c->stage.weighted};
    if (const MotionRefusal r = motion_fused_supported(st, p)) return fail(c, r.code, "%s: %s", who, r.why);
    if (!coeffs || !p || !value) return fail(c, EINCM_ERR_ARG, "%s: null pointer argument", who);
    HIPCHK(c, hipSetDevice(c->device));
    auto& mo = c->motion;
    const Geom& g = c->g;
    const int K = mo.model.n_coeffs;
    // q = M c and the bound of the field per window, before any launch: a window whose q (or bound) is not finite sits the launch out
    double mm[MOTION_NM];
    motion_monomial_bounds(mo.model, g.H, g.W, mm);
    std::vector<double> q((size_t)g.B * MOTION_NQ, 0.0);
    std::vector<uint8_t> act((size_t)g.B, 1), bad((size_t)g.B, 0);
    double vmax = 0.0;
    bool any_bad = false;
    for (int b = 0; b < g.B; ++b) {
        if (active && b < 64 && !active[b]) { act[b] = 0; continue; }        // (windows >= 64 always take part, as in every masked evaluation)
        double* qb = q.data() + (size_t)b * MOTION_NQ;
        motion_q(mo.model, coeffs + (size_t)b * K, qb);
        const double v = motion_abs_bound(qb, mm);
        if (!motion_q_usable(qb, v)) {
            for (int j = 0; j < MOTION_NQ; ++j) qb[j] = 0.0;
            act[b] = 0; bad[b] = 1; any_bad = true;
            continue;
        }
        vmax = std::max(vmax, v);
    }
    HIPCHK(c, ensure(c, mo.h_part, (size_t)c->maxB * (MOTION_PARTS + 1) * MOTION_NQ, true));
    HIPCHK(c, ensure(c, mo.tmm_zero, (size_t)c->maxB * g.ntiles * 4, true));
    if (grad) HIPCHK(c, ensure(c, mo.h_fpart, (size_t)std::max(c->gather.n, 1) * g.R * MOTION_NQ));
    if (grad && mo.seg0.empty()) {
        mo.seg0.resize((size_t)g.B + 1);
        const int64_t n = motion_slot_offsets(c->h_tilecount.data(), g.B, g.ntiles, c->stage.seg, 1, mo.seg0.data());
        if (n != c->gather.n) { mo.seg0.clear(); return fail(c, EINCM_ERR_STATE, "%s: internal: %lld segments counted, the gather's list has %d", who, (long long)n, c->gather.n); }
    }
    eincm_params pe = *p;
    pe.method = EINCM_METHOD_BILINEAR;             // (no resampling: the field is at sensor size)
    FlightGuard guard(c);                          // from the first launch on, every exit drains the stream
    int rc = eval_begin(c, q.data(), g.H, g.W, &pe, grad != nullptr, act.data(), DevIo{nullptr, nullptr, vmax}, true);
    if (!rc) rc = eval_end_launch(c);
    if (rc) return rc;
    const int sps = c->fl.plan.all_r ? 1 : g.R;    // slots per segment
    rc = guard.keep(eval_end_collect(c, value, nullptr, aux));                 // the one synchronisation
    if (rc != EINCM_OK && rc != EINCM_ERR_NONFINITE) return rc;
    bool nonfinite = any_bad;
    HostPhase hp(c, EINCM_HP_COLLECT);             // the host's share of the gradient: the slots in index order, then M^T mu
    for (int b = 0; b < g.B; ++b) {
        double* gb = grad ? grad + (size_t)b * K : nullptr;
        if (bad[b]) {
            value[b] = NAN;
            if (aux) aux[b].final_loss = aux[b].mean_rel_corr = aux[b].mean_rel_contrast = aux[b].mean_rel_iwe_divergence = aux[b].theta_total_variation = NAN;
            for (int k = 0; gb && k < K; ++k) gb[k] = NAN;
            continue;
        }
        if (!gb) continue;
        if (window_sat_out(g, b)) { for (int k = 0; k < K; ++k) gb[k] = 0.0; continue; }
        double mu[MOTION_NQ];
        motion_sum_slots(mo.h_fpart.p + (size_t)mo.seg0[b] * sps * MOTION_NQ, (mo.seg0[b + 1] - mo.seg0[b]) * sps, mu);
        motion_project(mo.model, mu, gb);
        if (copy_scan_finite(nullptr, gb, (size_t)K)) nonfinite = true;
    }
    if (nonfinite && rc == EINCM_OK) rc = fail(c, EINCM_ERR_NONFINITE, "loss or gradient is not finite");
    return rc;
}

}  // extern "C"
