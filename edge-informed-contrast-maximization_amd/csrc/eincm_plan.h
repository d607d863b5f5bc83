// eincm_plan.h — what the host decides and tabulates without a GPU: the launch policy of a staging and of an
// evaluation, the cut of the tile populations into segment lists, the host counting sort, the resampling tables and a few small
// rules.  eincm_api.hip owns the memory, enqueues the work and words the errors; everything here is a function of its arguments.
//
// The rule that keeps it so: this header includes no HIP and reads no environment (the switches arrive as Knobs arguments, read by
// eincm_api.hip).  Plain C++17, so tests/host/plan_check.cpp runs all of it on the CPU under the sanitizers (tests/test_host_plan.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "eincm.h"
#include "eincm_types.h"

namespace eincm {

// Packs host arrays into one block for a single upload: add appends `bytes` at the next multiple of `align` (zero padding) and returns
// their offset; i32 / f64 form a typed pointer into a copy of the block.
struct Packer {
    std::vector<char> buf;
    size_t add(const void* p, size_t bytes, size_t align = 1) {
        const size_t off = (buf.size() + align - 1) / align * align;
        buf.resize(off + bytes, 0);
        if (bytes) std::memcpy(buf.data() + off, p, bytes);
        return off;
    }
    static const int32_t* i32(const char* base, size_t off) { return reinterpret_cast<const int32_t*>(base + off); }
    static const double* f64(const char* base, size_t off) { return reinterpret_cast<const double*>(base + off); }
};

// A segment list: the binned events of every (window, source tile) cut into segments of at most `seg` events (balanced_seg_len), the
// event kernels' unit of work; their workgroups take the segments longest first (block_to_work).  Staging builds four lists over the
// same bins (cut_segments, build_list): the gather's, the splat's, the splat's short one and the 2-DoF gather's.
struct SegList {
    int seg = 0;                       // events per segment
    int n = 0;                         // segments
    double tspan = 1.0;                // time span (fraction of the window) its LDS windows are sized for (cut_segments)
    Item* d_items = nullptr;           // (max_items)
    int32_t* d_order = nullptr;        // (max_items) the segments by decreasing length
    std::vector<Item> h_items;         // host sides of the two (kept until the upload has completed); h_items only where the host cuts them
    std::vector<int32_t> h_order;
    int32_t* d_win_item0 = nullptr;    // (B + 1) first segment of every window: gather and 2-DoF gather lists
    std::vector<int32_t> h_win_item0;  // its host copy, where the host cuts the segments
    Window* d_wins = nullptr;          // (max_items, maxR) destination windows under the current theta: gather and splat lists
    int32_t* d_itembase = nullptr;     // (B * ntiles) first segment of every (window, tile): gather and splat lists, device binning
    // blocks of an event kernel: every (segment, reference time) pair, padded to a multiple of 8 segments (block_to_work)
    unsigned grid(int R) const { return (unsigned)(((n + NXCD - 1) / NXCD) * NXCD * R); }
};

constexpr int SEG_SHORT = 8192;         // events per segment of the splat's short list
constexpr int MIN_SEG = 64;             // the shortest segments EINCM_SEG / EINCM_SEG_SPLAT / EINCM_SEG_2DOF may ask for: what the lists' capacity allows for

// The cut of the bins (counts: events per (window, tile), nbins = B * ntiles) at `seg` events per segment, in the order k_items emits
// the segments: every segment's length into lens, the list's time span, and the longest-first order into L.h_order.  want_items: the
// host cuts the segments themselves too (L.h_items, and the first one of every window, L.h_win_item0); otherwise both stay empty.
inline void cut_segments(const int32_t* counts, size_t nbins, int ntiles, int seg, int64_t N, bool want_items, SegList& L,
                         std::vector<int32_t>& lens) {
    // L.tspan, for the choice of the LDS window capacity (plan_eval): a tile of n events is cut into ceil(n / seg) segments, each spanning
    // about 1 / that of the time.  Not the mean: sparse tiles (sensor noise between the edges) hold one segment that spans the WHOLE
    // window, and their taps go to HBM one by one when the capacity follows the dense tiles (480x640 with 10^7 events at 16x16 theta:
    // k_gather 110 -> 90 us with the larger windows).  It is the span that all but 3 % of the events stay within.
    constexpr int K = 64;
    int64_t by_nseg[K + 1] = {0};
    lens.clear();
    L.h_items.clear(); L.h_win_item0.clear();
    int64_t base = 0;
    for (size_t idx = 0; idx < nbins; ++idx) {
        if (want_items && idx % (size_t)ntiles == 0) L.h_win_item0.push_back((int32_t)lens.size());
        const int cnt = counts[idx], len = balanced_seg_len(cnt, seg);
        if (cnt > 0) by_nseg[std::min<int64_t>(((int64_t)cnt + seg - 1) / seg, K)] += cnt;
        for (int s0 = 0; s0 < cnt; s0 += len) {
            lens.push_back(std::min(len, cnt - s0));
            if (want_items) L.h_items.push_back(Item{(int32_t)(idx / ntiles), (int32_t)(idx % ntiles), (int32_t)(base + s0), lens.back(), 0.0, 0.0});
        }
        base += cnt;
    }
    if (want_items) L.h_win_item0.push_back((int32_t)lens.size());
    L.seg = seg;
    L.tspan = 1.0 / K;
    int64_t beyond = 0;
    const int64_t allow = (int64_t)(0.03 * (double)N);
    for (int k = 1; k <= K; ++k)                // spans 1, 1/2, 1/3, ...
        if ((beyond += by_nseg[k]) > allow) { L.tspan = 1.0 / k; break; }
    // the order the event kernels' workgroups take the segments in (block_to_work): by decreasing length, a stable counting sort
    int32_t maxlen = 0;
    for (const int32_t l : lens) maxlen = std::max(maxlen, l);
    std::vector<int32_t> start((size_t)maxlen + 2, 0);
    for (const int32_t l : lens) ++start[(size_t)(maxlen - l) + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    L.h_order.resize(lens.size());
    for (size_t i = 0; i < lens.size(); ++i) L.h_order[(size_t)start[(size_t)(maxlen - lens[i])]++] = (int32_t)i;
}

// ---------------------------------------------------------------------------------------------
// jax.image.scale_and_translate per-axis weight matrix (S7; theta_utils.py:25-35), fp64 on the host.
// A is (n_out, n_in): out = A @ in.
// ---------------------------------------------------------------------------------------------
inline double kern_eval(int method, double x) {
    switch (method) {
        case EINCM_METHOD_BILINEAR: return std::max(0.0, 1.0 - std::fabs(x));
        case EINCM_METHOD_LANCZOS3:
        case EINCM_METHOD_LANCZOS5: {
            const double radius = (method == EINCM_METHOD_LANCZOS3) ? 3.0 : 5.0;
            if (x > radius) return 0.0;
            if (!(x > 1e-3)) return 1.0;
            const double y = radius * std::sin(M_PI * x) * std::sin(M_PI * x / radius);
            return y / (M_PI * M_PI * x * x);
        }
        case EINCM_METHOD_CUBIC: {
            if (x >= 2.0) return 0.0;
            if (x >= 1.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
            return ((1.5 * x - 2.5) * x) * x + 1.0;
        }
    }
    return 0.0;
}

inline void resample_matrix(int n_in, int n_out, int method, std::vector<double>& A) {
    A.assign((size_t)n_out * n_in, 0.0);
    const double scale = (double)n_out / (double)n_in;
    const double inv_scale = 1.0 / scale;
    const double kernel_scale = std::max(inv_scale, 1.0);
    const double thresh = 1000.0 * 1.1920928955078125e-07;   // 1000 * float32 eps
    for (int o = 0; o < n_out; ++o) {
        const double sample_f = ((double)o + 0.5) * inv_scale - 0.5;
        double total = 0.0;
        for (int i = 0; i < n_in; ++i) {
            const double x = std::fabs(sample_f - (double)i) / kernel_scale;
            const double wgt = kern_eval(method, x);
            A[(size_t)o * n_in + i] = wgt;
            total += wgt;
        }
        const bool inside = (sample_f >= -0.5) && (sample_f <= (double)n_in - 0.5);
        for (int i = 0; i < n_in; ++i) {
            double& a = A[(size_t)o * n_in + i];
            a = (std::fabs(total) > thresh) ? a / (total != 0.0 ? total : 1.0) : 0.0;
            if (!inside) a = 0.0;
        }
    }
}

// Everything the kernels read of a (h, w) -> (H, W) resampling (ensure_resample uploads it): the two matrices, the non-zero range
// [x, y) of every row of each (Int2 has int2's layout), the coarse cells under every 32x32 tile (what k_gather's own projection
// walks), and whether every tile touches at most PG_MAXC x PG_MAXC of them.
struct Int2 { int x, y; };
struct ResampleTables {
    std::vector<double> AH, AW;        // (H, h), (W, w)
    std::vector<Int2> rowtap, coltap;  // (H), (W)
    std::vector<TileRange> tilerng;    // (ntiles)
    bool fits = true;
};
inline void build_resample(int h, int w, int H, int W, int method, ResampleTables& t) {
    resample_matrix(h, H, method, t.AH);
    resample_matrix(w, W, method, t.AW);
    auto taps = [](const std::vector<double>& A, int n_out, int n_in, std::vector<Int2>& tap) {
        tap.resize((size_t)n_out);
        for (int o = 0; o < n_out; ++o) {
            int lo = n_in, hi = 0;
            for (int i = 0; i < n_in; ++i) if (A[(size_t)o * n_in + i] != 0.0) { lo = std::min(lo, i); hi = std::max(hi, i + 1); }
            if (lo >= hi) { lo = 0; hi = 0; }
            tap[(size_t)o] = Int2{lo, hi};
        }
    };
    taps(t.AH, H, h, t.rowtap);
    taps(t.AW, W, w, t.coltap);
    const std::vector<Int2>&rt = t.rowtap, &ct = t.coltap;
    const int tilesX = (W + TS - 1) / TS, tilesY = (H + TS - 1) / TS;
    t.tilerng.resize((size_t)tilesX * tilesY);
    t.fits = true;
    for (int ty = 0; ty < tilesY; ++ty)
        for (int tx = 0; tx < tilesX; ++tx) {
            int ilo = h, ihi = 0, jlo = w, jhi = 0;
            for (int y = ty * TS; y < std::min(ty * TS + TS, H); ++y) if (rt[y].y > rt[y].x) { ilo = std::min(ilo, rt[y].x); ihi = std::max(ihi, rt[y].y); }
            for (int x = tx * TS; x < std::min(tx * TS + TS, W); ++x) if (ct[x].y > ct[x].x) { jlo = std::min(jlo, ct[x].x); jhi = std::max(jhi, ct[x].y); }
            TileRange q;
            q.ilo = ilo < ihi ? ilo : 0; q.ni = std::max(ihi - ilo, 0); q.jlo = jlo < jhi ? jlo : 0; q.nj = std::max(jhi - jlo, 0);
            t.fits = t.fits && q.ni <= PG_MAXC && q.nj <= PG_MAXC;
            t.tilerng[(size_t)ty * tilesX + tx] = q;
        }
}

// The non-zero run of every row of a resample matrix A (n_out, n_in): lo, cnt and the weights padded to the longest run.
inline int resample_runs(const std::vector<double>& A, int n_in, int n_out, std::vector<int32_t>& lo, std::vector<int32_t>& cnt,
                         std::vector<double>& wt) {
    lo.assign(n_out, 0); cnt.assign(n_out, 0);
    int stride = 1;
    for (int o = 0; o < n_out; ++o) {
        int a = n_in, b = 0;
        for (int i = 0; i < n_in; ++i) if (A[(size_t)o * n_in + i] != 0.0) { a = std::min(a, i); b = std::max(b, i + 1); }
        if (a < b) { lo[o] = a; cnt[o] = b - a; stride = std::max(stride, b - a); }
    }
    wt.assign((size_t)n_out * stride, 0.0);
    for (int o = 0; o < n_out; ++o)
        for (int k = 0; k < cnt[o]; ++k) wt[(size_t)o * stride + k] = A[(size_t)o * n_in + lo[o] + k];
    return stride;
}

// The tap tables of a (h, w) -> (H, W) resampling as k_flow_encode and k_flow_error read them, packed for one upload:
// row weights | column weights | rlo | rcnt | clo | ccnt
struct TapTables {
    Packer tab;
    size_t o_cw = 0, o_rlo = 0, o_rcnt = 0, o_clo = 0, o_ccnt = 0;
    int rstride = 1, cstride = 1;
};

inline void build_taps(int h, int w, int H, int W, int method, TapTables& t) {
    std::vector<double> AH, AW, rwt, cwt;
    std::vector<int32_t> rlo, rcnt, clo, ccnt;
    resample_matrix(h, H, method, AH);
    resample_matrix(w, W, method, AW);
    t.rstride = resample_runs(AH, h, H, rlo, rcnt, rwt);
    t.cstride = resample_runs(AW, w, W, clo, ccnt, cwt);
    t.tab.add(rwt.data(), rwt.size() * 8);
    t.o_cw = t.tab.add(cwt.data(), cwt.size() * 8);
    t.o_rlo = t.tab.add(rlo.data(), (size_t)H * 4); t.o_rcnt = t.tab.add(rcnt.data(), (size_t)H * 4);
    t.o_clo = t.tab.add(clo.data(), (size_t)W * 4); t.o_ccnt = t.tab.add(ccnt.data(), (size_t)W * 4);
}

inline void multi_ref_weights(int R, double* w) {
    double s = 0.0;
    for (int r = 0; r < R; ++r) {
        // np.linspace(-1.5, 1.5, R): start + r*step with step = 3/(R-1); R == 1 -> [-1.5]
        const double x = (R > 1) ? (-1.5 + (double)r * (3.0 / (double)(R - 1))) : -1.5;
        w[r] = std::exp(-0.5 * x * x) / std::sqrt(2.0 * M_PI);
        s += w[r];
    }
    for (int r = 0; r < R; ++r) w[r] /= s;
}

// float64 mode: the scale of a window's u64 IWE accumulator.  No pixel can exceed N_b / (2 pi) (one tap per event and pixel), so
// 2^ishift with N_b / (2 pi) * 2^ishift < 2^62, capped at 2^52
inline int f64_ishift(int64_t n_events) {
    const double bound = std::max(1.0, (double)n_events * 0.15915494309189535);
    return std::min(52, 62 - (int)std::ceil(std::log2(bound)));
}

// NL-means: the shift that divides a patch distance by the next power of two >= tw^2 (eincm_preprocess_image)
inline int nlm_shift(int tw) { int s = 0; while ((1 << s) < tw * tw) ++s; return s; }

// ---- host binning (sensors with more tiles than the LDS histogram holds, or EINCM_HOST_BINNING=1) ----

// The first event a staging refuses: event `index` of window `win`, outside the sensor (bad_xy) or with a non-finite timestamp.
struct EventRefusal {
    int win = -1; int64_t index = 0; bool bad_xy = false;
    explicit operator bool() const { return win >= 0; }
};

// The most events of weight > 0 on one source pixel of a window (WinConst.cntmax before its floor of 1); events of weight 0 are not
// counted.  xy are the window's n events as x | y << 16, in any order, w their weights (NULL: ones).  bin_events counts with it, and
// so does a re-weighting of a host-binned batch.
inline unsigned most_on_one_pixel(int H, int W, int64_t n, const uint32_t* xy, const float* w) {
    std::vector<uint32_t> pc((size_t)H * W, 0u);
    unsigned m = 0u;
    for (int64_t i = 0; i < n; ++i)
        if (!w || w[i] > 0.0f) m = std::max(m, ++pc[(size_t)(xy[i] >> 16) * W + (xy[i] & 0xffffu)]);
    return m;
}

// A stable counting sort of the batch's events by (window, tile) into sxy (x | y << 16) and st (both max(N, 1) long), the events per
// (window, tile) into tilecount, and per window the running maxima cntmax (most events on one source pixel) and dtmax (max |t - tau|;
// both B long, as the caller initialised them).  Stops at the first event it refuses.
inline EventRefusal bin_events(const Geom& g, const int64_t* n_events, const int16_t* const* xs, const int16_t* const* ys,
                               const double* const* ts, const double* edge_ts, int64_t N, std::vector<int32_t>& tilecount,
                               std::vector<uint32_t>& sxy, std::vector<double>& st, std::vector<unsigned>& cntmax,
                               std::vector<double>& dtmax, const float* const* weights = nullptr, std::vector<float>* sw = nullptr,
                               std::vector<uint32_t>* sidx = nullptr) {
    // sw (a weighted batch): the weights in the order of sxy, ones for a window without (weights[b] NULL).  sidx (a keep-order batch,
    // DESIGN.md section 29): where the event of every slot of sxy stood in the batch as it was handed over, window after window
    const int H = g.H, W = g.W;
    if (sw) sw->resize((size_t)std::max<int64_t>(N, 1));
    if (sidx) sidx->resize((size_t)std::max<int64_t>(N, 1));
    tilecount.assign((size_t)g.B * g.ntiles, 0);
    sxy.resize((size_t)std::max<int64_t>(N, 1));
    st.resize((size_t)std::max<int64_t>(N, 1));
    std::vector<int64_t> cnt((size_t)g.ntiles + 1);
    int64_t base = 0;
    for (int b = 0; b < g.B; ++b) {
        const int64_t n = n_events[b];
        const int16_t* x = xs[b]; const int16_t* y = ys[b]; const double* t = ts[b];
        const float* wb = (sw && weights) ? weights[b] : nullptr;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t i = 0; i < n; ++i) {
            for (int r = 0; r < g.R; ++r) dtmax[b] = std::max(dtmax[b], std::fabs(t[i] - edge_ts[b * g.R + r]));
            if (x[i] < 0 || x[i] >= W || y[i] < 0 || y[i] >= H) return EventRefusal{b, i, true};
            if (!std::isfinite(t[i])) return EventRefusal{b, i, false};
            ++cnt[(size_t)(y[i] / TS) * g.tilesX + (x[i] / TS) + 1];
        }
        for (int k = 0; k < g.ntiles; ++k) tilecount[(size_t)b * g.ntiles + k] = (int32_t)cnt[k + 1];
        for (int k = 0; k < g.ntiles; ++k) cnt[k + 1] += cnt[k];
        std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            const int tile = (y[i] / TS) * g.tilesX + (x[i] / TS);
            const int64_t d = base + pos[tile]++;
            sxy[d] = (uint32_t)(uint16_t)x[i] | ((uint32_t)(uint16_t)y[i] << 16);
            st[d] = t[i];
            if (sw) (*sw)[d] = wb ? wb[i] : 1.0f;
            if (sidx) (*sidx)[d] = (uint32_t)(base + i);
        }
        // (the sorted slots hold the window's events as x | y << 16 beside their weights: any order counts the same)
        cntmax[b] = std::max(cntmax[b], most_on_one_pixel(H, W, n, sxy.data() + base, wb ? sw->data() + base : nullptr));
        base += n;
    }
    return EventRefusal{};
}

// One edge image to fp32 with its moments: the sum, the sum of squares and the largest magnitude of the fp32 values
inline void edge_moments(const double* e, size_t img, float* o, double& sE, double& sEE, double& eabs) {
    double s = 0.0, ss = 0.0, mx = 0.0;
    for (size_t i = 0; i < img; ++i) { const float f = (float)e[i]; o[i] = f; s += (double)f; ss += (double)f * (double)f; mx = std::max(mx, std::fabs((double)f)); }
    sE = s; sEE = ss; eabs = mx;
}

// ---- LDS destination windows ----

// largest width of an LDS destination window of `cap` pixels (Geom.winmaxw)
inline int win_maxw(int cap) { return std::max(40, (int)std::lround(std::sqrt((double)cap * 1.4))); }

// LDS destination-window geometry chosen for one list in one evaluation (fit_window)
struct WinFit {
    int cap, maxw;                     // capacity (pixels) and largest width
    bool pal;                          // bank-aligned row pitch (win_pitch)
    bool fits;                         // the list's windows fit the largest capacity class
};

// LDS window capacity for the segments of one list, chosen per evaluation (plan_eval): the host knows theta, hence the largest
// displacement (vmax * tspan) a segment of the list can see; the window's side is the tile plus that plus the splat's margin.
// LDS holds pitch x height words per window, the pitch being the width, or the width rounded up to the 32 banks (win_pitch).
// pitch: 1 takes the aligned pitch where it does not push the window into a larger capacity class (its gain is a few per cent of
// bank conflicts, a class costs workgroups per CU: 8 windows of 10^6 events whose theta needs 66-pixel windows: 96 x 66 words = the
// 6912 class, 5 workgroups per CU, 2-DoF gather 62 -> 68 us); 0 keeps pitch = width; -1 too, sized on the unrounded side (the
// theta-grid gather's rule).  floor_k: the smallest capacity class the list takes.
inline WinFit fit_window(double vmax, double tspan, double margin, int floor_k, int pitch) {
    static const int caps[] = {2304, 3072, 4608, 6912};      // 6912 keeps k_gather's LDS (window + accumulators + Theta tile) under 64 KiB
    const double side = TS + margin + vmax * tspan, sd = std::ceil(side);
    const double need = pitch < 0 ? side * side : sd * sd;
    int cap = caps[3];
    for (int k = floor_k; k < 4; ++k) if (need <= caps[k]) { cap = caps[k]; break; }
    return WinFit{cap, win_maxw(cap), pitch > 0 && std::ceil(sd / 32.0) * 32.0 * sd <= (double)cap, need <= (double)caps[3]};
}

// ---- the plans ----

// What rides beside ev_xy / ev_t through staging's kernels: nothing, the per-event weights, the weights and the index back into the
// batch as handed over.  The value indexes the instantiations of k_bin_scatter, k_spread and k_segsort.
enum StagePayload { PAYLOAD_NONE, PAYLOAD_WEIGHTS, PAYLOAD_WEIGHTS_ORDER };

// Every decision of one staging, taken once by plan_staging before its first HIP call; the phases of stage_windows only read it, and
// the context keeps the one of the staged batch (plan_eval, eincm_get_launch_policy).
struct StagePlan {
    Geom g{};                           // the batch's geometry as staged (an evaluation sets the mask, capacities and pitch of the context's copy)
    int64_t N = 0;                      // events of the batch
    int seg = 0, seg_s = 0, seg_2 = 0;  // events per segment of the gather's, the splat's and the 2-DoF gather's list
    bool splat_short = false;           // the splat gets its short list (8192) beside a longer one
    int pitch = 0;                      // regime of the bank-aligned LDS pitch (win_pitch): 0 never, 1 k_splat where it costs no capacity class, 2 the 2-DoF gather too; plan_eval decides per evaluation
    bool sort_segments = true;          // k_segsort deals the gather's copy of the events (EINCM_NO_SEGSORT: a plain copy)
    bool spread = true;                 // k_spread re-deals the splat's copy (EINCM_NO_SPREAD: time order)
    bool host_binning = false;          // the host sorts the events by (window, tile), not the kernels of eincm_binning.hip.h
    bool defer_constants = false;       // EINCM_SW_DEFER_CONSTANTS: the caller sums the shards' IUEs before the window constants are formed
    bool wide = false;                  // a window has a handful of events: 61-bit fixed point in the per-pixel gradient sums (grad_shift_pixel)
    StagePayload payload = PAYLOAD_NONE;     // the batch's payload state: the two flags below as one value (plan_staging)
    bool weighted = false;              // a window with events carries per-event weights: the payload ev_w rides beside ev_xy / ev_t and the event kernels run their weighted forms
    bool keep_order = false;            // EINCM_SW_KEEP_ORDER: both layouts keep the index of every slot into the batch as handed over, and the batch is a weighted one whatever it was handed, so a later eincm_set_weights changes no plan
};

// Does a staging carry per-event weights?  weights: NULL, or one pointer per window, NULL where a window's weights are all ones.
// Weights of a window without events change nothing, so they do not make the batch a weighted one.
inline bool batch_weighted(int n_windows, const int64_t* n_events, const float* const* weights) {
    if (!weights) return false;
    for (int b = 0; b < n_windows; ++b) if (weights[b] && n_events[b] > 0) return true;
    return false;
}

// The first weight a staging refuses: not finite, or outside [0, 1] (the bounds behind both fixed-point scales assume w <= 1, and
// neither accumulator is signed)
struct WeightRefusal {
    int win = -1; int64_t index = 0; float value = 0.0f;
    explicit operator bool() const { return win >= 0; }
};
inline WeightRefusal check_weights(int n_windows, const int64_t* n_events, const float* const* weights) {
    if (!weights) return WeightRefusal{};
    for (int b = 0; b < n_windows; ++b) {
        const float* w = weights[b];
        if (!w) continue;
        for (int64_t i = 0; i < n_events[b]; ++i)
            if (!(w[i] >= 0.0f && w[i] <= 1.0f)) return WeightRefusal{b, i, w[i]};     // (a NaN fails both comparisons)
    }
    return WeightRefusal{};
}

// What the planning reads of a context; eincm_ctx derives from it, so both plans take the context by const reference.
struct PlanCtx {
    int H = 0, W = 0;
    int seg = 0;                   // events per segment of the gather list (0 = choose per batch); EINCM_SEG overrides
    int seg_s = 0;                 // ... of the splat list; EINCM_SEG_SPLAT overrides
    bool host_binning = false;
    int wincap = WIN_CAP_DEFAULT;
    bool wincap_fixed = false;     // EINCM_WINCAP pins the capacity; otherwise it is chosen per evaluation from max|theta|
    bool fp64 = false;             // float64 mode (EINCM_CF_FP64, eincm_kernels_f64.hip.h)
    StagePlan stage;               // the plan the staged batch was staged from (plan_staging)
    Geom g{};
    SegList gather;                // walked by k_gather / k_count / k_mask / the fp64 kernels, on the gather's copy of the events
    SegList splat;                 // shorter segments walked by k_splat
    SegList splat_sh;              // the splat's SHORT list (8192) beside a 16384-event one: a 2-DoF theta too large for the long segments' windows walks it (launch_forward)
    // the segments the 2-DoF gather walks, on the SPLAT's copy of the events (it has no per-pixel accumulators, so the time-ordered copy
    // serves it, and it wants shorter segments than the theta-grid gather does: round-2 tuning)
    SegList gather_2;
    bool itembase_valid = false;   // the gather and splat lists' d_itembase hold the first segment of every (window, tile) for the staged batch
    bool device_results = false;   // eincm_set_device_results: results stay in HBM until eincm_finish_collect (event-sharded mode over RCCL)
    bool proj_in_gather = false;   // every tile touches <= PG_MAXC x PG_MAXC cells: k_gather projects its tile itself
    int splat_rad = 1;             // radius of eincm_set_splat_window's window: 1 runs k_splat / k_gather, any other k_splat_r / k_gather_r
    int obj_th = 32, obj_tw = 42;  // tile size of the adaptive objective kinds (eincm_objectives.hip.h)
};

// The switches a staging reads from the environment, at every staging (eincm_api.hip reads them)
struct StageKnobs {
    int seg_2 = 0;                      // EINCM_SEG_2DOF (0: not set)
    bool has_pitch = false; int pitch = 0;   // EINCM_PITCH_ALIGNED
    bool no_segsort = false, no_spread = false;
};

// Every decision of one staging, from the context and the checked arguments.  No HIP calls, no side effects.
inline StagePlan plan_staging(const PlanCtx& c, int n_windows, int n_refs, const int64_t* n_events, uint32_t flags, const StageKnobs& k,
                              const float* const* weights = nullptr) {
    StagePlan P;
    P.keep_order = (flags & EINCM_SW_KEEP_ORDER) != 0;
    P.weighted = P.keep_order || batch_weighted(n_windows, n_events, weights);
    P.payload = P.keep_order ? PAYLOAD_WEIGHTS_ORDER : P.weighted ? PAYLOAD_WEIGHTS : PAYLOAD_NONE;
    const int H = c.H, W = c.W;
    Geom& g = P.g;
    g.H = H; g.W = W; g.R = n_refs; g.B = n_windows;
    g.tilesX = (W + TS - 1) / TS; g.tilesY = (H + TS - 1) / TS; g.ntiles = g.tilesX * g.tilesY;
    g.igx = (W + IG_COLS - 1) / IG_COLS; g.nig = g.igx * ((H + IG_ROWS - 1) / IG_ROWS);
    g.pstride = std::max(g.ntiles, NSPART);
    g.gmax_n = g.R * g.nig;
    g.wincap = c.wincap; g.winmaxw = win_maxw(c.wincap);
    g.wincap_a = g.wincap; g.winmaxw_a = g.winmaxw;
    for (int b = 0; b < n_windows; ++b) P.N += n_events[b];
    const int64_t N = P.N;

    // Segment lengths (events per workgroup and reference time), measured on MI355X with the longest-first order of block_to_work
    // (tools/dev_tune_seg.py, profiles/r02/segment_tuning.txt).  Per-workgroup fixed cost (window clear / flush, G-window load,
    // reductions) favours long segments, the end of the launch (the last workgroups run on a mostly idle chip) short ones; x
    // estimates the workgroups of a launch at 8192-event segments against the 2048 the chip holds at once.
    //   k_gather: x >= 4000 (8 windows x 10^6 events, one window of 10^7): 16384 (96.9 -> 91.7 us, 167 -> 140 us);
    //             x < 1000 (one 10^6-event window): 4096 (22.8 us against 25.5 with 8192 and 41 with 16384); else 8192.
    //   k_splat:  bound by LDS atomics, it gains nothing beyond 8192 (108 us at 8192 and 16384, 122 at 4096, 186 at 2048 on the
    //             8-window batch) and loses nothing with it on a single window (22.7 vs 23.5 us; theta grids 22.3 vs 24.5).
    //   theta grids / dense theta: the gather walks the list with the longer segments (one 10^6-event window at 16x16: 35.8 us
    //             with 4096, 30.3 with 8192, 28.6 with 16384; the 8-window batch 157 / 144 / 139 with 8192 / 16384 / 32768).
    const double x_wg = ((double)N / 8192.0 + 0.5 * n_windows * g.ntiles) * n_refs;
    const double per_tile = (double)N / ((double)n_windows * g.ntiles);
    // Round 3: the gather's list always has long segments (what its theta-grid form wants: thtile, accumulator clear and flush per
    // workgroup); its 2-DoF form walks a list of its own (seg_2: round-2 tuning; with tiles of several segments as seg_s below:
    // 480x640 with 10^7 events 90 -> 82 us).
    P.seg = c.seg > 0 ? c.seg : 16384;
    P.seg_2 = (x_wg >= 4000.0 && per_tile < 16384.0) ? 16384 : (x_wg < 1000.0 ? 4096 : 8192);
    if (k.seg_2 >= MIN_SEG && k.seg_2 <= MAX_SEG) P.seg_2 = k.seg_2;
    // (late round 3: k_splat is no longer bound by the LDS atomic unit, so its per-workgroup fixed work - 24 of 90 us on the 8-window
    // batch: window derivation and clear 14, flush 10 - shows: 16384-event segments there, 90.1 -> 85.2 us; 104 -> 100 us at 16x16)
    // ... but only where a tile holds about one such segment: with tiles of several segments (480x640, 10^7 events: 33 000 per tile) the long
    // segments double the duration of EVERY workgroup and the kernel ends in a tail of few resident waves (k_splat 93 -> 137 us there).
    // (4 windows of 10^6 events: 52.4 -> 49.7 us; 2 windows: equal; 1: 18.8 vs 19.7 the other way; one window at R = 1: 4096, 0.066 vs
    // 0.075 ms per evaluation)
    P.seg_s = c.seg_s > 0 ? c.seg_s : (x_wg >= 3000.0 && per_tile < 16384.0 ? 16384 : (x_wg >= 400.0 ? 8192 : 4096));
    // beside a splat list of longer segments, the short one: the same events cut into 8192-event segments, for evaluations whose theta is
    // too large for the windows of the long segments (twice the time span, hence twice the spread)
    P.splat_short = P.seg_s > SEG_SHORT && N > 0;
    // The bank-aligned LDS pitch (win_pitch) goes with the same regime - many resident windows, about one segment per tile: both event
    // kernels 2 % faster on the bench batch; everywhere else pitch = width is the faster layout (profiles/r03/pitch_by_shape.txt: one
    // window of 10^6 events 72 -> 62 us per evaluation, 2 x 3*10^6 143 -> 128, 480x640 with 5*10^6 173 -> 126, with 10^7 220 -> 184).
    P.pitch = (x_wg >= 3000.0 && per_tile < 16384.0) ? 1 : 0;
    if (k.has_pitch) P.pitch = std::max(0, std::min(2, k.pitch));
    g.pitch_aligned = P.pitch;
    P.sort_segments = !k.no_segsort;
    P.spread = !k.no_spread;
    P.host_binning = c.host_binning;
    P.defer_constants = (flags & EINCM_SW_DEFER_CONSTANTS) != 0;
    P.wide = std::any_of(n_events, n_events + n_windows, [&](int64_t n) { return n * (int64_t)n_refs < 4096; });
    return P;
}

// theta and gradient of an evaluation whose caller keeps them in HBM (eincm_loss_grad_device, eincm_bfgs_eval)
struct DevIo {
    const double* theta = nullptr;      // (B,h,w,2) in the caller's device buffer; nullptr: theta comes from the host
    double* grad = nullptr;             // the gradient goes there, device to device (nullptr: it stays in the engine's block)
    double vmax = -1.0;                 // bounds |theta| for the window-capacity choice (< 0: unknown, largest windows)
};

// ---- the event kernels' launch forms ----

// The instantiations of the four event kernels the library contains, as data: eincm_api.hip binds every row to its kernel, in this
// order, and launches nothing else, so a row here is a kernel that exists and the other way round.  plan_forms names the row an
// evaluation runs; tests/test_host_plan.py asserts it cell by cell and that the rows are exactly what the plans can reach.
struct SplatKey {
    int mode;                           // THETA_CONST / THETA_TILE / THETA_POLY
    int rad;                            // radius of the splat window: 1 is k_splat, 0 / 2 / 3 k_splat_r
    int threads;                        // per workgroup
    int weighted;                       // the weighted form
};
struct GatherKey {
    int mode, rad;                      // as the splat's: radius 1 is k_gather, 0 / 2 / 3 k_gather_r
    int wide;                           // 61-bit per-pixel sums (StagePlan.wide) as a template argument: k_gather's grid and motion forms (k_gather_r takes it at run time)
    int threads;
    int proj, all_r;                    // the tile's gradient projected onto the theta cells in the gather; one workgroup per segment for all reference times
    int weighted;
};
constexpr bool operator==(const SplatKey& a, const SplatKey& b) {
    return a.mode == b.mode && a.rad == b.rad && a.threads == b.threads && a.weighted == b.weighted;
}
constexpr bool operator==(const GatherKey& a, const GatherKey& b) {
    return a.mode == b.mode && a.rad == b.rad && a.wide == b.wide && a.threads == b.threads && a.proj == b.proj && a.all_r == b.all_r &&
           a.weighted == b.weighted;
}
// k_splat: 512 threads per workgroup in every compile-time mode: 93 vs 94 us on the 8-window batch, 18.8 vs 23.2 us on one window
// (1024: 102 us; the gather is slower with 512: 93.5 vs 81.7 us).  The gather of a grid or a motion model: 44 KB of LDS (G window +
// i64 accumulators + Theta tile) fit 3 workgroups per CU: 512 threads each keep 24 waves there.
constexpr int NT_TILE = 512;
// k_splat<mode, threads, weighted>
inline constexpr SplatKey SPLAT_FORMS[] = {
    {THETA_CONST, 1, NT_TILE, 0}, {THETA_CONST, 1, NT_TILE, 1}, {THETA_TILE, 1, NT_TILE, 0}, {THETA_TILE, 1, NT_TILE, 1},
    {THETA_POLY, 1, NT_TILE, 0},
};
// k_splat_r<mode, rad>
inline constexpr SplatKey SPLAT_R_FORMS[] = {
    {THETA_CONST, 0, NT, 0}, {THETA_CONST, 2, NT, 0}, {THETA_CONST, 3, NT, 0}, {THETA_TILE, 0, NT, 0}, {THETA_TILE, 2, NT, 0}, {THETA_TILE, 3, NT, 0},
};
// k_gather<mode, wide, threads, proj, all_r, weighted>
inline constexpr GatherKey GATHER_FORMS[] = {
    {THETA_CONST, 1, 0, NT, 0, 0, 0},      {THETA_CONST, 1, 0, NT, 0, 0, 1},
    {THETA_TILE, 1, 0, NT_TILE, 0, 0, 0},  {THETA_TILE, 1, 0, NT_TILE, 0, 0, 1},  {THETA_TILE, 1, 1, NT_TILE, 0, 0, 0},  {THETA_TILE, 1, 1, NT_TILE, 0, 0, 1},
    {THETA_TILE, 1, 0, NT_TILE, 1, 0, 0},  {THETA_TILE, 1, 0, NT_TILE, 1, 0, 1},  {THETA_TILE, 1, 1, NT_TILE, 1, 0, 0},  {THETA_TILE, 1, 1, NT_TILE, 1, 0, 1},
    {THETA_TILE, 1, 0, NT_TILE, 1, 1, 0},  {THETA_TILE, 1, 0, NT_TILE, 1, 1, 1},  {THETA_TILE, 1, 1, NT_TILE, 1, 1, 0},  {THETA_TILE, 1, 1, NT_TILE, 1, 1, 1},
    {THETA_POLY, 1, 0, NT_TILE, 0, 0, 0},  {THETA_POLY, 1, 1, NT_TILE, 0, 0, 0},  {THETA_POLY, 1, 0, NT_TILE, 0, 1, 0},  {THETA_POLY, 1, 1, NT_TILE, 0, 1, 0},
};
// k_gather_r<mode, rad>
inline constexpr GatherKey GATHER_R_FORMS[] = {
    {THETA_CONST, 0, 0, NT, 0, 0, 0}, {THETA_CONST, 2, 0, NT, 0, 0, 0}, {THETA_CONST, 3, 0, NT, 0, 0, 0},
    {THETA_TILE, 0, 0, NT, 0, 0, 0},  {THETA_TILE, 2, 0, NT, 0, 0, 0},  {THETA_TILE, 3, 0, NT, 0, 0, 0},
};
// the row of `rows` that equals k; -1: the library holds no such kernel
template <typename K, size_t N> constexpr int form_row(const K (&rows)[N], const K& k) {
    for (size_t i = 0; i < N; ++i) if (rows[i] == k) return (int)i;
    return -1;
}

enum class ListId { GATHER, SPLAT, SPLAT_SHORT, GATHER_2DOF };   // PlanCtx's gather / splat / splat_sh / gather_2 (seg_list)
enum class EventCopy { SPLAT, GATHER };                          // the splat's copy of the events and weights (time order, k_spread), or the gather's (k_segsort)

// How an evaluation launches its splat: the kernel (key; row: its place in SPLAT_FORMS, or in SPLAT_R_FORMS where the radius is not 1)
// and what must agree with it.
struct SplatForm {
    SplatKey key{};
    int row = -1;
    size_t lds = 0;                     // dynamic LDS bytes: the window, the Theta tile, the polynomial's scratch
    ListId list = ListId::SPLAT;        // the list it walks
    int wincap = 0, winmaxw = 0;        // the window capacity and largest width of its Geom: the plan's, capped for k_splat_r's u64 windows
};
// ... and its gather (filled for a gradient evaluation only)
struct GatherForm {
    GatherKey key{};
    int row = -1;                       // in GATHER_FORMS, or in GATHER_R_FORMS where the radius is not 1
    size_t lds = 0;                     // the G window, the accumulators and the Theta tile of a grid, the polynomial's scratch
    ListId list = ListId::GATHER;
    EventCopy copy = EventCopy::GATHER; // the events and weights it reads
    int wg_per_seg = 0;                 // workgroups per segment: one per reference time, or 1 (all_r)
    int wincap = 0, winmaxw = 0, pitch_aligned = 0;   // wincap_a, winmaxw_a and pitch_aligned of its Geom (the 2-DoF gather: its own list's, win_2)
};

// Every decision of one evaluation, taken once by plan_eval before its first launch; the launch and assembly code only read it.
struct EvalPlan {
    enum Shape { IDENTITY, TWO_DOF, GRID, MOTION } shape = GRID;   // theta (h, w) = the sensor's / (1, 1) / any other grid / a motion model's polynomial inside the event kernels (plan_motion)
    enum ThetaSrc { THETA_DEVICE, THETA_ARGS, THETA_PINNED, THETA_PIECES } theta_src = THETA_PIECES;   // where k_theta reads theta
    int h = 0, w = 0; size_t nth = 0;   // nth: doubles of one window's theta
    bool want_grad = false, full_aux = false, div_grad = false;
    EvalParams ep{};
    bool obj = false; ObjGeom og{};     // a contrast / correlation kind other than the defaults (eincm_objectives.hip.h)
    // LDS windows (fit_window): the splat's and the gather's (into Geom), the 2-DoF gather's, and whether k_splat walks splat_sh
    int wincap = 0, winmaxw = 0, pitch_aligned = 0, wincap_a = 0, winmaxw_a = 0;
    WinFit win_2{}; bool splat_short = false;
    bool use_arg = false, use_arg_big = false;   // theta rides in the arguments of every kernel (ThetaArg) / of k_theta (ThetaArgMid, Big)
    bool need_theta_image = false;      // k_theta runs (a 2-DoF theta skips it unless somebody reads d_Theta)
    bool host_asm = false;              // scalar assembly and the 2-DoF gradient sum on the host (see h_g11)
    bool grid_tail = false;             // host-assembled theta grid: the gather's tail finishes dL/dtheta (and adds the TV term's)
    bool stream_stats = false, g2_from_imgrad = false;   // k_stats_stream, not k_iwe_finish + k_stats; contrast energy from k_imgrad
    bool tv_proj = false, proj = false; // k_tv / the theta-grid gather project their tile's gradient onto the theta cells themselves
    bool all_r = false;                 // ... the gather with one workgroup per segment for all reference times
    bool events_projected = false; int nsrc = 0;   // k_project's sources: the event term's dL/dTheta image unless projected, the TV term's
    bool zero_copy_out = false;         // k_final writes the results straight into pinned host memory
    SplatForm splat; GatherForm gather; // the event kernels' launches (plan_forms); gather: of a gradient evaluation
};

constexpr int MOTION_PLAN_ARG_WINDOWS = (THETA_ARG_MAX - 4) / 12;   // windows whose q rides in the event kernels' arguments beside (cx, cy, s) (POLY_ARG_WINDOWS)
constexpr size_t ZERO_COPY_MAX = 65536;   // doubles of theta / gradient that cross PCIe by zero-copy access to pinned host memory (a 64-window batch at 16x16: 32768)

inline EvalPlan::Shape theta_shape(const Geom& g, int h, int w) {
    return (h == g.H && w == g.W) ? EvalPlan::IDENTITY : (h == 1 && w == 1) ? EvalPlan::TWO_DOF : EvalPlan::GRID;
}
inline int correlation_kind(const eincm_params* p) { return (int)((p->flags & EINCM_PF_CORRELATION_MASK) >> 8); }
inline bool other_kinds(const eincm_params* p) { return p->contrast_kind > EINCM_CONTRAST_VARIANCE || correlation_kind(p) != EINCM_CORRELATION_MSE; }

// ---- selectable objective kinds (eincm_objectives.hip.h) ----
inline ObjGeom obj_geom(const PlanCtx& c, int ck, int rk, int need) {
    ObjGeom og{};
    og.th = c.obj_th; og.tw = c.obj_tw;
    og.nty = c.g.H / og.th; og.ntx = c.g.W / og.tw; og.ncells = og.nty * og.ntx;
    og.ck = ck; og.rk = rk; og.need = need;
    return og;
}

// The switches an evaluation takes from the environment, read once per process (eincm_api.hip reads them)
struct EvalKnobs {
    bool no_big_arg = false;            // EINCM_NO_BIG_THETA_ARG
    bool no_host_asm = false;           // EINCM_NO_HOST_ASM
    int all_r = -1;                     // EINCM_GATHER_ALL_R (-1: not set)
};

// The LDS window capacities of an evaluation as staged (a pinned capacity, EINCM_WINCAP), and - plan_windows - chosen from vmax, a
// bound of |theta| over the evaluation's windows.  Shared by plan_eval and plan_motion.
inline void plan_windows_preset(const PlanCtx& c, EvalPlan& P) {
    const Geom& g = c.g;
    P.wincap = g.wincap; P.winmaxw = g.winmaxw; P.wincap_a = g.wincap_a; P.winmaxw_a = g.winmaxw_a;
    P.pitch_aligned = c.stage.pitch != 0 ? 1 : 0;
    P.win_2 = WinFit{c.wincap, win_maxw(c.wincap), c.stage.pitch >= 2, true};   // (a pinned capacity, EINCM_WINCAP: the pitch as staged)
}
inline void plan_windows(const PlanCtx& c, EvalPlan& P, double vmax, bool two_dof) {
    // the window's margin: +-(radius + 1) pixels (the taps and the rounding); 4 for the default 3x3 splat
    const double margin = 2.0 * (c.splat_rad + 1);
    // Where a larger window costs no residency it is taken at once (a capacity is an allocation, the windows themselves stay as small
    // as their segments need): the 2-DoF kernels hold nothing but the window in LDS, 4608 words = 18 KiB still gives the 8 workgroups
    // of 4 waves a CU can hold; the theta-grid gather carries 32 KiB beside its window and runs 3 workgroups per CU up to 5461 words.
    // The theta-grid splat (window + 16 KiB Theta tile) pays for capacity with workgroups per CU (6 / 5 / 4 / 3), so it takes what it needs.
    // Each list's windows are sized for its time span: what all but 3 % of the events' segments stay within (cut_segments; the mean
    // tile would size them for the dense tiles alone and send the taps of the sparse ones, whose single segment spans the whole window, to HBM)
    const int floor_s = two_dof ? 2 : 0, pitch_s = c.stage.pitch != 0 ? 1 : 0;
    WinFit s = fit_window(vmax, c.splat.tspan, margin, floor_s, pitch_s);
    // a 2-DoF theta whose spread over a long splat segment outgrows the largest window: the short list (half the time span); the taps
    // of a window that is too small go to HBM one by one (117 px per window: 1220 us on the long list, 544 us on the short one)
    P.splat_short = two_dof && c.splat_sh.n > 0 && !s.fits;
    if (P.splat_short) s = fit_window(vmax, c.splat_sh.tspan, margin, floor_s, pitch_s);
    P.wincap = s.cap; P.winmaxw = s.maxw; P.pitch_aligned = s.pal ? 1 : 0;
    // the gather's own list: longer segments see a longer time span, hence a larger displacement spread; a window too small for it
    // sends taps down the direct path
    const WinFit a = fit_window(vmax, c.gather.tspan, margin, 2, -1);
    P.wincap_a = a.cap; P.winmaxw_a = a.maxw;
    // and the 2-DoF gather's list (pitch = width: at the aligned pitch it measured equal on the bench batch and 63 -> 68 us on another
    // batch of the same shape, profiles/r03/pitch_by_shape.txt; EINCM_PITCH_ALIGNED=2 aligns it too)
    P.win_2 = fit_window(vmax, c.gather_2.tspan, margin, 2, c.stage.pitch >= 2 ? 1 : 0);
}

inline const SegList& seg_list(const PlanCtx& c, ListId id) {
    return id == ListId::GATHER ? c.gather : id == ListId::SPLAT ? c.splat : id == ListId::SPLAT_SHORT ? c.splat_sh : c.gather_2;
}

// The event kernels' launch forms of a planned evaluation (its shape, windows, proj and all_r are set): which instantiation runs, and
// the threads, LDS bytes, list, event copy and window geometry that must agree with its template arguments.  A combination the entry
// points refuse (weights or a motion model with another splat window, weights with a motion model) has no row: the launch reports it.
inline void plan_forms(const PlanCtx& c, EvalPlan& P) {
    const bool two_dof = P.shape == EvalPlan::TWO_DOF, fused = P.shape == EvalPlan::MOTION;
    const int mode = two_dof ? THETA_CONST : fused ? THETA_POLY : THETA_TILE, rad = c.splat_rad, wt = c.stage.weighted ? 1 : 0;
    const size_t theta_tile = two_dof ? 0 : TS * TS * 2 * sizeof(double);      // LDS beside the window: the tile's double2 velocities
    const size_t scratch = fused ? POLY_SCRATCH_BYTES : 0;
    SplatForm& s = P.splat;
    s.list = P.splat_short ? ListId::SPLAT_SHORT : ListId::SPLAT;              // (a 2-DoF theta derives its windows itself)
    if (rad == 1) {
        s.key = SplatKey{mode, rad, NT_TILE, wt};
        s.row = form_row(SPLAT_FORMS, s.key);
        s.wincap = P.wincap; s.winmaxw = P.winmaxw;
        s.lds = (size_t)s.wincap * sizeof(float) + theta_tile + scratch;
    } else {
        // another splat window (eincm_splat_window.hip.h): u64 LDS windows, capped so that they fit beside the Theta tile
        s.key = SplatKey{mode, rad, NT, wt};
        s.row = form_row(SPLAT_R_FORMS, s.key);
        s.wincap = std::min(P.wincap, two_dof ? SW_CAP_CONST : SW_CAP_TILE); s.winmaxw = win_maxw(s.wincap);
        s.lds = (size_t)s.wincap * sizeof(unsigned long long) + theta_tile + scratch;
    }
    if (!P.want_grad) return;
    // Theta grids / dense theta / motion models: the gather walks its own segment list (long segments: its per-workgroup costs - Theta
    // tile, accumulator clear and flush - want them long even for one window) on its own copy of the events (k_segsort); 2-DoF theta:
    // the 2-DoF gather list (shorter segments) on the splat's copy, deriving its windows itself (no window table)
    GatherForm& a = P.gather;
    a.list = two_dof ? ListId::GATHER_2DOF : ListId::GATHER;
    a.copy = two_dof ? EventCopy::SPLAT : EventCopy::GATHER;
    a.wg_per_seg = P.all_r ? 1 : c.g.R;
    a.wincap = two_dof ? P.win_2.cap : P.wincap_a; a.winmaxw = two_dof ? P.win_2.maxw : P.winmaxw_a;
    a.pitch_aligned = two_dof ? (P.win_2.pal ? 1 : 0) : P.pitch_aligned;
    a.lds = (size_t)a.wincap * sizeof(float) + (two_dof ? 0 : TS * TS * 2 * sizeof(double) + theta_tile) + scratch;
    const bool templated = rad == 1 && !two_dof;        // the grid and motion forms of k_gather: 512 threads, `wide` a template argument
    a.key = GatherKey{mode, rad, templated && c.stage.wide ? 1 : 0, templated ? NT_TILE : NT, P.proj ? 1 : 0, P.all_r ? 1 : 0, wt};
    a.row = rad == 1 ? form_row(GATHER_FORMS, a.key) : form_row(GATHER_R_FORMS, a.key);
}

// Every decision of one evaluation, from the context's state, the call's device-resident theta (io) and its checked arguments.
// No HIP calls, no side effects (eval_begin's).
inline EvalPlan plan_eval(const PlanCtx& c, const DevIo& io, const EvalKnobs& knobs, const double* theta_host, int h, int w,
                          const eincm_params* p, bool want_grad) {
    const Geom& g = c.g;
    EvalPlan P;
    P.shape = theta_shape(g, h, w);
    const bool identity = P.shape == EvalPlan::IDENTITY, two_dof = P.shape == EvalPlan::TWO_DOF;
    P.h = h; P.w = w; P.nth = (size_t)h * w * 2;
    P.want_grad = want_grad;
    P.full_aux = (p->flags & EINCM_PF_FULL_AUX) != 0;
    P.div_grad = p->delta != 0.0 && want_grad;
    EvalParams& ep = P.ep;
    ep.alpha = p->alpha; ep.beta = p->beta; ep.gamma = p->gamma; ep.delta = p->delta;
    ep.cur_pyr_lvl = p->cur_pyr_lvl; ep.contrast_kind = p->contrast_kind;
    ep.want_div = (P.full_aux || p->delta != 0.0) ? 1 : 0;
    ep.want_tv = ((p->cur_pyr_lvl <= 0) && (p->gamma != 0.0 || P.full_aux)) ? 1 : 0;
    ep.use_tv_grad = (ep.want_tv && p->gamma != 0.0 && want_grad && !(p->flags & EINCM_PF_NO_TV_GRAD)) ? 1 : 0;
    ep.h = h; ep.w = w; ep.identity = identity ? 1 : 0;
    P.obj = other_kinds(p);
    const int ck = p->contrast_kind, rk = correlation_kind(p);
    if (P.obj) P.og = obj_geom(c, ck, rk, (ck == EINCM_CONTRAST_ADAPTIVE_GRAD_MAG ? OBJ_NEED_TILE_GM : 0) |
                                          ((ck == EINCM_CONTRAST_GRAD_MAG || rk == EINCM_CORRELATION_JOINT_CONTRAST) ? OBJ_NEED_GM : 0) |
                                          (rk == EINCM_CORRELATION_JOINT_CONTRAST ? OBJ_NEED_JOINT : 0));
    if (c.fp64) return P;           // f64_launch: one segment list, one launch form, none of the launch policy below
    const size_t nall = (size_t)g.B * P.nth;

    // theta in the kernel arguments: up to THETA_ARG_MAX doubles in every kernel's; k_theta alone takes a larger one in its own (a 16x16
    // grid of one window: 4 KiB), the event kernels then read the Theta image, or a 2-DoF theta from the pinned staging buffer
    P.use_arg = !io.theta && !identity && nall <= (size_t)THETA_ARG_MAX;
    P.use_arg_big = !io.theta && !identity && nall <= (size_t)THETA_ARG_BIG && !knobs.no_big_arg;
    P.theta_src = io.theta ? EvalPlan::THETA_DEVICE
                : (P.use_arg_big && (P.use_arg || !two_dof)) ? EvalPlan::THETA_ARGS
                : nall <= ZERO_COPY_MAX ? EvalPlan::THETA_PINNED : EvalPlan::THETA_PIECES;
    // (device-resident theta: no host copy for ensure_theta_image to rebuild the image from)
    P.need_theta_image = !two_dof || ep.want_tv || io.theta;

    // LDS window capacity for this evaluation: the host knows theta, hence the largest displacement a segment can see.
    // Small windows give 8 workgroups per CU; windows too small for the flow push taps onto the slow direct-to-HBM path.
    plan_windows_preset(c, P);
    if (!c.wincap_fixed) {
        double vmax = 0.0;
        const size_t stride = nall > 8192 ? nall / 8192 : 1;            // dense theta: sample (any capacity is correct; 65536 samples cost 90 us)
        if (io.theta) vmax = (io.vmax >= 0.0 && std::isfinite(io.vmax)) ? io.vmax : 1e9;      // unknown: the largest windows
        else if (stride == 1) { for (size_t i = 0; i < nall; ++i) { const double a = std::fabs(theta_host[i]); vmax = std::max(vmax, a <= 1.7e308 ? a : 0.0); } }   // (vectorises)
        else for (size_t i = 0; i < nall; i += stride) { const double a = std::fabs(theta_host[i]); if (a > vmax && std::isfinite(a)) vmax = a; }
        plan_windows(c, P, vmax, two_dof);
    }

    // 2-DoF theta with nothing but the contrast and correlation terms (every level above 0 of the reference's pyramid at its first
    // level, and the bench workload), or a theta grid whose gather's tail finishes the gradient (not with another splat window), TV
    // included (k_tv projects its own gradient, the tail combines it; a 2-DoF theta with TV keeps k_final): host assembly
    const bool tail_ok = c.splat_rad == 1 && P.shape == EvalPlan::GRID && c.proj_in_gather && c.itembase_valid && nall <= ZERO_COPY_MAX &&
                         !io.theta;
    P.host_asm = want_grad && ((two_dof && !ep.want_tv) || tail_ok) && !ep.want_div && !P.full_aux && !knobs.no_host_asm && !c.device_results &&
                 !io.theta;
    P.grid_tail = P.host_asm && P.shape == EvalPlan::GRID;
    // Gradient evaluations with the grad-mag contrast take the contrast energy from k_imgrad (which computes the Scharr images anyway),
    // so the statistics are a pure streaming reduction.  A new objective kind: k_stats_stream -> k_obj_parts -> k_obj_grad -> gather;
    // k_final / host_assemble still do the gradient sums and the TV / divergence terms, obj_assemble the contrast and correlation ones.
    P.g2_from_imgrad = want_grad && ep.contrast_kind == EINCM_CONTRAST_GRAD_MAG && !P.obj;
    P.stream_stats = P.host_asm || (P.g2_from_imgrad && g.ntiles >= NSPART) || P.obj;
    // theta grids coarse enough for it: k_tv and k_gather project their tile's gradient onto the theta cells themselves (no k_project)
    P.tv_proj = ep.use_tv_grad && P.shape == EvalPlan::GRID && c.proj_in_gather;
    P.proj = want_grad && P.shape == EvalPlan::GRID && c.proj_in_gather && c.splat_rad == 1;
    // the in-gather projection on big launches: one workgroup per segment for all reference times (8 windows of 10^6 events at 16x16:
    // 792 workgroups of 5 reference times each instead of 3960: 148 -> 135 us; one window: 99 workgroups, 29 -> 84 us - so only where the
    // segments alone fill the chip's 768 workgroup slots of this kernel)
    P.all_r = P.proj && (knobs.all_r >= 0 ? knobs.all_r != 0 : c.gather.n >= 700);
    // k_project's sources: the event term's dL/dTheta image unless a gather projected it (2-DoF: partials), the TV term's unless k_tv did
    P.events_projected = two_dof || P.proj;
    P.nsrc = (!want_grad || identity) ? 0 : (P.events_projected ? 0 : 1) + ((ep.use_tv_grad && !P.tv_proj) ? 1 : 0);
    // small results (everything but a dense gradient) are written by k_final straight into pinned host memory: no D2H copy command
    P.zero_copy_out = !c.device_results && !io.theta && !identity && nall <= ZERO_COPY_MAX;
    plan_forms(c, P);
    return P;
}

// The fused evaluation of a motion model (shape MOTION): the event kernels form the tile's Theta from the
// window's polynomial themselves and the gather reduces its tile to the twelve moments, so there is no theta image, no window table
// and no dense gradient.  Planned like the 2-DoF shape where that fits - the kernels derive their windows, the capacities come from
// the host's bound of the field (vmax; not finite: unknown, the largest windows), theta rides in the event kernels' arguments, the
// results land in pinned memory without a copy command - and like the dense shape where the outputs must be the expanded path's
// bits: the image passes and k_final are the ones plan_eval gives a device-resident dense theta (no host assembly: the host's sums
// of the contrast energy are in another order than k_final's).  all_r: one gather workgroup per segment walks all reference times,
// by the theta-grid rule (the segments alone fill the chip's workgroup slots).  The caller has refused what motion_fused_supported refuses.
inline EvalPlan plan_motion(const PlanCtx& c, const EvalKnobs& knobs, double vmax, const eincm_params* p, bool want_grad) {
    static const double no_theta = 0.0;               // (plan_eval reads no theta of a device-resident one)
    DevIo io;
    io.theta = &no_theta; io.vmax = vmax;
    EvalPlan P = plan_eval(c, io, knobs, nullptr, c.g.H, c.g.W, p, want_grad);
    P.shape = EvalPlan::MOTION;
    P.theta_src = EvalPlan::THETA_ARGS;
    P.use_arg = c.g.B <= MOTION_PLAN_ARG_WINDOWS;
    P.need_theta_image = false;
    P.all_r = want_grad && c.g.R > 1 && (knobs.all_r >= 0 ? knobs.all_r != 0 : c.gather.n >= 700);
    P.events_projected = true;                        // (by the gather itself, onto the moments)
    P.zero_copy_out = true;
    plan_forms(c, P);                                 // (again: the shape and all_r are the motion model's now)
    return P;
}

// The thirteen fields of eincm_get_launch_policy (EINCM_LP_*): the plan of the staged batch and its lists' time spans, and what the
// last evaluation chose (P; evaluated: one has run since the staging - never on a float64 context)
inline void launch_policy(const PlanCtx& c, const EvalPlan& P, bool evaluated, double* out) {
    const StagePlan& S = c.stage;
    out[EINCM_LP_SEG_GATHER] = S.seg; out[EINCM_LP_SEG_SPLAT] = S.seg_s; out[EINCM_LP_SEG_GATHER_2DOF] = S.seg_2;
    out[EINCM_LP_SEG_SPLAT_SHORT] = S.splat_short ? SEG_SHORT : 0; out[EINCM_LP_PITCH_POLICY] = S.pitch;
    out[EINCM_LP_SPAN_SPLAT] = c.splat.tspan; out[EINCM_LP_SPAN_GATHER] = c.gather.tspan; out[EINCM_LP_SPAN_GATHER_2DOF] = c.gather_2.tspan;
    out[EINCM_LP_CAP_SPLAT] = evaluated ? P.wincap : 0; out[EINCM_LP_CAP_GATHER] = evaluated ? P.wincap_a : 0;
    out[EINCM_LP_CAP_GATHER_2DOF] = evaluated ? P.win_2.cap : 0;
    out[EINCM_LP_PITCH_ALIGNED] = evaluated ? ((P.pitch_aligned ? 1 : 0) | (P.win_2.pal ? 2 : 0)) : 0;
    out[EINCM_LP_SPLAT_SHORT] = evaluated && P.splat_short ? 1 : 0;
}

}  // namespace eincm
