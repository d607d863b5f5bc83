/* eincm.h — C-ABI of libeincm_hip.so: the MI355X (gfx950) EINCM objective-and-gradient engine.
 *
 * Drop-in boundary for ONE path of robotic-vision-lab/Edge-Informed-Contrast-Maximization:
 *     loss(theta, events, edge_maps) -> (value, grad)
 * i.e. eincm.losses.loss_func (src/eincm/losses.py:108-205) and the gradient the reference obtains through
 * jaxopt.ScipyMinimize(jit=True) -> jax.value_and_grad (src/eincm/solver.py:165-173).  The reference has no
 * FFI of its own (pure Python on JAX); the binding a maintainer would add is a ctypes stub, shown in
 * INTEGRATION.md.  Plain pointers and sizes only; no torch / HIP types cross this boundary.
 *
 * Conventions
 *   - all host arrays are C-order (row major), caller-owned; nothing is retained after a call returns
 *   - theta / grad / value / ts / edges / edge_ts are double (the SciPy side of the reference is float64,
 *     SURVEY 8b); x, y are int16 (the reference's event wire format, exp_mgr.py:283-284)
 *   - a context is NOT thread-safe; one context per (GPU, caller thread); every call is synchronous except the *_async forms
 *   - return value: 0 = ok, < 0 = error (see EINCM_ERR_*); eincm_last_error() gives the message
 */
#ifndef EINCM_H
#define EINCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EINCM_ABI_VERSION 6   /* 2: eincm_iwe_device_ptr hands out the u64 fixed-point accumulator of the IWE stack; 3: eincm_set_timed_kernels, eincm_set_windows_ptrs;
                                * 4: eincm_loss_grad_masked, eincm_set_device_results / eincm_finish_launch / eincm_grad_device_ptr / eincm_finish_collect, eincm_get_host_profile;
                               * 5: eincm_get_warped_events, eincm_loss_grad_device, eincm_loss_grad_masked_async, eincm_set_timing_period;
                               * 6: eincm_get_launch_policy; added since without a new version: eincm_rectify_events, eincm_remap_cubic, eincm_flow_decode,
                               *    eincm_flow_encode (the DSEC data path), eincm_bfgs_* (BFGS with its state in HBM), eincm_get_memory,
                               *    eincm_flow_eval_stage, eincm_flow_errors (batched flow errors of solved thetas), eincm_lbfgs_* (that BFGS with a limited-memory
                               *    inverse Hessian), eincm_set_motion_model, eincm_loss_grad_motion, eincm_motion_field (parametric motion-field models),
                               *    eincm_loss_grad_motion_fused (the model evaluated inside the event kernels), eincm_set_windows_weighted (per-event weights),
                               *    eincm_event_support (the event-support filter), eincm_event_filter (the refractory and polarity-aware
                               *    filter), eincm_event_scores (an image stack sampled at the warped events), eincm_theta_advect (a solved theta
                               *    carried along its own flow to the next window), eincm_event_responsibilities (those scores normalised over
                               *    the models of a group: the E-step of a motion segmentation), eincm_contrast_landscape (the integer contrast of
                               *    the warped events on a grid of candidate motion coefficients), eincm_set_weights, eincm_get_stage_order,
                               *    eincm_get_staged_weights (a batch staged with EINCM_SW_KEEP_ORDER takes new weights in place), eincm_compose_motions
                               *    (a motion segmentation composed into one flow field and a label image), eincm_densify_motions (that
                               *    composition made dense: every pixel takes the label of its nearest labelled pixel), eincm_label_prior,
                               *    eincm_get_staged_prior, eincm_event_responsibilities_spatial (a per-pixel label prior from the staged
                               *    weights, and the E-step that reads a prior image stack), eincm_carry_label_prior, eincm_adopt_carried_prior,
                               *    eincm_get_carried_prior (a segmentation's label prior carried along the models' own motions to the next window) */

#define EINCM_OK               0
#define EINCM_ERR_ARG         -1   /* bad argument (shape, null pointer, out-of-range event coordinate) */
#define EINCM_ERR_HIP         -2   /* HIP runtime error (message holds hipGetErrorString) */
#define EINCM_ERR_STATE       -3   /* call out of order (e.g. loss_grad before set_windows) */
#define EINCM_ERR_NONFINITE   -4   /* loss or gradient is NaN/Inf (outputs are still written) */
#define EINCM_ERR_UNSUPPORTED -5   /* valid request this build does not implement (e.g. a device-resident entry point of an EINCM_CF_FP64 context) */

/* contrast objective: 0 = mean squared Scharr gradient magnitude of the raw IWE (losses.py:70, the reference's
 * live objective); 1 = variance of the IWE (contrast_objectives.py:29-39; BASELINE config "variance-only") */
#define EINCM_CONTRAST_GRAD_MAG 0
#define EINCM_CONTRAST_VARIANCE 1
/* the tiled ("adaptive") contrasts of contrast_objectives.py:42-87: the sum over the whole th x tw tiles (eincm_set_objective_tiles,
 * default 32 x 42; the ragged right / bottom remainder is ignored) of the tile's mean squared Scharr gradient magnitude, the Scharr
 * taken on each tile alone with zero padding at the tile border (2), or of the tile's population variance (3) */
#define EINCM_CONTRAST_ADAPTIVE_GRAD_MAG 2
#define EINCM_CONTRAST_ADAPTIVE_VARIANCE 3

/* correlation objective K(E_r, n_r) on the edge map and the min-max-normalised IWE (correlation_objectives.py:46-130), selected by
 * EINCM_PF_CORRELATION(kind) in eincm_params.flags.  Sign rule: error-type kinds enter the loss as -K (mse, adaptive_mse, as
 * losses.py:65 does), similarity-type kinds as +K (hadamard, joint_contrast), so that every kind rewards a larger relative
 * correlation.  Not in EINCM_CF_FP64 contexts (EINCM_ERR_UNSUPPORTED) for any kind but the defaults. */
#define EINCM_CORRELATION_MSE            0   /* mean((E - n)^2)                                     (default) */
#define EINCM_CORRELATION_ADAPTIVE_MSE   1   /* sum over the whole tiles of mean((E - n)^2)                   */
#define EINCM_CORRELATION_HADAMARD       2   /* mean(E * n)                                                   */
#define EINCM_CORRELATION_JOINT_CONTRAST 3   /* mean squared Scharr gradient magnitude of E + n (zero padding) */

/* scale_to_sensor_size_method (theta_utils.py:25-35 -> jax.image.scale_and_translate kernels) */
#define EINCM_METHOD_BILINEAR 0    /* 'linear' / 'bilinear' / 'triangle' */
#define EINCM_METHOD_LANCZOS3 1
#define EINCM_METHOD_LANCZOS5 2
#define EINCM_METHOD_CUBIC    3    /* 'cubic' / 'bicubic' */

/* eincm_params.flags */
#define EINCM_PF_NO_TV_GRAD 2u     /* leave the TV term out of the gradient (its value stays in the loss): event-sharded
                                      evaluation adds the replicated TV gradient on one shard only */
#define EINCM_PF_FULL_AUX   1u     /* also evaluate the report-only terms: IWE divergence (losses.py:79-81),
                                      TV at any gamma (losses.py:75), FWL (losses.py:84) */
#define EINCM_PF_CORRELATION_MASK 0x700u                                   /* bits 8-10: EINCM_CORRELATION_* */
#define EINCM_PF_CORRELATION(k)   ((((uint32_t)(k)) << 8) & EINCM_PF_CORRELATION_MASK)

/* eincm_create flags */
#define EINCM_CF_TIMING     1u     /* every stage timed with HIP events (eincm_get_timings): attached to the launch where a stage is one
                                     * kernel, marker events otherwise and around the whole evaluation; costs ~10 % of a step */
#define EINCM_CF_TIMING_DOMINANT 2u /* the two event kernels (k_splat, k_gather) are launched with their own start / stop events
                                     * (hipExtLaunchKernelGGL: no marker packets on the stream) and the events are read when the
                                     * timings are asked for, not after every evaluation; total_ms stays 0 in this mode.
                                     * eincm_set_timed_kernels narrows it to one of the two */

#define EINCM_CF_FP64 4u          /* float64 mode: the same objective and gradient with fp64 arithmetic after the warp (fp64 taps, a u64 IWE
                                    * accumulator at >= 2^40 per unit, fp64 images, an exact 128-bit fixed-point gradient sum; DESIGN.md
                                    * section 10).  The reference's jax_enable_x64: true.  Not with the timing flags, the device-resident
                                    * entry points (eincm_loss_grad_device, eincm_set_device_results ... eincm_finish_collect,
                                    * eincm_iwe_device_ptr), event-sharded staging or eincm_tiled_objectives: those return EINCM_ERR_UNSUPPORTED */

typedef struct eincm_ctx eincm_ctx;

/* The keyword arguments hydra binds to loss_func (configs/theta_loss_func/default.yaml:1-9) */
typedef struct eincm_params {
    double   alpha;          /* contrast weight            losses.py:116 */
    double   beta;           /* correlation weight         losses.py:117 */
    double   gamma;          /* total-variation weight     losses.py:118 (live only if cur_pyr_lvl <= 0, :171) */
    double   delta;          /* IWE-divergence weight      losses.py:119 */
    int32_t  cur_pyr_lvl;    /* losses.py:120 */
    int32_t  method;         /* EINCM_METHOD_*             losses.py:123 */
    int32_t  contrast_kind;  /* EINCM_CONTRAST_* */
    uint32_t flags;          /* EINCM_PF_* */
} eincm_params;

/* aux_info of loss_func (losses.py:195-203) without the two arrays (scaled_theta: eincm_get_scaled_theta,
 * multi_ref_weights: eincm_multi_ref_weights) */
typedef struct eincm_aux {
    double final_loss;
    double mean_rel_corr;
    double mean_rel_contrast;
    double mean_rel_iwe_divergence;   /* NaN unless EINCM_PF_FULL_AUX or delta != 0 */
    double theta_total_variation;     /* 0 if cur_pyr_lvl > 0; NaN if cur_pyr_lvl <= 0, gamma == 0 and no FULL_AUX */
} eincm_aux;

/* per-reference-time scalars of compute_loss_objectives (losses.py:89-105); arrays are [EINCM_MAX_REFS] */
#define EINCM_MAX_REFS 16
typedef struct eincm_objectives_out {
    int32_t n_refs;
    int32_t _pad;
    double correlations[EINCM_MAX_REFS];
    double zero_correlations[EINCM_MAX_REFS];
    double rel_correlations[EINCM_MAX_REFS];
    double contrasts[EINCM_MAX_REFS];
    double zero_contrast;
    double rel_contrasts[EINCM_MAX_REFS];
    double theta_total_variation;
    double theta_divergence;
    double iwe_divergences[EINCM_MAX_REFS];
    double zero_iwe_divergence;
    double rel_iwe_divergences[EINCM_MAX_REFS];
    double flow_warp_losses[EINCM_MAX_REFS];
    double multi_ref_weights[EINCM_MAX_REFS];
    double variances[EINCM_MAX_REFS];          /* extra: var(IWE_r) (contrast_kind = variance) */
    double zero_variance;
} eincm_objectives_out;

/* device time of the last eincm_loss_grad call, per kernel, from HIP events on the engine's stream */
#define EINCM_N_STAGES 10
typedef struct eincm_timings {
    float ms[EINCM_N_STAGES];   /* index = EINCM_STAGE_* ; 0 when the stage did not run */
    float total_ms;             /* first kernel start -> results on host */
} eincm_timings;
#define EINCM_STAGE_CLEAR   0
#define EINCM_STAGE_THETA   1   /* theta upsample + per-tile velocity bounds */
#define EINCM_STAGE_SPLAT   2   /* warp + 3x3 Gaussian splat -> IWE stack (dominant) */
#define EINCM_STAGE_STATS   3   /* min/max/moments/contrast reductions */
#define EINCM_STAGE_IMGRAD  4   /* dL/dIWE image */
#define EINCM_STAGE_GATHER  5   /* backward gather -> dL/dTheta */
#define EINCM_STAGE_TV      6
#define EINCM_STAGE_PROJECT 7   /* adjoint resample dL/dTheta -> dL/dtheta */
#define EINCM_STAGE_FINAL   8
#define EINCM_STAGE_COPY    9

int         eincm_abi_version(void);
const char* eincm_last_error(const eincm_ctx* ctx);   /* ctx may be NULL: error of the last failed eincm_create */

/* One context = one GPU + one stream + capacity for a batch of up to max_windows independent event windows
 * of one sensor size (H, W), each with the same number of reference times.  Windows are what
 * MultipleLevelEINCMSolver.set_datasample holds (solver.py:185-194). */
eincm_ctx*  eincm_create(int device, int H, int W, int max_refs, int max_windows, int64_t max_events_total,
                         uint32_t flags);
void        eincm_destroy(eincm_ctx* ctx);

/* Stage a batch of windows (replaces solver.set_datasample + the theta-independent half of
 * compute_loss_objectives, losses.py:54-55,66,71,80): copies events/edges to HBM, bins events by source
 * tile, and evaluates the zero-warp constants (IUE, its contrast / variance / divergence, zero_corrs).
 *   n_events[b]            events in window b (sum <= max_events_total)
 *   xs, ys, ts             windows concatenated, sum(n_events) entries; 0 <= x < W, 0 <= y < H
 *   edges                  (n_windows, n_refs, H, W); edge_ts (n_windows, n_refs)                      */
int eincm_set_windows(eincm_ctx* ctx, int n_windows, int n_refs, const int64_t* n_events,
                      const int16_t* xs, const int16_t* ys, const double* ts,
                      const double* edges, const double* edge_ts);

/* eincm_set_windows with flags.  EINCM_SW_DEFER_CONSTANTS: stage only; the zero-warp constants are finished later by
 * eincm_forward_iwe(theta = NULL) -> [sum the IWE stacks of all shards] -> eincm_finish_constants (event-sharded mode). */
#define EINCM_SW_DEFER_CONSTANTS 1u
/* EINCM_SW_KEEP_ORDER (eincm_set_windows_ex, _ptrs, _weighted): staging keeps, beside each of its two sorted copies
 * of the events, the position of every slot's event in the batch as it was handed over (4 B per event and copy), and the weights in
 * that order (4 B per event; ones where a window was handed none).  Such a batch is a weighted batch whatever it was handed (all-ones
 * weights give the unweighted batch's bits), with the refusals of one: EINCM_ERR_UNSUPPORTED on a float64 context, with a splat window
 * other than 3, with EINCM_SW_DEFER_CONSTANTS.  It takes new weights without being staged again: eincm_set_weights, and
 * eincm_event_responsibilities with EINCM_RS_APPLY.  The three buffers are allocated by the first staging that asks for them. */
#define EINCM_SW_KEEP_ORDER      2u
int eincm_set_windows_ex(eincm_ctx* ctx, int n_windows, int n_refs, const int64_t* n_events,
                         const int16_t* xs, const int16_t* ys, const double* ts,
                         const double* edges, const double* edge_ts, uint32_t flags);
/* The same with one pointer per window (xs[b], ys[b], ts[b]: n_events[b] values; edges[b]: (n_refs, H, W); edge_ts: (n_windows, n_refs)
 * contiguous): a batch is staged straight from the caller's per-window arrays, as the reference holds them (one datasample tuple per
 * window, src/eincm/solver.py:185-194) - concatenating 8 x 10^6 events on the host first cost 20 of 28 ms. */
int eincm_set_windows_ptrs(eincm_ctx* ctx, int n_windows, int n_refs, const int64_t* n_events,
                           const int16_t* const* xs, const int16_t* const* ys, const double* const* ts,
                           const double* const* edges, const double* edge_ts, uint32_t flags);
/* The same with per-event weights: weights[b] holds n_events[b] floats, finite and within [0, 1]; weights == NULL,
 * or weights[b] == NULL, stands for ones.  I_r[p] = sum_e w_e k_e(p) in every IWE (the zero-warp one included) and dL/dw_e carries the
 * same factor; an event of weight 0 behaves as an absent one in the loss, the gradient, the TV event mask and the count images, and
 * stays in n_events and in eincm_get_warped_events.  The weights are data: there is no dL/dw.  Refused with EINCM_ERR_ARG: a weight
 * out of range or not finite (checked on the host arrays, before the GPU is touched); with EINCM_ERR_UNSUPPORTED: a weighted batch on
 * a float64 context, with a splat window other than 3, or with EINCM_SW_DEFER_CONSTANTS.  eincm_loss_grad_motion_fused refuses a
 * weighted batch (eincm_loss_grad_motion serves it).  A later staging without weights drops the weighted state. */
int eincm_set_windows_weighted(eincm_ctx* ctx, int n_windows, int n_refs, const int64_t* n_events,
                               const int16_t* const* xs, const int16_t* const* ys, const double* const* ts,
                               const double* const* edges, const double* edge_ts, const float* const* weights, uint32_t flags);

/* New weights for the staged events, in place.  weights: NULL, or one host pointer per staged window, each NULL
 * (ones) or n_events[b] floats, finite and within [0, 1], in the order the window's events were handed over.  One upload, one gather
 * through the indices that EINCM_SW_KEEP_ORDER kept, and what staging derives from the weights is formed again: the event mask, the
 * most events on one pixel, the zero-warp constants.  Edges, segment lists and the events themselves are left alone.  Afterwards the
 * context answers every call with the bytes of a fresh eincm_set_windows_weighted(..., weights, EINCM_SW_KEEP_ORDER) of the same
 * windows; the last evaluation, a BFGS begun and the launch policy's evaluation are gone, as after a staging.  Refused before anything
 * is touched (the staged batch and its last evaluation stay): EINCM_ERR_STATE nothing staged, an evaluation in flight, or a batch
 * staged without EINCM_SW_KEEP_ORDER; EINCM_ERR_ARG a weight out of range or not finite. */
int eincm_set_weights(eincm_ctx* ctx, const float* const* weights);
/* The indices a keep-order staging kept: for every slot of the splat's copy of the events (order_splat) and of the gather's
 * (order_gather), sum(n_events) values each, the position of its event in the batch as handed over.  Either may be NULL.  For tests and
 * tools.  EINCM_ERR_STATE without a batch staged with EINCM_SW_KEEP_ORDER. */
int eincm_get_stage_order(eincm_ctx* ctx, uint32_t* order_splat, uint32_t* order_gather);
/* The staged weights of a keep-order batch in the order the events were handed over, window after window: sum(n_events) floats, what
 * the last staging, eincm_set_weights or EINCM_RS_APPLY left.  EINCM_ERR_STATE without a batch staged with EINCM_SW_KEEP_ORDER. */
int eincm_get_staged_weights(eincm_ctx* ctx, float* weights);

/* value_and_grad(loss_func) for every staged window (losses.py:108-205 + its reverse pass).
 *   theta  (n_windows, h, w, 2)     value (n_windows)     grad (n_windows, h, w, 2) or NULL (forward only)
 *   aux    (n_windows) or NULL                                                                         */
int eincm_loss_grad(eincm_ctx* ctx, const double* theta, int h, int w, const eincm_params* p,
                    double* value, double* grad, eincm_aux* aux);

/* Asynchronous form of eincm_loss_grad: _async copies theta, enqueues the whole evaluation on the context's stream and returns;
 * _wait synchronises that stream and hands over (value, grad, aux) exactly as eincm_loss_grad does.  One host thread can keep
 * several contexts in flight this way (one HIP stream each): the host's work for one context (e.g. a solver's line-search bookkeeping)
 * overlaps another context's kernels - the pipelined lockstep solver runs 8 pyramid solves in 0.18 s instead of 0.24 s on two contexts.
 * (Evaluation throughput alone does not gain since round 2: both event kernels are throughput-bound)  No other
 * call on the context is allowed between the two. */
int eincm_loss_grad_async(eincm_ctx* ctx, const double* theta, int h, int w, const eincm_params* p, int want_grad);
int eincm_loss_grad_wait(eincm_ctx* ctx, double* value, double* grad, eincm_aux* aux);

/* eincm_loss_grad for a SUBSET of the staged windows: active[b] != 0 selects window b (NULL = all).  The workgroups of the other
 * windows leave at once, so the call costs about what its active windows cost; their value comes back NaN and their gradient zero.
 * What a lockstep batch solver needs once some of its windows have converged (the reference has no such caller: it solves one window
 * at a time, src/eincm/solver.py:209-216).  Windows beyond the 64th are always evaluated. */
int eincm_loss_grad_masked(eincm_ctx* ctx, const double* theta, int h, int w, const eincm_params* p, const uint8_t* active,
                           double* value, double* grad, eincm_aux* aux);
/* ... and its asynchronous form (collected by eincm_loss_grad_wait): a lockstep solver that drives two contexts keeps the GPU busy with
 * one group of windows while the host advances the other group's line searches */
int eincm_loss_grad_masked_async(eincm_ctx* ctx, const double* theta, int h, int w, const eincm_params* p, const uint8_t* active, int want_grad);

/* handover_loss_func (losses.py:208-276) and d/d(alpha_handover) = <dL/dtheta_ho, prev - theta>:
 *   theta_ho = a*prev_theta + (1-a)*theta;  a (n_windows), value (n_windows), dvalue_da (n_windows) or NULL */
int eincm_handover_loss_grad(eincm_ctx* ctx, const double* alpha_handover, const double* prev_theta,
                             const double* theta, int h, int w, const eincm_params* p,
                             double* value, double* dvalue_da);

/* compute_loss_objectives (losses.py:49-105) on a full-resolution Theta (n_windows, H, W, 2): forward only. */
int eincm_objectives(eincm_ctx* ctx, const double* Theta, eincm_objectives_out* out /* n_windows */);

/* Device images of the last evaluation, copied to host (parity tests / plotting):
 *   iwes (n_windows, n_refs, H, W) float;  zero_iwe (n_windows, H, W) float;
 *   image_grad = dL/dIWE (n_windows, n_refs, H, W) float;  scaled_theta (n_windows, H, W, 2) double   */
int eincm_get_iwes(eincm_ctx* ctx, float* iwes);
int eincm_get_zero_iwe(eincm_ctx* ctx, float* zero_iwe);
int eincm_get_image_grad(eincm_ctx* ctx, float* image_grad);
int eincm_get_scaled_theta(eincm_ctx* ctx, double* scaled_theta);
/* The same images as float64 (the fp64 images of an EINCM_CF_FP64 context; an fp32 context's images widened).  The float forms
 * above return an EINCM_CF_FP64 context's images rounded to float. */
int eincm_get_iwes_f64(eincm_ctx* ctx, double* iwes);
int eincm_get_zero_iwe_f64(eincm_ctx* ctx, double* zero_iwe);
int eincm_get_image_grad_f64(eincm_ctx* ctx, double* image_grad);

/* Integer image of the rounded warped coordinates under the Theta of the last evaluation:
 * counts[b,r,ry,rx] = #{events of window b with round(warp(x,y,t; tau_r)) = (rx,ry)}, JAX wrap/drop index rule
 * (the centre tap of events_to_pdf_frame, src/utils/event_utils.py:32-33,59).  counts (n_windows, n_refs, H, W) uint32.
 * The IWE is a float image; this is its integer skeleton and must equal the reference's bit for bit.
 * Overwrites the dL/dIWE image of the last evaluation (eincm_get_image_grad must be called before it) in fp32 contexts;
 * an EINCM_CF_FP64 context keeps it. */
int eincm_get_count_images(eincm_ctx* ctx, uint32_t* counts);

/* The warped coordinates themselves: warped_xs[r,i] = x_i - Theta[y_i,x_i,0]*(t_i - tau_r) (and ys with component 1) of ONE window's events,
 * in the order they were handed to eincm_set_windows, under the Theta of the last evaluation: the 'warped_xs' / 'warped_ys' entries of
 * compute_loss_objectives (src/eincm/losses.py:58,90-91; per_pix_warp, src/eincm/event_warpers.py:28-37), read only by plotters.
 * warped_xs, warped_ys: (n_refs, n_events[window]) float64 each.  Same operations as the evaluation's warp (product rounded first). */
int eincm_get_warped_events(eincm_ctx* ctx, int window, double* warped_xs, double* warped_ys);

/* Per-event scores: an image stack sampled at the warped events, the adjoint of the splat without the derivative,
 *     s[r, e] = sum over d in {-1,0,1}^2 of  k_{e,r}(d) * F_r[ wrap_drop(round(x'_{e,r}) + d) ]
 * for EVERY event of the staged batch in one call, under the Theta of the last evaluation (the one eincm_get_warped_events uses, also
 * after a 2-DoF, motion-model or fused evaluation).  The warp is the evaluation's, the tap weights k are the splat's for the 3x3 window
 * with the 1/(2 pi), the index rule is the splat's (negative indices wrap once, anything still outside is dropped); a dropped tap
 * contributes 0.  Events are taken in the order they were handed to eincm_set_windows*, window after window.
 *   images       (n_windows, n_refs, H, W) float on the host, or NULL: the IWEs of the last evaluation as eincm_get_iwes returns them,
 *                read on the device without a trip through the host
 *   ref_weights  NULL: window b's block of `scores` is (n_refs, n_events[b]) floats; or n_refs finite doubles omega: the block is
 *                (n_events[b]) floats, sum_r (float)omega_r * s[r, e], summed in fp32 in ascending r.  The blocks follow one another.
 *   selfs        NULL, or laid out as `scores`: sum over the undropped taps of k_{e,r}(d)^2 (combined: sum_r (float)omega_r * self[r, e]),
 *                the event's own unit-weight share of an IWE at its own taps.  A caller forms the leave-one-out score against the IWE as
 *                scores - w_e * selfs with the weight w_e the event was staged with (1 without weights); the kernel never reads the
 *                staged weights.  With H, W >= 3 the three taps of an axis are distinct pixels after the wrap, so the event met each
 *                of its pixels once and the subtraction removes exactly its own share.
 * Arithmetic: fp32 after the fp64 warp.  k(d) = ky * kx is one rounded product; the nine taps are added in one fixed order, rows
 * dy = -1, 0, +1 and within a row dx = -1, 0, +1, by one fused multiply-add each onto a sum that starts at +0, skipping dropped taps.
 * No atomics and no reduction across threads: every run gives the same bytes.  An event whose taps are all dropped (Theta far out of
 * frame) scores exactly 0.
 * Refused before anything is written, in this order: EINCM_ERR_STATE an evaluation in flight; EINCM_ERR_ARG scores == NULL;
 * EINCM_ERR_STATE nothing staged or no evaluation yet; EINCM_ERR_UNSUPPORTED an EINCM_CF_FP64 context, a splat window other than 3
 * (as a weighted batch), an event-sharded staging (EINCM_SW_DEFER_CONSTANTS); EINCM_ERR_ARG a ref_weights entry that is not finite;
 * EINCM_ERR_STATE images == NULL after an evaluation that left windows out (eincm_loss_grad_masked: their IWEs are not current).  A
 * batch with no events at all is valid and writes nothing; a window without events has an empty block. */
int eincm_event_scores(eincm_ctx* ctx, const float* images, const double* ref_weights, float* scores, float* selfs);

/* The E-step of a segmentation into several motions.  The staged batch of B windows is G = B / n_models groups
 * of K = n_models consecutive windows; window b = g * K + l is model l of group g.  The windows of a group have equal n_events and
 * event i of each of them is one event seen under K motions (each window's own staged events are read: nothing else is assumed about
 * them being shared).  Under the last evaluation's Theta, as eincm_event_scores, and for event i of group g:
 *     s_l, q_l  the combined score and self of eincm_event_scores for window g * K + l with omega = ref_weights: the same operations
 *               in the same order, the same bits
 *     a_l  = s_l - w_l * q_l with EINCM_RS_EXCLUDE_SELF (w_l = weights_in[b][i]; a NULL entry or a NULL array is ones), else s_l
 *     a_l  = a_l > 0 ? a_l : +0          (a NaN becomes +0)
 *     p_l  = (float)prior[b] * a_l,      T = sum_l p_l in ascending l from +0
 *     T not > 0 or not finite: the event is unsupported, p_l = (float)prior[b] and T is summed again
 *     w'_l = p_l / T
 * in fp32 without contraction, every operation rounded once; the division is correctly rounded (the plain `/` of a build without
 * fast-math flags, which emits v_div_scale / v_div_fmas / v_div_fixup).
 *   images        as eincm_event_scores: (B, n_refs, H, W) floats, or NULL for the IWEs of the last evaluation
 *   ref_weights   n_refs finite doubles (required)
 *   weights_in    NULL, or B host pointers, each NULL or n_events[b] floats: what the windows were staged with
 *   prior         NULL (ones) or B doubles pi, each finite and >= 0 as a float, every group's float sum positive and finite
 *   flags         0 or any of EINCM_RS_EXCLUDE_SELF, EINCM_RS_STAGED_WEIGHTS, EINCM_RS_APPLY (the last two: below); other bits are reserved
 *   weights_out   NULL, or window b's block of n_events[b] floats w', the blocks one after another: what
 *                 eincm_set_windows_weighted takes back
 *   labels        NULL, or one byte per event of a group, group after group: the lowest l with the largest p_l
 *   mass          NULL, or B doubles: sum_i w' in fp64 in one fixed order (64 events of a wave by halving, the four waves of a
 *                 256-event block in ascending order, the blocks in ascending order from +0); no float atomics, the same bytes on every run
 *   n_unsupported NULL, or G exact counts
 * Refused before anything is written, in this order: EINCM_ERR_STATE an evaluation in flight; EINCM_ERR_ARG all four outputs NULL;
 * EINCM_ERR_STATE nothing staged or no evaluation yet; EINCM_ERR_UNSUPPORTED an EINCM_CF_FP64 context, a splat window other than 3,
 * an event-sharded staging; EINCM_ERR_ARG n_models outside 1 .. EINCM_RS_MAX_MODELS, B not a multiple of n_models, unequal n_events
 * inside a group, ref_weights NULL or not finite, a bad prior; EINCM_ERR_STATE images == NULL after an evaluation that left windows
 * out.  A batch with no events at all is valid and writes nothing.
 * A batch staged with EINCM_SW_KEEP_ORDER has two more flags (without such a batch either is EINCM_ERR_STATE,
 * checked after the refusals above).  EINCM_RS_STAGED_WEIGHTS: w_l is the context's own copy of the staged weights and weights_in must
 * be NULL (EINCM_ERR_ARG otherwise).  EINCM_RS_APPLY: the w' become the staged weights of all B windows as eincm_set_weights would set
 * them, without leaving the device; the four outputs may then all be NULL, and those given are the same bytes as without the flag. */
#define EINCM_RS_MAX_MODELS   8
#define EINCM_RS_EXCLUDE_SELF 1u   /* flags: leave the event's own share out of its score (the leave-one-out score against the IWE) */
#define EINCM_RS_STAGED_WEIGHTS 2u /* flags: w_l comes from the keep-order batch's staged weights, not from weights_in */
#define EINCM_RS_APPLY        4u   /* flags: the responsibilities become the staged weights, in place */
int eincm_event_responsibilities(eincm_ctx* ctx, int n_models, const float* images, const double* ref_weights,
                                 const float* const* weights_in, const double* prior, uint32_t flags,
                                 float* weights_out, uint8_t* labels, double* mass, int64_t* n_unsupported);

/* The contrast landscape over motion coefficients: a global, derivative-free look at the objective that seeds
 * the motion models.  For every window b of the staged batch and every candidate j of n_candidates, the events of the window are
 * warped by the context's motion model (eincm_set_motion_model) at the candidate's coefficients and counted per cell.  The raw events
 * are read as they were staged; staged weights are ignored.  For an event e (x_e, y_e, t_e) that takes part:
 *     q      = M c, formed as eincm_loss_grad_motion forms it (every product rounded, the sum left to right)
 *     Theta  = the model's field at the event's own pixel (y_e, x_e): the bits of eincm_motion_field there
 *     dt     = t_e - t_ref[b]
 *     w      = (double)x_e - Theta_x * dt, and the same in y: the product rounded before the subtraction, no fused multiply-add
 *     r      = rint(w), half to even
 *     the event is in the sensor iff 0 <= r_x < W and 0 <= r_y < H, tested on the doubles (false for a NaN)
 *     outside the sensor the event is DROPPED: the reference's wrap of negative indices to the far side of the image does not apply
 *     an in-sensor event adds 1 to cell (r_y >> log2 cell, r_x >> log2 cell) of a ceil(H / cell) x ceil(W / cell) image of counts
 *   n_candidates  V, 1 .. EINCM_CL_MAX_CANDIDATES
 *   coeffs        (B, V, K) doubles, all finite; K the model's n_coeffs
 *   t_ref         (B) finite doubles
 *   cell          1, 2, 4 or 8
 *   keep          NULL, or B host pointers, each NULL (all events) or n_events[b] bytes: non-zero means the event takes part
 *   sumsq         NULL, or (B, V): the sum over the cells of count^2
 *   n_in          NULL, or (B, V): the number of in-sensor events
 * Every result is an integer: counts by integer atomics in LDS, the squares summed in 64-bit integers, no float accumulated anywhere
 * and nothing accumulated across workgroups, so every run gives the same bytes.  A window without events gives zeros.  Allowed on
 * EINCM_CF_FP64 contexts and with any splat window: it uses neither.
 * Refused before anything is written, in this order: EINCM_ERR_STATE an evaluation in flight; EINCM_ERR_ARG sumsq and n_in both NULL;
 * EINCM_ERR_STATE nothing staged; EINCM_ERR_STATE no motion model set; EINCM_ERR_UNSUPPORTED an event-sharded staging; EINCM_ERR_ARG
 * n_candidates out of range or cell not one of the four; EINCM_ERR_ARG coeffs or t_ref NULL; EINCM_ERR_ARG a coefficient or a t_ref
 * that is not finite (the message names its window and index). */
#define EINCM_CL_MAX_CANDIDATES 4096
int eincm_contrast_landscape(eincm_ctx* ctx, int n_candidates, const double* coeffs, const double* t_ref, int cell,
                             const uint8_t* const* keep, uint64_t* sumsq, uint32_t* n_in);

/* A motion segmentation composed into one flow field and a label image.  The staged batch of B windows is read
 * as G = B / n_models groups of K = n_models consecutive windows that hold the same events, as eincm_event_responsibilities reads it;
 * l is a model of a group, p a sensor pixel, e an event of the group at its raw integer pixel (x_e, y_e).  With w the staged weight of
 * event e in window g * K + l (what eincm_set_windows_weighted, eincm_set_weights or EINCM_RS_APPLY left; 1 in an unweighted batch):
 *     q(w)          = (uint32) rintf(w * 4096.0f): the scaling is exact, the rounding half to even; q <= 4096 as w lies in [0, 1]
 *     mass[g, l, p] = sum of q(w) over the events of window g * K + l with (y_e, x_e) = p, as uint32
 *     total[g, l]   = sum_p mass[g, l, p], as uint64
 *     label[g, p]   = the lowest l with the largest mass[g, l, p] if that mass is > 0, else EINCM_ML_NO_LABEL
 *     f_l(p)        = the motion model's field at p for coeffs[g * K + l]: the bits of eincm_motion_field there
 *     EINCM_ML_HARD:  Theta[g, p] = f_label(p)
 *     EINCM_ML_SOFT:  S = sum_l mass[g, l, p] as uint64, a_l = (double)mass_l / (double)S; Theta = a_0 * f_0, then Theta = Theta + a_l * f_l
 *                     for l = 1 .. K - 1 in order, per component: every division, product and sum rounded on its own, no contraction
 *     a pixel with S = 0 (no event, or every weight quantised to 0) keeps the label EINCM_ML_NO_LABEL and takes the fill:
 *     EINCM_ML_FILL_ZERO: Theta = (0, 0);  EINCM_ML_FILL_DOMINANT: Theta = f_d(p), d the lowest l with the largest total[g, l], or
 *     (0, 0) if that total is 0
 *   n_models  K, 1 .. EINCM_RS_MAX_MODELS
 *   coeffs    (B, K_c) finite doubles, K_c the n_coeffs of the context's motion model (eincm_set_motion_model)
 *   flags     one of EINCM_ML_HARD, EINCM_ML_SOFT | one of EINCM_ML_FILL_ZERO, EINCM_ML_FILL_DOMINANT; other bits are reserved
 *   theta     NULL, or (G, H, W, 2) doubles          labels  NULL, or (G, H, W) bytes
 *   mass      NULL, or (G, n_models, H, W) uint32    total   NULL, or (G, n_models) uint64
 * Integer up to one thread's fp64 blend: no float is accumulated across threads and nothing is accumulated by global atomics, so every
 * run gives the same bytes.  It reads no IWE, so it needs no evaluation, and the splat window does not matter to it.  A batch with no
 * events is valid: its masses and totals are 0, its labels EINCM_ML_NO_LABEL, its Theta all fill.
 * Refused before anything is written, in this order: EINCM_ERR_STATE an evaluation in flight; EINCM_ERR_ARG all four outputs NULL;
 * EINCM_ERR_STATE nothing staged or no motion model set; EINCM_ERR_UNSUPPORTED an EINCM_CF_FP64 context, an event-sharded staging
 * (EINCM_SW_DEFER_CONSTANTS); EINCM_ERR_ARG n_models outside 1 .. EINCM_RS_MAX_MODELS, B not a multiple of n_models, unequal n_events
 * inside a group, coeffs NULL or not finite (the message names window and index), unknown flag bits; EINCM_ERR_UNSUPPORTED a 32x32
 * source tile of one window with 2^20 events or more (then no pixel's sum can reach 2^32: (2^20 - 1) * 4096 < 2^32). */
#define EINCM_ML_HARD          0u   /* flags: every labelled pixel takes the flow of its label */
#define EINCM_ML_SOFT          1u   /* flags: every labelled pixel takes the mass-weighted blend of the models' flows */
#define EINCM_ML_FILL_ZERO     0u   /* flags: a pixel without mass takes (0, 0) */
#define EINCM_ML_FILL_DOMINANT 2u   /* flags: a pixel without mass takes the flow of the group's model of the largest total mass */
#define EINCM_ML_NO_LABEL      255  /* labels: no event with a weight that quantises above 0 fired here */
int eincm_compose_motions(eincm_ctx* ctx, int n_models, const double* coeffs, unsigned flags, double* theta, uint8_t* labels,
                          uint32_t* mass, uint64_t* total);

/* The composition of eincm_compose_motions made dense: a pixel without events takes the label of the nearest
 * pixel that has one, by an exact Euclidean feature transform with a fixed tie rule.  The staged batch, n_models, coeffs, q(w),
 * mass[g, l, p], total[g, l], f_l(p), the label rule, the soft blend and the two flags are eincm_compose_motions'.  Per group g:
 *     site        pixel s is a site iff S(s) = sum_l mass[g, l, s] (as uint64) >= min_site_mass; n_sites[g] counts the sites
 *     nearest     the nearest site of p = (x, y) is the site (x', y') that minimises the key (d2, y', x') lexicographically,
 *                 d2 = (x - x')^2 + (y - y')^2: equal distances go to the lowest row, then to the lowest column.  A site's nearest
 *                 site is itself.  nearest[g, p] = y' * W + x', dist2[g, p] = d2; a group without a site has nearest = -1 and
 *                 dist2 = EINCM_MD_NONE everywhere.  Both are reported whatever max_dist2 is
 *     reached     p is reached iff it has a nearest site and d2 <= max_dist2 (EINCM_MD_UNBOUNDED: no bound)
 *     labels      a reached pixel takes the label of mass[g, :, nearest]; any other pixel EINCM_ML_NO_LABEL
 *     Theta       a reached pixel is composed from the mass vector of its nearest site and the models' fields AT p:
 *                 EINCM_ML_HARD f_label(p), EINCM_ML_SOFT the blend of eincm_compose_motions with the site's masses and f_l(p).
 *                 Any other pixel takes the fill of eincm_compose_motions: EINCM_ML_FILL_ZERO or EINCM_ML_FILL_DOMINANT
 *   min_site_mass  >= 1; 4096 is one event of weight 1, so 2 * 4096 keeps a lone event from owning a cell
 *   theta     NULL, or (G, H, W, 2) doubles     labels  NULL, or (G, H, W) bytes     dist2  NULL, or (G, H, W) uint32
 *   nearest   NULL, or (G, H, W) int32          n_sites NULL, or (G) uint32
 * With min_site_mass = 1 and max_dist2 = 0 theta and labels are the bytes of eincm_compose_motions with the same flags.  Integer up
 * to one thread's fp64 blend, no global atomics: every run gives the same bytes.
 * Refused before anything is written, in the order and with the codes of eincm_compose_motions (EINCM_ERR_ARG all five outputs
 * NULL), then: EINCM_ERR_ARG min_site_mass = 0; EINCM_ERR_UNSUPPORTED a sensor wider than 16384 pixels. */
#define EINCM_MD_NONE      0xFFFFFFFFu   /* dist2: the group has no site */
#define EINCM_MD_UNBOUNDED 0xFFFFFFFFu   /* max_dist2: every pixel of a group with a site is reached */
int eincm_densify_motions(eincm_ctx* ctx, int n_models, const double* coeffs, unsigned flags, uint32_t min_site_mass, uint32_t max_dist2,
                          double* theta, uint8_t* labels, uint32_t* dist2, int32_t* nearest, uint32_t* n_sites);

/* The per-pixel label prior of a segmentation's E-step: every model's share of the mass that the staged
 * weights put into a neighbourhood of a pixel.  The staged batch, n_models, q(w) and mass[g, l, p] are eincm_compose_motions'.  With
 * r = radius, for group g, model l and sensor pixel p = (x, y):
 *     S[g, l, p] = sum of mass[g, l, p'] over the sensor pixels p' = (x', y') with |y' - y| <= r and |x' - x| <= r, as uint64 (a pixel
 *                  outside the sensor counts 0)
 *     n_l = S[g, l, p] + floor_mass,   T = n_0 + n_1 + ... + n_{K-1}, as uint64
 *     P[g * K + l, p] = T == 0 ? 1.0f : (float)((double)n_l / (double)T)
 * T < 2^53 (a pixel's mass is below 2^32, a window holds at most 17^2 pixels, K <= 8), so both conversions to double are exact: one
 * correctly rounded fp64 division and one rounding to float.
 *   n_models    K, 1 .. EINCM_RS_MAX_MODELS         radius  r, 0 .. EINCM_LP_MAX_RADIUS
 *   floor_mass  added to every model's sum (4096 is one event of weight 1): it keeps a model alive where it has no mass yet
 *   flags       0; every bit is reserved
 *   prior       NULL, or (B, H, W) floats            smoothed  NULL, or (G, n_models, H, W) uint64
 * Whatever is downloaded, P stays in the context's device memory as the STAGED PRIOR, which eincm_event_responsibilities_spatial reads
 * in place with EINCM_RS_PRIOR_STAGED.  It is allocated by the first call, dropped by the next eincm_set_windows (any form) and kept
 * across eincm_set_weights and EINCM_RS_APPLY: an EM forms the prior from the weights that its E-step is about to replace.
 * Integer up to one thread's division, no atomics across workgroups: every run gives the same bytes.  It needs staged windows and no
 * evaluation, no motion model, and the splat window does not matter to it.  A batch with no events is valid: S = 0 everywhere.
 * Refused before anything is written, in the order and with the codes of eincm_compose_motions for the faults the two share:
 * EINCM_ERR_STATE an evaluation in flight; EINCM_ERR_STATE nothing staged; EINCM_ERR_UNSUPPORTED an EINCM_CF_FP64 context, an
 * event-sharded staging; EINCM_ERR_ARG n_models outside 1 .. EINCM_RS_MAX_MODELS, B not a multiple of n_models, unequal n_events
 * inside a group, radius outside 0 .. EINCM_LP_MAX_RADIUS, unknown flag bits; EINCM_ERR_UNSUPPORTED a 32x32 source tile of one window
 * with 2^20 events or more.  A refused call leaves the staged prior as it was. */
#define EINCM_LP_MAX_RADIUS 8
int eincm_label_prior(eincm_ctx* ctx, int n_models, int radius, uint32_t floor_mass, unsigned flags, float* prior, uint64_t* smoothed);

/* The staged prior, downloaded: (B, H, W) floats.  EINCM_ERR_STATE without one (no eincm_label_prior since the last eincm_set_windows). */
int eincm_get_staged_prior(eincm_ctx* ctx, float* prior);

/* A segmentation's label prior carried to the next window: every model's mass image is pushed along THAT
 * MODEL'S OWN motion field, so that transparent layers each move their own way, and the label prior is formed on what arrives.  The
 * staged batch, n_models, q(w) and mass[g, l, p] are eincm_compose_motions'; f_l(p) is its field of coeffs[g * K + l] at p, the bits of
 * eincm_motion_field.  For group g and model l:
 *     source    every sensor pixel p = (x, y) with M = mass[g, l, p] > 0 lands at q = p + f_l(p) * tau[g], each product and sum rounded
 *               on its own in fp64.  q not finite or outside (-1, W) x (-1, H): the source deposits nothing
 *     deposit   (x0, y0) = floor(q); the fractions are rounded to 10 bits each, ix = rint((qx - x0) * 1024), iy likewise, ties to even;
 *               tap (x0 + dx, y0 + dy), dx, dy in {0, 1}, has the weight (dx ? ix : 1024 - ix) * (dy ? iy : 1024 - iy): the four sum
 *               to 2^20.  accum[g, l, tap] += M * weight for every tap of weight > 0 on the sensor, as uint64; a tap off the sensor is
 *               dropped
 *     dropped[g, l] = the sum of M * weight over the dropped taps, plus M * 2^20 for every source that deposits nothing, so that
 *               sum_p accum[g, l, p] + dropped[g, l] = 2^20 * sum_p mass[g, l, p] exactly
 *     carried[g, l, p] = min((accum[g, l, p] + 2^19) >> 20, 2^32 - 1) as uint32: half up, saturating
 *     prior     eincm_label_prior's P with carried in the place of mass, radius and floor_mass as there
 * No accumulator overflows: accum <= 2^20 * 4096 * n_events of the model's window, and a batch holds at most 2 * 10^9 < 2^31 events.
 *   n_models    K, 1 .. EINCM_RS_MAX_MODELS            coeffs   (B, n_coeffs) doubles, n_coeffs the motion model's (eincm_set_motion_model)
 *   tau         (G) finite doubles: how far along its field every group's mass moves, in the field's own time unit (px per tau = 1);
 *               0 leaves it where it is, a negative tau moves it backwards
 *   radius, floor_mass   eincm_label_prior's             flags    0; every bit is reserved
 *   prior       NULL, or (B, H, W) floats                carried  NULL, or (G, n_models, H, W) uint32
 *   accum       NULL, or (G, n_models, H, W) uint64      dropped  NULL, or (G, n_models) uint64
 * Whatever is downloaded, P stays in the context's device memory as the CARRIED PRIOR.  It is not the staged prior: that of the staged
 * batch stays as it was, and eincm_set_windows leaves the carried prior alone.  An accepted call marks it invalid at its start and valid
 * once its result is whole.  Integer up to k_label_prior's one division: 64-bit integer atomics, whose sums do not depend on the order
 * of arrival, so every run gives the same bytes.  Coefficients that are not finite, or so large that f * tau is not, are accepted:
 * their sources count in dropped.
 * Refused before anything is written, in the order and with the codes of eincm_label_prior (all of them, its EINCM_ERR_UNSUPPORTED
 * for an EINCM_CF_FP64 context, an event-sharded staging and a crowded tile included), then: EINCM_ERR_ARG coeffs or tau NULL;
 * EINCM_ERR_ARG a tau that is not finite (the message names the group); EINCM_ERR_STATE no motion model set; EINCM_ERR_ARG n_coeffs
 * other than the model's; EINCM_ERR_ARG unknown flag bits; EINCM_ERR_UNSUPPORTED a window of more than 2^32 - 1 events (staging
 * refuses those long before).  A refused call leaves the carried prior as it was, valid or not. */
int eincm_carry_label_prior(eincm_ctx* ctx, int n_models, const double* coeffs, int n_coeffs, const double* tau, int radius,
                            uint32_t floor_mass, unsigned flags, float* prior, uint32_t* carried, uint64_t* accum, uint64_t* dropped);

/* The carried prior becomes the staged prior of the batch that is staged now, by one copy on the device: afterwards
 * eincm_event_responsibilities_spatial reads it with EINCM_RS_PRIOR_STAGED as it reads eincm_label_prior's.  The carried prior stays
 * valid, so it can be adopted again after another staging.  Refused in this order: EINCM_ERR_STATE an evaluation in flight, nothing
 * staged, no valid carried prior; EINCM_ERR_ARG n_models, the staged B or the sensor other than those the carried prior was formed
 * with. */
int eincm_adopt_carried_prior(eincm_ctx* ctx, int n_models);

/* The carried prior, downloaded: (B, H, W) floats of the batch it was formed on.  EINCM_ERR_STATE without a valid one. */
int eincm_get_carried_prior(eincm_ctx* ctx, float* prior);

/* The E-step with a prior image: eincm_event_responsibilities whose mixing weight of model l is
 * prior[b] * P[b, y_e, x_e] at the event's raw pixel (x_e, y_e), the staged coordinates of event i of window b = g * K + l.  Every
 * argument it shares with eincm_event_responsibilities means the same, and so does everything not restated here: s_l, q_l, a_l, the
 * order of the sums, the correctly rounded division, the labels, mass, n_unsupported, EINCM_RS_STAGED_WEIGHTS and EINCM_RS_APPLY.
 *     c_l  = (float)prior[b] * P[b, y_e, x_e]
 *     p_l  = c_l * a_l,      T = sum_l p_l in ascending l from +0
 *     T not > 0 or not finite: the event is unsupported, p_l = c_l and T is summed again; if that T is not > 0 or not finite either,
 *     p_l = (float)prior[b] and T is summed once more.  The event counts as unsupported once, whichever fallback it ends on
 *     w'_l = p_l / T
 * in fp32 without contraction.  With P = 1 everywhere the four outputs are the bytes of eincm_event_responsibilities.
 *   prior_images  (B, H, W) floats, each finite and >= 0, or NULL with EINCM_RS_PRIOR_STAGED: the staged prior of eincm_label_prior
 *                 is read in place
 * Refused as eincm_event_responsibilities refuses, in its order, and after that: EINCM_ERR_ARG prior_images together with
 * EINCM_RS_PRIOR_STAGED; EINCM_ERR_ARG neither of the two; EINCM_ERR_STATE EINCM_RS_PRIOR_STAGED without a staged prior; EINCM_ERR_ARG
 * a value of prior_images that is not finite or is < 0 (the message names window and pixel). */
#define EINCM_RS_PRIOR_STAGED 8u   /* flags: the prior stack is the context's staged prior, not prior_images */
int eincm_event_responsibilities_spatial(eincm_ctx* ctx, int n_models, const float* images, const double* ref_weights,
                                         const float* const* weights_in, const double* prior, const float* prior_images, uint32_t flags,
                                         float* weights_out, uint8_t* labels, double* mass, int64_t* n_unsupported);

/* compute_weights_for_multi_reference (losses.py:39-46) */
int eincm_multi_ref_weights(int n_refs, double* w);

/* weight matrix of jax.image.scale_and_translate along one axis (theta_utils.py:25-35): A (n_out, n_in) */
int eincm_resample_matrix(int n_in, int n_out, int method, double* A);

int eincm_get_timings(eincm_ctx* ctx, eincm_timings* t);
/* EINCM_CF_TIMING_DOMINANT contexts: which of the two event kernels carry timing events from the next evaluation on (both by
 * default).  A timed launch costs ~6 us of an evaluation; a throughput measurement times only the kernel it reports. */
int eincm_set_timed_kernels(eincm_ctx* ctx, int splat, int gather);
/* ... and on every `period`-th evaluation only (1 = every evaluation): a timed launch costs ~6 us of a 240 us step; eincm_get_timings_total
 * reports how many evaluations its sums cover.  The counter restarts with the call. */
int eincm_set_timing_period(eincm_ctx* ctx, int period);

/* Host-side wall time (microseconds, summed since the last reset) the calling thread spent in the phases of the evaluations of
 * this context, and their number: [EINCM_HP_BEGIN] argument checks, theta staging and the launches of the forward half,
 * [EINCM_HP_LAUNCH] the launches of the second half, [EINCM_HP_WAIT] waiting for the stream, [EINCM_HP_COLLECT] handing the
 * results over (incl. the host-side scalar assembly of 2-DoF evaluations).  A diagnostic: what an evaluation costs besides its kernels. */
#define EINCM_HP_BEGIN 0
#define EINCM_HP_LAUNCH 1
#define EINCM_HP_WAIT 2
#define EINCM_HP_COLLECT 3
#define EINCM_N_HOST_PHASES 4
int eincm_get_host_profile(eincm_ctx* ctx, double* us /* EINCM_N_HOST_PHASES */, int64_t* n_evals, int reset);
/* Diagnostic: how the staged batch is cut into work and how the last evaluation was launched (no counterpart in the reference; the
 * numbers behind DESIGN.md section 4.2 "where those rules hold").  Staging decides the segment lengths and whether the batch is in
 * the regime of the bank-aligned LDS pitch; every evaluation decides the LDS window capacities from max|theta| and the time span
 * that all but 3 % of the events' segments stay within.  Entries of the last evaluation are 0 before the first one. */
#define EINCM_LP_SEG_GATHER 0        /* events per segment: the theta-grid gather's list */
#define EINCM_LP_SEG_SPLAT 1         /* ... k_splat's list */
#define EINCM_LP_SEG_GATHER_2DOF 2   /* ... the 2-DoF gather's list */
#define EINCM_LP_SEG_SPLAT_SHORT 3   /* ... k_splat's short list for very large 2-DoF theta (0: none was built) */
#define EINCM_LP_PITCH_POLICY 4      /* 0: LDS windows at pitch = width; 1: k_splat's at the bank-aligned pitch where that costs no capacity class; 2: the 2-DoF gather's too */
#define EINCM_LP_SPAN_SPLAT 5        /* fraction of a window's duration the capacity of k_splat's windows is sized for */
#define EINCM_LP_SPAN_GATHER 6
#define EINCM_LP_SPAN_GATHER_2DOF 7
#define EINCM_LP_CAP_SPLAT 8         /* last evaluation: LDS window capacity in 32-bit words, k_splat */
#define EINCM_LP_CAP_GATHER 9        /* ... theta-grid gather */
#define EINCM_LP_CAP_GATHER_2DOF 10  /* ... 2-DoF gather */
#define EINCM_LP_PITCH_ALIGNED 11    /* last evaluation: bit 0 k_splat, bit 1 the 2-DoF gather took the aligned pitch */
#define EINCM_LP_SPLAT_SHORT 12      /* last evaluation: k_splat walked its short list */
#define EINCM_N_LAUNCH_POLICY 13
int eincm_get_launch_policy(eincm_ctx* ctx, double* out /* EINCM_N_LAUNCH_POLICY */);

/* What the context holds right now: [0] bytes of device memory, [1] bytes of pinned host memory, [2] the number of live allocations
 * behind the two, [3] bytes of the scratch block the one-shot operators share (part of [0]).  Read from the context's own books: no
 * HIP call.  Two reads around a call that are equal show that the call allocated nothing. */
int eincm_get_memory(eincm_ctx* ctx, int64_t out[4]);
/* sums of the per-evaluation timings since the last reset, and how many evaluations they cover (a bench reads them once after
 * its timed loop instead of calling eincm_get_timings inside it) */
int eincm_get_timings_total(eincm_ctx* ctx, eincm_timings* sum, int64_t* n_evals, int reset);

/* The evaluation with theta AND gradient resident in HBM, for a caller whose optimiser lives on the GPU: only the scalars cross PCIe
 * (a dense theta at 480x640 otherwise moves 2 x 4.9 MB per evaluation: ~380 of its ~590 us).  The reference's optimiser is on the host
 * (src/eincm/solver.py:165-173), so this has no counterpart there.
 *   theta_dev      (n_windows, h, w, 2) float64 in the memory of the context's device, complete when the call is made (the engine runs
 *                  on its own stream: synchronise the stream that produced theta first)
 *   theta_abs_max  an upper bound of |theta| (px per unit time) if the caller has one, < 0 otherwise: it only selects the capacity of
 *                  the LDS windows (any value is correct - results agree to a fixed-point quantum; a bound far too small or unknown costs speed)
 *   value          (n_windows) on the HOST; aux optional, on the host
 *   grad_dev       (n_windows, h, w, 2) float64 on the device, or NULL for a forward-only evaluation; complete on return
 * EINCM_ERR_NONFINITE reports a non-finite value or theta (the device gradient is not scanned). */
int eincm_loss_grad_device(eincm_ctx* ctx, const double* theta_dev, int h, int w, const eincm_params* p, double theta_abs_max,
                           double* value, double* grad_dev, eincm_aux* aux);

/* Event-sharded mode over a GPU collective (RCCL): keep the results of the finishing half in HBM so that the caller can all-reduce
 * the gradient there, instead of bouncing it through the host.  eincm_set_device_results(ctx, 1) once; then per evaluation
 *   eincm_forward_iwe -> [all-reduce the IWE accumulator] -> eincm_finish_launch (returns with the gradient complete in HBM)
 *   -> [all-reduce eincm_grad_device_ptr's n_doubles doubles] -> eincm_finish_collect (copies value / gradient / aux to the host).
 * 2-DoF evaluations run their scalar assembly on the GPU again in this mode (k_final), so that the gradient exists in HBM. */
int eincm_set_device_results(eincm_ctx* ctx, int on);
int eincm_finish_launch(eincm_ctx* ctx);
int eincm_grad_device_ptr(eincm_ctx* ctx, void** dptr, int64_t* n_doubles);
int eincm_finish_collect(eincm_ctx* ctx, double* value, double* grad, eincm_aux* aux);

/* Event-sharded evaluation: the events of the SAME windows are split over several contexts (one per GPU);
 * edges and edge_ts are replicated.  The IWE is additive over events (src/utils/event_utils.py:59 is a pure sum), so
 *   every shard:  eincm_forward_iwe(theta)            k_theta + k_splat on its own events; returns stream-synchronised
 *   caller:       all-reduce(sum) of the IWE stacks   (RCCL on eincm_iwe_device_ptr; (n_windows, n_refs, H, W) int64: the engine
 *                                                      accumulates pixel * 2^30 as 64-bit integers, so the sum over shards is exact
 *                                                      and independent of the reduction order)
 *   every shard:  eincm_finish_loss_grad              statistics ... gradient on the summed stack
 * gives the same value on every shard and gradients that SUM to the full gradient (pass EINCM_PF_NO_TV_GRAD on all but
 * one shard).  Staging: eincm_set_windows_ex(..., EINCM_SW_DEFER_CONSTANTS), all-reduce(max) of the event masks
 * (eincm_mask_device_ptr, uint8), eincm_forward_iwe(theta = NULL), all-reduce(sum) of the IWE stacks, eincm_finish_constants. */
int eincm_forward_iwe(eincm_ctx* ctx, const double* theta, int h, int w, const eincm_params* p, int want_grad);
int eincm_finish_loss_grad(eincm_ctx* ctx, double* value, double* grad, eincm_aux* aux);
int eincm_finish_constants(eincm_ctx* ctx);
int eincm_iwe_device_ptr(eincm_ctx* ctx, void** dptr, int64_t* n_words);   /* n_words 64-bit integers */
int eincm_mask_device_ptr(eincm_ctx* ctx, void** dptr, int64_t* n_bytes);

/* ---- the step that produces `edges`, and the tiled objectives ------------------------------------ */
#define EINCM_EDT_EXPONENTIAL 0   /* 1 - exp(-d / alpha)        img_utils.py:232, :382 */
#define EINCM_EDT_LINEAR 1        /* d                          img_utils.py:376       */
#define EINCM_EDT_LINEAR_BOUND 2  /* min(d, d_sat)              img_utils.py:378       */
#define EINCM_EDT_LOGARITHMIC 3   /* log(d + 1)                 img_utils.py:380       */

/* Inverse (exponential) distance transform of binary edge images: replaces eincm_inv_exp_dist_transform
 * (src/utils/img_utils.py:229-233, scipy.ndimage.distance_transform_edt) and RTEF_IEDT.compute_edge_iedt
 * (img_utils.py:236-410, Meijster transform) - both are  1 - minmax(f(d))  of the exact Euclidean distance d to the
 * nearest edge pixel.  edge_img (n, H, W) uint8, non-zero = edge, H x W = the context's sensor; out (n, H, W) double;
 * sqdist (n, H, W) int32 or NULL receives d^2 (integer work: equals the reference's bit for bit).
 * An image without any edge pixel has no distance transform: EINCM_ERR_ARG. */
int eincm_inv_dist_transform(eincm_ctx* ctx, const uint8_t* edge_img, int n, int formulation, double alpha, double d_sat,
                             double* out, int32_t* sqdist);

/* smoothen_edges (img_utils.py:210-220): cv.GaussianBlur of a float64 image with the kernel size derived from sigma
 * (round(8 sigma + 1) | 1 taps), separable, BORDER_REFLECT_101.  src, dst (n, H, W) double; may alias. */
int eincm_gaussian_blur(eincm_ctx* ctx, const double* src, int n, double sigma, double* dst);

/* image_to_edge (img_utils.py:192-208): cv.Canny(src, threshold1, threshold2, None, aperture_size, l2_gradient) of 8-bit
 * grayscale images - OpenCV's integer Canny (Sobel with BORDER_REPLICATE, sector NMS, hysteresis over 8-connected survivors;
 * DESIGN.md section 13), exact.  src, dst (n, H, W) uint8, H x W = the context's sensor; dst is 0 / 255.  The thresholds are
 * swapped if threshold1 > threshold2; negative or non-finite ones and n < 1 are EINCM_ERR_ARG, aperture_size != 3 is
 * EINCM_ERR_UNSUPPORTED.  Integer work: fp32 and EINCM_CF_FP64 contexts give the same bytes. */
int eincm_canny(eincm_ctx* ctx, const uint8_t* src, int n, double threshold1, double threshold2, int aperture_size, int l2_gradient,
                uint8_t* dst);

/* preprocess_image (img_utils.py:131-189), the clean-up in front of Canny, on 8-bit grayscale images; the stages selected by
 * `stages` run in this order, each on the previous stage's uint8 output:
 *   EINCM_PRE_NLMEANS    cv.fastNlMeansDenoising(img, None, denoise_h, denoise_template_win, denoise_search_win), NORM_L2
 *   EINCM_PRE_CLAHE      cv.createCLAHE(clahe_clip_limit, (clahe_tiles_x, clahe_tiles_y)).apply; tiles_x splits the width
 *   EINCM_PRE_UNSHARP    cv.addWeighted(img, sharpen_alpha, cv.GaussianBlur(img, None, 0, sharpen_sigma), sharpen_beta, 0): the
 *                        8-bit fixed-point blur with cvRound(6 sigma + 1) | 1 taps (sharpen_sigma is sigmaX as OpenCV receives it)
 *   EINCM_PRE_BILATERAL  cv.bilateralFilter(img, bilateral_d, bilateral_sigma_color, bilateral_sigma_space)
 * Borders are BORDER_REFLECT_101.  src, dst (n, H, W) uint8, H x W = the context's sensor; they may alias.  Only the selected stages'
 * fields are read.  EINCM_ERR_ARG, before any device work: stages 0 or outside EINCM_PRE_ALL, n < 1, denoise_h <= 0 or
 * non-finite, even or non-positive window sizes, a tile count below 1 or above its image side, a non-finite clip limit, sharpen_sigma
 * <= 0 or non-finite, non-finite sharpen weights or bilateral sigmas.  EINCM_ERR_UNSUPPORTED: denoise_template_win > 7,
 * denoise_search_win > 21, more than 129 blur taps, a bilateral radius above 32.  Integer work and float32 work in a fixed order:
 * the same bytes on every run and in fp32 and EINCM_CF_FP64 contexts. */
#define EINCM_PRE_NLMEANS 1
#define EINCM_PRE_CLAHE 2
#define EINCM_PRE_UNSHARP 4
#define EINCM_PRE_BILATERAL 8
#define EINCM_PRE_ALL 15
typedef struct eincm_preprocess_params {
    int32_t stages;                               /* EINCM_PRE_* bits */
    double denoise_h;                             /* filter strength h */
    int32_t denoise_template_win, denoise_search_win;   /* odd; <= 7 and <= 21 */
    double clahe_clip_limit;                      /* <= 0: no clipping */
    int32_t clahe_tiles_x, clahe_tiles_y;         /* tileGridSize (x splits the width) */
    double sharpen_sigma, sharpen_alpha, sharpen_beta;
    int32_t bilateral_d;                          /* <= 0: radius cvRound(1.5 sigma_space) */
    double bilateral_sigma_color, bilateral_sigma_space;  /* <= 0 becomes 1 */
} eincm_preprocess_params;
int eincm_preprocess_image(eincm_ctx* ctx, const uint8_t* src, int n, const eincm_preprocess_params* params, uint8_t* dst);

/* extract_tiles (img_utils.py:105-120) + compute_adaptive_* (contrast_objectives.py:42-87, correlation_objectives.py:105-130)
 * and their pairwise siblings (correlation_objectives.py:28-102), on the images of the LAST evaluation, per (window, ref):
 * contrast-type objectives on the raw IWE (as losses.py:70 does), pair-type ones on (edges, min-max-normalised IWE)
 * (as losses.py:65 does).  Whole tiles only; the ragged remainder is ignored, as in the reference. */
typedef struct eincm_tiled_out {
    int32_t n_refs, n_tiles;
    double adaptive_mean_gradient_magnitude[EINCM_MAX_REFS];
    double adaptive_variance[EINCM_MAX_REFS];
    double adaptive_mean_squared_error[EINCM_MAX_REFS];
    double sum_squared_error[EINCM_MAX_REFS];
    double mean_hadamard_product[EINCM_MAX_REFS];
    double sum_hadamard_product[EINCM_MAX_REFS];
    double joint_contrast[EINCM_MAX_REFS];
} eincm_tiled_out;
int eincm_tiled_objectives(eincm_ctx* ctx, int tile_h, int tile_w, eincm_tiled_out* out /* n_windows */);

/* Tile size of the adaptive objective kinds in the differentiable loss (EINCM_CONTRAST_ADAPTIVE_*, EINCM_CORRELATION_ADAPTIVE_MSE),
 * per context, default 32 x 42 (contrast_objectives.py:56-59); 1 <= tile <= sensor in each dimension, else EINCM_ERR_ARG.  The
 * zero-warp values of the kinds are computed again on the next evaluation that needs them.  eincm_tiled_objectives keeps its own
 * arguments. */
int eincm_set_objective_tiles(eincm_ctx* ctx, int tile_h, int tile_w);

/* Size s of the Gaussian splat that forms every IWE of the context (events_to_pdf_frame's window_size, event_utils.py:13-61): every
 * event adds exp(-|q|^2 / 2) / (2 pi) at the (2w+1)^2 pixels round(x) + d, d in [-w, w]^2, w = s / 2 (integer division: 2 behaves as 3,
 * 4 as 5, 6 as 7, 1 is the centre tap alone).  1 <= s <= EINCM_SPLAT_WINDOW_MAX, else EINCM_ERR_ARG; default 3.  It applies to the
 * zero-warp, warped, forward-only and handover IWEs; the count images and eincm_get_warped_events do not depend on it.  On a staged
 * batch the window constants (c0, zero_corrs, d0, the zero-warp values of the objective kinds) are formed again at once; after an
 * event-sharded staging (EINCM_SW_DEFER_CONSTANTS) a change is EINCM_ERR_STATE, so is a call while an asynchronous evaluation is in
 * flight.  An EINCM_CF_FP64 context accepts 3 only (EINCM_ERR_UNSUPPORTED). */
#define EINCM_SPLAT_WINDOW_MAX 7
int eincm_set_splat_window(eincm_ctx* ctx, int window_size);

/* MVSEC's ground-truth flow of a batch of evaluation windows: estimate_gt_flow / _prop_flow (mvsec_loader.py:322-433) with the index
 * and time arithmetic done by the caller (evaluation.gt_flow_plan), DESIGN.md section 15.  Window b has mode[b] and the steps
 * [step_off[b], step_off[b + 1]) of (step_frame, step_num, step_den):
 *   EINCM_GTF_DIRECT     exactly one step: out = ((double)g[f] * num) / den, x and y (the window fits one GT interval)
 *   EINCM_GTF_PROPAGATE  each pixel's float32 position walks the steps in order: read the frame's flow at (rintf(cx), rintf(cy)), 0
 *                        outside the frame or at NaN (cv.remap INTER_NEAREST, constant 0 border); a 0 read clears that component's
 *                        mask; cx = (float)((double)cx + fx * num), unfused.  out = mask ? (double)(cx - (float)x) : 0, per component.
 *                        step_den is not read in this mode.
 * gt_x, gt_y (n_frames, H, W), H x W = the context's sensor, float (elem_bytes 4) or double (elem_bytes 8); a float stack gives the
 * same output as the same stack widened to double.  out (n_windows, H, W, 2) double.  EINCM_ERR_ARG, before any device work: a null
 * pointer, n_frames < 1, n_windows < 1, elem_bytes not 4 or 8, an unknown mode, step_off[0] != 0, a window with no steps or a direct
 * window with more than one, a step_frame outside [0, n_frames), a non-finite step_num, a zero or non-finite step_den.  No reduction
 * and no atomics: the same bytes on every run and in fp32 and EINCM_CF_FP64 contexts. */
#define EINCM_GTF_DIRECT 0
#define EINCM_GTF_PROPAGATE 1
int eincm_gt_flow(eincm_ctx* ctx, const void* gt_x, const void* gt_y, int elem_bytes, int n_frames, int n_windows, const int32_t* mode,
                  const int32_t* step_off, const int32_t* step_frame, const double* step_num, const double* step_den, double* out);

/* The DSEC data path.  Arrays in memory only: no file is read or written.
 *
 * DSECDataLoader.rectify_events (dsec_loader.py:145-171) for one chunk of n <= 2^30 events.  rectify_map (H, W, 2) float, channel 0 = x,
 * H x W the context's sensor: (rx, ry) = rectify_map[y][x]; rec = (int16)rint(r), rint in float, half to even; an event is kept iff
 * 0 <= rec_x < W and 0 <= rec_y < H.  keep (n) gets 1 / 0 per event, rec_x and rec_y (capacity n) the kept events' coordinates in
 * stream order (a stable compaction; the same bytes on every run), *n_kept their number.  A non-null rectify_map is uploaded, checked and
 * becomes the context's map; a later chunk of the same recording passes NULL.  EINCM_ERR_ARG: a map entry that is not finite or
 * whose rounding does not fit int16 (checked once, when the map is handed over; the context then has no map), an event coordinate outside
 * the sensor (the outputs are not written).  EINCM_ERR_STATE: NULL map and no map in the context. */
int eincm_rectify_events(eincm_ctx* ctx, const float* rectify_map, const int16_t* x, const int16_t* y, int64_t n, int16_t* rec_x,
                         int16_t* rec_y, uint8_t* keep, int64_t* n_kept);

/* The spatiotemporal support filter (background-activity filter) of a raw event stream, one chunk of n <= 2^30 events per call
 * (DESIGN.md section 23).  Stream order is the order handed over; times are finite and non-decreasing.  The neighbours of pixel p are
 * the pixels q != p within Chebyshev distance radius (1..3) of p, inside the sensor and not masked.  For event e at p, neighbour q is
 * supported iff q's most recent event j < e in stream order has t[e] - t[j] <= tau (one double subtraction, one compare; no earlier
 * event: not supported; equal times support the later index only).  support[e] = the number of supported neighbours (uint8, may be
 * NULL), weights[e] = (float)min(support, full_support) / (float)full_support, 1 <= full_support <= (2 radius + 1)^2 - 1.  An event's
 * own pixel never supports it.  pixel_mask (H, W) uint8 or NULL, non-zero = masked: events there get support 0 and weight 0 and give
 * no support.  The context carries, from chunk to chunk, the time of every pixel's last event (allocated by the first call) and the
 * time of the last event handed over; reset != 0 clears both before the chunk, so any split of a stream into consecutive chunks
 * gives the bytes of the unsplit call.  n == 0 is valid and writes nothing.  EINCM_ERR_ARG, before any output is written and with
 * the carried state unchanged, naming the first offender's index: a coordinate outside the sensor, a non-finite time, a time smaller
 * than its predecessor's (or than the carried last time when reset == 0); also tau not finite or negative, radius or full_support
 * out of range, n outside [0, 2^30], a null x, y, t or weights with n > 0.  EINCM_ERR_STATE: an evaluation is in flight.  Integer
 * counts and no floating-point sums: the same bytes on every run, in fp32 and EINCM_CF_FP64 contexts. */
int eincm_event_support(eincm_ctx* ctx, const int16_t* x, const int16_t* y, const double* t, int64_t n, double tau, int radius,
                        int full_support, const uint8_t* pixel_mask, int reset, float* weights, uint8_t* support);

/* The refractory and polarity-aware filter of a raw event stream, one chunk of n <= 2^30 events per call.
 * An operator beside eincm_event_support: stream order, finite non-decreasing times, the neighbour window, the mask, the refusals
 * and the chunking are that operator's, and the carried state is its own (eincm_event_support's is not touched).  p (n) int8 or
 * NULL: the polarity class of event e is p[e] > 0, NULL puts every event in class 0.  Per event e at pixel P, in stream order:
 *   kept = P not masked and not (t[e] - last_any[P] < refractory), last_any[P] being the time of P's previous event whatever
 *          became of it (none: kept; refractory == 0 keeps every unmasked event; equal times on one pixel with refractory > 0 drop
 *          the later index); then last_any[P] = t[e], for masked events too;
 *   a kept event with radius > 0 counts the neighbours q (as eincm_event_support) with t[e] - L(q) <= tau, where L(q) is the time
 *          of q's last KEPT event: of class c_e under EINCM_EF_POLARITY, of either class without; then last_kept[c_e][P] = t[e].
 *          radius == 0 switches the support stage off (full_support must be 1); a kept event still updates last_kept.
 * keep[e] = kept (uint8); support[e] (uint8, may be NULL) is 0 for dropped events and for radius == 0; weights[e] =
 * (float)min(support, full_support) / (float)full_support with radius > 0, kept ? 1 : 0 with radius == 0.  The context carries the
 * three (H, W) maps last_any, last_kept[0], last_kept[1] (allocated by the first call) and the time of the last event handed over;
 * reset != 0 clears them before the chunk, so any split of a stream into consecutive chunks gives the bytes of the unsplit call.
 * With refractory == 0 and flags == 0, weights and support are the bytes of eincm_event_support.  n == 0 is valid and writes
 * nothing.  EINCM_ERR_ARG, before any output is written and with the carried state unchanged: an event refused as
 * eincm_event_support refuses it (naming the first offender's index); n, refractory, tau, radius, full_support or flags out of
 * range (the first of that order); a flag other than EINCM_EF_POLARITY, EINCM_EF_POLARITY with p == NULL; a null x, y, t, keep or
 * weights with n > 0.  EINCM_ERR_STATE: an evaluation is in flight.  Integer maxima and counts, no floating-point sums: the same
 * bytes on every run, in fp32 and EINCM_CF_FP64 contexts. */
#define EINCM_EF_POLARITY 1   /* flags: support counts only neighbours' kept events of the event's own polarity class */
int eincm_event_filter(eincm_ctx* ctx, const int16_t* x, const int16_t* y, const double* t, const int8_t* p, int64_t n,
                       double refractory, double tau, int radius, int full_support, int flags,
                       const uint8_t* pixel_mask, int reset, uint8_t* keep, float* weights, uint8_t* support);

/* cv.remap(src, map, None, INTER_CUBIC) of 8-bit single-channel images, constant border 0, as a written contract (DESIGN.md section 16;
 * parity with OpenCV itself is not pinned).  src (n, src_h, src_w), 1 <= src_h, src_w <= 32766, independent of the sensor; map (H, W, 2)
 * float, channel 0 = x, one map for the stack; dst (n, H, W).  Per component p = map * 32 in float; NaN: the pixel is 0; p clamped to
 * +-2^30 and rounded half to even to s; integer part s >> 5 clamped to int16, fraction s & 31.  table (32, 32, 16) int32: row
 * (fy, fx) holds the 4 x 4 weights (ky major) of that fraction pair, each within +-32768 and each row summing to 32768 (else
 * EINCM_ERR_ARG; engine.remap_cubic_table builds the contract's).  Taps (iy - 1 .. iy + 2, ix - 1 .. ix + 2), a tap outside the
 * source adds 0; dst = clamp((sum + 2^14) >> 15, 0, 255). */
int eincm_remap_cubic(eincm_ctx* ctx, const uint8_t* src, int n, int src_h, int src_w, const float* map, const int32_t* table, uint8_t* dst);

/* DSECDataLoader.flow_16bit_to_float (dsec_loader.py:247-266): flow16 (n, H, W, 3) uint16 -> flow (n, H, W, 2) double,
 * ((double)c - 32768) / 128 where channel 2 is 1 and 0 elsewhere, and valid (n, H, W) 1 / 0.  *n_bad: pixels whose channel 2 is neither
 * 0 nor 1 (the reference asserts on them); if any, EINCM_ERR_ARG (the outputs are written all the same). */
int eincm_flow_decode(eincm_ctx* ctx, const uint16_t* flow16, int n, double* flow, uint8_t* valid, int64_t* n_bad);

/* dsec_npz_to_png.py:84-96: theta (n, h, w, 2) double is scaled to (H, W) with the bilinear scale_and_translate weights of
 * eincm_resample_matrix and coded as (uint16)trunc(v * 128 + 32768) in double into channels 0 and 1 of out (n, H, W, 3), in one kernel.
 * Channel 2: 0, or valid[n][H][W] != 0 where valid is not NULL.  *n_bad: pixels with a value that is not finite or codes outside
 * [0, 65536) (stored as 0); if any, EINCM_ERR_ARG.  1 <= n <= 65535. */
int eincm_flow_encode(eincm_ctx* ctx, const double* theta, int n, int h, int w, const uint8_t* valid, uint16_t* out, int64_t* n_bad);

/* ---- A solved theta carried along its own flow to the next window ------------------------------------------
 * theta (n, h, w, 2) double, h <= H, w <= W, with tau[n] and gain[n].  Per field: Theta = theta scaled to the sensor (theta itself
 * where (h, w) == (H, W), else eincm_flow_errors' tap sums for `method`); source pixel p lands at q = p + Theta(p) tau and deposits
 * Q = llrint(Theta 2^13) into the four pixels around q with integer bilinear weights (two 10-bit fractions; the four sum to 2^20) by
 * 64-bit integer atomics: taps outside the sensor are dropped, a source whose q is not finite or outside (-1, W) x (-1, H) deposits
 * nothing.  Coverage c = sum of weights 2^-20.  Where c >= min_coverage the difference D = (sum w Q / sum w) 2^-13 - Q(Theta(p)) 2^-13;
 * elsewhere D = 0 (EINCM_TA_FILL_SOURCE) or -Theta(p) (EINCM_TA_FILL_ZERO).  out_theta (n, h, w, 2) = gain (theta + R(D)), R the
 * separable resampling (H, W) -> (h, w) with eincm_resample_matrix's weights for `method`, columns then rows, as ordered float64 sums
 * (the identity for a dense theta).  So tau = 0 returns gain theta and a uniform field returns gain times itself, exactly.
 * out_dense (n, H, W, 2) double = Theta + D and out_coverage (n, H, W) float = c are optional (NULL: not computed, no scratch).
 * Float64 and integer arithmetic of its own: the same bytes on every run and in fp32 and EINCM_CF_FP64 contexts; nothing staged or
 * evaluated is touched.  EINCM_ERR_ARG, in this order: a NULL theta, tau, gain or out_theta; n outside 1..65535; h or w outside
 * 1..H / 1..W; a sensor of more than 2^21 pixels; an unknown method; an unknown fill; a tau or gain that is not finite; min_coverage
 * outside (0, 1]; a theta value that is not finite or with |theta| L > 511, L = the largest product of the absolute row and column
 * tap sums (1 for bilinear and for a dense theta).  EINCM_ERR_STATE (after the cheap checks, before the value range): an evaluation
 * is in flight. */
#define EINCM_TA_FILL_SOURCE 0
#define EINCM_TA_FILL_ZERO   1
int eincm_theta_advect(eincm_ctx* ctx, const double* theta, int n, int h, int w, int method, const double* tau, const double* gain, int fill,
                       double min_coverage, double* out_theta, double* out_dense, float* out_coverage);

/* ---- Flow errors of a batch of solved thetas -------------------------------------------------------------
 * sparse_flow_error (flow_eval.py:14-76) on per_pix_theta_to_flow (theta_utils.py:40-73) of every window of a batch: stage the ground
 * truth once, evaluate many thetas against it.  "valid" below is the reference's mask: both components are not +-inf and
 * sqrt(x x + y y) > 0 in double (false for NaN and for a norm that underflows to 0).
 *
 * eincm_flow_eval_stage keeps, in device memory of the context that no other call touches, gt_flow (n_windows, H, W, 2) and one flag
 * byte per pixel: bit 0 = an evaluation event of the window sits on the pixel AND (eval_mask is NULL OR eval_mask[b][y][x] != 0),
 * bit 1 = the GT flow is valid.  Window b's events are the next n_events[b] entries of xs / ys (the windows' events concatenated);
 * a window may have none.  eval_mask (n_windows, H, W) or NULL.  It is independent of eincm_set_windows: a staging, an evaluation or
 * any other operator in between leaves it intact; a later eincm_flow_eval_stage replaces it.
 * EINCM_ERR_ARG before any device work and without allocating: a null pointer (eval_mask excepted), n_windows outside 1..65535, a
 * negative n_events.  EINCM_ERR_STATE: an evaluation is in flight.  EINCM_ERR_ARG after the events were looked at: an event outside the
 * sensor; the context then has NO staged flow evaluation.
 *
 * eincm_flow_errors evaluates theta (n_windows, h, w, 2) of the staged batch, h <= H, w <= W.  The predicted flow of a pixel with
 * bit 0 is theta itself where (h, w) == (H, W), else sum_i a_i (sum_j b_j theta[i0 + i][j0 + j]) over the non-zero runs of the rows of
 * eincm_resample_matrix(h, H, method) and (w, W, method), j inside i, unfused (eincm_flow_encode's arithmetic, for every method).
 * Where it is valid the pixel counts in n_pred; where bit 1 is set too it is in the intersection: ee = sqrt(dx dx + dy dy),
 * ree = ee / (sqrt(gx gx + gy gy) + eps), eps = 2^-52, unfused, IEEE sqrt and division.  out[b]: n_ee (intersection), n_pred, n_gt,
 * n_over[k] = pixels with ee > N_k strictly (N = 1, 2, 3, 5, 10, 20), sum_ee and sum_ree in the fixed order of DESIGN.md section 18,
 * aee = sum_ee / n_ee and aree = sum_ree / n_ee (NaN where n_ee == 0), anpe[k] = (double)(n_over[k] * 100) / ((double)n_ee + eps).
 * ee_map (n_windows, H, W) or NULL: ee in the intersection, NaN elsewhere.  NaN / inf in theta or the GT are data.  The same bytes on
 * every run and in fp32 and EINCM_CF_FP64 contexts; both calls return with the stream drained.
 * EINCM_ERR_ARG before any device work: a null pointer (ee_map excepted), an unknown method, h or w < 1, h > H or w > W.
 * EINCM_ERR_STATE: no staged flow evaluation, an evaluation in flight. */
typedef struct eincm_flow_error_out {
    int64_t n_ee, n_pred, n_gt;
    int64_t n_over[6];                    /* N = 1, 2, 3, 5, 10, 20 */
    double sum_ee, sum_ree, aee, aree;
    double anpe[6];
} eincm_flow_error_out;
int eincm_flow_eval_stage(eincm_ctx* ctx, int n_windows, const double* gt_flow, const int64_t* n_events, const int16_t* xs,
                          const int16_t* ys, const uint8_t* eval_mask);
int eincm_flow_errors(eincm_ctx* ctx, const double* theta, int h, int w, int method, eincm_flow_error_out* out, double* ee_map);

/* ---- BFGS with its state in HBM --------------------------------------------------------------------------
 * B = the staged windows (at most EINCM_BFGS_MAX_WINDOWS), each an independent BFGS minimisation (SciPy's _minimize_bfgs) over
 * n = 2 h w <= EINCM_BFGS_MAX_N unknowns.  The point X, its gradient G, the direction P, the trial point Xt, its gradient Gt (B, n) and
 * the inverse Hessian H (B, n, n) live in the context's device memory, allocated at the first eincm_bfgs_begin and grown on demand.
 * The host keeps the line search, which needs phi(a) = f(X + a P) and phi'(a) = Gt . P only, and sees scalars.  Every sum is an
 * ordered float64 sum in a fixed association: the same bits on every call and in every context.  Masks are (n_windows) bytes, NULL =
 * every window; the state of a window outside the mask is not touched.  All calls return with the context's stream drained.
 * Refusals: EINCM_ERR_STATE before eincm_set_windows, before eincm_bfgs_begin (or after a later eincm_set_windows), while an
 * asynchronous evaluation is in flight, with eincm_set_device_results on; EINCM_ERR_ARG for n above the maximum, more windows than
 * EINCM_BFGS_MAX_WINDOWS, a null pointer, an unknown accept mode; EINCM_ERR_UNSUPPORTED in an EINCM_CF_FP64 context (the device-resident
 * evaluation does not exist there). */
#define EINCM_BFGS_MAX_N 1024
#define EINCM_BFGS_MAX_WINDOWS 64
/* eincm_bfgs_accept: what happens to window b */
#define EINCM_BFGS_SKIP   0   /* nothing */
#define EINCM_BFGS_UPDATE 1   /* s = a P, y = Gt - G, r = 1 / y.s (1000 where y.s == 0), w = (c / 2) s - r H y with c = r (1 + r y.Hy);
                                 H += s w^T + w s^T (bit-symmetric), X <- Xt, G <- Gt, P = -H G */
#define EINCM_BFGS_MOVE   2   /* X <- Xt, G <- Gt only: the step that ends a minimisation (SciPy tests the new gradient before it updates H) */
#define EINCM_BFGS_INIT   3   /* X <- Xt, G <- Gt, P = -G: after the first evaluation (H = I since eincm_bfgs_begin) */
/* scalars of a window after eincm_bfgs_accept, EINCM_BFGS_NS doubles */
#define EINCM_BFGS_S_DPHI0  0   /* G . P: phi'(0) of the next line search */
#define EINCM_BFGS_S_GMAX   1   /* max |G| */
#define EINCM_BFGS_S_PNORM  2   /* |P|_2 */
#define EINCM_BFGS_S_XMAX   3   /* max |X|; with the next one a bound of |theta| at any step: max|X| + |a| max|P| */
#define EINCM_BFGS_S_PMAX   4   /* max |P| */
#define EINCM_BFGS_S_GNORM  5   /* |G|_2 (SciPy's first step guess: old_old_fval = f0 + |g0|_2 / 2) */
#define EINCM_BFGS_S_YS     6   /* y . s and y . H y of an EINCM_BFGS_UPDATE (0 otherwise) */
#define EINCM_BFGS_S_YHY    7
#define EINCM_BFGS_NS 8
/* Start minimisations over theta grids (h, w, 2) at x0_host (n_windows, h, w, 2) for the windows of `active`: X = x0, H = I, P = G = 0. */
int eincm_bfgs_begin(eincm_ctx* ctx, const double* x0_host, int h, int w, const uint8_t* active);
/* One function evaluation per window of `active`, on the context's stream with one synchronisation: Xt = X + alpha[b] P, the masked loss
 * and gradient with theta = Xt and the gradient into Gt (both in HBM), dphi[b] = Gt . P and gmax[b] = max |Gt|.  alpha, value, dphi,
 * gmax: (n_windows) on the host; entries outside the mask are not written, except value (NaN, as eincm_loss_grad_masked).
 * EINCM_ERR_NONFINITE as eincm_loss_grad_device (the outputs are written). */
int eincm_bfgs_eval(eincm_ctx* ctx, const eincm_params* p, const double* alpha, const uint8_t* active, double* value, double* dphi,
                    double* gmax);
/* The two steps around the engine on their own, for any objective whose gradient the caller computes on the device: eincm_bfgs_trial
 * forms Xt; the caller writes the gradient at Xt into Gt (eincm_bfgs_trial_ptrs: n_doubles = n_windows * n each; the writes must be
 * complete when eincm_bfgs_reduce is called); eincm_bfgs_reduce returns dphi and gmax as eincm_bfgs_eval does. */
int eincm_bfgs_trial(eincm_ctx* ctx, const double* alpha, const uint8_t* active);
int eincm_bfgs_reduce(eincm_ctx* ctx, const uint8_t* active, double* dphi, double* gmax);
int eincm_bfgs_trial_ptrs(eincm_ctx* ctx, void** xt_dptr, void** gt_dptr, int64_t* n_doubles);
/* Device pointers of X, G, P (n_windows * n doubles each) and H (n_windows * n * n), and the two sizes: the whole state as arrays
 * (inspection, tests, a caller that seeds H). */
int eincm_bfgs_state_ptrs(eincm_ctx* ctx, void** x_dptr, void** g_dptr, void** p_dptr, void** hess_inv_dptr, int* n_windows, int* n);
/* End of a line search: accept_mode[b] (EINCM_BFGS_*) with the step alpha[b] whose evaluation was the window's last one.
 * scalars_out (n_windows, EINCM_BFGS_NS) on the host: the rows of the windows that took part are new, the others keep their last values. */
int eincm_bfgs_accept(eincm_ctx* ctx, const double* alpha, const uint8_t* accept_mode, double* scalars_out);
/* X and G (n_windows, n) and, unless NULL, H (n_windows, n, n) to the host; x or g may be NULL. */
int eincm_bfgs_fetch(eincm_ctx* ctx, double* x, double* g, double* hess_inv);

/* ---- The limited-memory form of that state ------------------------------------------------------------------
 * The same minimisations with the inverse Hessian kept as a ring of at most `history` pairs (s, y) per window instead of a matrix, so n
 * is bounded by memory alone: theta grids beyond EINCM_BFGS_MAX_N unknowns and the dense per-pixel theta.  eincm_lbfgs_begin puts the
 * context's optimiser state into this form; eincm_bfgs_eval / _trial / _reduce / _trial_ptrs / _accept / _fetch then operate on it
 * (eincm_bfgs_fetch requires hess_inv == NULL, eincm_bfgs_state_ptrs returns NULL for H), with the accept modes and scalars above and
 * two differences: an EINCM_BFGS_UPDATE stores the pair s = a P, y = Gt - G only if y.s > 2.220446049250313e-16 y.y (the oldest pair
 * leaves a full ring) and takes P = sum_j delta_j b_j from the dot-matrix form of the two-loop recursion over the basis b = [s.., y.., G];
 * and slot EINCM_BFGS_S_YHY holds y.y.  EINCM_BFGS_INIT empties the ring.  eincm_bfgs_begin switches the state back to the dense form.
 * Refusals: those of eincm_bfgs_begin except its bound on n; EINCM_ERR_ARG for a history outside 1 .. EINCM_LBFGS_MAX_HISTORY or an
 * unknown initial_scale. */
#define EINCM_LBFGS_MAX_HISTORY 16
#define EINCM_LBFGS_SCALE_IDENTITY  0   /* the recursion starts from H0 = I */
#define EINCM_LBFGS_SCALE_LAST_PAIR 1   /* ... from H0 = (y.s / y.y) I of the newest pair (I while the ring is empty) */
int eincm_lbfgs_begin(eincm_ctx* ctx, const double* x0_host, int h, int w, const uint8_t* active, int history, int initial_scale);
/* Device pointers of the rings S and Y (n_windows, history, n) by ring slot, the dot matrix D (n_windows, 2 history + 1, 2 history + 1)
 * and the coefficients delta (n_windows, 2 history + 1), both indexed s of slot k at k, y of slot k at history + k, G at 2 history, and of
 * the int32 ring head (the oldest pair's slot) and count (n_windows each): inspection and tests. */
int eincm_lbfgs_history_ptrs(eincm_ctx* ctx, void** s_dptr, void** y_dptr, void** d_dptr, void** delta_dptr, void** head_dptr,
                             void** count_dptr, int* history);

/* ---- Parametric motion-field models as a theta mode --------------------------------------------------------
 * The unknowns of a window are K <= 12 coefficients c of a polynomial motion field of degree <= 2 instead of a theta grid.  With the
 * normalised coordinates u = (x - cx) / scale, v = (y - cy) / scale and the monomials m = [1, u, v, u u, u v, v v], q = M c (M row
 * major (12, K), a left-to-right sum over k) gives
 *     Theta_x(x, y) = ((((q0 m0 + q1 m1) + q2 m2) + q3 m3) + q4 m4) + q5 m5,     Theta_y likewise from q6 .. q11,
 * in px per unit time: every product rounded, the sums left to right, u u, u v, v v rounded once each.  The evaluation is the dense
 * device-resident one (eincm_loss_grad_device) on that field; the gradient is M^T mu with the moments mu_j = sum_pix m_j dL/dTheta_x
 * (j < 6) or m_(j-6) dL/dTheta_y, ordered float64 sums: the same bits on every call and in every context.
 * Refusals: EINCM_ERR_ARG for n_coeffs outside 1 .. EINCM_MOTION_MAX_COEFFS, a non-finite M, cx or cy, a scale that is not a positive
 * finite number, a null pointer; EINCM_ERR_STATE with no model set, no staged windows, an evaluation in flight or
 * eincm_set_device_results on; EINCM_ERR_UNSUPPORTED in an EINCM_CF_FP64 context (it has no device-resident evaluation). */
#define EINCM_MOTION_MAX_COEFFS 12
#define EINCM_MOTION_NQ 12              /* polynomial coefficients q of the two components */
typedef struct eincm_motion_model {
    int32_t n_coeffs;                   /* K */
    double cx, cy, scale;               /* the centre (principal point) in px and the normalising length (focal length) in px */
    double M[EINCM_MOTION_NQ * EINCM_MOTION_MAX_COEFFS];   /* (12, K) row major: the first 12 K entries are read */
} eincm_motion_model;
/* The model of every later eincm_loss_grad_motion / eincm_motion_field (copied); NULL clears it. */
int eincm_set_motion_model(eincm_ctx* ctx, const eincm_motion_model* model);
/* Loss and gradient with respect to the coefficients.  coeffs (n_windows, K) and grad (n_windows, K) or NULL on the host; active
 * (n_windows) bytes or NULL: windows outside it get value NaN and gradient 0, as eincm_loss_grad_masked gives.  p->method is not read
 * (the field is at sensor size); the TV term's share is in the gradient.  EINCM_ERR_NONFINITE as eincm_loss_grad_device (the outputs
 * are written).  eincm_get_scaled_theta afterwards returns the field. */
int eincm_loss_grad_motion(eincm_ctx* ctx, const double* coeffs, const eincm_params* p, const uint8_t* active, double* value, double* grad,
                           eincm_aux* aux);
/* The field alone: Theta (n_windows, H, W, 2) on the host. */
int eincm_motion_field(eincm_ctx* ctx, const double* coeffs, double* Theta);
/* eincm_loss_grad_motion by the fused path: the event kernels form the field of their source tile from the
 * window's polynomial and reduce the tile's gradient to the twelve moments themselves; no Theta image and no dense gradient exist
 * during the evaluation.  Same arguments and the same masked-window contract (value NaN, gradient 0, coefficients not read).  The
 * value, the IWE stack and every image pass are the bits eincm_loss_grad_motion gives; the gradient is the same sum in another order.
 * A window whose q = M c (or the bound of its field) is not finite sits the launch out: its value and gradient are NaN and the call
 * returns EINCM_ERR_NONFINITE with the other windows' outputs written.  EINCM_ERR_UNSUPPORTED, with the reason in eincm_last_error,
 * where the path does not apply: the TV term active (level <= 0 and gamma != 0), EINCM_PF_FULL_AUX, a splat window other than 3, an
 * EINCM_CF_FP64 context; EINCM_ERR_STATE as eincm_loss_grad_motion.  eincm_get_scaled_theta, eincm_get_count_images and
 * eincm_get_warped_events afterwards build the field from the evaluation's q. */
int eincm_loss_grad_motion_fused(eincm_ctx* ctx, const double* coeffs, const eincm_params* p, const uint8_t* active, double* value, double* grad,
                                 eincm_aux* aux);

#ifdef __cplusplus
}
#endif
#endif /* EINCM_H */
