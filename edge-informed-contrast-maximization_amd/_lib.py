"""ctypes binding of libeincm_hip.so (C-ABI: include/eincm.h).  No CPU fallback: a missing library raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EINCM_LIB') or os.path.join(_HERE, 'libeincm_hip.so')      # EINCM_LIB: a developer's variant build (tools/build_variant.sh)

MAX_REFS = 16
N_STAGES = 10
STAGE_NAMES = ('clear', 'theta', 'splat', 'stats', 'imgrad', 'gather', 'tv', 'project', 'final', 'copy')

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_NONFINITE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
CONTRAST_GRAD_MAG, CONTRAST_VARIANCE = 0, 1
CONTRAST_ADAPTIVE_GRAD_MAG, CONTRAST_ADAPTIVE_VARIANCE = 2, 3
CONTRAST_KINDS = {'grad_mag': 0, 'variance': 1, 'adaptive_grad_mag': 2, 'adaptive_variance': 3}
CORRELATION_MSE, CORRELATION_ADAPTIVE_MSE, CORRELATION_HADAMARD, CORRELATION_JOINT_CONTRAST = 0, 1, 2, 3
CORRELATION_KINDS = {'mse': 0, 'adaptive_mse': 1, 'hadamard': 2, 'joint_contrast': 3}
PF_CORRELATION_SHIFT = 8
PF_CORRELATION_MASK = 0x700    # eincm_params.flags bits 8-10: the correlation kind
DEFAULT_OBJECTIVE_TILE = (32, 42)
SPLAT_WINDOW_MAX = 7         # EINCM_SPLAT_WINDOW_MAX: splat window sizes 1..7 (eincm_set_splat_window)
DEFAULT_SPLAT_WINDOW = 3
METHODS = {'linear': 0, 'bilinear': 0, 'triangle': 0, 'lanczos3': 1, 'lanczos5': 2, 'cubic': 3, 'bicubic': 3}
PF_FULL_AUX = 1
PF_NO_TV_GRAD = 2
SW_DEFER_CONSTANTS = 1
SW_KEEP_ORDER = 2           # EINCM_SW_KEEP_ORDER: staging keeps its event order (Engine.set_windows(..., keep_order=True))
CF_TIMING = 1
CF_TIMING_DOMINANT = 2
CF_FP64 = 4                # float64 mode (Engine(..., precision='fp64'))
PRECISIONS = ('fp32', 'fp64')
BFGS_MAX_N, BFGS_MAX_WINDOWS = 1024, 64                              # EINCM_BFGS_MAX_N, EINCM_BFGS_MAX_WINDOWS
BFGS_SKIP, BFGS_UPDATE, BFGS_MOVE, BFGS_INIT = 0, 1, 2, 3            # eincm_bfgs_accept modes (EINCM_BFGS_*)
BFGS_S_DPHI0, BFGS_S_GMAX, BFGS_S_PNORM, BFGS_S_XMAX, BFGS_S_PMAX, BFGS_S_GNORM, BFGS_S_YS, BFGS_S_YHY = range(8)   # EINCM_BFGS_S_*
BFGS_NS = 8
LBFGS_MAX_HISTORY = 16                                               # EINCM_LBFGS_MAX_HISTORY
LBFGS_SCALES = {'identity': 0, 'last_pair': 1}                       # EINCM_LBFGS_SCALE_*
MOTION_MAX_COEFFS, MOTION_NQ = 12, 12                                # EINCM_MOTION_MAX_COEFFS, EINCM_MOTION_NQ
TA_FILL_SOURCE, TA_FILL_ZERO = 0, 1                                  # EINCM_TA_FILL_*
TA_FILLS = {'source': TA_FILL_SOURCE, 'zero': TA_FILL_ZERO}
RS_MAX_MODELS, RS_EXCLUDE_SELF = 8, 1                                # EINCM_RS_MAX_MODELS, EINCM_RS_EXCLUDE_SELF
RS_STAGED_WEIGHTS, RS_APPLY = 2, 4                                   # EINCM_RS_STAGED_WEIGHTS, EINCM_RS_APPLY (a keep-order batch)
RS_PRIOR_STAGED = 8                                                  # EINCM_RS_PRIOR_STAGED (eincm_event_responsibilities_spatial)
LP_MAX_RADIUS = 8                                                    # EINCM_LP_MAX_RADIUS (eincm_label_prior)
CL_MAX_CANDIDATES = 4096                                             # EINCM_CL_MAX_CANDIDATES
CL_CELLS = (1, 2, 4, 8)                                              # the cell sizes of eincm_contrast_landscape
ML_HARD, ML_SOFT, ML_FILL_ZERO, ML_FILL_DOMINANT = 0, 1, 0, 2        # EINCM_ML_* flags of eincm_compose_motions
ML_MODES = {'hard': ML_HARD, 'soft': ML_SOFT}
ML_FILLS = {'zero': ML_FILL_ZERO, 'dominant': ML_FILL_DOMINANT}
ML_NO_LABEL = 255                                                    # EINCM_ML_NO_LABEL
ML_Q_ONE = 4096                                                      # the quantised weight of 1 (csrc/eincm_motion_layers.h)
MD_NONE, MD_UNBOUNDED = 0xFFFFFFFF, 0xFFFFFFFF                       # EINCM_MD_NONE (dist2), EINCM_MD_UNBOUNDED (max_dist2) of eincm_densify_motions


class Params(C.Structure):
    _fields_ = [('alpha', C.c_double), ('beta', C.c_double), ('gamma', C.c_double), ('delta', C.c_double),
                ('cur_pyr_lvl', C.c_int32), ('method', C.c_int32), ('contrast_kind', C.c_int32), ('flags', C.c_uint32)]


class Aux(C.Structure):
    _fields_ = [('final_loss', C.c_double), ('mean_rel_corr', C.c_double), ('mean_rel_contrast', C.c_double),
                ('mean_rel_iwe_divergence', C.c_double), ('theta_total_variation', C.c_double)]


_A = C.c_double * MAX_REFS


class ObjectivesOut(C.Structure):
    _fields_ = [('n_refs', C.c_int32), ('_pad', C.c_int32),
                ('correlations', _A), ('zero_correlations', _A), ('rel_correlations', _A),
                ('contrasts', _A), ('zero_contrast', C.c_double), ('rel_contrasts', _A),
                ('theta_total_variation', C.c_double), ('theta_divergence', C.c_double),
                ('iwe_divergences', _A), ('zero_iwe_divergence', C.c_double), ('rel_iwe_divergences', _A),
                ('flow_warp_losses', _A), ('multi_ref_weights', _A), ('variances', _A), ('zero_variance', C.c_double)]


PRE_NLMEANS, PRE_CLAHE, PRE_UNSHARP, PRE_BILATERAL = 1, 2, 4, 8      # eincm_preprocess_params.stages (EINCM_PRE_*)
PRE_ALL = 15
PRE_STAGES = {'nlmeans': 1, 'clahe': 2, 'unsharp': 4, 'bilateral': 8}


class PreprocessParams(C.Structure):
    _fields_ = [('stages', C.c_int32), ('denoise_h', C.c_double),
                ('denoise_template_win', C.c_int32), ('denoise_search_win', C.c_int32),
                ('clahe_clip_limit', C.c_double), ('clahe_tiles_x', C.c_int32), ('clahe_tiles_y', C.c_int32),
                ('sharpen_sigma', C.c_double), ('sharpen_alpha', C.c_double), ('sharpen_beta', C.c_double),
                ('bilateral_d', C.c_int32), ('bilateral_sigma_color', C.c_double), ('bilateral_sigma_space', C.c_double)]


class TiledOut(C.Structure):
    _fields_ = [('n_refs', C.c_int32), ('n_tiles', C.c_int32),
                ('adaptive_mean_gradient_magnitude', _A), ('adaptive_variance', _A), ('adaptive_mean_squared_error', _A),
                ('sum_squared_error', _A), ('mean_hadamard_product', _A), ('sum_hadamard_product', _A), ('joint_contrast', _A)]


GTF_DIRECT, GTF_PROPAGATE = 0, 1        # eincm_gt_flow window modes (EINCM_GTF_*)
GTF_MODES = {'direct': GTF_DIRECT, 'propagate': GTF_PROPAGATE}

EDT_FORMULATIONS = {'exponential': 0, 'linear': 1, 'linear-bound': 2, 'logarithmic': 3}


FLOW_ERROR_THRESHOLDS = (1, 2, 3, 5, 10, 20)          # the N of A{N}PE (flow_eval.py:67-73)


class FlowErrorOut(C.Structure):
    _fields_ = [('n_ee', C.c_int64), ('n_pred', C.c_int64), ('n_gt', C.c_int64), ('n_over', C.c_int64 * 6),
                ('sum_ee', C.c_double), ('sum_ree', C.c_double), ('aee', C.c_double), ('aree', C.c_double), ('anpe', C.c_double * 6)]


class MotionModel(C.Structure):            # eincm_motion_model: M is (12, K) row major in its first 12 K entries
    _fields_ = [('n_coeffs', C.c_int32), ('cx', C.c_double), ('cy', C.c_double), ('scale', C.c_double),
                ('M', C.c_double * (MOTION_NQ * MOTION_MAX_COEFFS))]


class Timings(C.Structure):
    _fields_ = [('ms', C.c_float * N_STAGES), ('total_ms', C.c_float)]


# every symbol include/eincm.h declares: (name, restype, argtypes)
_P = C.c_void_p
_D = C.POINTER(C.c_double)
SIGNATURES = [
    ('eincm_abi_version', C.c_int, []),
    ('eincm_last_error', C.c_char_p, [_P]),
    ('eincm_create', _P, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint32]),
    ('eincm_destroy', None, [_P]),
    ('eincm_set_windows', C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int16),
                                    C.POINTER(C.c_int16), _D, _D, _D]),
    # the hot calls take raw addresses (c_void_p): ndarray.ctypes.data costs 1 us, data_as(POINTER(c_double)) 2.2 us per argument
    ('eincm_loss_grad', C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(Params), _P, _P, C.POINTER(Aux)]),
    ('eincm_loss_grad_async', C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(Params), C.c_int]),
    ('eincm_loss_grad_wait', C.c_int, [_P, _P, _P, C.POINTER(Aux)]),
    ('eincm_handover_loss_grad', C.c_int, [_P, _D, _D, _D, C.c_int, C.c_int, C.POINTER(Params), _D, _D]),
    ('eincm_objectives', C.c_int, [_P, _D, C.POINTER(ObjectivesOut)]),
    ('eincm_get_iwes', C.c_int, [_P, C.POINTER(C.c_float)]),
    ('eincm_get_zero_iwe', C.c_int, [_P, C.POINTER(C.c_float)]),
    ('eincm_get_image_grad', C.c_int, [_P, C.POINTER(C.c_float)]),
    ('eincm_get_scaled_theta', C.c_int, [_P, _D]),
    ('eincm_get_count_images', C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ('eincm_get_iwes_f64', C.c_int, [_P, _D]),
    ('eincm_get_zero_iwe_f64', C.c_int, [_P, _D]),
    ('eincm_get_image_grad_f64', C.c_int, [_P, _D]),
    ('eincm_loss_grad_device', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_double, C.POINTER(C.c_double), C.c_void_p,
                                        C.POINTER(Aux)]),
    ('eincm_set_timing_period', C.c_int, [_P, C.c_int]),
    ('eincm_get_warped_events', C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ('eincm_multi_ref_weights', C.c_int, [C.c_int, _D]),
    ('eincm_resample_matrix', C.c_int, [C.c_int, C.c_int, C.c_int, _D]),
    ('eincm_get_timings', C.c_int, [_P, C.POINTER(Timings)]),
    ('eincm_set_timed_kernels', C.c_int, [_P, C.c_int, C.c_int]),
    ('eincm_loss_grad_masked_async', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_void_p, C.c_int]),
    ('eincm_loss_grad_masked', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_get_host_profile', C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    ('eincm_get_launch_policy', C.c_int, [_P, C.POINTER(C.c_double)]),
    ('eincm_get_memory', C.c_int, [_P, C.POINTER(C.c_int64)]),
    ('eincm_get_timings_total', C.c_int, [_P, C.POINTER(Timings), C.POINTER(C.c_int64), C.c_int]),
    ('eincm_set_windows_ex', C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int16),
                                       C.POINTER(C.c_int16), _D, _D, _D, C.c_uint32]),
    ('eincm_set_windows_ptrs', C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.c_uint32]),
    # ... and per-event weights: one float pointer per window, NULL for ones
    ('eincm_set_windows_weighted', C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.POINTER(C.c_void_p),
                                             C.c_uint32]),
    ('eincm_forward_iwe', C.c_int, [_P, _D, C.c_int, C.c_int, C.POINTER(Params), C.c_int]),
    ('eincm_finish_loss_grad', C.c_int, [_P, _D, _D, C.POINTER(Aux)]),
    ('eincm_finish_constants', C.c_int, [_P]),
    ('eincm_set_device_results', C.c_int, [_P, C.c_int]),
    ('eincm_finish_launch', C.c_int, [_P]),
    ('eincm_grad_device_ptr', C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ('eincm_finish_collect', C.c_int, [_P, _D, _D, C.POINTER(Aux)]),
    ('eincm_iwe_device_ptr', C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ('eincm_mask_device_ptr', C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ('eincm_inv_dist_transform', C.c_int, [_P, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_double, C.c_double, _D,
                                           C.POINTER(C.c_int32)]),
    ('eincm_gaussian_blur', C.c_int, [_P, _D, C.c_int, C.c_double, _D]),
    ('eincm_canny', C.c_int, [_P, C.POINTER(C.c_uint8), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    ('eincm_preprocess_image', C.c_int, [_P, C.POINTER(C.c_uint8), C.c_int, C.POINTER(PreprocessParams), C.POINTER(C.c_uint8)]),
    ('eincm_tiled_objectives', C.c_int, [_P, C.c_int, C.c_int, C.POINTER(TiledOut)]),
    ('eincm_set_objective_tiles', C.c_int, [_P, C.c_int, C.c_int]),
    ('eincm_set_splat_window', C.c_int, [_P, C.c_int]),
    ('eincm_gt_flow', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32), _D, _D, _D]),
    # the DSEC data path (raw addresses: the arrays are large and typed on the numpy side)
    ('eincm_rectify_events', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int64)]),
    ('eincm_remap_cubic', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_flow_decode', C.c_int, [_P, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ('eincm_flow_encode', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    # the event-support filter (raw addresses, as above)
    ('eincm_event_support', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p]),
    # the refractory and polarity-aware event filter (raw addresses, as above)
    ('eincm_event_filter', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int,
                                     C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # per-event scores: an image stack sampled at the warped events (raw addresses, as above)
    ('eincm_event_scores', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the E-step of a motion segmentation: those scores normalised over the models of a group (raw addresses)
    ('eincm_event_responsibilities', C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    # a keep-order batch takes new weights in place (raw addresses, as above)
    ('eincm_set_weights', C.c_int, [_P, C.c_void_p]),
    ('eincm_get_stage_order', C.c_int, [_P, C.c_void_p, C.c_void_p]),
    ('eincm_get_staged_weights', C.c_int, [_P, C.c_void_p]),
    # the contrast landscape over motion coefficients (raw addresses, as above)
    ('eincm_contrast_landscape', C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # a motion segmentation composed into one flow field and a label image (raw addresses, as above)
    ('eincm_compose_motions', C.c_int, [_P, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # that composition made dense: every pixel takes the label of its nearest labelled pixel (raw addresses, as above)
    ('eincm_densify_motions', C.c_int, [_P, C.c_int, C.c_void_p, C.c_uint, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    # the per-pixel label prior, and the E-step that reads a prior image stack (raw addresses, as above)
    ('eincm_label_prior', C.c_int, [_P, C.c_int, C.c_int, C.c_uint32, C.c_uint, C.c_void_p, C.c_void_p]),
    ('eincm_get_staged_prior', C.c_int, [_P, C.c_void_p]),
    ('eincm_event_responsibilities_spatial', C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the label prior carried along the models' own motions to the next window (raw addresses, as above)
    ('eincm_carry_label_prior', C.c_int, [_P, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_uint, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    ('eincm_adopt_carried_prior', C.c_int, [_P, C.c_int]),
    ('eincm_get_carried_prior', C.c_int, [_P, C.c_void_p]),
    # a solved theta carried along its own flow to the next window (raw addresses, as above)
    ('eincm_theta_advect', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    # flow errors of a batch of thetas against staged ground truth
    ('eincm_flow_eval_stage', C.c_int, [_P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_flow_errors', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(FlowErrorOut), C.c_void_p]),
    # BFGS with its state in HBM (raw addresses: called once per lockstep tick)
    ('eincm_bfgs_begin', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ('eincm_bfgs_eval', C.c_int, [_P, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_bfgs_trial', C.c_int, [_P, C.c_void_p, C.c_void_p]),
    ('eincm_bfgs_reduce', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_bfgs_trial_ptrs', C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ('eincm_bfgs_state_ptrs', C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ('eincm_bfgs_accept', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('eincm_bfgs_fetch', C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ... in the limited-memory form
    ('eincm_lbfgs_begin', C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    ('eincm_lbfgs_history_ptrs', C.c_int, [_P] + [C.POINTER(C.c_void_p)] * 6 + [C.POINTER(C.c_int)]),
    # parametric motion-field models
    ('eincm_set_motion_model', C.c_int, [_P, C.POINTER(MotionModel)]),
    ('eincm_loss_grad_motion', C.c_int, [_P, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Aux)]),
    ('eincm_motion_field', C.c_int, [_P, C.c_void_p, C.c_void_p]),
    ('eincm_loss_grad_motion_fused', C.c_int, [_P, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Aux)]),
]

_lib = None


class EincmLibraryMissing(ImportError):
    pass


def load():
    """Load libeincm_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EincmLibraryMissing(
            f'{LIB_PATH} not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). This engine has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)           # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
