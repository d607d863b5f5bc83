"""Host-side mirror of the reference's objective callables, backed by the HIP engine.

Same names, argument order and meaning as upstream src/eincm/losses.py:
    loss_func(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls,
              sensor_size, scale_to_sensor_size_method) -> (final_loss, aux_info)          losses.py:108-205
    handover_loss_func(alpha_handover, prev_theta, theta, xs, ..., method) -> loss          losses.py:208-276
    compute_loss_objectives(theta, xs, ys, ts, edges, edge_ts, sensor_size) -> dict         losses.py:49-105 (all 15 keys)
so the hydra plugin point (configs/theta_loss_func/default.yaml:1-2, ``_target_: eincm.losses.loss_func``)
can name this module instead.  The reference differentiates ``loss_func`` with JAX inside jaxopt; a HIP
engine cannot be traced, so the gradient is exposed explicitly as ``value_and_grad_loss_func`` /
``value_and_grad_handover_loss_func`` (what jax.value_and_grad would return) and consumed by
``solver.ScipyMinimize``.  ``motion_loss_func`` / ``value_and_grad_motion_loss_func`` are the same callables over the coefficients of
a parametric motion-field model (``motion.MotionModel``, passed as ``model=``) in place of theta.

The event window is staged on the GPU once and reused for every evaluation, like the reference's closed-over
device-resident ``*args``: engines are cached by the identity of the (xs, ys, ts, edges, edge_ts) arrays.  JAX arrays are
immutable, numpy arrays are not: a cheap content fingerprint (<= 256 strided samples of every array plus its last element)
is a BEST-EFFORT check for in-place edits - an edit of a few elements between two calls can go unnoticed, and the stale
staged window would then be evaluated.  Code that edits a cached array in place calls ``clear_engine_cache()``.

``event_weights=`` (every callable; None by default) hands the window's per-event weights to the staging; the
array joins the five others in the cache's identity and fingerprint.  It stands in front of ``precision``, which stays the last
parameter of the reference-shaped callables.
"""
import functools
import weakref

import numpy as np

from . import _lib as L
from .engine import Engine, check_motion_path, check_precision, check_tile_size, check_window_size, make_params

_CACHE = []            # [(refs tuple, key, Engine)] most-recent first
_CACHE_SIZE = 2


def _as_np(a):
    return a if isinstance(a, np.ndarray) else np.asarray(a)


def _fingerprint(arrs):
    """Content check of the cached arrays: <= 256 strided samples of each plus its last element, as bytes.  It runs on EVERY call of the
    loss callables (an evaluation takes 45-90 us on the GPU), so it must stay in the microseconds: strided VIEWS of contiguous arrays
    (``ndarray.flat[::k]`` on a 10^6-element array cost 60 us per array)."""
    parts = []
    for a in arrs:
        n = a.size
        if n:
            f = a.reshape(-1) if a.flags.c_contiguous else a.flat            # no copy of a non-contiguous array either
            parts.append(np.asarray(f[::max(1, n // 256)]).tobytes())
            parts.append(np.asarray(f[n - 1]).tobytes())
    return hash(tuple(parts))


def engine_for(xs, ys, ts, edges, edge_ts, sensor_size, device=0, precision='fp32', tile_size=None, window_size=L.DEFAULT_SPLAT_WINDOW,
               event_weights=None):
    """Engine holding this window (staged on first use; reused while the same, unmodified array objects are passed).  One engine per
    precision: 'fp64' is the float64 mode (Engine(..., precision='fp64')).  tile_size: (tile_h, tile_w) of the adaptive objective
    kinds, set on the engine (None: the default 32 x 42).  window_size: the splat window of every IWE (events_to_pdf_frame's
    window_size, 1..7, default 3), set on the engine.  event_weights: per-event weights of the window (engine.check_event_weights; DESIGN.md
    section 22) or None; the array is part of the cache's identity and fingerprint like the five others."""
    check_precision(precision)
    tiles = L.DEFAULT_OBJECTIVE_TILE if tile_size is None else check_tile_size(tile_size, sensor_size)
    window = check_window_size(window_size)
    eng = _engine_for(xs, ys, ts, edges, edge_ts, sensor_size, device, precision, event_weights)
    if eng.objective_tiles != tiles:
        eng.set_objective_tiles(tiles)
    if eng.splat_window != window:
        eng.set_splat_window(window)
    return eng


def _engine_for(xs, ys, ts, edges, edge_ts, sensor_size, device, precision, event_weights=None):
    arrs = tuple(_as_np(a) for a in (xs, ys, ts, edges, edge_ts))
    if event_weights is not None:          # a sixth array of the key, the identity check and the fingerprint; staged by set_window
        arrs += (_as_np(event_weights),)
    fp = _fingerprint(arrs)
    key = (tuple(int(s) for s in sensor_size), device, precision) + tuple((a.shape, a.dtype.str) for a in arrs)
    for i, (refs, k, eng) in enumerate(_CACHE):
        if k[:-1] == key and all(r() is a for r, a in zip(refs, arrs)):
            if k[-1] != fp:                       # same objects, edited in place: stage again
                _CACHE.pop(i)[2].close()
                break
            if i:
                _CACHE.insert(0, _CACHE.pop(i))
            return eng
    key = key + (fp,)
    eng = Engine(sensor_size, max_events_total=max(len(arrs[0]), 1), max_refs=max(len(np.atleast_1d(arrs[4])), 1),
                 max_windows=1, device=device, precision=precision)
    eng.set_window(*arrs)
    try:
        refs = tuple(weakref.ref(a) for a in arrs)
    except TypeError:       # not weak-referenceable (e.g. a list was converted): do not cache
        return eng
    _CACHE.insert(0, (refs, key, eng))
    while len(_CACHE) > _CACHE_SIZE:
        _CACHE.pop()[2].close()
    return eng


def clear_engine_cache():
    while _CACHE:
        _CACHE.pop()[2].close()


def _aux_dict(eng, a, with_arrays):
    d = {'final_loss': a['final_loss'], 'mean_rel_corr': a['mean_rel_corr'], 'mean_rel_contrast': a['mean_rel_contrast'],
         'mean_rel_iwe_divergence': a['mean_rel_iwe_divergence'], 'theta_total_variation': a['theta_total_variation']}
    if with_arrays:
        from .engine import multi_ref_weights
        d['scaled_theta'] = eng.scaled_theta()[0]
        d['multi_ref_weights'] = multi_ref_weights(eng.R)
    return d


def value_and_grad_loss_func(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls,
                             sensor_size, scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG,
                             full_aux=False, aux_arrays=False, correlation_kind='mse', tile_size=None,
                             window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32'):
    """((final_loss, aux_info), grad) — the shape jax.value_and_grad(loss_func, has_aux=True) returns.  precision='fp64': the engine's
    float64 mode (what the reference computes with jax_enable_x64: true)."""
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, full_aux, correlation_kind)
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, tile_size=tile_size, window_size=window_size,
                     event_weights=event_weights)
    v, g, aux = eng.loss_grad(np.asarray(theta, dtype=np.float64), p, want_grad=True, want_aux=True)
    return (float(v[0]), _aux_dict(eng, aux[0], aux_arrays)), g[0]


def loss_func(theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
              scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG, correlation_kind='mse',
              tile_size=None, window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32'):
    """(final_loss, aux_info) as losses.py:108-205; forward only, every aux entry evaluated."""
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, True, correlation_kind)
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, tile_size=tile_size, window_size=window_size,
                     event_weights=event_weights)
    v, _, aux = eng.loss_grad(np.asarray(theta, dtype=np.float64), p, want_grad=False, want_aux=True)
    return float(v[0]), _aux_dict(eng, aux[0], True)


def _motion_engine(model, xs, ys, ts, edges, edge_ts, sensor_size, precision, tile_size, window_size, path='expanded', event_weights=None):
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, tile_size=tile_size, window_size=window_size,
                     event_weights=event_weights)
    if eng.motion_model is not model:
        eng.set_motion_model(model)
    eng.set_motion_path(path)              # (every call: the engine is shared with the callables of the other paths)
    return eng


def _value_and_grad_motion(path, coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
                           scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG, full_aux=False, aux_arrays=False,
                           correlation_kind='mse', tile_size=None, window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32', *, model):
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, full_aux, correlation_kind)
    eng = _motion_engine(model, xs, ys, ts, edges, edge_ts, sensor_size, precision, tile_size, window_size, path, event_weights)
    v, g, aux = eng.loss_grad_motion(np.asarray(coeffs, dtype=np.float64), p, want_grad=True, want_aux=True)
    return (float(v[0]), _aux_dict(eng, aux[0], aux_arrays)), g[0]


def _motion_loss(path, coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
                 scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG, correlation_kind='mse', tile_size=None,
                 window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32', *, model):
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, True, correlation_kind)
    eng = _motion_engine(model, xs, ys, ts, edges, edge_ts, sensor_size, precision, tile_size, window_size, path, event_weights)
    v, _, aux = eng.loss_grad_motion(np.asarray(coeffs, dtype=np.float64), p, want_grad=False, want_aux=True)
    return float(v[0]), _aux_dict(eng, aux[0], True)


def value_and_grad_motion_loss_func(coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
                                    scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG, full_aux=False,
                                    aux_arrays=False, correlation_kind='mse', tile_size=None, window_size=L.DEFAULT_SPLAT_WINDOW,
                                    event_weights=None, precision='fp32', *, model):
    """((final_loss, aux_info), grad (K,)) of loss_func on the field model.field(coeffs) of a motion.MotionModel, differentiated
    with respect to the coefficients.  The field is at sensor size: the scaling method is not read.
    By the expanded path; motion_loss_funcs(path) gives the same callable on another."""
    return _value_and_grad_motion('expanded', coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls,
                                  sensor_size, scale_to_sensor_size_method, contrast_kind, full_aux, aux_arrays, correlation_kind, tile_size,
                                  window_size, event_weights, precision, model=model)


def motion_loss_func(coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
                     scale_to_sensor_size_method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG, correlation_kind='mse',
                     tile_size=None, window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32', *, model):
    """(final_loss, aux_info) of loss_func on model.field(coeffs); forward only, every aux entry evaluated."""
    return _motion_loss('expanded', coeffs, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta, cur_pyr_lvl, n_pyr_lvls, sensor_size,
                        scale_to_sensor_size_method, contrast_kind, correlation_kind, tile_size, window_size, event_weights, precision, model=model)


def motion_loss_funcs(path='expanded'):
    """(motion_loss_func, value_and_grad_motion_loss_func) evaluating by ``path``: 'expanded' | 'fused' | 'auto' as
    Engine.set_motion_path takes it; the module's own pair is motion_loss_funcs('expanded').  The callables take
    the arguments of that pair.  path is validated here, before any engine exists.  The forward-only callable evaluates every aux
    entry, which needs the Theta image: with 'fused' it raises, with 'auto' it takes the expanded path."""
    path = check_motion_path(path)
    return functools.partial(_motion_loss, path), functools.partial(_value_and_grad_motion, path)


def value_and_grad_handover_loss_func(alpha_handover, prev_theta, theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma,
                                      delta, cur_pyr_lvl, n_pyr_lvls, sensor_size, scale_to_sensor_size_method='bilinear',
                                      contrast_kind=L.CONTRAST_GRAD_MAG, correlation_kind='mse', tile_size=None,
                                      window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32'):
    """(loss, d loss / d alpha_handover) of losses.py:269-276."""
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, False, correlation_kind)
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, tile_size=tile_size, window_size=window_size,
                     event_weights=event_weights)
    v, dv = eng.handover_loss_grad(float(np.asarray(alpha_handover).reshape(-1)[0]), prev_theta, theta, p, want_grad=True)
    return float(v[0]), float(dv[0])


def handover_loss_func(alpha_handover, prev_theta, theta, xs, ys, ts, edges, edge_ts, alpha, beta, gamma, delta,
                       cur_pyr_lvl, n_pyr_lvls, sensor_size, scale_to_sensor_size_method='bilinear',
                       contrast_kind=L.CONTRAST_GRAD_MAG, correlation_kind='mse', tile_size=None,
                       window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32'):
    """loss only, as losses.py:208-276."""
    p = make_params(alpha, beta, gamma, delta, cur_pyr_lvl, scale_to_sensor_size_method, contrast_kind, False, correlation_kind)
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, tile_size=tile_size, window_size=window_size,
                     event_weights=event_weights)
    v, _ = eng.handover_loss_grad(float(np.asarray(alpha_handover).reshape(-1)[0]), prev_theta, theta, p, want_grad=False)
    return float(v[0])


def compute_loss_objectives(theta, xs, ys, ts, edges, edge_ts, sensor_size, warped_events=True,
                            window_size=L.DEFAULT_SPLAT_WINDOW, event_weights=None, precision='fp32'):
    """losses.py:49-105 on a full-resolution theta (H,W,2): every key of the reference dict.  The per-event ``warped_xs`` /
    ``warped_ys`` ((R, n_events) float64, read by plotters only) cost a 2*R*n_events*8-byte copy: ``warped_events=False`` skips them."""
    eng = engine_for(xs, ys, ts, edges, edge_ts, sensor_size, precision=precision, window_size=window_size, event_weights=event_weights)
    d = eng.objectives(np.asarray(theta, dtype=np.float64))[0]
    if warped_events:
        d['warped_xs'], d['warped_ys'] = eng.warped_events(0)
    return d
