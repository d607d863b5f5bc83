"""The step after the path: report metrics of a solved theta (EVAL phase of the reference).

  sparse_flow_error     restates src/evaluations/flow_eval.py:14-76 in numpy: same masks (finite and non-zero predicted
                        AND ground-truth flow, optional event mask), same keys {'errors': AEE, AREE, A{1,2,3,5,10,20}PE;
                        'counts': n_ee, n_pred, n_gt}
  evaluate_theta_array  mirrors src/evaluations/theta_eval.py:14-95: compute_loss_objectives on the evaluation events
                        (HIP engine, forward only) + flow error + the same ``evals`` keys
  gt_flow_plan          the index and time arithmetic of MVSECDataLoader.estimate_gt_flow (src/dataloaders/mvsec_loader.py:322-408)
  estimate_gt_flow      MVSEC's ground-truth flow of evaluation windows: the plans above, walked by one HIP kernel over
                        (pixel, window)
  flow_16bit_to_float   DSEC's GT flow format (src/dataloaders/dsec_loader.py:247-266), decoded on the GPU
  dsec_submission_flow  DSEC's submission format of a solved theta (src/dsec_npz_to_png.py:84-96): up-sampling and 16-bit coding in one
                        HIP kernel
  BatchThetaEvaluator   the two evaluation functions above for a whole batch of windows: the events, edges and ground truth are staged
                        once, every later call uploads the thetas only and the masked reductions of all windows run in one HIP kernel
                        
The masked reductions of the per-window functions (sparse_flow_error, evaluate_theta_array) are O(H*W) and stay on the host; every
objective term comes from the GPU.
"""
import sys

import numpy as np

from . import losses
from . import _lib as L
from .engine import (Engine, GtFlowPlan, check_flow_eval_batch, check_gt_flow_plans, check_precision, check_window_size,
                     resample_matrix)

EPSN = sys.float_info.epsilon


def make_event_mask(xs, ys, sensor_size):
    """utils/event_utils.py:64-76."""
    H, W = sensor_size
    m = np.zeros((H, W), dtype=bool)
    m[np.asarray(ys).astype(np.int64), np.asarray(xs).astype(np.int64)] = True
    return m


def per_pix_theta_to_flow(theta, xs, ys, ts=None):
    """utils/theta_utils.py:40-73 (dt = 1): theta at pixels holding events, zero elsewhere."""
    theta = np.asarray(theta, dtype=np.float64)
    return theta * make_event_mask(xs, ys, theta.shape[:2])[:, :, None]


def sparse_flow_error(pred_flow, gt_flow, event_mask=None):
    """flow_eval.py:14-76."""
    pred_flow = np.asarray(pred_flow, dtype=np.float64)
    gt_flow = np.asarray(gt_flow, dtype=np.float64)
    mask_pred = (~np.isinf(pred_flow[..., 0])) & (~np.isinf(pred_flow[..., 1])) & (np.linalg.norm(pred_flow, axis=-1) > 0)
    if event_mask is not None:
        mask_pred = mask_pred & np.asarray(event_mask, dtype=bool)
    mask_gt = (~np.isinf(gt_flow[..., 0])) & (~np.isinf(gt_flow[..., 1])) & (np.linalg.norm(gt_flow, axis=-1) > 0)
    both = mask_pred & mask_gt
    pred_m, gt_m = pred_flow[both], gt_flow[both]
    ee = np.linalg.norm(pred_m - gt_m, axis=-1)
    ree = ee / (np.linalg.norm(gt_m, axis=-1) + EPSN)
    cnts = {'n_ee': int(ee.shape[0]), 'n_pred': int(mask_pred.sum()), 'n_gt': int(mask_gt.sum())}
    with np.errstate(invalid='ignore'):
        errs = {'AEE': float(ee.mean()) if ee.size else float('nan'), 'AREE': float(ree.mean()) if ee.size else float('nan')}
    for n in (1, 2, 3, 5, 10, 20):
        errs[f'A{n}PE'] = float((ee > n).sum() * 100 / (cnts['n_ee'] + EPSN))
    return {'errors': errs, 'counts': cnts}


def evaluate_theta_array(theta_array, eval_xs, eval_ys, eval_ts, edges, edge_ts, gt_flow, alpha, beta, gamma, delta,
                         sensor_size, err_eval_event_mask=None, window_size=3, precision='fp32'):
    """theta_eval.py:14-95 -> (evals dict, loss_obj dict).  The per-event warped coordinates (not used by the evaluation) and the IWE stay on the GPU;
    ``iwe_var`` is var(IWE at the first reference time) = flow_warp_losses[0] * var(IUE).  precision='fp64': the engine's float64 mode.
    window_size: the splat window of the evaluation IWE (theta_eval.py:36 keeps events_to_pdf_frame's default, 3)."""
    lo = losses.compute_loss_objectives(theta_array, eval_xs, eval_ys, eval_ts, edges, edge_ts, sensor_size, warped_events=False,
                                        precision=precision, window_size=window_size)
    mean_rel_contrast = float(lo['rel_contrasts'].mean())
    mean_rel_corr = float(lo['rel_correlations'].mean())
    mean_rel_iwe_div = float(lo['rel_iwe_divergences'].mean())
    tot_var, theta_div = lo['theta_total_variation'], lo['theta_divergence']
    loss = alpha * (-mean_rel_contrast) + beta * (-mean_rel_corr) + gamma * tot_var + delta * mean_rel_iwe_div
    evals = {}
    if gt_flow is not None:
        fe = sparse_flow_error(per_pix_theta_to_flow(theta_array, eval_xs, eval_ys), gt_flow, err_eval_event_mask)
        evals.update(fe['errors'])
        evals.update(fe['counts'])
        evals['n_pixels'] = int(sensor_size[0] * sensor_size[1])
    evals.update({
        'loss': loss, 'iwe_var': float(lo['variances'][0]), 'mean_rel_contrast': mean_rel_contrast,
        'mean_rel_corr': mean_rel_corr, 'theta_tot_var': tot_var, 'theta_div': theta_div,
        'fwl': float(lo['flow_warp_losses'][0]), 'mean_rel_iwe_div': mean_rel_iwe_div,
        'rel_iwe_divergences': lo['rel_iwe_divergences'], 'rel_contrasts': lo['rel_contrasts'],
        'rel_correlations': lo['rel_correlations'], 'flow_warp_losses': lo['flow_warp_losses'],
        'multi_ref_weights': lo['multi_ref_weights'],
    })
    return evals, lo


SCORE_SOURCES = ('iwe', 'edges')


def event_scores(theta, xs, ys, ts, edges, edge_ts, source='iwe', sensor_size=None, ref_weights=None, exclude_self=False,
                 event_weights=None, method='bilinear', engine=None):
    """Per-event scores of one window under ``theta`` (Engine.event_scores), in the argument shape of
    evaluate_theta_array: how much image lies under each event once it is warped.  source 'iwe': the window's own IWEs at theta
    (exclude_self=True gives the leave-one-out score); 'edges': the edge stack, min-max normalised per image (staging.normalize_edges)
    - the edge map under each warped event.  theta: (h,w,2) of any pyramid size, scaled to the sensor with ``method``.
    ref_weights None: (R, n) float32; (R,) numbers: (n,), combined over the reference times.  engine None: the cached engine of
    losses.engine_for; an engine handed over is staged with the window and left open.  Arguments are checked before a GPU context is
    asked for."""
    from .engine import check_ref_weights, check_event_weights, make_params
    if source not in SCORE_SOURCES:
        raise ValueError(f'source {source!r}: one of {SCORE_SOURCES}')
    if exclude_self and source != 'iwe':
        raise ValueError("exclude_self subtracts the event's share of the IWE: it goes with source='iwe'")
    e = np.asarray(edges, dtype=np.float64)
    R = len(np.atleast_1d(edge_ts))
    H, W = (int(sensor_size[0]), int(sensor_size[1])) if sensor_size is not None else tuple(int(v) for v in e.shape[-2:])
    if e.shape != (R, H, W):
        raise ValueError(f'edges must be ({R},{H},{W}), got {e.shape}')
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim != 3 or th.shape[2] != 2:
        raise ValueError(f'theta must be (h,w,2), got {th.shape}')
    rw = check_ref_weights(ref_weights, R)
    if event_weights is not None:
        event_weights = check_event_weights(event_weights, len(xs))
    p = make_params(1.0, 0.0, 0.0, 0.0, 1, method)
    if engine is None:
        eng = losses.engine_for(xs, ys, ts, edges, edge_ts, (H, W), event_weights=event_weights)
    else:
        eng = engine
        eng.set_window(xs, ys, ts, edges, edge_ts, event_weights)
    images = None
    if source == 'edges':
        from .staging import normalize_edges
        images = normalize_edges(e).astype(np.float32)
    return eng.event_scores(images=images, ref_weights=rw, exclude_self=exclude_self, theta=th, params=p)[0]


class BatchThetaEvaluator:
    """evaluate_theta_array / sparse_flow_error for a batch of evaluation windows that is staged once and evaluated many times: what
    EINCMThetaSolverCallback._evaluate_theta (callbacks.py:131-170) asks for at every iterate of every window of a lockstep batch.

    windows: a list of (eval_xs, eval_ys, eval_ts, edges, edge_ts); gt_flows: (n, H, W, 2) or None (no flow keys, as
    evaluate_theta_array with gt_flow None); err_eval_event_masks: None or (n, H, W); method: how a theta below the sensor's size is
    scaled to it.  The evaluator owns an Engine unless one is handed over (which it then stages on and does not close).  Every argument
    is checked before a GPU context is asked for."""

    def __init__(self, sensor_size, windows, gt_flows, alpha, beta, gamma, delta, err_eval_event_masks=None, method='bilinear',
                 window_size=3, precision='fp32', engine=None):
        self.H, self.W = int(sensor_size[0]), int(sensor_size[1])
        windows = list(windows)
        if not windows:
            raise ValueError('no windows')
        for b, w in enumerate(windows):
            if len(w) != 5:
                raise ValueError(f'window {b} must be (eval_xs, eval_ys, eval_ts, edges, edge_ts)')
        if not isinstance(method, str) or method not in L.METHODS:
            raise ValueError(f'method {method!r} not supported; one of {sorted(L.METHODS)}')
        check_precision(precision)
        window_size = check_window_size(window_size)
        if gt_flows is None and err_eval_event_masks is not None:
            raise ValueError('err_eval_event_masks without gt_flows')
        if gt_flows is not None:
            if len(gt_flows) != len(windows):
                raise ValueError(f'{len(gt_flows)} ground-truth flows for {len(windows)} windows')
            check_flow_eval_batch(gt_flows, [(w[0], w[1]) for w in windows], err_eval_event_masks, (self.H, self.W))
        self.n = len(windows)
        self.params = tuple(float(v) for v in (alpha, beta, gamma, delta))
        self.method = method
        self.has_gt = gt_flows is not None
        self._own = engine is None
        self.engine = None
        if engine is None:
            engine = Engine((self.H, self.W), max(sum(len(w[0]) for w in windows), 1),
                            max_refs=max(len(np.atleast_1d(w[4])) for w in windows), max_windows=self.n, precision=precision)
        elif (engine.H, engine.W) != (self.H, self.W):
            raise ValueError(f'sensor_size {(self.H, self.W)} is not the engine\'s {(engine.H, engine.W)}')
        self.engine = engine
        try:
            if engine.splat_window != window_size:
                engine.set_splat_window(window_size)
            engine.set_windows(windows)
            if self.has_gt:
                engine.flow_eval_stage(gt_flows, [(w[0], w[1]) for w in windows], err_eval_event_masks)
        except Exception:
            self.close()
            raise
        self._A = {}                       # (h, w) -> the two resample matrices of that theta shape

    def close(self):
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _thetas(self, thetas):
        t = np.asarray(thetas, dtype=np.float64)
        if t.ndim == 3 and self.n == 1:
            t = t[None]
        if t.ndim != 4 or t.shape[0] != self.n or t.shape[3] != 2:
            raise ValueError(f'thetas must be ({self.n}, h, w, 2), got {np.shape(thetas)}')
        return t

    def flow_errors(self, thetas, ee_map=False):
        """Engine.flow_errors of the staged batch: a list of sparse_flow_error's dicts (and the error maps with ee_map=True)."""
        if not self.has_gt:
            raise ValueError('the evaluator was built without gt_flows')
        return self.engine.flow_errors(self._thetas(thetas), self.method, ee_map=ee_map)

    def scaled_thetas(self, thetas):
        """thetas (n, h, w, 2) scaled to the sensor: A_H theta A_W^T with the engine's resample matrices."""
        t = self._thetas(thetas)
        h, w = t.shape[1:3]
        if (h, w) == (self.H, self.W):
            return t
        if (h, w) not in self._A:
            self._A[(h, w)] = (resample_matrix(h, self.H, self.method), resample_matrix(w, self.W, self.method))
        A_H, A_W = self._A[(h, w)]
        rows = np.matmul(A_H, t.reshape(self.n, h, w * 2)).reshape(self.n, self.H, w, 2)          # two matrix products, not one 4-index sum
        return np.ascontiguousarray(np.matmul(rows.transpose(0, 1, 3, 2), A_W.T).transpose(0, 1, 3, 2))

    def evaluate(self, thetas):
        """evaluate_theta_array for every window: one Engine.objectives call on the scaled thetas and one flow_errors call.  Returns a
        list of (evals, loss_obj) with evaluate_theta_array's keys (the flow keys only where gt_flows were given)."""
        t = self._thetas(thetas)
        los = self.engine.objectives(self.scaled_thetas(t))
        fes = self.engine.flow_errors(t, self.method) if self.has_gt else [None] * self.n
        alpha, beta, gamma, delta = self.params
        res = []
        for lo, fe in zip(los, fes):
            mean_rel_contrast = float(lo['rel_contrasts'].mean())
            mean_rel_corr = float(lo['rel_correlations'].mean())
            mean_rel_iwe_div = float(lo['rel_iwe_divergences'].mean())
            tot_var, theta_div = lo['theta_total_variation'], lo['theta_divergence']
            loss = alpha * (-mean_rel_contrast) + beta * (-mean_rel_corr) + gamma * tot_var + delta * mean_rel_iwe_div
            evals = {}
            if fe is not None:
                evals.update(fe['errors'])
                evals.update(fe['counts'])
                evals['n_pixels'] = int(self.H * self.W)
            evals.update({
                'loss': loss, 'iwe_var': float(lo['variances'][0]), 'mean_rel_contrast': mean_rel_contrast,
                'mean_rel_corr': mean_rel_corr, 'theta_tot_var': tot_var, 'theta_div': theta_div,
                'fwl': float(lo['flow_warp_losses'][0]), 'mean_rel_iwe_div': mean_rel_iwe_div,
                'rel_iwe_divergences': lo['rel_iwe_divergences'], 'rel_contrasts': lo['rel_contrasts'],
                'rel_correlations': lo['rel_correlations'], 'flow_warp_losses': lo['flow_warp_losses'],
                'multi_ref_weights': lo['multi_ref_weights'],
            })
            res.append((evals, lo))
        return res


def gt_flow_plan(gt_ts, t_start, t_end):
    """estimate_gt_flow's index and time arithmetic (mvsec_loader.py:325-400), in float64, as a GtFlowPlan:
      idx = searchsorted(gt_ts, t_start, 'right') - 1; gt_dt = gt_ts[idx+1] - gt_ts[idx]; dt = t_end - t_start;
      pre_dt = gt_ts[idx+1] - t_start
      gt_dt >= dt and pre_dt >= dt:  'direct', one step (idx, dt, gt_dt)
      otherwise 'propagate':  (idx, pre_dt / gt_dt), then (idx', 1.0) for every idx' = idx+1, ... while gt_ts[idx'+1] < t_end,
                              then (idx', (t_end - gt_ts[idx']) / (gt_ts[idx'+1] - gt_ts[idx']))   (den 1.0 in every step)
    Two refusals (ValueError) where the reference misbehaves: t_start before gt_ts[0] (it would read gt[-1], the last frame) and a
    window that does not end inside the last full GT interval (it raises IndexError).  A non-finite scale or a zero interval in a
    direct window is a ValueError too."""
    ts = np.asarray(gt_ts, dtype=np.float64)
    if ts.ndim != 1 or ts.size < 2:
        raise ValueError(f'gt_ts must be 1-D with at least two timestamps, got shape {ts.shape}')
    t_start, t_end = np.float64(t_start), np.float64(t_end)
    n = ts.size
    idx = int(np.searchsorted(ts, t_start, side='right')) - 1
    if idx < 0:
        raise ValueError(f't_start {t_start!r} precedes the first GT timestamp {ts[0]!r}')
    past = f'window [{t_start!r}, {t_end!r}] does not end inside the last full GT interval (gt_ts[-1] = {ts[-1]!r})'
    if idx + 1 >= n:
        raise ValueError(past)
    gt_dt = ts[idx + 1] - ts[idx]
    dt = t_end - t_start
    pre_dt = ts[idx + 1] - t_start
    with np.errstate(divide='ignore', invalid='ignore'):
        if gt_dt >= dt and pre_dt >= dt:
            plan = GtFlowPlan('direct', ((idx, float(dt), float(gt_dt)),))
        else:
            steps = [(idx, float(pre_dt / gt_dt), 1.0)]
            idx += 1
            while True:
                if idx + 1 >= n:
                    raise ValueError(past)
                if not ts[idx + 1] < t_end:
                    break
                steps.append((idx, 1.0, 1.0))
                idx += 1
            steps.append((idx, float((t_end - ts[idx]) / (ts[idx + 1] - ts[idx])), 1.0))
            plan = GtFlowPlan('propagate', tuple(steps))
    check_gt_flow_plans([plan], n)
    return plan


def estimate_gt_flow(gt_x, gt_y, gt_ts, t_start, t_end, engine=None):
    """MVSECDataLoader.estimate_gt_flow (mvsec_loader.py:322-433) on the GPU.  gt_x, gt_y: (n_frames,H,W) float32 or float64 GT flow
    stacks (already cropped); gt_ts: their (n_frames,) timestamps.  t_start, t_end: scalars, or 1-D arrays of window bounds
    (broadcast).  One engine call for all windows; engine None: a cached small context per sensor size.  Returns (H,W,2) float64 for
    scalar bounds, (B,H,W,2) for arrays: the ``flow_gt`` of the reference's datasample."""
    a, b = np.asarray(t_start, dtype=np.float64), np.asarray(t_end, dtype=np.float64)
    scalar = a.ndim == 0 and b.ndim == 0
    a, b = np.broadcast_arrays(np.atleast_1d(a), np.atleast_1d(b))
    if a.ndim != 1:
        raise ValueError(f'window bounds must be scalars or 1-D, got shape {a.shape}')
    plans = [gt_flow_plan(gt_ts, s, e) for s, e in zip(a, b)]
    if engine is None:
        from .edges import _engine
        engine = _engine(np.shape(gt_x)[-2:])
    out = engine.gt_flow(gt_x, gt_y, plans)
    return out[0] if scalar else out


def flow_16bit_to_float(flow_16bit, engine=None):
    """DSECDataLoader.flow_16bit_to_float (dsec_loader.py:247-266) on the GPU.  flow_16bit: (H, W, 3) uint16, or a stack (B, H, W, 3).
    Returns (flow_map float64 (..., H, W, 2), valid2D bool (..., H, W)): (c - 2^15) / 128 where the third channel is 1, exactly 0
    elsewhere.  ValueError: not uint16, not (.., 3), or a pixel whose third channel is neither 0 nor 1 (the reference asserts)."""
    from .engine import check_flow_16bit
    a, single = check_flow_16bit(flow_16bit)
    if engine is None:
        from .edges import _engine
        engine = _engine(a.shape[1:3])
    flow, valid = engine.flow_decode(a)
    return (flow[0], valid[0]) if single else (flow, valid)


def dsec_submission_flow(theta, sensor_size=(480, 640), valid=None, engine=None):
    """The 16-bit flow image dsec_npz_to_png.py:84-96 writes for a solved theta pyramid level.  theta: (h, w, 2) or a batch (B, h, w, 2);
    it is scaled to sensor_size with the bilinear scale_and_translate and coded as uint16(trunc(v * 128 + 2^15)) into channels 0 and 1,
    in one kernel.  Channel 2 is 0 as the reference leaves it, or ``valid`` ((H, W) / (B, H, W)) where given.  Returns (..., H, W, 3)
    uint16.  ValueError: a value that is not finite or codes outside [0, 65536) (the reference's cast is undefined there)."""
    from .engine import check_theta_batch
    H, W = int(sensor_size[0]), int(sensor_size[1])
    t, v, single = check_theta_batch(theta, valid, (H, W))
    if engine is None:
        from .edges import _engine
        engine = _engine((H, W))
    elif (engine.H, engine.W) != (H, W):
        raise ValueError(f'sensor_size {(H, W)} is not the engine\'s {(engine.H, engine.W)}')
    out = engine.flow_encode(t, v)
    return out[0] if single else out
