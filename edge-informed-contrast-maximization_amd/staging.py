"""The step before the path: turning a loader's raw window into the staged tuple the loss consumes.

Restates, for numpy inputs, the two rules of the reference that define the hot path's input ranges:
  * event-count fitting ``des_n_events`` (src/dataloaders/mvsec_loader.py:272-295, dsec_loader.py:294-319): the window
    [idx_start, idx_end) of a time-sorted event stream is grown symmetrically when short (ceil/floor of the deficiency,
    clamped to the stream) and cut to the latest / earliest ``des_n_events`` events when long;
  * time normalisation (src/experiments/e00/exp_mgr.py:318-327): ``(t - t0) / (t1 - t0 + eps)`` for event and image
    timestamps, so events of the evaluation window land in [0, 1) and a grown window slightly outside it.
Edge extraction (exp_mgr.py:334-350) is edges.frames_to_edges: stage_datasample runs it on ``datasample['images']`` unless
the caller passes ``edges``, a stack of smoothed edge images that ``normalize_edges`` takes through the chain's last step.

mvsec_datasamples restates MVSECDataLoader.get_sample_between_two_image_timestamps (mvsec_loader.py:247-320) for arrays in memory,
its ``flow_gt`` from evaluation.estimate_gt_flow; eval_event_slice is the evaluation-event rule of exp_mgr.py:301-313.
"""
import sys

import numpy as np

EPSN = sys.float_info.epsilon


def fit_event_window(n_stream, idx_start, idx_end, des_n_events, prefer_latest_events=True):
    """Return (idx_start, idx_end, n_event_deficiency) after the reference's pad / truncate rule."""
    if des_n_events is None:
        return int(idx_start), int(idx_end), 0
    deficiency = int(des_n_events) - (int(idx_end) - int(idx_start))
    if deficiency > 0:
        idx_start = max(0, int(idx_start) - int(np.ceil(deficiency / 2)))
        idx_end = min(int(idx_end) + int(np.floor(deficiency / 2)), int(n_stream))
    elif deficiency < 0:
        if prefer_latest_events:
            idx_start = int(idx_end) - int(des_n_events)
        else:
            idx_end = int(idx_start) + int(des_n_events)
    return int(idx_start), int(idx_end), deficiency


def select_events(stream_t, t_start, t_end, des_n_events=None, prefer_latest_events=True):
    """Slice of a time-sorted stream covering [t_start, t_end] (searchsorted left/right as mvsec_loader.py:272-273),
    fitted to des_n_events.  Returns (slice, n_event_deficiency)."""
    i0 = int(np.searchsorted(stream_t, t_start, side='left'))
    i1 = int(np.searchsorted(stream_t, t_end, side='right'))
    i0, i1, d = fit_event_window(len(stream_t), i0, i1, des_n_events, prefer_latest_events)
    return slice(i0, i1), d


def normalize_times(ts, image_ts, start_time, end_time, time_scaler=1.0):
    """exp_mgr.py:322-324."""
    den = (end_time - start_time) + EPSN
    ts_n = ((np.asarray(ts, dtype=np.float64) - start_time) / den) * time_scaler
    image_ts_n = ((np.asarray(image_ts, dtype=np.float64) - start_time) / den) * time_scaler
    return ts_n, image_ts_n


def normalize_edges(edge_images):
    """Min-max normalise each edge image to [0, 1] (exp_mgr.py:343-350 via img_utils.py:24-25)."""
    out = []
    for e in edge_images:
        e = np.asarray(e, dtype=np.float64)
        out.append((e - e.min()) / (e.max() - e.min() + EPSN))
    return np.stack(out)


def stage_datasample(datasample, edges=None, **edge_kw):
    """The part of EINCMExperiment.stage_datasample (exp_mgr.py:278-376) that feeds the loss: returns
    (xs:int16, ys:int16, ts:float64, edges:(R,H,W) float64, edge_ts:float64) ready for solver.set_datasample.
    edges None: built from datasample['images'] by edges.frames_to_edges(images, **edge_kw) (Canny and smoothing on the GPU).
    Otherwise each given edge image is min-max normalised (normalize_edges), and edge_kw must be empty."""
    if edges is not None and edge_kw:
        raise TypeError(f'edge extraction arguments {sorted(edge_kw)} given with ready edges')
    ev = datasample['events']
    start_time, end_time = datasample['eval_ts_us'] if 'eval_ts_us' in datasample else datasample['eval_ts']
    ts, image_ts = normalize_times(ev['t'], datasample['image_ts'], float(start_time), float(end_time))
    from .engine import as_int16_coords       # rounds float coordinates half-to-even (event_warpers.py:29-30), range-checks
    xs = np.ascontiguousarray(as_int16_coords(ev['x'], 'x'))
    ys = np.ascontiguousarray(as_int16_coords(ev['y'], 'y'))
    if edges is None:
        from .edges import frames_to_edges
        return xs, ys, ts, frames_to_edges(datasample['images'], **edge_kw), image_ts
    return xs, ys, ts, normalize_edges(edges), image_ts


def eval_event_slice(ts, eval_ts, n_event_deficiency):
    """The events the reference evaluates (exp_mgr.py:301-313).  When the window was padded (n_event_deficiency > 0), only those
    strictly inside eval_ts: i0, i1 = searchsorted(ts, eval_ts) on the raw times, slice(max(0, i0 + 1), min(n, i1 - 1)).  Otherwise
    (a cut window, or n_event_deficiency 0 or None) all of them."""
    n = len(ts)
    if n_event_deficiency is not None and n_event_deficiency > 0:
        i0, i1 = np.searchsorted(np.asarray(ts), np.asarray(eval_ts, dtype=np.float64)[:2])
        return slice(max(0, int(i0) + 1), min(n, int(i1) - 1))
    return slice(0, n)


def mvsec_datasamples(events, images, image_ts, gt_x, gt_y, gt_ts, image_indices, dt, des_n_events=30000, prefer_latest_events=True,
                      load_more_images=True, engine=None):
    """get_sample_between_two_image_timestamps (mvsec_loader.py:247-320) for each index of image_indices, without the IMU keys.
    events: {'x','y','t','p'} arrays, time-sorted; images (n,H,W) and image_ts (n,); gt_x, gt_y (n_gt,H,W) and gt_ts (n_gt,): the
    already cropped and pruned sequence.  dt: the image step (the config's ``dt``).  The window of index i runs from image_ts[i] to
    image_ts[i + dt]; its ``flow_gt`` comes from one evaluation.estimate_gt_flow call for the whole batch (engine None: a cached
    context; any object with a gt_flow(gt_x, gt_y, plans) method is used as given).  Returns a list of dicts with keys events, images,
    image_ts, flow_gt, eval_ts, n_event_deficiency, orig_n_events, each ready for stage_datasample."""
    from .evaluation import estimate_gt_flow
    dt = int(dt)
    image_ts = np.asarray(image_ts)
    idxs = [int(i) for i in np.atleast_1d(image_indices)]
    for i in idxs:
        if i < 0 or i + dt >= len(image_ts) or dt < 1:
            raise ValueError(f'image index {i} with dt {dt}: images {i}..{i + dt} outside the {len(image_ts)} images')
    t_ev = np.asarray(events['t'])
    t0 = image_ts[idxs]
    t1 = image_ts[[i + dt for i in idxs]]
    flow_gt = estimate_gt_flow(gt_x, gt_y, gt_ts, t0, t1, engine=engine)
    out = []
    for b, i in enumerate(idxs):
        if load_more_images:
            imgs, imgs_ts = images[i:i + dt + 1], image_ts[i:i + dt + 1]
        else:
            imgs, imgs_ts = images[[i, i + dt]], np.array([t0[b], t1[b]])
        orig_n_events = int(np.searchsorted(t_ev, t1[b], side='right') - np.searchsorted(t_ev, t0[b], side='left'))
        sl, deficiency = select_events(t_ev, t0[b], t1[b], des_n_events, prefer_latest_events)
        out.append({
            'events': {k: np.asarray(events[k])[sl] for k in ('x', 'y', 't', 'p')},
            'images': imgs,
            'image_ts': imgs_ts,
            'flow_gt': flow_gt[b],
            'eval_ts': imgs_ts[[0, -1]],
            'n_event_deficiency': None if des_n_events is None else deficiency,
            'orig_n_events': orig_n_events,
        })
    return out
