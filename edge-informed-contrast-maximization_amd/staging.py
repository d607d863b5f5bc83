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

The DSEC data path (DSECDataLoader, src/dataloaders/dsec_loader.py), for arrays in memory as well:
rectify_events (:145-171), dsec_image_mapping and map_images_to_rect_event (:188-245), dsec_datasamples (:173-186, :285-350).
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


def stage_datasample(datasample, edges=None, event_weights=None, **edge_kw):
    """The part of EINCMExperiment.stage_datasample (exp_mgr.py:278-376) that feeds the loss: returns
    (xs:int16, ys:int16, ts:float64, edges:(R,H,W) float64, edge_ts:float64) ready for solver.set_datasample.
    edges None: built from datasample['images'] by edges.frames_to_edges(images, **edge_kw) (Canny and smoothing on the GPU).
    Otherwise each given edge image is min-max normalised (normalize_edges), and edge_kw must be empty.
    event_weights: one weight per event of the sample (engine.check_event_weights: finite, within [0, 1]);
    the tuple then carries them as float32 in a sixth place, as Engine.set_windows takes it.  None: the 5-tuple, as ever."""
    if edges is not None and edge_kw:
        raise TypeError(f'edge extraction arguments {sorted(edge_kw)} given with ready edges')
    tup = _stage_datasample(datasample, edges, edge_kw)
    if event_weights is None:
        return tup
    from .engine import check_event_weights
    return tup + (check_event_weights(event_weights, len(tup[0])),)


def _stage_datasample(datasample, edges, edge_kw):
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


def _dsec_engine(engine, sensor_size):
    if engine is not None:
        return engine
    from .edges import _engine
    return _engine(sensor_size)


def rectify_events(events, rectify_map, engine=None, chunk=1 << 22):
    """DSECDataLoader.rectify_events (dsec_loader.py:145-171).  events: {'x','y','t','p'} arrays of a recording; rectify_map (H, W, 2)
    float32, channel 0 = x.  x and y go through Engine.rectify_events in chunks of ``chunk`` events (the result does not depend on it);
    t and p never travel: the keep mask is applied to them here.  Returns the rectified {'x','y','t','p'} (x, y int16).  ValueError:
    a map that is not (H, W, 2) float32 of the engine's sensor, a map entry that is not finite or does not round into int16, an event
    coordinate outside the sensor (the reference asserts), arrays of different lengths."""
    from .engine import check_chunk, check_event_coords, check_rectify_map
    m = np.asarray(rectify_map)
    if m.ndim != 3:
        raise ValueError(f'rectify_map must be (H, W, 2), got {m.shape}')
    m = check_rectify_map(m, m.shape[:2] if engine is None else (engine.H, engine.W))
    missing = [k for k in ('x', 'y', 't', 'p') if k not in events]
    if missing:
        raise ValueError(f'events lack {missing}')
    x, y = check_event_coords(events['x'], events['y'])
    t, p = np.asarray(events['t']), np.asarray(events['p'])
    if t.shape != x.shape or p.shape != x.shape:
        raise ValueError(f'events t {t.shape} and p {p.shape} must have the length of x {x.shape}')
    chunk = check_chunk(chunk)
    rec_x, rec_y, keep, _ = _dsec_engine(engine, m.shape[:2]).rectify_events(x, y, m, chunk=chunk)
    return {'x': rec_x, 'y': rec_y, 't': t[keep], 'p': p[keep]}


def event_support_weights(events, sensor_size, tau, radius=1, full_support=1, pixel_mask=None, chunk=1 << 22, return_support=False,
                          engine=None):
    """Per-event weights of a raw stream from the spatiotemporal support filter (Engine.event_support).
    events: {'x','y','t',...} arrays in stream order; ``tau`` in the unit of events['t'] (the raw times, not the normalised ones of
    stage_datasample, whose ``event_weights=`` takes the result).  engine None: the cached small context of edges._engine.  The
    arguments are checked here, before a context is made.  Returns float32 weights (n,), and the uint8 support too when asked."""
    from .engine import (check_chunk, check_event_coords, check_event_support_args, check_event_times, check_pixel_mask,
                         event_support_first_offender)
    missing = [k for k in ('x', 'y', 't') if k not in events]
    if missing:
        raise ValueError(f'events lack {missing}')
    H, W = (int(sensor_size[0]), int(sensor_size[1])) if engine is None else (engine.H, engine.W)
    if (H, W) != (int(sensor_size[0]), int(sensor_size[1])):
        raise ValueError(f'sensor_size {tuple(sensor_size)} is not the engine\'s ({H}, {W})')
    x, y = check_event_coords(events['x'], events['y'])
    t = check_event_times(events['t'], x.shape[0])
    tau, radius, full_support = check_event_support_args(tau, radius, full_support)
    mask = check_pixel_mask(pixel_mask, (H, W))
    chunk = check_chunk(chunk)
    bad = event_support_first_offender(x, y, t, (H, W)) if engine is None else None      # (an engine handed over looks itself)
    if bad is not None:
        raise ValueError(bad[1])
    return _dsec_engine(engine, (H, W)).event_support(x, y, t, tau, radius=radius, full_support=full_support, pixel_mask=mask, chunk=chunk,
                                                      return_support=return_support)


def event_filter_weights(events, sensor_size, refractory=0.0, tau=0.0, radius=1, full_support=1, polarity=False, pixel_mask=None,
                         chunk=1 << 22, return_support=False, engine=None):
    """The keep mask and per-event weights of a raw stream from the refractory and polarity-aware filter (Engine.event_filter,
    DESIGN.md section 24).  events: {'x','y','t',...} arrays in stream order, with 'p' where ``polarity=True`` asks for it (it is
    handed over whenever it is there); ``refractory`` and ``tau`` in the unit of events['t'].  engine None: the cached small context
    of edges._engine.  The arguments are checked here, before a context is made.  Returns (keep bool (n,), weights float32 (n,)),
    and the uint8 support too when asked: ``stage_datasample(event_weights=)`` takes the weights, dropped events weigh 0."""
    from .engine import (check_chunk, check_event_coords, check_event_filter_args, check_event_polarity, check_event_times,
                         check_pixel_mask, event_support_first_offender)
    missing = [k for k in ('x', 'y', 't') if k not in events]
    if missing:
        raise ValueError(f'events lack {missing}')
    H, W = (int(sensor_size[0]), int(sensor_size[1])) if engine is None else (engine.H, engine.W)
    if (H, W) != (int(sensor_size[0]), int(sensor_size[1])):
        raise ValueError(f'sensor_size {tuple(sensor_size)} is not the engine\'s ({H}, {W})')
    x, y = check_event_coords(events['x'], events['y'])
    t = check_event_times(events['t'], x.shape[0])
    refractory, tau, radius, full_support, _ = check_event_filter_args(refractory, tau, radius, full_support, polarity)
    p = check_event_polarity(events.get('p'), x.shape[0], polarity)
    mask = check_pixel_mask(pixel_mask, (H, W))
    chunk = check_chunk(chunk)
    bad = event_support_first_offender(x, y, t, (H, W)) if engine is None else None      # (an engine handed over looks itself)
    if bad is not None:
        raise ValueError(bad[1])
    return _dsec_engine(engine, (H, W)).event_filter(x, y, t, p, refractory=refractory, tau=tau, radius=radius, full_support=full_support,
                                                     polarity=bool(polarity), pixel_mask=mask, chunk=chunk, return_support=return_support)


def weights_from_scores(scores, ref_weights=None, full_score=None):
    """Per-event weights from per-event scores (Engine.event_scores): an event that lands on nothing after motion
    compensation weighs little.  scores: (R, n) per reference time, or (n,) already combined.  (R, n) scores are combined over r with
    ``ref_weights`` ((R,); None: the loss's own compute_weights_for_multi_reference(R), losses.py:39-46), divided by ``full_score``
    (a positive number; None: the median of the positive combined scores, so that half of the events that hit anything weigh 1), and
    clipped to [0, 1].  Plain numpy; the float32 result is what ``stage_datasample(event_weights=)`` takes."""
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim not in (1, 2) or not np.isfinite(s).all():
        raise ValueError(f'scores must be finite, (R, n) or (n,), got shape {s.shape}')
    if s.ndim == 2:
        R = s.shape[0]
        if ref_weights is None:
            x = np.linspace(-1.5, 1.5, R)
            w = np.exp(-0.5 * x * x)
            w = w / w.sum()
        else:
            w = np.asarray(ref_weights, dtype=np.float64)
            if w.shape != (R,) or not np.isfinite(w).all():
                raise ValueError(f'ref_weights must be ({R},) finite numbers, got shape {w.shape}')
        s = w @ s
    elif ref_weights is not None:
        raise ValueError('ref_weights given with scores that are already combined')
    if full_score is None:
        pos = s[s > 0.0]
        full_score = float(np.median(pos)) if pos.size else 1.0
    full_score = float(full_score)
    if not (np.isfinite(full_score) and full_score > 0.0):
        raise ValueError(f'full_score {full_score!r}: a positive number')
    return np.clip(s / full_score, 0.0, 1.0).astype(np.float32)


def hot_pixel_mask(xs, ys, sensor_size, max_count):
    """(H, W) uint8, 1 at the pixels with more than ``max_count`` events: ready for ``pixel_mask=``.  Plain numpy."""
    from .engine import check_event_coords
    H, W = int(sensor_size[0]), int(sensor_size[1])
    x, y = check_event_coords(xs, ys)
    if x.size and (x.min() < 0 or x.max() >= W or y.min() < 0 or y.max() >= H):
        raise ValueError(f'event coordinates outside the {H}x{W} sensor')
    if isinstance(max_count, bool) or not isinstance(max_count, (int, np.integer)) or max_count < 0:
        raise ValueError(f'max_count {max_count!r}: an integer >= 0')
    counts = np.bincount(y.astype(np.int64) * W + x.astype(np.int64), minlength=H * W)
    return (counts.reshape(H, W) > max_count).astype(np.uint8)


def _k_matrix(cam_to_cam, name):
    cm = np.asarray(cam_to_cam['intrinsics'][name]['camera_matrix'], dtype=np.float64)
    if cm.shape != (4,) or not np.all(np.isfinite(cm)):
        raise ValueError(f'intrinsics.{name}.camera_matrix must be four finite numbers (fx, fy, cx, cy), got {cm!r}')
    return np.array([[cm[0], 0.0, cm[2]], [0.0, cm[1], cm[3]], [0.0, 0.0, 1.0]])


def dsec_image_mapping(cam_to_cam, sensor_size=(480, 640)):
    """construct_mapping_for_image (dsec_loader.py:188-218) from the dict of a sequence's cam_to_cam.yaml: for every pixel of the
    rectified event camera, where it lies in the rectified frame camera.  P = K_r1 . R . K_r0^-1 with R the rotation part of
    T_r1_1 . T_1_0 . T_r0_0^-1, that is R_rect1 . R_10 . R_rect0^T (a rotation's inverse is its transpose); (u, v, s) = P (x, y, 1);
    map = (u / s, v / s) in float64, cast to float32.  Rotations stay 3 x 3 matrices: the reference's round trip through quaternions
    (scipy Rotation) is not made, which can move the float64 values by their last bits before the cast.
    Returns (H, W, 2) float32.  ValueError: a missing key, a matrix of the wrong shape, a non-finite entry."""
    H, W = int(sensor_size[0]), int(sensor_size[1])
    if H < 1 or W < 1:
        raise ValueError(f'sensor_size {sensor_size!r}: positive (H, W)')
    try:
        K_r0, K_r1 = _k_matrix(cam_to_cam, 'camRect0'), _k_matrix(cam_to_cam, 'camRect1')
        ex = cam_to_cam['extrinsics']
        R_r0_0, R_r1_1 = np.asarray(ex['R_rect0'], dtype=np.float64), np.asarray(ex['R_rect1'], dtype=np.float64)
        T_10 = np.asarray(ex['T_10'], dtype=np.float64)
    except (KeyError, TypeError) as e:
        raise ValueError(f'cam_to_cam lacks {e}: intrinsics.camRect0/camRect1.camera_matrix, extrinsics.R_rect0/R_rect1/T_10') from None
    if R_r0_0.shape != (3, 3) or R_r1_1.shape != (3, 3) or T_10.shape != (4, 4):
        raise ValueError(f'R_rect0 {R_r0_0.shape}, R_rect1 {R_r1_1.shape} must be (3, 3) and T_10 {T_10.shape} (4, 4)')
    if not (np.all(np.isfinite(R_r0_0)) and np.all(np.isfinite(R_r1_1)) and np.all(np.isfinite(T_10))):
        raise ValueError('non-finite extrinsics')
    P = K_r1 @ (R_r1_1 @ T_10[:3, :3] @ R_r0_0.T) @ np.linalg.inv(K_r0)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    hom = np.stack([xs, ys, np.ones_like(xs)], axis=-1) @ P.T
    return np.ascontiguousarray((hom[..., :2] / hom[..., 2:3]).astype(np.float32))


def map_images_to_rect_event(images, mapping, engine=None):
    """map_image_to_rect_event (dsec_loader.py:243-245) for a stack: cv.remap(img, mapping, None, INTER_CUBIC) under the contract of
    DESIGN.md section 16, one GPU call for the stack.  images (n, Hs, Ws) or (Hs, Ws) uint8; mapping (H, W, 2) float32
    (dsec_image_mapping).  Returns (n, H, W) or (H, W) uint8, ready for edges.frames_to_edges."""
    from .engine import check_remap_args
    a, m, single = check_remap_args(images, mapping)
    out = _dsec_engine(engine, m.shape[:2]).remap_cubic(a, m)
    return out[0] if single else out


def dsec_datasamples(events, images, image_ts_us, eval_ts_us, t_offset, eval_indices, des_n_events=1_500_000, prefer_latest_events=True,
                     flow_gt_16bit=None, mapping=None, engine=None):
    """DSECDataLoader.get_sample (dsec_loader.py:285-350) with precompute_eval_event_indices / precompute_eval_image_indices (:173-186)
    for each index of eval_indices, on arrays in memory.  events: {'x','y','t','p'}, rectified (rectify_events) and time-sorted, t
    without the offset; images (n, Hs, Ws) uint8 with image_ts_us (n,); eval_ts_us (n_eval, 3): start, end, file index (the train split's two columns do when flow_gt_16bit is given); t_offset: the
    recording's offset.  Both ends of a window are searchsorted(..., 'left'): the events on t against eval_ts_us - t_offset, the images
    on image_ts_us against eval_ts_us, the image slice start : end + 1.  The event window is fitted to des_n_events by
    fit_event_window; the returned t has t_offset added.  mapping (H, W, 2) float32: the window's images go through one remap_cubic
    call (map_images_to_rect_event); None: they are handed on as they are.  flow_gt_16bit (len(eval_indices), H, W, 3) uint16, the GT
    images of the requested windows in order: decoded by one flow_decode call into the keys flow_gt, valid2D; None: the key file_idx
    instead (the reference's test split).  Keys besides: events, images, image_ts, eval_ts_us, n_event_deficiency, orig_n_events.
    The reference sets n_event_deficiency only when des_n_events is not None (with None its get_sample fails on the first call);
    here it is None then.  Each dict goes through stage_datasample as it is."""
    ev_ts = np.asarray(eval_ts_us)
    if ev_ts.ndim != 2 or ev_ts.shape[1] < (2 if flow_gt_16bit is not None else 3):
        raise ValueError(f'eval_ts_us must be (n_eval, 3): start, end, file index (the index may be absent with flow_gt_16bit); got {ev_ts.shape}')
    image_ts_us = np.asarray(image_ts_us)
    if image_ts_us.ndim != 1 or len(images) != len(image_ts_us):
        raise ValueError(f'{len(images)} images and image_ts_us of shape {image_ts_us.shape}')
    missing = [k for k in ('x', 'y', 't', 'p') if k not in events]
    if missing:
        raise ValueError(f'events lack {missing}')
    ev = {k: np.asarray(events[k]) for k in ('x', 'y', 't', 'p')}
    n = len(ev['t'])
    if any(a.shape != (n,) for a in ev.values()):
        raise ValueError('events x, y, t, p must be 1-D of one length')
    if des_n_events is not None and (isinstance(des_n_events, bool) or int(des_n_events) != des_n_events or des_n_events < 1):
        raise ValueError(f'des_n_events {des_n_events!r}: a positive integer or None')
    idxs = [int(i) for i in np.atleast_1d(eval_indices)]
    for i in idxs:
        if not 0 <= i < len(ev_ts):
            raise ValueError(f'eval index {i} outside the {len(ev_ts)} evaluation windows')
    flow = valid = None
    if flow_gt_16bit is not None:
        from .engine import check_flow_16bit
        f16, _ = check_flow_16bit(flow_gt_16bit)
        if np.ndim(flow_gt_16bit) != 4 or f16.shape[0] != len(idxs):
            raise ValueError(f'flow_gt_16bit must hold one (H, W, 3) image per requested window ({len(idxs)}), got {np.shape(flow_gt_16bit)}')
    if mapping is not None:
        from .engine import check_remap_args
        check_remap_args(np.asarray(images)[:1], mapping)
    ev_start = np.searchsorted(ev['t'], ev_ts[:, 0] - t_offset, side='left')
    ev_end = np.searchsorted(ev['t'], ev_ts[:, 1] - t_offset, side='left')
    im_start = np.searchsorted(image_ts_us, ev_ts[:, 0], side='left')
    im_end = np.searchsorted(image_ts_us, ev_ts[:, 1], side='left')
    if flow_gt_16bit is not None and idxs:
        flow, valid = _dsec_engine(engine, f16.shape[1:3]).flow_decode(f16)
    out = []
    for b, i in enumerate(idxs):
        i0, i1 = int(ev_start[i]), int(ev_end[i])
        orig_n_events = i1 - i0
        i0, i1, deficiency = fit_event_window(n, i0, i1, des_n_events, prefer_latest_events)
        imgs = images[int(im_start[i]):int(im_end[i]) + 1]
        if mapping is not None and len(imgs):
            imgs = map_images_to_rect_event(imgs, mapping, engine=engine)
        d = {
            'events': {'x': ev['x'][i0:i1], 'y': ev['y'][i0:i1], 't': ev['t'][i0:i1] + t_offset, 'p': ev['p'][i0:i1]},
            'images': imgs,
            'image_ts': image_ts_us[int(im_start[i]):int(im_end[i]) + 1],
            'eval_ts_us': ev_ts[i, :2],
        }
        if flow is None:
            d['file_idx'] = ev_ts[i, 2]
        else:
            d['flow_gt'], d['valid2D'] = flow[b], valid[b]
        d['n_event_deficiency'] = None if des_n_events is None else deficiency
        d['orig_n_events'] = orig_n_events
        out.append(d)
    return out
