"""Python handle on one eincm_ctx (include/eincm.h): a batch of event windows resident on one MI355X."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib as L


class EincmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'eincm error {code}: {msg}')
        self.code = code


class NonFiniteLoss(EincmError):
    pass


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def as_int16_coords(a, what='coordinates'):
    """Event coordinates as int16, the reference's wire format.  Integer arrays are range-checked and cast; float arrays
    (e.g. rectified coordinates handed straight to loss_func) are rounded half-to-even first, like ``jnp.round(xs).astype(int16)``
    in per_pix_warp (upstream src/eincm/event_warpers.py:29-30).  Values outside the int16 range raise instead of wrapping."""
    a = np.asarray(a)
    if a.dtype == np.int16:
        return a
    if a.dtype.kind not in 'iuf':
        raise TypeError(f'{what} must be integer or floating point, got {a.dtype}')
    if a.dtype.kind == 'f':
        if a.size and not np.all(np.isfinite(a)):
            raise ValueError(f'{what} contain non-finite values')
        a = np.rint(a)
    if a.size and (a.min() < -32768 or a.max() > 32767):
        raise ValueError(f'{what} outside the int16 range [-32768, 32767]')
    return a.astype(np.int16)


def _kind_code(kind, names, what):
    """A kind given by name or integer code -> its code; anything else is a ValueError."""
    if isinstance(kind, str):
        if kind not in names:
            raise ValueError(f'{what} {kind!r} unknown; one of {sorted(names)}')
        return names[kind]
    if isinstance(kind, (bool, np.bool_)) or not isinstance(kind, (int, np.integer)) or int(kind) not in names.values():
        raise ValueError(f'{what} {kind!r} unknown; a name of {sorted(names)} or a code 0..{len(names) - 1}')
    return int(kind)


def contrast_kind_code(kind):
    """'grad_mag' | 'variance' | 'adaptive_grad_mag' | 'adaptive_variance', or 0..3."""
    return _kind_code(kind, L.CONTRAST_KINDS, 'contrast_kind')


def correlation_kind_code(kind):
    """'mse' | 'adaptive_mse' | 'hadamard' | 'joint_contrast', or 0..3."""
    return _kind_code(kind, L.CORRELATION_KINDS, 'correlation_kind')


def check_tile_size(tile_size, sensor_size=None):
    """(tile_h, tile_w) of the adaptive objective kinds: positive integers, at most the sensor size when it is given."""
    try:
        th, tw = (int(v) for v in tile_size)
        ok = all(float(v) == int(v) for v in tile_size)
    except (TypeError, ValueError):
        raise ValueError(f'tile_size {tile_size!r}: a pair of positive integers (tile_h, tile_w)') from None
    if not ok or th < 1 or tw < 1 or (sensor_size is not None and (th > sensor_size[0] or tw > sensor_size[1])):
        raise ValueError(f'tile_size {tile_size!r}: 1 <= tile <= sensor {tuple(sensor_size) if sensor_size is not None else ""}')
    return th, tw


def check_window_size(window_size):
    """Splat window size of events_to_pdf_frame (event_utils.py:13-61): an int in 1..7 (bool and float are refused); radius size // 2."""
    if isinstance(window_size, bool) or not isinstance(window_size, (int, np.integer)) or not 1 <= int(window_size) <= L.SPLAT_WINDOW_MAX:
        raise ValueError(f'window_size {window_size!r}: an integer in 1..{L.SPLAT_WINDOW_MAX}')
    return int(window_size)


def check_history(history, limit=L.LBFGS_MAX_HISTORY):
    """Pairs (s, y) the limited-memory BFGS state keeps per window: an int in 1..EINCM_LBFGS_MAX_HISTORY on the device (bool and float
    are refused); ``limit=None``: any positive int (the host state has no bound)."""
    if isinstance(history, bool) or not isinstance(history, (int, np.integer)) or int(history) < 1 or (limit is not None and int(history) > limit):
        raise ValueError(f'history {history!r}: an integer in 1..{limit}' if limit is not None else f'history {history!r}: a positive integer')
    return int(history)


def check_initial_scale(initial_scale):
    """'last_pair' (H0 = y.s / y.y of the newest pair) or 'identity' (H0 = I)."""
    if not isinstance(initial_scale, str) or initial_scale not in L.LBFGS_SCALES:
        raise ValueError(f"initial_scale {initial_scale!r}: 'last_pair' or 'identity'")
    return initial_scale


def check_canny_args(threshold1, threshold2, aperture_size):
    """cv.Canny's arguments as eincm_canny takes them: finite, non-negative thresholds and aperture 3 (5, 7 and Scharr are not
    implemented).  Checked before any GPU call."""
    ths = []
    for name, v in (('threshold1', threshold1), ('threshold2', threshold2)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f'{name} {v!r}: a finite, non-negative number')
        ths.append(float(v))
    if isinstance(aperture_size, bool) or not isinstance(aperture_size, (int, np.integer)) or int(aperture_size) != 3:
        raise ValueError(f'aperture_size {aperture_size!r}: only 3 is implemented')
    return ths[0], ths[1], 3


PREPROCESS_DEFAULTS = dict(denoise_h=4.0, denoise_template_win=3, denoise_search_win=11, clahe_clip_limit=5.0, clahe_tiles=(10, 10),
                           sharpen_sigma=3.0, sharpen_alpha=1.5, sharpen_beta=-0.5, bilateral_d=5, bilateral_sigma_color=15.0,
                           bilateral_sigma_space=15.0)


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f'{name} {v!r}: a finite number')
    return float(v)


def _integer(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f'{name} {v!r}: an integer')
    return int(v)


def preprocess_stages(stages):
    """'all', an EINCM_PRE_* bit mask, a stage name ('nlmeans', 'clahe', 'unsharp', 'bilateral') or an iterable of names."""
    if isinstance(stages, str):
        stages = L.PRE_ALL if stages == 'all' else [stages]
    if isinstance(stages, (int, np.integer)) and not isinstance(stages, bool):
        mask = int(stages)
    else:
        mask = 0
        for name in stages:
            if name not in L.PRE_STAGES:
                raise ValueError(f'stage {name!r}: one of {sorted(L.PRE_STAGES)}')
            mask |= L.PRE_STAGES[name]
    if mask < 1 or mask & ~L.PRE_ALL:
        raise ValueError(f'stages {stages!r}: a non-empty set of the four stages')
    return mask


def make_preprocess_params(shape, stages='all', **kw):
    """eincm_preprocess_params for a (H, W) sensor, with eincm_preprocess_image's checks made here, before
    any GPU call.  Keywords and defaults: PREPROCESS_DEFAULTS (the reference's preprocess_image defaults, with sharpen_sigma the
    sigmaX OpenCV receives); only the selected stages' keywords are checked."""
    unknown = set(kw) - set(PREPROCESS_DEFAULTS)
    if unknown:
        raise TypeError(f'unknown preprocessing arguments {sorted(unknown)}')
    a = dict(PREPROCESS_DEFAULTS, **kw)
    H, W = int(shape[0]), int(shape[1])
    p = L.PreprocessParams()
    p.stages = mask = preprocess_stages(stages)
    if mask & L.PRE_NLMEANS:
        h = _number('denoise_h', a['denoise_h'])
        tw, sw = _integer('denoise_template_win', a['denoise_template_win']), _integer('denoise_search_win', a['denoise_search_win'])
        if h <= 0:
            raise ValueError(f'denoise_h {h!r}: positive')
        for name, v, top in (('denoise_template_win', tw, 7), ('denoise_search_win', sw, 21)):
            if v < 1 or v % 2 == 0:
                raise ValueError(f'{name} {v}: odd and positive')
            if v > top:
                raise ValueError(f'{name} {v}: at most {top} is implemented')
        p.denoise_h, p.denoise_template_win, p.denoise_search_win = h, tw, sw
    if mask & L.PRE_CLAHE:
        clip = _number('clahe_clip_limit', a['clahe_clip_limit'])
        grid = a['clahe_tiles']
        if not isinstance(grid, (tuple, list)) or len(grid) != 2:
            raise ValueError(f'clahe_tiles {grid!r}: (tiles_x, tiles_y)')
        tx, ty = _integer('clahe_tiles', grid[0]), _integer('clahe_tiles', grid[1])
        if not (1 <= tx <= W and 1 <= ty <= H):
            raise ValueError(f'clahe_tiles {tx, ty}: (tiles_x, tiles_y) with 1 <= tiles_x <= W = {W}, 1 <= tiles_y <= H = {H}')
        p.clahe_clip_limit, p.clahe_tiles_x, p.clahe_tiles_y = clip, tx, ty
    if mask & L.PRE_UNSHARP:
        sigma = _number('sharpen_sigma', a['sharpen_sigma'])
        if sigma <= 0:
            raise ValueError(f'sharpen_sigma {sigma!r}: positive')
        if round(sigma * 3 * 2 + 1) > 129:
            raise ValueError(f'sharpen_sigma {sigma!r}: more than 129 blur taps is not implemented')
        p.sharpen_sigma = sigma
        p.sharpen_alpha = _number('sharpen_alpha', a['sharpen_alpha'])
        p.sharpen_beta = _number('sharpen_beta', a['sharpen_beta'])
    if mask & L.PRE_BILATERAL:
        d = _integer('bilateral_d', a['bilateral_d'])
        sc = _number('bilateral_sigma_color', a['bilateral_sigma_color'])
        ss = _number('bilateral_sigma_space', a['bilateral_sigma_space'])
        r = d // 2 if d > 0 else round((ss if ss > 0 else 1.0) * 1.5)
        if r > 32:
            raise ValueError(f'bilateral_d {d}, sigma_space {ss}: radius {r} > 32 is not implemented')
        p.bilateral_d, p.bilateral_sigma_color, p.bilateral_sigma_space = d, sc, ss
    return p


class Memory(NamedTuple):
    """Engine.memory(): what the context holds (eincm_get_memory).  scratch_bytes is part of device_bytes."""
    device_bytes: int
    pinned_bytes: int
    allocations: int
    scratch_bytes: int


class GtFlowPlan(NamedTuple):
    """One window of eincm_gt_flow, made by evaluation.gt_flow_plan.  mode: 'direct' or 'propagate'; steps: a
    tuple of (frame, num, den).  A direct window has one step, out = g[frame] * num / den; a propagate window moves every pixel through
    its steps in order by g[frame] * num (den is 1.0 there and not read)."""
    mode: str
    steps: tuple


def check_gt_flow_plans(plans, n_frames):
    """eincm_gt_flow's checks of a list of GtFlowPlan against a stack of n_frames frames, made here before any GPU call.  Returns the
    (first, last) frame the plans read."""
    plans = list(plans)
    if not plans:
        raise ValueError('no windows')
    lo, hi = None, None
    for b, plan in enumerate(plans):
        mode, steps = plan
        if mode not in L.GTF_MODES:
            raise ValueError(f'window {b}: mode {mode!r}, one of {sorted(L.GTF_MODES)}')
        if len(steps) < 1:
            raise ValueError(f'window {b} has no steps')
        if mode == 'direct' and len(steps) != 1:
            raise ValueError(f'window {b}: a direct window has {len(steps)} steps (1)')
        for f, num, den in steps:
            if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= f < n_frames:
                raise ValueError(f'window {b}: frame {f!r} outside [0, {n_frames})')
            if not np.isfinite(num):
                raise ValueError(f'window {b}: scale {num!r} is not finite')
            if mode == 'direct' and (den == 0 or not np.isfinite(den)):
                raise ValueError(f'window {b}: den {den!r} must be finite and non-zero')
            lo = int(f) if lo is None else min(lo, int(f))
            hi = int(f) if hi is None else max(hi, int(f))
    return lo, hi


def gt_flow_stacks(gt_x, gt_y, sensor_size):
    """The (n_frames, H, W) x and y flow stacks in the type eincm_gt_flow reads: float32 when both are float32, else float64 (the same
    output: DESIGN.md section 15)."""
    gx, gy = np.asarray(gt_x), np.asarray(gt_y)
    H, W = int(sensor_size[0]), int(sensor_size[1])
    for name, a in (('gt_x', gx), ('gt_y', gy)):
        if a.ndim != 3 or a.shape[1:] != (H, W):
            raise ValueError(f'{name} must be (n_frames, {H}, {W}), got {a.shape}')
        if a.dtype not in (np.float32, np.float64):
            raise ValueError(f'{name} must be float32 or float64, got {a.dtype}')
    if gx.shape != gy.shape:
        raise ValueError(f'gt_x {gx.shape} and gt_y {gy.shape} differ')
    dt = np.float32 if gx.dtype == gy.dtype == np.float32 else np.float64
    return gx.astype(dt, copy=False), gy.astype(dt, copy=False)


_remap_table = None


def remap_cubic_table():
    """The (32, 32, 16) int32 weight table of the remap contract.  Row (fy, fx), entry ky * 4 + kx.  1-D Keys
    cubic, A = -0.75, in float32 at f / 32; 2-D weight rint(wy * wx * 32768) (float32 product, half to even); then the row is made to
    sum to 32768: the difference is added to the largest of the central 2 x 2 weights when the sum is short and taken off the smallest
    when it is over (first in row-major order on a tie).  int32, so that the single weight 32768 of fraction (0, 0) is held exactly."""
    global _remap_table
    if _remap_table is None:
        f32 = np.float32
        A = f32(-0.75)
        x = np.arange(32, dtype=f32) / f32(32)
        x1, xm = x + f32(1), f32(1) - x
        c = np.empty((32, 4), dtype=f32)
        c[:, 0] = ((A * x1 - f32(5) * A) * x1 + f32(8) * A) * x1 - f32(4) * A
        c[:, 1] = ((A + f32(2)) * x - (A + f32(3))) * x * x + f32(1)
        c[:, 2] = ((A + f32(2)) * xm - (A + f32(3))) * xm * xm + f32(1)
        c[:, 3] = f32(1) - c[:, 0] - c[:, 1] - c[:, 2]
        w = (c[:, None, :, None] * c[None, :, None, :]).astype(f32) * f32(32768)          # (fy, fx, ky, kx)
        t = np.rint(w).astype(np.int32)
        for fy in range(32):
            for fx in range(32):
                d = int(t[fy, fx].sum()) - 32768
                if d:
                    mid = t[fy, fx, 1:3, 1:3].reshape(-1)
                    k = int(np.argmax(mid)) if d < 0 else int(np.argmin(mid))         # argmax / argmin: the first on a tie
                    t[fy, fx, 1 + k // 2, 1 + k % 2] -= d
        _remap_table = np.ascontiguousarray(t.reshape(32, 32, 16))
        _remap_table.setflags(write=False)
    return _remap_table


def check_rectify_map(rectify_map, sensor_size, what='rectify_map'):
    """A (H, W, 2) float32 map, C-contiguous.  Shape and type only: the values are checked on the GPU, once per map."""
    H, W = int(sensor_size[0]), int(sensor_size[1])
    m = np.asarray(rectify_map)
    if m.shape != (H, W, 2):
        raise ValueError(f'{what} must be ({H}, {W}, 2), got {m.shape}')
    if m.dtype != np.float32:
        raise ValueError(f'{what} must be float32, got {m.dtype}')
    return np.ascontiguousarray(m)


def check_event_coords(x, y):
    """The x and y of an event stream as 1-D int16 arrays of one length (integer input only: a raw stream has no fractions)."""
    x, y = np.asarray(x), np.asarray(y)
    for name, a in (('x', x), ('y', y)):
        if a.ndim != 1:
            raise ValueError(f'event {name} must be 1-D, got shape {a.shape}')
        if a.dtype.kind not in 'iu':
            raise ValueError(f'event {name} must be an integer array, got {a.dtype}')
    if x.shape != y.shape:
        raise ValueError(f'event x {x.shape} and y {y.shape} differ in length')
    return np.ascontiguousarray(as_int16_coords(x, 'x')), np.ascontiguousarray(as_int16_coords(y, 'y'))


def check_chunk(chunk):
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= 1 << 30:
        raise ValueError(f'chunk {chunk!r}: an integer number of events in [1, 2^30]')
    return int(chunk)


def chunk_walk(n, chunk):
    """The [i0, i1) pieces of a stream of n events, ``chunk`` at a time.  An empty stream is one empty piece: it still reaches the
    library once (a map handed over is checked, a carried state is cleared)."""
    for i0 in ([0] if n == 0 else range(0, n, chunk)):
        yield i0, min(n, i0 + chunk)


EVENT_SUPPORT_MAX_RADIUS = 3      # ES_MAX_RADIUS (csrc/eincm_event_support.h)


def check_event_times(t, n):
    """The times of a raw stream as a 1-D float64 array of n elements.  Floating input is widened; integer input (microsecond ticks)
    goes to float64 only if every value has magnitude <= 2^53, where the conversion is exact."""
    a = np.asarray(t)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f'event t must be 1-D with {n} elements, got shape {a.shape}')
    if a.dtype.kind == 'b' or a.dtype.kind not in 'iuf':
        raise ValueError(f'event t must be floating or integer, got {a.dtype}')
    if a.dtype.kind in 'iu' and a.size and (int(a.max()) > 1 << 53 or int(a.min()) < -(1 << 53)):
        raise ValueError('integer event times beyond 2^53 do not convert to float64 exactly')
    return np.ascontiguousarray(a, dtype=np.float64)


def check_event_support_args(tau, radius, full_support):
    """(tau, radius, full_support) of the event-support filter as (float, int, int); ValueError as eincm_event_support refuses them."""
    try:
        tau = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f'tau {tau!r}: a finite number >= 0') from None
    if not np.isfinite(tau) or tau < 0.0:
        raise ValueError(f'tau = {tau!r} (finite and >= 0)')
    for name, v in (('radius', radius), ('full_support', full_support)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'{name} {v!r}: an integer')
    if not 1 <= radius <= EVENT_SUPPORT_MAX_RADIUS:
        raise ValueError(f'radius = {radius} outside [1, {EVENT_SUPPORT_MAX_RADIUS}]')
    most = (2 * int(radius) + 1) ** 2 - 1
    if not 1 <= full_support <= most:
        raise ValueError(f'full_support = {full_support} outside [1, {most}] for radius {radius}')
    return tau, int(radius), int(full_support)


EVENT_FILTER_POLARITY = 1         # EINCM_EF_POLARITY (include/eincm.h)


def check_event_filter_args(refractory, tau, radius, full_support, polarity):
    """(refractory, tau, radius, full_support, flags) of the event filter; ValueError as eincm_event_filter refuses them.  radius 0
    switches the support stage off and leaves full_support one value."""
    try:
        refractory = float(refractory)
    except (TypeError, ValueError):
        raise ValueError(f'refractory {refractory!r}: a finite number >= 0') from None
    if not np.isfinite(refractory) or refractory < 0.0:
        raise ValueError(f'refractory = {refractory!r} (finite and >= 0)')
    if isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) and radius == 0:
        tau, _, _ = check_event_support_args(tau, 1, 1)
        if isinstance(full_support, bool) or not isinstance(full_support, (int, np.integer)) or full_support != 1:
            raise ValueError(f'full_support = {full_support!r} with radius 0 (the support stage is off: 1)')
    else:
        tau, radius, full_support = check_event_support_args(tau, radius, full_support)
    if not isinstance(polarity, (bool, np.bool_)):
        raise ValueError(f'polarity {polarity!r}: True or False')
    return refractory, tau, int(radius), int(full_support), EVENT_FILTER_POLARITY if polarity else 0


def check_event_polarity(ps, n, polarity):
    """None, or the polarity classes of a raw stream as int8 (1 where the input is > 0: {0, 1} and {-1, +1} recordings alike)."""
    if ps is None:
        if polarity:
            raise ValueError('polarity=True needs the events\' polarities')
        return None
    a = np.asarray(ps)
    if a.ndim != 1 or a.shape[0] != n:
        raise ValueError(f'event p must be 1-D with {n} elements, got shape {a.shape}')
    if a.dtype.kind not in 'biu':
        raise ValueError(f'event p must be a boolean or integer array, got {a.dtype}')
    return np.ascontiguousarray(a > 0, dtype=np.int8)


def check_pixel_mask(pixel_mask, shape):
    """None, or the (H, W) mask as uint8 with 1 where the input is non-zero."""
    if pixel_mask is None:
        return None
    m = np.asarray(pixel_mask)
    if m.shape != tuple(shape) or m.dtype.kind not in 'biu':
        raise ValueError(f'pixel_mask must be a bool or integer array of shape {tuple(shape)}, got {m.dtype} {m.shape}')
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def event_support_first_offender(xs, ys, ts, shape, carried=-np.inf):
    """The first event eincm_event_support refuses, as (index, why), or None: a coordinate outside the sensor, a non-finite time, a
    time smaller than its predecessor's (``carried`` for event 0).  An event's refusal depends on itself and on its predecessor's
    time alone, so the first of the stream is the smallest index of the vectorised test."""
    H, W = shape
    n = xs.shape[0]
    if n == 0:
        return None
    # a good stream, in a few reductions: every coordinate inside, and times that never step back between two finite ends are all
    # finite (a NaN fails both comparisons it takes part in; an infinity cannot lie between finite neighbours of a sorted run)
    if (xs.min() >= 0 and xs.max() < W and ys.min() >= 0 and ys.max() < H and np.isfinite(ts[0]) and np.isfinite(ts[-1])
            and not ts[0] < carried and bool(np.all(ts[1:] >= ts[:-1]))):
        return None
    prev = np.concatenate(([carried], ts[:-1]))
    coord = (xs < 0) | (xs >= W) | (ys < 0) | (ys >= H)
    time = ~np.isfinite(ts)
    with np.errstate(invalid='ignore'):
        order = ts < prev
    bad = coord | time | order
    if not bad.any():
        return None
    e = int(np.argmax(bad))
    if coord[e]:
        return e, f'event {e}: ({int(xs[e])}, {int(ys[e])}) outside the {H}x{W} sensor'
    if time[e]:
        return e, f'event {e}: time {ts[e]!r} is not finite'
    return e, f'event {e}: time {ts[e]!r} is smaller than its predecessor\'s {prev[e]!r}'


def check_raw_stream(xs, ys, ts, pixel_mask, chunk, shape):
    """What the operators on a raw stream take before their own arguments: (x, y int16, t float64, mask uint8 or None, chunk) of a
    stream on a sensor of ``shape``.  ValueError: every refusal of the arrays, and the first event the C contract refuses."""
    x, y = check_event_coords(xs, ys)
    t = check_event_times(ts, x.shape[0])
    mask = check_pixel_mask(pixel_mask, shape)
    chunk = check_chunk(chunk)
    bad = event_support_first_offender(x, y, t, shape)
    if bad is not None:
        raise ValueError(bad[1])
    return x, y, t, mask, chunk


def check_remap_args(src, mapping):
    """src (n, Hs, Ws) or (Hs, Ws) uint8 with 1 <= Hs, Ws <= 32766; mapping (H, W, 2) float32.  Returns (src as a stack, mapping, single)."""
    a = np.asarray(src)
    if a.dtype != np.uint8:
        raise ValueError(f'remap input must be uint8, got {a.dtype}')
    single = a.ndim == 2
    a = np.ascontiguousarray(a[None] if single else a)
    if a.ndim != 3 or a.shape[0] < 1 or not (1 <= a.shape[1] <= 32766 and 1 <= a.shape[2] <= 32766):
        raise ValueError(f'remap input must be (n, Hs, Ws) or (Hs, Ws) with n >= 1 and 1 <= Hs, Ws <= 32766, got {np.shape(src)}')
    m = np.asarray(mapping)
    if m.ndim != 3 or m.shape[2] != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f'mapping must be (H, W, 2), got {m.shape}')
    if m.dtype != np.float32:
        raise ValueError(f'mapping must be float32, got {m.dtype}')
    return a, np.ascontiguousarray(m), single


def check_flow_16bit(flow_16bit):
    """(B, H, W, 3) or (H, W, 3) uint16 (dsec_loader.py:249-252).  Returns (stack, single)."""
    a = np.asarray(flow_16bit)
    if a.dtype != np.uint16:
        raise ValueError(f'16-bit flow must be uint16, got {a.dtype}')
    single = a.ndim == 3
    a = a[None] if single else a
    if a.ndim != 4 or a.shape[3] != 3 or a.shape[0] < 1:
        raise ValueError(f'16-bit flow must be (B, H, W, 3) or (H, W, 3), got {np.shape(flow_16bit)}')
    return np.ascontiguousarray(a), single


def check_theta_batch(theta, valid, sensor_size):
    """theta (B, h, w, 2) or (h, w, 2) as float64; valid None or (B, H, W) / (H, W).  Returns (theta, valid uint8 or None, single)."""
    t = np.asarray(theta)
    if t.dtype.kind not in 'fiu':
        raise ValueError(f'theta must be numeric, got {t.dtype}')
    single = t.ndim == 3
    t = t[None] if single else t
    if t.ndim != 4 or t.shape[3] != 2 or min(t.shape[:3]) < 1 or t.shape[0] > 65535:
        raise ValueError(f'theta must be (B, h, w, 2) or (h, w, 2) with 1 <= B <= 65535, got {np.shape(theta)}')
    t = np.ascontiguousarray(t, dtype=np.float64)
    v = None
    if valid is not None:
        v = np.asarray(valid)
        v = v[None] if single and v.ndim == 2 else v
        if v.shape != (t.shape[0], int(sensor_size[0]), int(sensor_size[1])):
            raise ValueError(f'valid must be {(t.shape[0], int(sensor_size[0]), int(sensor_size[1]))}, got {np.shape(valid)}')
        v = np.ascontiguousarray(v != 0).astype(np.uint8)
    return t, v, single


def check_flow_eval_batch(gt_flows, events, eval_masks, sensor_size):
    """The arguments of Engine.flow_eval_stage, checked without a GPU.  gt_flows (n, H, W, 2) float32 or float64 (widened exactly);
    events: one (xs, ys) per window, any integer or float coordinates as_int16_coords takes; eval_masks None or (n, H, W), non-zero =
    evaluate.  Returns (gt float64, n_events int64 (n,), xs int16 concatenated, ys, masks uint8 or None)."""
    H, W = int(sensor_size[0]), int(sensor_size[1])
    g = np.asarray(gt_flows)
    if g.dtype not in (np.float32, np.float64):
        raise ValueError(f'gt_flows must be float32 or float64, got {g.dtype}')
    if g.ndim != 4 or g.shape[0] < 1 or g.shape[1:] != (H, W, 2):
        raise ValueError(f'gt_flows must be (n, {H}, {W}, 2) with n >= 1, got {g.shape}')
    n = g.shape[0]
    if n > 65535:
        raise ValueError(f'{n} windows: at most 65535 in one staging')
    events = list(events)
    if len(events) != n:
        raise ValueError(f'{len(events)} event lists for {n} ground-truth flows')
    xs, ys = [], []
    for b, e in enumerate(events):
        if len(e) != 2:
            raise ValueError(f'window {b}: events must be (xs, ys)')
        x, y = as_int16_coords(e[0], 'xs'), as_int16_coords(e[1], 'ys')
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError(f'window {b}: xs {x.shape} and ys {y.shape} must be 1-D of one length')
        xs.append(x)
        ys.append(y)
    m = None
    if eval_masks is not None:
        m = np.asarray(eval_masks)
        if m.dtype.kind not in 'biuf':
            raise ValueError(f'eval_masks must be boolean or numeric, got {m.dtype}')
        if m.shape != (n, H, W):
            raise ValueError(f'eval_masks must be {(n, H, W)}, got {m.shape}')
        m = np.ascontiguousarray(m != 0).astype(np.uint8)
    n_events = np.array([len(x) for x in xs], dtype=np.int64)
    cat = lambda a: np.ascontiguousarray(np.concatenate(a)) if n_events.sum() else np.zeros(1, np.int16)      # noqa: E731 (a valid address)
    return np.ascontiguousarray(g, dtype=np.float64), n_events, cat(xs), cat(ys), m


def check_flow_eval_thetas(thetas, n_windows, sensor_size, method):
    """thetas (n, h, w, 2), or (h, w, 2) for one staged window, no finer than the sensor; method a name of _lib.METHODS.  Returns
    (thetas float64, method code)."""
    if not isinstance(method, str) or method not in L.METHODS:
        raise ValueError(f'method {method!r} not supported; one of {sorted(L.METHODS)}')
    t = np.asarray(thetas)
    if t.dtype.kind not in 'fiu':
        raise ValueError(f'thetas must be numeric, got {t.dtype}')
    if t.ndim == 3 and n_windows == 1:
        t = t[None]
    if t.ndim != 4 or t.shape[3] != 2 or t.shape[0] != n_windows or min(t.shape[1:3]) < 1:
        raise ValueError(f'thetas must be ({n_windows}, h, w, 2), got {np.shape(thetas)}')
    if t.shape[1] > int(sensor_size[0]) or t.shape[2] > int(sensor_size[1]):
        raise ValueError(f'thetas {t.shape[1:3]} are finer than the sensor {tuple(int(v) for v in sensor_size)}')
    return np.ascontiguousarray(t, dtype=np.float64), L.METHODS[method]


def check_motion_model(model, sensor_size):
    """A motion.MotionModel for this sensor (or None, which clears the engine's model); anything else is a ValueError."""
    if model is None:
        return None
    from .motion import MotionModel
    if not isinstance(model, MotionModel):
        raise ValueError(f'model must be a motion.MotionModel or None, got {type(model).__name__}')
    if tuple(model.sensor_size) != tuple(int(s) for s in sensor_size):
        raise ValueError(f'the model was built for sensor size {model.sensor_size}, the engine has {tuple(sensor_size)}')
    return model


def check_motion_coeffs(coeffs, n_windows, model):
    """coeffs as a C-contiguous float64 (B, K) array; (K,) stands for it when B == 1."""
    if model is None:
        raise ValueError('no motion model set (Engine.set_motion_model)')
    c = np.asarray(coeffs)
    if c.dtype.kind not in 'fiu':
        raise ValueError(f'coeffs must be numeric, got dtype {c.dtype}')
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.ndim == 1 and n_windows == 1:
        c = c[None]
    if c.shape != (n_windows, model.n_coeffs):
        raise ValueError(f'coeffs must be ({n_windows},{model.n_coeffs}), got {np.shape(coeffs)}')
    return c


MOTION_PATHS = ('expanded', 'fused', 'auto')


def check_motion_path(path):
    """'expanded' (the Theta image and the dense gradient), 'fused' (the polynomial inside the event kernels,
    section 21) or 'auto' (fused where it applies and is the faster one); anything else is a ValueError."""
    if path not in MOTION_PATHS:
        raise ValueError(f"path {path!r}: one of 'expanded', 'fused', 'auto'")
    return path


def check_event_weights(weights, n):
    """Per-event weights of one window as the contiguous float32 array staging hands over: ``n`` values, finite and
    within [0, 1], rounded to float32 once, here.  Anything else is a ValueError, raised before any library call."""
    w = np.asarray(weights)
    if w.dtype.kind not in 'fiub':
        raise ValueError(f'weights must be numbers, got dtype {w.dtype}')
    if w.shape != (int(n),):
        raise ValueError(f'weights must be ({int(n)},), one per event, got {w.shape}')
    if w.size:
        # two passes and no copy of a float32 array (a batch of 8 x 10^6 weights is staged in milliseconds); a NaN anywhere makes both NaN,
        # and the range is checked on the values as given, before the rounding
        lo, hi = float(w.min()), float(w.max())
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError('weights must be finite')
        if lo < 0.0 or hi > 1.0:
            raise ValueError(f'weights must lie within [0, 1], got {lo if lo < 0.0 else hi!r} (signed weights are out of scope; larger '
                             'ones would break the fixed-point bounds: scale them down)')
    return np.ascontiguousarray(w, dtype=np.float32)


def event_scores_layout(n_events, n_refs, combined):
    """(offsets (B,), lengths (B,), total) of the windows' blocks in the ``scores`` / ``selfs`` arrays of eincm_event_scores, in floats
    (csrc/eincm_event_scores.h: sc_block_offset, sc_block_len, sc_total, restated; tests/test_event_scores_interface.py compares the
    two): (n_refs, n_events[b]) per window, or (n_events[b]) in the combined form, one block after the other."""
    n = np.asarray(n_events, dtype=np.int64).reshape(-1)
    lengths = n if combined else n * int(n_refs)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if n.size else np.zeros(0, np.int64)
    return offsets, lengths.astype(np.int64), int(lengths.sum())


def event_responsibilities_layout(n_events, n_models):
    """(weight offsets (B,), weight total, label offsets (G,), label lengths (G,), label total) of eincm_event_responsibilities
    (csrc/eincm_responsibilities.h: rs_weights_offset, rs_weights_total, rs_labels_offset, rs_group_events, rs_labels_total, restated;
    tests/test_responsibilities_interface.py compares the two): window b's block of ``weights_out`` is n_events[b] floats, group g's
    block of ``labels`` one byte per event of its first window, each kind one block after the other."""
    n = np.asarray(n_events, dtype=np.int64).reshape(-1)
    K = int(n_models)
    w_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if n.size else np.zeros(0, np.int64)
    lab_len = n[:(n.size // K) * K:K].astype(np.int64)
    lab_off = np.concatenate([[0], np.cumsum(lab_len)[:-1]]).astype(np.int64) if lab_len.size else np.zeros(0, np.int64)
    return w_off, int(n.sum()), lab_off, lab_len, int(lab_len.sum())


RS_OUTPUTS = ('weights', 'labels', 'mass', 'n_unsupported')


def check_responsibility_args(n_models, n_events, prior, want):
    """The arguments of Engine.event_responsibilities that csrc/eincm_responsibilities.h refuses too, checked without a GPU: n_models
    within 1 .. RS_MAX_MODELS and dividing the batch, equal event counts inside a group, prior None or (B,) finite and >= 0 as float32
    with a positive sum in every group, want a non-empty subset of RS_OUTPUTS.  Returns (n_models, prior float64 or None, want)."""
    if isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer)) or not 1 <= int(n_models) <= L.RS_MAX_MODELS:
        raise ValueError(f'n_models must be an integer within 1 .. {L.RS_MAX_MODELS}, got {n_models!r}')
    K = int(n_models)
    n = np.asarray(n_events, dtype=np.int64).reshape(-1)
    if n.size % K:
        raise ValueError(f'the {n.size} staged windows are not a whole number of groups of {K} models')
    if n.size and (n.reshape(-1, K) != n.reshape(-1, K)[:, :1]).any():
        raise ValueError('the windows of a group must have equal numbers of events (they are one event list under several motions)')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in RS_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a non-empty choice of {RS_OUTPUTS} without repeats, got {want!r}')
    if prior is not None:
        p = np.asarray(prior)
        if p.dtype.kind not in 'fiub' or p.shape != (n.size,):
            raise ValueError(f'prior must be ({n.size},) numbers, one per staged window, got {p.dtype} {p.shape}')
        prior = np.ascontiguousarray(p, dtype=np.float64)
        with np.errstate(over='ignore'):
            p32 = prior.astype(np.float32)
        if not (np.isfinite(prior).all() and np.isfinite(p32).all()) or (prior < 0).any():
            raise ValueError('prior must be finite and >= 0')
        s = p32.reshape(-1, K).sum(axis=1, dtype=np.float32) if n.size else np.ones(0, np.float32)
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("every group's prior must have a positive (finite) sum")
    return K, prior, want


CL_OUTPUTS = ('sumsq', 'n_in')


def check_contrast_landscape_args(coeffs, n_events, n_coeffs, t_ref, cell, keep, want):
    """The arguments of Engine.contrast_landscape that csrc/eincm_contrast_landscape.h refuses too, and every shape, checked without a
    GPU.  n_events: the staged windows' event counts (B,); n_coeffs: K of the engine's motion model, None when none is set.  coeffs
    (B, V, K), or (V, K) when B == 1, finite, 1 <= V <= CL_MAX_CANDIDATES; t_ref None (0.5 for every window), a number or (B,), finite;
    cell one of CL_CELLS; keep None or B entries, each None or (n_events[b],) of booleans or integers; want a non-empty choice of
    CL_OUTPUTS.  Returns (coeffs (B, V, K) float64, t_ref (B,) float64, cell, keep as None or a list of None / uint8 arrays, want)."""
    n = np.asarray(n_events, dtype=np.int64).reshape(-1)
    B = n.size
    if B < 1:
        raise ValueError('no windows staged (Engine.set_windows)')
    if n_coeffs is None:
        raise ValueError('no motion model set (Engine.set_motion_model)')
    K = int(n_coeffs)
    c = np.asarray(coeffs)
    if c.dtype.kind not in 'fiu':
        raise ValueError(f'coeffs must be numeric, got dtype {c.dtype}')
    if c.ndim == 2 and B == 1:
        c = c[None]
    if c.ndim != 3 or c.shape[0] != B or c.shape[2] != K:
        raise ValueError(f'coeffs must be ({B}, V, {K})' + (f' or (V, {K})' if B == 1 else '') + f', got {np.shape(coeffs)}')
    if not 1 <= c.shape[1] <= L.CL_MAX_CANDIDATES:
        raise ValueError(f'the number of candidates must lie within 1 .. {L.CL_MAX_CANDIDATES}, got {c.shape[1]}')
    c = np.ascontiguousarray(c, dtype=np.float64)
    if not np.isfinite(c).all():
        raise ValueError('coeffs must be finite')
    t = np.asarray(0.5 if t_ref is None else t_ref)
    if t.dtype.kind not in 'fiu' or t.shape not in ((), (B,)):
        raise ValueError(f't_ref must be a number or ({B},) numbers, got {t.dtype} {t.shape}')
    t = np.ascontiguousarray(np.broadcast_to(t.astype(np.float64), (B,)))
    if not np.isfinite(t).all():
        raise ValueError('t_ref must be finite')
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or int(cell) not in L.CL_CELLS:
        raise ValueError(f'cell must be one of {L.CL_CELLS}, got {cell!r}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in CL_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a non-empty choice of {CL_OUTPUTS} without repeats, got {want!r}')
    if keep is not None:
        if isinstance(keep, np.ndarray) and keep.ndim == 1 and B == 1:
            keep = [keep]
        if len(keep) != B:
            raise ValueError(f'keep must hold {B} entries, one per staged window, got {len(keep)}')
        masks = []
        for b, k in enumerate(keep):
            if k is None:
                masks.append(None)
                continue
            k = np.asarray(k)
            if k.dtype.kind not in 'biu' or k.shape != (int(n[b]),):
                raise ValueError(f'keep[{b}] must be ({int(n[b])},) booleans or integers, got {k.dtype} {k.shape}')
            masks.append(np.ascontiguousarray(k != 0, dtype=np.uint8))
        keep = masks
    return c, t, int(cell), keep, want


ML_OUTPUTS = ('theta', 'labels', 'mass', 'total')


def compose_motions_layout(n_groups, n_models, sensor_size):
    """The shapes of eincm_compose_motions' four outputs and where a group's block starts in each, in elements of the output's own type
    (csrc/eincm_motion_layers.h: ml_theta_offset, ml_labels_offset, ml_mass_offset, ml_total_offset, restated;
    tests/test_motion_layers_interface.py compares the two): a dict name -> (shape, dtype, offsets (G,) int64)."""
    G, K, H, W = int(n_groups), int(n_models), int(sensor_size[0]), int(sensor_size[1])
    g = np.arange(G, dtype=np.int64)
    return {'theta': ((G, H, W, 2), np.float64, g * (H * W * 2)), 'labels': ((G, H, W), np.uint8, g * (H * W)),
            'mass': ((G, K, H, W), np.uint32, g * (K * H * W)), 'total': ((G, K), np.uint64, g * K)}


def check_compose_args(n_models, coeffs, n_windows, n_coeffs, mode, fill, want):
    """The arguments of Engine.compose_motions, checked without a GPU: n_models an integer within 1 .. RS_MAX_MODELS; mode one of
    ML_MODES and fill one of ML_FILLS; want a non-empty choice of ML_OUTPUTS without repeats; coeffs a numeric (B, K_c) array, B the
    staged windows and K_c the model's coefficients where the engine knows them (n_windows 0: nothing staged, n_coeffs None: no model
    - the library refuses those itself).  What depends on the staged batch or on the values - nothing staged, no model, the context's
    precision, B not a multiple of n_models, unequal groups, a coefficient that is not finite, a crowded tile - is left to the library,
    so that those refusals carry the codes and the sentences of csrc/eincm_motion_layers.h.  Returns (n_models, coeffs float64
    C-contiguous, flags, want)."""
    if isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer)) or not 1 <= int(n_models) <= L.RS_MAX_MODELS:
        raise ValueError(f'n_models must be an integer within 1 .. {L.RS_MAX_MODELS}, got {n_models!r}')
    if mode not in L.ML_MODES:
        raise ValueError(f'mode {mode!r} unknown; one of {tuple(L.ML_MODES)}')
    if fill not in L.ML_FILLS:
        raise ValueError(f'fill {fill!r} unknown; one of {tuple(L.ML_FILLS)}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in ML_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a non-empty choice of {ML_OUTPUTS} without repeats, got {want!r}')
    c = np.asarray(coeffs)
    if c.dtype.kind not in 'fiu':
        raise ValueError(f'coeffs must be numeric, got dtype {c.dtype}')
    rows = 'B' if not n_windows else str(int(n_windows))
    cols = 'K_c' if n_coeffs is None else str(int(n_coeffs))
    if c.ndim != 2 or (n_windows and c.shape[0] != n_windows) or (n_coeffs is not None and c.shape[1] != n_coeffs):
        raise ValueError(f'coeffs must be ({rows}, {cols}): one row of model coefficients per staged window, got {np.shape(coeffs)}')
    return int(n_models), np.ascontiguousarray(c, dtype=np.float64), L.ML_MODES[mode] | L.ML_FILLS[fill], want


MF_OUTPUTS = ('theta', 'labels', 'dist2', 'nearest', 'n_sites')


def densify_motions_layout(n_groups, sensor_size):
    """The shapes of eincm_densify_motions' five outputs and where a group's block starts in each, in elements of the output's own
    type (csrc/eincm_motion_fill.h: mf_theta_offset ... mf_nsites_offset, restated; tests/test_host_motion_fill.py compares the two):
    a dict name -> (shape, dtype, offsets (G,) int64)."""
    G, H, W = int(n_groups), int(sensor_size[0]), int(sensor_size[1])
    g = np.arange(G, dtype=np.int64)
    return {'theta': ((G, H, W, 2), np.float64, g * (H * W * 2)), 'labels': ((G, H, W), np.uint8, g * (H * W)),
            'dist2': ((G, H, W), np.uint32, g * (H * W)), 'nearest': ((G, H, W), np.int32, g * (H * W)), 'n_sites': ((G,), np.uint32, g)}


def check_densify_args(n_models, coeffs, n_windows, n_coeffs, mode, fallback, min_site_mass, max_distance, want):
    """The arguments of Engine.densify_motions, checked without a GPU.  n_models, coeffs and mode as check_compose_args takes them;
    fallback one of ML_FILLS (what a pixel that no site reaches takes); min_site_mass an integer within 1 .. 2^32 - 1; max_distance
    None (no bound) or a finite number >= 0 in pixels, which becomes max_dist2 = floor(float64(max_distance)^2), at most 0xFFFFFFFE;
    want a non-empty choice of MF_OUTPUTS without repeats.  What depends on the staged batch or on the values is left to the library,
    as there.  Returns (n_models, coeffs float64 C-contiguous, flags, min_site_mass, max_dist2, want)."""
    if mode not in L.ML_MODES:
        raise ValueError(f'mode {mode!r} unknown; one of {tuple(L.ML_MODES)}')
    if fallback not in L.ML_FILLS:
        raise ValueError(f'fallback {fallback!r} unknown; one of {tuple(L.ML_FILLS)}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in MF_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a non-empty choice of {MF_OUTPUTS} without repeats, got {want!r}')
    if isinstance(min_site_mass, bool) or not isinstance(min_site_mass, (int, np.integer)) or not 1 <= int(min_site_mass) <= 0xFFFFFFFF:
        raise ValueError(f'min_site_mass must be an integer within 1 .. 2^32 - 1 (4096 is one event of weight 1), got {min_site_mass!r}')
    if max_distance is None:
        max_dist2 = L.MD_UNBOUNDED
    else:
        if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)) \
                or not np.isfinite(max_distance) or max_distance < 0:
            raise ValueError(f'max_distance must be None or a finite number >= 0, got {max_distance!r}')
        d = np.float64(max_distance)
        with np.errstate(over='ignore'):
            max_dist2 = int(min(np.floor(d * d), np.float64(0xFFFFFFFE)))
    K, c, flags, _ = check_compose_args(n_models, coeffs, n_windows, n_coeffs, mode, fallback, ('theta',))
    return K, c, flags, int(min_site_mass), max_dist2, want


LP_OUTPUTS = ('prior', 'smoothed')


def label_prior_layout(n_groups, n_models, sensor_size):
    """The shapes of eincm_label_prior's two outputs and where a group's block starts in each, in elements of the output's own type
    (csrc/eincm_label_prior.h: lp_prior_offset, lp_smoothed_offset, restated; tests/test_host_label_prior.py compares the two): a dict
    name -> (shape, dtype, offsets (G,) int64).  'prior' is per window, window g * n_models + l model l of group g."""
    G, K, H, W = int(n_groups), int(n_models), int(sensor_size[0]), int(sensor_size[1])
    g = np.arange(G, dtype=np.int64)
    return {'prior': ((G * K, H, W), np.float32, g * (K * H * W)), 'smoothed': ((G, K, H, W), np.uint64, g * (K * H * W))}


def check_label_prior_args(n_models, radius, floor_mass, want):
    """The arguments of Engine.label_prior, checked without a GPU: n_models an integer within 1 .. RS_MAX_MODELS, radius an integer
    within 0 .. LP_MAX_RADIUS, floor_mass an integer within 0 .. 2^32 - 1, want a choice of LP_OUTPUTS without repeats that may be
    empty (the prior is staged all the same).  What depends on the staged batch is left to the library, so that those refusals carry
    the codes and the sentences of csrc/eincm_label_prior.h.  Returns (n_models, radius, floor_mass, want)."""
    if isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer)) or not 1 <= int(n_models) <= L.RS_MAX_MODELS:
        raise ValueError(f'n_models must be an integer within 1 .. {L.RS_MAX_MODELS}, got {n_models!r}')
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= L.LP_MAX_RADIUS:
        raise ValueError(f'radius must be an integer within 0 .. {L.LP_MAX_RADIUS}, got {radius!r}')
    if isinstance(floor_mass, bool) or not isinstance(floor_mass, (int, np.integer)) or not 0 <= int(floor_mass) <= 0xFFFFFFFF:
        raise ValueError(f'floor_mass must be an integer within 0 .. 2^32 - 1 (4096 is one event of weight 1), got {floor_mass!r}')
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in LP_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a choice of {LP_OUTPUTS} without repeats, got {want!r}')
    return int(n_models), int(radius), int(floor_mass), want


LC_OUTPUTS = ('prior', 'carried', 'accum', 'dropped')


def label_carry_layout(n_groups, n_models, sensor_size):
    """The shapes of eincm_carry_label_prior's four outputs and where a group's block starts in each, in elements of the output's own
    type (csrc/eincm_label_carry.h: lc_prior_offset, lc_carried_offset, lc_accum_offset, lc_dropped_offset, restated;
    tests/test_host_label_carry.py compares the two): a dict name -> (shape, dtype, offsets (G,) int64).  'prior' is per window, window
    g * n_models + l model l of group g."""
    G, K, H, W = int(n_groups), int(n_models), int(sensor_size[0]), int(sensor_size[1])
    g = np.arange(G, dtype=np.int64)
    return {'prior': ((G * K, H, W), np.float32, g * (K * H * W)), 'carried': ((G, K, H, W), np.uint32, g * (K * H * W)),
            'accum': ((G, K, H, W), np.uint64, g * (K * H * W)), 'dropped': ((G, K), np.uint64, g * K)}


def check_label_carry_args(n_models, coeffs, n_windows, n_coeffs, tau, radius, floor_mass, want):
    """The arguments of Engine.carry_label_prior, checked without a GPU.  n_models, radius and floor_mass as check_label_prior_args
    takes them; want a choice of LC_OUTPUTS without repeats that may be empty (the prior is carried all the same); coeffs a numeric
    (B, K_c) array as check_compose_args takes it, except that its values need not be finite (a source whose field is not finite is
    dropped); tau a finite number or (G,) of them, G = B / n_models where the engine knows B (n_windows 0: nothing staged - the library
    refuses that itself).  What depends on the staged batch is left to the library, so that those refusals carry the codes and the
    sentences of csrc/eincm_label_carry.h.  Returns (n_models, coeffs float64 C-contiguous, tau (G,) float64 or as handed over where G
    is unknown, radius, floor_mass, want)."""
    K, r, floor, _ = check_label_prior_args(n_models, radius, floor_mass, ())
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in LC_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f'want must be a choice of {LC_OUTPUTS} without repeats, got {want!r}')
    c = np.asarray(coeffs)
    if c.dtype.kind not in 'fiu':
        raise ValueError(f'coeffs must be numeric, got dtype {c.dtype}')
    rows = 'B' if not n_windows else str(int(n_windows))
    cols = 'K_c' if n_coeffs is None else str(int(n_coeffs))
    if c.ndim != 2 or (n_windows and c.shape[0] != n_windows) or (n_coeffs is not None and c.shape[1] != n_coeffs):
        raise ValueError(f'coeffs must be ({rows}, {cols}): one row of model coefficients per staged window, got {np.shape(coeffs)}')
    t = np.asarray(tau)
    if t.dtype.kind not in 'fiu' or t.ndim > 1:
        raise ValueError(f'tau must be a finite number or (G,) of them, got {tau!r}')
    t = t.astype(np.float64)
    if not np.isfinite(t).all():
        raise ValueError(f'tau must be finite, got {tau!r}')
    if n_windows and n_windows % K == 0:
        G = n_windows // K
        if t.shape not in ((), (G,)):
            raise ValueError(f'tau must be a finite number or ({G},) of them, one per group, got shape {t.shape}')
        t = np.ascontiguousarray(np.broadcast_to(t, (G,)))
    return K, np.ascontiguousarray(c, dtype=np.float64), t, r, floor, want


def check_prior_images(prior_images, n_windows, sensor_size):
    """The caller's prior stack of Engine.event_responsibilities_spatial as contiguous float32 (B, H, W), every value finite and >= 0 as
    the float the kernel takes; (H, W) stands for it when B == 1.  None stays None (the staged prior).  Anything else is a ValueError,
    raised before any library call."""
    if prior_images is None:
        return None
    a = np.asarray(prior_images)
    if a.dtype.kind not in 'fiub':
        raise ValueError(f'prior_images must be numbers, got dtype {a.dtype}')
    shape = (int(n_windows), int(sensor_size[0]), int(sensor_size[1]))
    if a.ndim == 2 and shape[0] == 1:
        a = a[None]
    if a.shape != shape:
        raise ValueError(f'prior_images must be {shape}' + (f' or {shape[1:]}' if shape[0] == 1 else '') + f', got {np.shape(prior_images)}')
    with np.errstate(over='ignore'):
        a = np.ascontiguousarray(a, dtype=np.float32)
    bad = ~np.isfinite(a) | (a < 0)
    if bad.any():
        b, y, x = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f'prior_images must be finite and >= 0: window {b}, pixel (x {x}, y {y}) holds {float(a[b, y, x])!r}')
    return a


def check_score_images(images, n_windows, n_refs, sensor_size):
    """The caller's image stack of Engine.event_scores as contiguous float32 (B,R,H,W); (R,H,W) stands for it when B == 1.  None stays
    None (the IWEs of the last evaluation).  Anything else is a ValueError, raised before any library call."""
    if images is None:
        return None
    a = np.asarray(images)
    if a.dtype.kind not in 'fiub':
        raise ValueError(f'images must be numbers, got dtype {a.dtype}')
    shape = (int(n_windows), int(n_refs), int(sensor_size[0]), int(sensor_size[1]))
    if a.ndim == 3 and shape[0] == 1:
        a = a[None]
    if a.shape != shape:
        raise ValueError(f'images must be {shape}' + (f' or {shape[1:]}' if shape[0] == 1 else '') + f', got {np.shape(images)}')
    return np.ascontiguousarray(a, dtype=np.float32)


def check_ref_weights(ref_weights, n_refs):
    """The reference-time weights of Engine.event_scores as (R,) float64, finite; None stays None (the per-reference form)."""
    if ref_weights is None:
        return None
    w = np.asarray(ref_weights)
    if w.dtype.kind not in 'fiub' or w.shape != (int(n_refs),):
        raise ValueError(f'ref_weights must be ({int(n_refs)},) numbers, got {w.dtype} {w.shape}')
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.isfinite(w).all():
        raise ValueError('ref_weights must be finite')
    return w


def check_theta_advect_args(thetas, tau, gain, method, fill, min_coverage, sensor_size):
    """The arguments of Engine.advect_theta, checked without a GPU (csrc/eincm_theta_advect.h refuses the same).  thetas (n, h, w, 2)
    or (h, w, 2), no finer than the sensor; tau and gain scalars or (n,), finite; method a name of _lib.METHODS; fill 'source' or
    'zero'; min_coverage in (0, 1].  The value range of thetas is the library's check (it depends on the method's taps).  Returns
    (thetas float64, tau (n,), gain (n,), method code, fill code, min_coverage, single)."""
    if not isinstance(method, str) or method not in L.METHODS:
        raise ValueError(f'method {method!r} not supported; one of {sorted(L.METHODS)}')
    if not isinstance(fill, str) or fill not in L.TA_FILLS:
        raise ValueError(f'fill {fill!r} not supported; one of {sorted(L.TA_FILLS)}')
    t = np.asarray(thetas)
    if t.dtype.kind not in 'fiu':
        raise ValueError(f'thetas must be numeric, got {t.dtype}')
    single = t.ndim == 3
    t = t[None] if single else t
    if t.ndim != 4 or t.shape[3] != 2 or min(t.shape[:3]) < 1 or t.shape[0] > 65535:
        raise ValueError(f'thetas must be (n, h, w, 2) or (h, w, 2) with 1 <= n <= 65535, got {np.shape(thetas)}')
    if t.shape[1] > int(sensor_size[0]) or t.shape[2] > int(sensor_size[1]):
        raise ValueError(f'thetas {t.shape[1:3]} are finer than the sensor {tuple(int(v) for v in sensor_size)}')
    n = t.shape[0]

    def per_field(name, v):
        a = np.asarray(v)
        if a.dtype.kind not in 'fiu' or a.shape not in ((), (n,)):
            raise ValueError(f'{name} must be a number or ({n},) numbers, got {a.dtype} {a.shape}')
        a = np.ascontiguousarray(np.broadcast_to(a.astype(np.float64), (n,)))
        if not np.isfinite(a).all():
            raise ValueError(f'{name} must be finite')
        return a
    tau, gain = per_field('tau', tau), per_field('gain', gain)
    mc = _number('min_coverage', min_coverage)
    if not (0.0 < mc <= 1.0):
        raise ValueError(f'min_coverage must lie in (0, 1], got {min_coverage!r}')
    return np.ascontiguousarray(t, dtype=np.float64), tau, gain, L.METHODS[method], L.TA_FILLS[fill], mc, single


def event_weights_refusal(precision, splat_window, sharded=False):
    """Why a weighted batch cannot be staged on an engine of this precision and splat window (not built), or
    None.  csrc/eincm_api.hip (check_staging) refuses the same."""
    if precision == 'fp64':
        return 'per-event weights are not supported in fp64 mode'
    if int(splat_window) != 3:
        return f'per-event weights have the 3x3 splat window only, the engine has {int(splat_window)}'
    if sharded:
        return 'per-event weights are not supported by the event-sharded engine'
    return None


def keep_order_refusal(precision, splat_window, sharded=False):
    """Why a batch cannot be staged with keep_order=True on an engine of this precision and splat window (a
    keep-order batch is a weighted one whatever it is handed, so it is refused where weights are, in its own words), or None.
    csrc/eincm_api.hip (check_staging) refuses the same."""
    if precision == 'fp64':
        return 'keep_order is not supported in fp64 mode'
    if int(splat_window) != 3:
        return f'keep_order has the 3x3 splat window only, the engine has {int(splat_window)}'
    if sharded:
        return 'keep_order is not supported by the event-sharded engine (defer_constants)'
    return None


def check_weight_list(weights, n_events):
    """The argument of Engine.set_weights, checked without a GPU: a list of one entry per staged window, each None (ones) or the
    window's weights as check_event_weights takes them.  Returns the list of float32 arrays and Nones."""
    n = np.asarray(n_events, dtype=np.int64).reshape(-1)
    if weights is None or isinstance(weights, np.ndarray) or not hasattr(weights, '__len__') or len(weights) != n.size:
        raise ValueError(f'weights must be a list of {n.size} entries, one per staged window (an array, or None for ones)')
    return [None if w is None else check_event_weights(w, int(n[b])) for b, w in enumerate(weights)]


def motion_fused_refusal(precision, splat_window, params, weighted=False):
    """Why the fused path does not apply to this engine and these parameters (csrc/eincm_motion.h: motion_fused_supported, the part of
    it that Python can see before a GPU call), or None.  weighted: the staged batch carries per-event weights."""
    if weighted:
        return 'the fused motion path has no weighted form: the staged batch carries per-event weights'
    if precision == 'fp64':
        return 'the fused motion path is not supported in fp64 mode'
    if int(splat_window) != 3:
        return f'the fused motion path has the 3x3 splat window only, the engine has {int(splat_window)}'
    if params.flags & L.PF_FULL_AUX:
        return 'the fused motion path cannot serve full_aux: it needs the Theta image during the evaluation'
    if params.cur_pyr_lvl <= 0 and params.gamma != 0.0:
        return 'the fused motion path cannot serve the TV term (level 0, gamma != 0): it needs the Theta image during the evaluation'
    return None


def motion_auto_takes_fused(n_windows, n_events, n_refs):
    """The rule of the path 'auto' where the fused path applies (csrc/eincm_motion.h: motion_auto_takes_fused): the fused path was the faster
    one in every cell of profiles/motion_fused.md (8 windows of 1e6 events, one 480x640 window, 64 windows of 3e4 events), so it is
    taken wherever it applies."""
    return True


def make_params(alpha, beta, gamma, delta, cur_pyr_lvl, method='bilinear', contrast_kind=L.CONTRAST_GRAD_MAG,
                full_aux=False, correlation_kind='mse'):
    """eincm_params.  contrast_kind / correlation_kind: a name or an integer code; the correlation kind rides in
    flags bits 8-10.  The defaults are the reference's loss_func (grad_mag, mse)."""
    if isinstance(method, str):
        if method not in L.METHODS:
            raise ValueError(f'scale_to_sensor_size_method {method!r} not supported; one of {sorted(L.METHODS)}')
        method = L.METHODS[method]
    ck = contrast_kind_code(contrast_kind)
    rk = correlation_kind_code(correlation_kind)
    flags = (L.PF_FULL_AUX if full_aux else 0) | (rk << L.PF_CORRELATION_SHIFT)
    return L.Params(float(alpha), float(beta), float(gamma), float(delta), int(cur_pyr_lvl), int(method), ck, flags)


def check_precision(precision):
    """'fp32' or 'fp64'; anything else is a ValueError."""
    if precision not in L.PRECISIONS:
        raise ValueError(f"precision {precision!r}: 'fp32' or 'fp64'")
    return precision


class Engine:
    """One GPU context.  ``set_windows`` stages a batch of B independent windows (B = 1 for the reference's
    single-window solver, solver.py:185-194); ``loss_grad`` evaluates value_and_grad(loss_func) for all of them."""

    def __init__(self, sensor_size, max_events_total, max_refs=8, max_windows=1, device=0, timing=False, precision='fp32'):
        # precision: 'fp32' (default) or 'fp64' - the same objective with fp64 arithmetic after the warp (the
        # reference's jax_enable_x64: true).  Checked before the GPU is touched.
        self.precision = check_precision(precision)
        self._ctx = None
        self._lib = L.load()
        self.H, self.W = int(sensor_size[0]), int(sensor_size[1])
        self.max_windows = int(max_windows)
        self.max_refs = int(max_refs)
        # timing: False | True (every stage bracketed by marker events, ~20 % slower) | 'dominant' (the two event kernels
        # launched with their own start/stop events, read out on demand: see set_timed_kernels)
        flags = 0 if not timing else (L.CF_TIMING_DOMINANT if timing == 'dominant' else L.CF_TIMING)
        if self.precision == 'fp64':
            flags |= L.CF_FP64
        self._ctx = self._lib.eincm_create(int(device), self.H, self.W, int(max_refs), int(max_windows),
                                           int(max_events_total), flags)
        if not self._ctx:
            raise EincmError(L.ERR_HIP, self._lib.eincm_last_error(None).decode())
        self.B = 0
        self.R = 0
        self.timing = bool(timing)
        self.objective_tiles = L.DEFAULT_OBJECTIVE_TILE
        self.splat_window = L.DEFAULT_SPLAT_WINDOW
        self._io = {}                      # (h, w) -> staging buffers of loss_grad with their addresses
        self.flow_eval_windows = 0         # windows of the staged flow evaluation (flow_eval_stage)
        self.motion_model = None           # the motion.MotionModel of loss_grad_motion / motion_field (set_motion_model)
        self.motion_path = 'expanded'      # how loss_grad_motion evaluates (set_motion_path): 'expanded' | 'fused' | 'auto'
        self._weighted = False             # the staged batch carries per-event weights (set_windows; the property `weighted`)
        self._keep_order = False           # the staged batch kept its event order (set_windows(..., keep_order=True); the property `keep_order`)
        self._carried_windows = 0          # B of the batch the carried prior was formed on (carry_label_prior; 0: none)

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_ctx', None):
            self._lib.eincm_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, allow_nonfinite=False):
        if rc == L.OK:
            return
        msg = self._lib.eincm_last_error(self._ctx).decode()
        if rc == L.ERR_NONFINITE:
            if allow_nonfinite:
                return
            raise NonFiniteLoss(rc, msg)
        raise EincmError(rc, msg)

    def _theta_batch(self, theta, what='theta'):
        """theta (an ndarray or a torch tensor) as the batch (B,h,w,2); (h,w,2) stands for it when B == 1."""
        th = theta[None] if theta.ndim == 3 else theta
        if th.ndim != 4 or th.shape[0] != self.B or th.shape[3] != 2:
            raise ValueError(f'{what} must be ({self.B},h,w,2), got {tuple(theta.shape)}')
        return th

    def _active_ptr(self, active):
        """(mask array | None, its address | None) of an ``active`` argument; the array keeps the address alive."""
        if active is None:
            return None, None
        act = np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        if act.shape != (self.B,):
            raise ValueError(f'active must be ({self.B},), got {act.shape}')
        return act, act.ctypes.data

    def _outputs(self, shape, want_grad, want_aux):
        """Fresh (value (B,), grad of ``shape`` | None, aux block | None) for one evaluation call to fill."""
        return (np.empty(self.B, dtype=np.float64), np.empty(shape, dtype=np.float64) if want_grad else None,
                (L.Aux * self.B)() if want_aux else None)

    def _collect(self, rc, value, grad, aux, allow_nonfinite):
        """The tail of every evaluation call: the return code's verdict, the aux block as a list of dicts."""
        self._check(rc, allow_nonfinite)
        return value, grad, None if aux is None else [{k: getattr(a, k) for k, _ in L.Aux._fields_} for a in aux]

    # -- staging ----------------------------------------------------------------------------------
    def set_windows(self, windows, defer_constants=False, keep_order=False):
        """windows: list of (xs, ys, ts, edges, edge_ts) tuples (the reference's datasample tuple), or of 6-tuples whose last element
        is the window's per-event weights (check_event_weights) or None for ones - the two may be mixed.
        defer_constants: event-sharded mode (see sharding.ShardedEngine): stage only, finish with finish_constants().
        keep_order: staging keeps the index from its sorted copies of the events back to the order handed over (DESIGN.md section
        29), so the batch takes new weights in place: set_weights, apply_responsibilities.  Such a batch is a weighted one whatever
        it was handed (all-ones weights give the unweighted batch's bits)."""
        B = len(windows)
        keep_order = bool(keep_order)
        if keep_order:
            why = keep_order_refusal(self.precision, self.splat_window, sharded=defer_constants)
            if why is not None:
                raise ValueError(why)
        for b, w in enumerate(windows):
            if len(w) not in (5, 6):
                raise ValueError(f'window {b}: a (xs, ys, ts, edges, edge_ts) or (xs, ys, ts, edges, edge_ts, weights) tuple, got {len(w)} elements')
        ws = [None if len(w) == 5 or w[5] is None else check_event_weights(w[5], len(w[0])) for w in windows]
        weighted = any(w is not None and w.size > 0 for w in ws)      # (weights of a window without events change nothing)
        if weighted:
            why = event_weights_refusal(self.precision, self.splat_window, sharded=defer_constants)
            if why is not None:
                raise ValueError(why)
        R = len(np.atleast_1d(windows[0][4]))
        n = np.array([len(w[0]) for w in windows], dtype=np.int64)
        # every window's arrays go over as they are (one pointer per window): no host-side concatenation of the batch
        xs = [np.ascontiguousarray(as_int16_coords(w[0], 'xs')) for w in windows]
        ys = [np.ascontiguousarray(as_int16_coords(w[1], 'ys')) for w in windows]
        ts = [np.ascontiguousarray(np.asarray(w[2], dtype=np.float64)) for w in windows]
        edges = [np.ascontiguousarray(np.asarray(w[3], dtype=np.float64)) for w in windows]
        edge_ts = np.ascontiguousarray(np.stack([np.atleast_1d(np.asarray(w[4], dtype=np.float64)) for w in windows]))
        for b, e in enumerate(edges):
            if e.shape != (R, self.H, self.W):
                raise ValueError(f'edges must be (R,{self.H},{self.W}) per window, got {e.shape} for window {b}')
        if edge_ts.shape != (B, R):
            raise ValueError('every window needs the same number of reference times')
        for b in range(B):
            if not (len(xs[b]) == len(ys[b]) == len(ts[b])):
                raise ValueError(f'window {b}: xs, ys, ts differ in length')
        one = np.zeros(1, np.int16), np.zeros(1, np.float64)           # a valid address for empty windows
        def ptrs(arrs, dummy):
            return (C.c_void_p * B)(*[(a if a.size else dummy).ctypes.data for a in arrs])
        flags = (L.SW_DEFER_CONSTANTS if defer_constants else 0) | (L.SW_KEEP_ORDER if keep_order else 0)
        if weighted or keep_order:        # one float pointer per window, NULL where a window has none (or for all of them)
            wp = per_window_ptrs(ws)
            rc = self._lib.eincm_set_windows_weighted(self._ctx, B, R, n.ctypes.data_as(C.POINTER(C.c_int64)),
                                                      ptrs(xs, one[0]), ptrs(ys, one[0]), ptrs(ts, one[1]), ptrs(edges, one[1]),
                                                      _dp(edge_ts), wp, flags)
        else:
            rc = self._lib.eincm_set_windows_ptrs(self._ctx, B, R, n.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  ptrs(xs, one[0]), ptrs(ys, one[0]), ptrs(ts, one[1]), ptrs(edges, one[1]),
                                                  _dp(edge_ts), flags)
        self._weighted = False          # (a refused staging leaves nothing staged)
        self._keep_order = False
        self._staged_weights = None
        self._check(rc)
        if B != self.B:
            self._io = {}
        self.B, self.R = B, R
        self.n_events = n
        self._weighted = weighted or keep_order
        self._keep_order = keep_order
        self._staged_weights = ws       # what the windows were handed (None: ones), for event_scores(exclude_self=True)

    def set_window(self, xs, ys, ts, edges, edge_ts, weights=None, keep_order=False):
        self.set_windows([(xs, ys, ts, edges, edge_ts, weights)], keep_order=keep_order)

    @property
    def keep_order(self):
        """The staged batch kept its event order (set_windows(..., keep_order=True)): set_weights and apply_responsibilities serve it."""
        return getattr(self, '_keep_order', False)

    def _need_keep_order(self, who):
        if not self.keep_order:
            raise ValueError(f'{who} needs a batch staged with keep_order=True (set_windows): without it staging keeps no index back to '
                             'the order of its events')

    def set_weights(self, weights):
        """New per-event weights for the staged events, in place: a list of B entries, each None (ones) or the
        window's weights as check_event_weights takes them.  The batch must have been staged with keep_order=True.  Everything is
        checked before anything is touched: a refused call leaves the staged batch and its last evaluation as they were.  Afterwards
        the engine answers as after a fresh set_windows of the same windows with these weights and keep_order=True, byte for byte; the
        last evaluation is gone, as after a staging."""
        ws = check_weight_list(weights, self.n_events if self.B else [])
        self._need_keep_order('set_weights')
        self._check(self._lib.eincm_set_weights(self._ctx, per_window_ptrs(ws)))
        self._staged_weights = ws

    def staged_weights(self):
        """The staged weights of a keep-order batch, downloaded: a list of B float32 (n_b,) arrays in the order the events were handed
        over, ones where a window was handed none - what the last set_windows, set_weights or apply_responsibilities left."""
        self._need_keep_order('staged_weights')
        w = np.empty(int(self.n_events.sum()), dtype=np.float32)
        self._check(self._lib.eincm_get_staged_weights(self._ctx, w.ctypes.data))
        off = np.concatenate([[0], np.cumsum(self.n_events)]).astype(np.int64)
        return [w[off[b]:off[b + 1]] for b in range(self.B)]

    def staged_order(self):
        """(order_splat, order_gather) of a keep-order batch, (N,) uint32 each: for every slot of the splat's and of the gather's copy of
        the events, the position of its event in the batch as handed over, window after window.  For tests and tools."""
        self._need_keep_order('staged_order')
        n = int(self.n_events.sum())
        a, b = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        self._check(self._lib.eincm_get_stage_order(self._ctx, a.ctypes.data, b.ctypes.data))
        return a, b

    def _self_weights(self):
        """The weights exclude_self subtracts the events' own shares with: a keep-order batch's come from the device (they may have
        been set there), any other's are what set_windows was handed."""
        if self.keep_order:
            return self.staged_weights()
        ws = getattr(self, '_staged_weights', None)
        if ws is None or len(ws) != self.B:
            raise ValueError('exclude_self needs the weights the batch was staged with, and this engine does not hold them: stage with set_windows')
        return ws

    @property
    def weighted(self):
        """The staged batch carries per-event weights (some window was handed weights; all-ones weights count)."""
        return getattr(self, '_weighted', False)

    # -- evaluation -------------------------------------------------------------------------------
    def loss_grad(self, theta, params, want_grad=True, want_aux=False, allow_nonfinite=True, active=None):
        """theta: (B,h,w,2) or (h,w,2) when B == 1.  Returns (value (B,), grad (B,h,w,2) | None, aux list | None).
        active: optional (B,) mask - only those windows are evaluated (the others: value NaN, gradient 0), at about their share of the cost."""
        th = self._theta_batch(theta if isinstance(theta, np.ndarray) else np.asarray(theta, dtype=np.float64))
        _, h, w, _ = th.shape
        # Staging buffers per theta shape with their addresses cached: `ndarray.ctypes.data` costs ~1 us per use, three of them per
        # call were 3 of the ~5 us this wrapper added to a 70 us evaluation.  The caller gets copies (a few hundred bytes at the
        # pyramid's sizes); a dense theta goes straight through.
        small = th.size <= 8192
        if small:
            bufs = self._io.get((h, w))
            if bufs is None:
                tb, vb, gb = np.empty((self.B, h, w, 2)), np.empty(self.B), np.empty((self.B, h, w, 2))
                bufs = self._io[(h, w)] = (tb, vb, gb, tb.ctypes.data, vb.ctypes.data, gb.ctypes.data)
            tb, vb, gb, p_th, p_v, p_g = bufs
            np.copyto(tb, th)
            aux = (L.Aux * self.B)() if want_aux else None
        else:
            th = np.ascontiguousarray(th, dtype=np.float64)
            vb, gb, aux = self._outputs(th.shape, want_grad, want_aux)
            p_th, p_v, p_g = th.ctypes.data, vb.ctypes.data, (gb.ctypes.data if want_grad else None)
        if active is not None:
            act, p_act = self._active_ptr(active)
            rc = self._lib.eincm_loss_grad_masked(self._ctx, p_th, h, w, C.byref(params), p_act, p_v, p_g if want_grad else None, aux)
        else:
            rc = self._lib.eincm_loss_grad(self._ctx, p_th, h, w, C.byref(params), p_v, p_g if want_grad else None, aux)
        if not small:
            return self._collect(rc, vb, gb, aux, allow_nonfinite)
        self._check(rc, allow_nonfinite)
        return vb.copy(), gb.copy() if want_grad else None, [{k: getattr(a, k) for k, _ in L.Aux._fields_} for a in aux] if want_aux else None

    # -- asynchronous evaluation: enqueue now, collect later (several contexts in flight, see EngineGroup) ----
    def loss_grad_async(self, theta, params, want_grad=True, active=None):
        """Enqueue an evaluation and return at once (theta is copied before the call returns); ``active`` as in loss_grad."""
        th = self._theta_batch(np.ascontiguousarray(np.asarray(theta, dtype=np.float64)))
        act, p_act = self._active_ptr(active)
        # (a refused launch - one already in flight - leaves self._async naming that one, so that it can still be collected)
        self._check(self._lib.eincm_loss_grad_masked_async(self._ctx, th.ctypes.data, th.shape[1], th.shape[2], C.byref(params),
                                                           p_act, 1 if want_grad else 0))
        self._async = (th.shape, bool(want_grad))

    def loss_grad_wait(self, want_aux=False, allow_nonfinite=True):
        if getattr(self, '_async', None) is None:
            raise EincmError(L.ERR_STATE, 'eincm_loss_grad_wait without eincm_loss_grad_async')
        shape, want_grad = self._async
        self._async = None
        value, grad, aux = self._outputs(shape, want_grad, want_aux)
        rc = self._lib.eincm_loss_grad_wait(self._ctx, value.ctypes.data, grad.ctypes.data if want_grad else None, aux)
        return self._collect(rc, value, grad, aux, allow_nonfinite)

    # -- the two halves of an evaluation (event-sharded mode) ------------------------------------------
    def forward_iwe(self, theta, params, want_grad=True):
        """k_theta + k_splat only; returns with the IWE stack complete in HBM.  theta=None: the theta = 0 constants pass."""
        if theta is None:
            rc = self._lib.eincm_forward_iwe(self._ctx, None, 1, 1, C.byref(make_params(1, 1, 0, 0, 1)), 0)
            self._check(rc)
            return None
        th = self._theta_batch(np.ascontiguousarray(np.asarray(theta, dtype=np.float64)))
        self._check(self._lib.eincm_forward_iwe(self._ctx, _dp(th), th.shape[1], th.shape[2], C.byref(params), 1 if want_grad else 0))
        return th.shape

    def finish_loss_grad(self, theta_shape, want_grad=True, want_aux=False, allow_nonfinite=True):
        value, grad, aux = self._outputs(theta_shape, want_grad, want_aux)
        rc = self._lib.eincm_finish_loss_grad(self._ctx, _dp(value), _dp(grad) if want_grad else None, aux)
        return self._collect(rc, value, grad, aux, allow_nonfinite)

    # -- the finishing half with the results kept in HBM (event-sharded mode over a GPU collective) ------------------
    def set_device_results(self, on=True):
        self._check(self._lib.eincm_set_device_results(self._ctx, 1 if on else 0))

    def finish_launch(self):
        self._check(self._lib.eincm_finish_launch(self._ctx))

    def grad_tensor(self, theta_shape):
        """torch view of the gradient of the launched evaluation in HBM, shaped like theta: all-reduce it in place."""
        return self._device_view(self._lib.eincm_grad_device_ptr, '<f8', 8, tuple(theta_shape))

    def finish_collect(self, theta_shape, want_grad=True, want_aux=False, allow_nonfinite=True):
        value, grad, aux = self._outputs(theta_shape, want_grad, want_aux)
        rc = self._lib.eincm_finish_collect(self._ctx, _dp(value), _dp(grad) if want_grad else None, aux)
        return self._collect(rc, value, grad, aux, allow_nonfinite)

    # -- theta and gradient resident in HBM (an optimiser that lives on the GPU) -------------------------------------------
    def loss_grad_device(self, theta, params, theta_abs_max=None, want_grad=True, want_aux=False, allow_nonfinite=True):
        """theta: torch float64 CUDA tensor (B,h,w,2) (or (h,w,2) when B == 1) on the engine's device.  Returns (value ndarray (B,),
        grad torch tensor like theta | None, aux list | None); nothing but the scalars crosses PCIe.  theta_abs_max: an upper bound of
        |theta| if the caller has one on the host (it only selects LDS window capacities; None = unknown)."""
        import torch
        if not (isinstance(theta, torch.Tensor) and theta.is_cuda and theta.dtype == torch.float64):
            raise TypeError('theta must be a float64 CUDA tensor')
        th = self._theta_batch(theta.contiguous())
        grad = torch.empty_like(th) if want_grad else None
        torch.cuda.current_stream(th.device).synchronize()              # the engine's kernels run on its own stream
        value, _, aux = self._outputs(None, False, want_aux)
        rc = self._lib.eincm_loss_grad_device(self._ctx, C.c_void_p(th.data_ptr()), int(th.shape[1]), int(th.shape[2]), C.byref(params),
                                              -1.0 if theta_abs_max is None else float(theta_abs_max), _dp(value),
                                              C.c_void_p(grad.data_ptr()) if want_grad else None, aux)
        return self._collect(rc, value, grad[0] if want_grad and theta.dim() == 3 else grad, aux, allow_nonfinite)

    # -- parametric motion-field models: the unknowns are K coefficients per window --------------------------
    def set_motion_model(self, model):
        """model: a motion.MotionModel built for this sensor size, or None to clear it."""
        model = check_motion_model(model, (self.H, self.W))
        self._check(self._lib.eincm_set_motion_model(self._ctx, None if model is None else C.byref(model.as_struct())))
        self.motion_model = model

    def set_motion_path(self, path):
        """How loss_grad_motion (and with it minimize_motion) evaluates from here on: 'expanded' (the default: the field as an image,
        the dense gradient reduced to the moments), 'fused' (the polynomial inside the event kernels, DESIGN.md section 21: the same
        value bit for bit, the gradient the same sum in another order; a ValueError from loss_grad_motion where it does not apply) or
        'auto' (fused where it applies and profiles/motion_fused.md found it the faster one, else expanded).  A setting of the engine,
        not a keyword of loss_grad_motion: the signatures of section 20's callables stay as they are."""
        self.motion_path = check_motion_path(path)

    def loss_grad_motion(self, coeffs, params, want_grad=True, want_aux=False, allow_nonfinite=True, active=None):
        """coeffs: (B,K), or (K,) when B == 1.  Returns (value (B,), grad (B,K) | None, aux list | None): the loss of the field
        model.field(coeffs) and its gradient with respect to the coefficients, the TV term's share included.  ``active`` as in loss_grad.
        The evaluation path is the engine's ``motion_path`` (set_motion_path; 'expanded' unless set)."""
        path = check_motion_path(self.motion_path)
        c = check_motion_coeffs(coeffs, self.B, self.motion_model)
        fused = False
        if path != 'expanded':
            why = motion_fused_refusal(self.precision, self.splat_window, params, self.weighted)
            if why is not None and path == 'fused':
                raise ValueError(why)
            fused = why is None and (path == 'fused' or motion_auto_takes_fused(self.B, int(np.sum(self.n_events)), self.R))
        call = self._lib.eincm_loss_grad_motion_fused if fused else self._lib.eincm_loss_grad_motion
        act, p_act = self._active_ptr(active)
        value, grad, aux = self._outputs(c.shape, want_grad, want_aux)
        rc = call(self._ctx, c.ctypes.data, C.byref(params), p_act, value.ctypes.data, grad.ctypes.data if want_grad else None, aux)
        return self._collect(rc, value, grad, aux, allow_nonfinite)

    def motion_field(self, coeffs):
        """Theta (B,H,W,2) of coeffs (B,K), expanded on the GPU: array_equal to model.field(coeffs)."""
        c = check_motion_coeffs(coeffs, self.B, self.motion_model)
        out = np.empty((self.B, self.H, self.W, 2), dtype=np.float64)
        self._check(self._lib.eincm_motion_field(self._ctx, c.ctypes.data, out.ctypes.data))
        return out

    # -- BFGS with its state in HBM: the host sees scalars, the vectors and the inverse Hessian stay on the GPU ----
    def _bfgs_alpha(self, alpha):
        al = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64))
        if al.shape != (self.B,):
            raise ValueError(f'alpha must be ({self.B},), got {al.shape}')
        return al

    def bfgs_begin(self, x0, active=None):
        """Start B minimisations at x0 (B,h,w,2): X = x0, H = I, for the windows of ``active`` (None = all)."""
        x = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
        if x.ndim != 4 or x.shape[0] != self.B or x.shape[3] != 2:
            raise ValueError(f'x0 must be ({self.B},h,w,2), got {x.shape}')
        act, p_act = self._active_ptr(active)
        self._check(self._lib.eincm_bfgs_begin(self._ctx, x.ctypes.data, x.shape[1], x.shape[2], p_act))
        self._bfgs_shape = x.shape
        out = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        self._bfgs_out = out + tuple(o.ctypes.data for o in out)

    def lbfgs_begin(self, x0, active=None, history=10, initial_scale='last_pair'):
        """``bfgs_begin`` with the inverse Hessian kept as a ring of ``history`` pairs (s, y) per window: any theta
        shape, the dense one included.  The other ``bfgs_*`` calls then operate on that form (no inverse Hessian to fetch)."""
        history, scale = check_history(history), L.LBFGS_SCALES[check_initial_scale(initial_scale)]
        x = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
        if x.ndim != 4 or x.shape[0] != self.B or x.shape[3] != 2:
            raise ValueError(f'x0 must be ({self.B},h,w,2), got {x.shape}')
        act, p_act = self._active_ptr(active)
        self._check(self._lib.eincm_lbfgs_begin(self._ctx, x.ctypes.data, x.shape[1], x.shape[2], p_act, history, scale))
        self._bfgs_shape = x.shape
        out = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        self._bfgs_out = out + tuple(o.ctypes.data for o in out)

    def lbfgs_history_tensors(self):
        """torch views of the limited form's history in HBM: the rings S, Y (B, m, n) by ring slot, D (B, 2m+1, 2m+1) and delta (B, 2m+1)
        (s of slot k at k, y of slot k at m + k, g at 2m), the int32 ring head and count (B,), and m."""
        ptr = [C.c_void_p() for _ in range(6)]
        m = C.c_int()
        self._check(self._lib.eincm_lbfgs_history_ptrs(self._ctx, *(C.byref(q) for q in ptr), C.byref(m)))
        B, n, m = self.B, int(np.prod(self._bfgs_shape[1:])), int(m.value)
        shapes = ((B, m, n), (B, m, n), (B, 2 * m + 1, 2 * m + 1), (B, 2 * m + 1), (B,), (B,))
        return tuple(self._view_at(q.value, '<f8' if i < 4 else '<i4', sh) for i, (q, sh) in enumerate(zip(ptr, shapes))) + (m,)

    def bfgs_eval(self, params, alpha, active=None, allow_nonfinite=True):
        """One evaluation at X + alpha[b] P per window of ``active``: (value, phi' = grad . P, max|grad|), each (B,); the trial point
        and its gradient stay in HBM.  Entries of the other windows are meaningless."""
        al = self._bfgs_alpha(alpha)
        act, p_act = self._active_ptr(active)
        v, d, g, p_v, p_d, p_g = self._bfgs_out
        rc = self._lib.eincm_bfgs_eval(self._ctx, C.byref(params), al.ctypes.data, p_act, p_v, p_d, p_g)
        self._check(rc, allow_nonfinite)
        return v.copy(), d.copy(), g.copy()

    def bfgs_trial(self, alpha, active=None):
        """Xt = X + alpha[b] P alone (see bfgs_trial_tensors)."""
        al = self._bfgs_alpha(alpha)
        act, p_act = self._active_ptr(active)
        self._check(self._lib.eincm_bfgs_trial(self._ctx, al.ctypes.data, p_act))

    def bfgs_reduce(self, active=None):
        """(phi', max|grad|) of the gradient the caller wrote into the trial gradient's view (torch work on it is synchronised first)."""
        import torch
        torch.cuda.current_stream(torch.device('cuda', torch.cuda.current_device())).synchronize()
        act, p_act = self._active_ptr(active)
        _, d, g, _, p_d, p_g = self._bfgs_out
        self._check(self._lib.eincm_bfgs_reduce(self._ctx, p_act, p_d, p_g))
        return d.copy(), g.copy()

    def bfgs_trial_tensors(self):
        """torch views (B, n) of the trial point Xt and its gradient Gt in HBM: any objective's gradient can be supplied on the device
        between bfgs_trial and bfgs_reduce."""
        xt, gt, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._lib.eincm_bfgs_trial_ptrs(self._ctx, C.byref(xt), C.byref(gt), C.byref(n)))
        shape = (self.B, int(n.value) // self.B)
        return self._view_at(xt.value, '<f8', shape), self._view_at(gt.value, '<f8', shape)

    def bfgs_state_tensors(self):
        """torch views of X, G, P (B, n) and the inverse Hessian H (B, n, n) in HBM (None in the limited form, which keeps none)."""
        x, g, p, h, nb, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
        self._check(self._lib.eincm_bfgs_state_ptrs(self._ctx, C.byref(x), C.byref(g), C.byref(p), C.byref(h), C.byref(nb), C.byref(n)))
        B, n = int(nb.value), int(n.value)
        return (self._view_at(x.value, '<f8', (B, n)), self._view_at(g.value, '<f8', (B, n)), self._view_at(p.value, '<f8', (B, n)),
                self._view_at(h.value, '<f8', (B, n, n)) if h.value else None)

    def bfgs_accept(self, alpha, modes):
        """End of a line search per window: modes[b] in _lib.BFGS_SKIP / UPDATE / MOVE / INIT with the step alpha[b] last evaluated.
        Returns the scalars (B, _lib.BFGS_NS) of the new iterates (rows of skipped windows: their last values)."""
        al = self._bfgs_alpha(alpha)
        md = np.ascontiguousarray(np.asarray(modes).astype(np.uint8))
        if md.shape != (self.B,):
            raise ValueError(f'modes must be ({self.B},), got {md.shape}')
        out = np.empty((self.B, L.BFGS_NS))
        self._check(self._lib.eincm_bfgs_accept(self._ctx, al.ctypes.data, md.ctypes.data, out.ctypes.data))
        return out

    def bfgs_fetch(self, want_hess_inv=False):
        """(x (B,h,w,2), grad (B,h,w,2), inverse Hessian (B,n,n) | None) on the host."""
        shape = self._bfgs_shape
        n = int(np.prod(shape[1:]))
        x, g = np.empty(shape), np.empty(shape)
        H = np.empty((self.B, n, n)) if want_hess_inv else None
        self._check(self._lib.eincm_bfgs_fetch(self._ctx, x.ctypes.data, g.ctypes.data, H.ctypes.data if want_hess_inv else None))
        return x, g, H

    def finish_constants(self):
        self._check(self._lib.eincm_finish_constants(self._ctx))

    def _device_view(self, getter, typestr, itemsize, shape):
        ptr, n = C.c_void_p(), C.c_int64()
        self._check(getter(self._ctx, C.byref(ptr), C.byref(n)))
        return self._view_at(ptr.value, typestr, shape)

    @staticmethod
    def _view_at(address, typestr, shape):
        import torch

        class _View:            # the CUDA array interface: a zero-copy torch tensor over the engine's HBM buffer
            __cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'data': (int(address), False), 'version': 2,
                                        'strides': None}
        return torch.as_tensor(_View(), device=torch.device('cuda', torch.cuda.current_device()))

    def iwe_tensor(self):
        """torch view of the IWE accumulator (B,R,H,W) in HBM, for an RCCL all-reduce(sum) between the two halves.  The engine sums
        pixel * 2^30 as 64-bit integers (exact, order-independent); the view is int64 (values stay below 2^63)."""
        return self._device_view(self._lib.eincm_iwe_device_ptr, '<i8', 8, (self.B, self.R, self.H, self.W))

    def mask_tensor(self):
        """torch view of the event-presence mask (B,H,W) uint8."""
        return self._device_view(self._lib.eincm_mask_device_ptr, '|u1', 1, (self.B, self.H, self.W))

    def handover_loss_grad(self, alpha_handover, prev_theta, theta, params, want_grad=True, allow_nonfinite=True):
        pt = np.ascontiguousarray(np.asarray(prev_theta, dtype=np.float64))
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
        if th.ndim == 3:
            th, pt = th[None], pt[None]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha_handover, dtype=np.float64), (self.B,)))
        _, h, w, _ = th.shape
        value = np.empty(self.B)
        dv = np.empty(self.B) if want_grad else None
        rc = self._lib.eincm_handover_loss_grad(self._ctx, _dp(a), _dp(pt), _dp(th), h, w, C.byref(params), _dp(value),
                                                _dp(dv) if want_grad else None)
        self._check(rc, allow_nonfinite)
        return value, dv

    def objectives(self, Theta):
        """compute_loss_objectives (losses.py:49-105) on full-resolution Theta (B,H,W,2); list of dicts."""
        T = np.ascontiguousarray(np.asarray(Theta, dtype=np.float64))
        if T.ndim == 3:
            T = T[None]
        if T.shape != (self.B, self.H, self.W, 2):
            raise ValueError(f'Theta must be ({self.B},{self.H},{self.W},2), got {T.shape}')
        out = (L.ObjectivesOut * self.B)()
        rc = self._lib.eincm_objectives(self._ctx, _dp(T), out)
        self._check(rc, True)
        res = []
        for o in out:
            d = {}
            for k, t in L.ObjectivesOut._fields_:
                if k in ('n_refs', '_pad'):
                    continue
                v = getattr(o, k)
                d[k] = np.array(v[:o.n_refs]) if t is L._A else float(v)
            res.append(d)
        return res

    def set_objective_tiles(self, tile_size):
        """Tile size (tile_h, tile_w) of the adaptive objective kinds of loss_grad (default 32 x 42, contrast_objectives.py:56-59)."""
        th, tw = check_tile_size(tile_size, (self.H, self.W))
        self._check(self._lib.eincm_set_objective_tiles(self._ctx, th, tw))
        self.objective_tiles = (th, tw)

    def set_splat_window(self, window_size):
        """Splat window size of every IWE of this context (events_to_pdf_frame's window_size, default 3).  On a
        staged batch the window constants are formed again.  fp64 engines accept 3 only, and so does a staged weighted batch."""
        s = check_window_size(window_size)
        if self.weighted and s != 3:
            raise ValueError(event_weights_refusal(self.precision, s))
        self._check(self._lib.eincm_set_splat_window(self._ctx, s))
        self.splat_window = s

    def tiled_objectives(self, tile_size=None):
        """extract_tiles + compute_adaptive_* and their pairwise siblings (contrast_objectives.py:42-87,
        correlation_objectives.py:28-130) on the images of the last evaluation; list of dicts of (R,) arrays."""
        th, tw = (32, 42) if tile_size is None else tile_size        # contrast_objectives.py:56-59
        out = (L.TiledOut * self.B)()
        self._check(self._lib.eincm_tiled_objectives(self._ctx, int(th), int(tw), out))
        res = []
        for o in out:
            d = {'n_tiles': int(o.n_tiles)}
            for k, t in L.TiledOut._fields_:
                if t is L._A:
                    d[k] = np.array(getattr(o, k)[:o.n_refs])
            res.append(d)
        return res

    # -- the step before the path: edge smoothing (SURVEY f-4) --------------------------------------
    def inv_dist_transform(self, edge_imgs, formulation='exponential', alpha=6.0, d_sat=6.0, return_sqdist=False):
        """1 - minmax(f(d)) of the exact Euclidean distance to the nearest edge pixel (img_utils.py:229-233, :236-410).
        edge_imgs: (n,H,W) or (H,W), non-zero = edge.  Returns float64 (and the int32 squared distances if asked)."""
        e = np.asarray(edge_imgs)
        single = e.ndim == 2
        e = np.ascontiguousarray((e[None] if single else e) != 0).astype(np.uint8)
        if e.shape[1:] != (self.H, self.W):
            raise ValueError(f'edge images must be ({self.H},{self.W}), got {e.shape[1:]}')
        if formulation not in L.EDT_FORMULATIONS:
            raise NotImplementedError(f'Invalid option: formulation={formulation!r}')      # img_utils.py:383-385
        out = np.empty(e.shape, dtype=np.float64)
        sq = np.empty(e.shape, dtype=np.int32) if return_sqdist else None
        self._check(self._lib.eincm_inv_dist_transform(
            self._ctx, e.ctypes.data_as(C.POINTER(C.c_uint8)), e.shape[0], L.EDT_FORMULATIONS[formulation], float(alpha),
            float(d_sat), _dp(out), sq.ctypes.data_as(C.POINTER(C.c_int32)) if return_sqdist else None))
        if single:
            out, sq = out[0], (sq[0] if return_sqdist else None)
        return (out, sq) if return_sqdist else out

    def gaussian_blur(self, imgs, sigma):
        """cv.GaussianBlur(float64 image, ksize from sigma, BORDER_REFLECT_101) (img_utils.py:210-220)."""
        a = np.asarray(imgs, dtype=np.float64)
        single = a.ndim == 2
        a = np.ascontiguousarray(a[None] if single else a)
        if a.shape[1:] != (self.H, self.W):
            raise ValueError(f'images must be ({self.H},{self.W}), got {a.shape[1:]}')
        out = np.empty_like(a)
        self._check(self._lib.eincm_gaussian_blur(self._ctx, _dp(a), a.shape[0], float(sigma), _dp(out)))
        return out[0] if single else out

    def canny(self, imgs, threshold1, threshold2, aperture_size=3, l2_gradient=True):
        """cv.Canny(img, threshold1, threshold2, None, aperture_size, l2_gradient) (img_utils.py:192-208).
        imgs: (n,H,W) or (H,W) uint8.  Returns the same shape, uint8 0 / 255."""
        th1, th2, ap = check_canny_args(threshold1, threshold2, aperture_size)
        a = np.asarray(imgs)
        if a.dtype != np.uint8:
            raise ValueError(f'Canny input must be uint8, got {a.dtype}')
        single = a.ndim == 2
        a = np.ascontiguousarray(a[None] if single else a)
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f'images must be ({self.H},{self.W}), got {a.shape[1:]}')
        out = np.empty_like(a)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.eincm_canny(self._ctx, a.ctypes.data_as(u8), a.shape[0], th1, th2, ap, 1 if l2_gradient else 0,
                                          out.ctypes.data_as(u8)))
        return out[0] if single else out

    def preprocess_image(self, imgs, stages='all', **params):
        """preprocess_image (img_utils.py:131-189): NL-means, CLAHE, unsharp mask, bilateral filter, the stages selected in that
        order.  imgs: (n,H,W) or (H,W) uint8.  Keywords: PREPROCESS_DEFAULTS.  Returns the same shape."""
        p = make_preprocess_params((self.H, self.W), stages, **params)
        a = np.asarray(imgs)
        if a.dtype != np.uint8:
            raise ValueError(f'preprocessing input must be uint8, got {a.dtype}')
        single = a.ndim == 2
        a = np.ascontiguousarray(a[None] if single else a)
        if a.ndim != 3 or a.shape[1:] != (self.H, self.W):
            raise ValueError(f'images must be ({self.H},{self.W}), got {a.shape[1:]}')
        out = np.empty_like(a)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.eincm_preprocess_image(self._ctx, a.ctypes.data_as(u8), a.shape[0], C.byref(p), out.ctypes.data_as(u8)))
        return out[0] if single else out

    def gt_flow(self, gt_x, gt_y, plans):
        """MVSEC's estimate_gt_flow (mvsec_loader.py:322-433) for a batch of windows.  gt_x, gt_y: (n_frames,H,W)
        float32 or float64 stacks; plans: a list of GtFlowPlan (evaluation.gt_flow_plan), or one.  Only the frames the plans read go
        to the GPU.  Returns (B,H,W,2) float64, or (H,W,2) for one plan."""
        single = isinstance(plans, GtFlowPlan)
        plans = [plans] if single else list(plans)
        gx, gy = gt_flow_stacks(gt_x, gt_y, (self.H, self.W))
        f0, f1 = check_gt_flow_plans(plans, gx.shape[0])
        gx, gy = np.ascontiguousarray(gx[f0:f1 + 1]), np.ascontiguousarray(gy[f0:f1 + 1])
        mode = np.array([L.GTF_MODES[m] for m, _ in plans], dtype=np.int32)
        off = np.zeros(len(plans) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(st) for _, st in plans])
        steps = [s for _, st in plans for s in st]
        frame = np.array([int(f) - f0 for f, _, _ in steps], dtype=np.int32)
        num = np.array([n for _, n, _ in steps], dtype=np.float64)
        den = np.array([d for _, _, d in steps], dtype=np.float64)
        out = np.empty((len(plans), self.H, self.W, 2), dtype=np.float64)
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.eincm_gt_flow(self._ctx, gx.ctypes.data, gy.ctypes.data, gx.itemsize, gx.shape[0], len(plans),
                                            mode.ctypes.data_as(i32), off.ctypes.data_as(i32), frame.ctypes.data_as(i32), _dp(num),
                                            _dp(den), _dp(out)))
        return out[0] if single else out

    # -- the DSEC data path --------------------------------------------------
    def _check_data(self, rc):
        """A refusal of the data itself (EINCM_ERR_ARG after the Python side has checked every shape) is a ValueError."""
        if rc == L.ERR_ARG:
            raise ValueError(self._lib.eincm_last_error(self._ctx).decode())
        self._check(rc)

    def rectify_events(self, x, y, rectify_map, chunk=1 << 22):
        """DSECDataLoader.rectify_events (dsec_loader.py:145-171): (rx, ry) = rectify_map[y, x], rounded half to even to int16; events
        that leave the sensor are dropped, the others keep their order.  x, y: integer arrays of a whole recording; rectify_map
        (H, W, 2) float32.  The stream is walked in chunks of ``chunk`` events; the result does not depend on it.  Returns
        (rec_x, rec_y, keep, n_kept): int16 arrays of the kept events, the bool mask over the input, the kept count.  ValueError: a map
        entry that is not finite or does not round into int16, an input coordinate outside the sensor."""
        m = check_rectify_map(rectify_map, (self.H, self.W))
        xs, ys = check_event_coords(x, y)
        chunk = check_chunk(chunk)
        n = xs.shape[0]
        rec_x, rec_y = np.empty(n, dtype=np.int16), np.empty(n, dtype=np.int16)
        keep = np.empty(n, dtype=np.uint8)
        kept, k = 0, C.c_int64(0)
        for i0, i1 in chunk_walk(n, chunk):
            self._check_data(self._lib.eincm_rectify_events(
                self._ctx, m.ctypes.data if i0 == 0 else None, xs.ctypes.data + 2 * i0, ys.ctypes.data + 2 * i0, i1 - i0,
                rec_x.ctypes.data + 2 * kept, rec_y.ctypes.data + 2 * kept, keep.ctypes.data + i0, C.byref(k)))
            kept += int(k.value)
        return rec_x[:kept], rec_y[:kept], keep.view(np.bool_), kept

    def event_support(self, xs, ys, ts, tau, radius=1, full_support=1, pixel_mask=None, chunk=1 << 22, return_support=False):
        """The spatiotemporal support filter (background-activity filter) of a raw stream: per event, the
        number of neighbouring pixels (Chebyshev distance <= radius, inside the sensor, not masked, never the event's own pixel)
        whose most recent earlier event lies at most ``tau`` back, and the weight min(support, full_support) / full_support as
        float32: what ``set_windows``, ``stage_datasample(event_weights=)`` and the ``losses`` callables take.  xs, ys: integer
        arrays in stream order; ts: finite, non-decreasing, floating or integer (integers of magnitude <= 2^53), ``tau`` in their
        unit.  pixel_mask (H, W), non-zero = masked: events there get weight 0 and support nobody.  The stream is walked in chunks
        of ``chunk`` events; the result does not depend on it.  Returns the weights (n,), and the uint8 support too when asked.
        ValueError, before the library is reached: every refusal of the C contract, with the index of the first offending event."""
        tau, radius, full_support = check_event_support_args(tau, radius, full_support)
        x, y, t, mask, chunk = check_raw_stream(xs, ys, ts, pixel_mask, chunk, (self.H, self.W))
        n = x.shape[0]
        weights, support = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint8)
        for i0, i1 in chunk_walk(n, chunk):
            self._check_data(self._lib.eincm_event_support(
                self._ctx, x.ctypes.data + 2 * i0, y.ctypes.data + 2 * i0, t.ctypes.data + 8 * i0, i1 - i0, tau, radius, full_support,
                None if mask is None else mask.ctypes.data, int(i0 == 0), weights.ctypes.data + 4 * i0, support.ctypes.data + i0))
        return (weights, support) if return_support else weights

    def event_filter(self, xs, ys, ts, ps=None, refractory=0.0, tau=0.0, radius=1, full_support=1, polarity=False, pixel_mask=None,
                     chunk=1 << 22, return_support=False):
        """The refractory and polarity-aware filter of a raw stream, beside ``event_support``.  An event is
        dropped when it follows its own pixel's previous event, kept or not, by less than ``refractory`` (or lies on a masked
        pixel); a kept event's support counts the neighbours whose last KEPT event lies at most ``tau`` back, of the event's own
        polarity class with ``polarity=True``.  ps: boolean or integer array (class 1 where > 0), needed only with
        ``polarity=True``.  ``radius=0`` switches the support stage off: the weights are then 1 for kept events.  Everything else
        (stream order, times, mask, chunking, refusals) is ``event_support``'s.  Returns (keep bool (n,), weights float32 (n,)), and
        the uint8 support too when asked; the staged lists are not shortened, callers index with ``keep``."""
        refractory, tau, radius, full_support, flags = check_event_filter_args(refractory, tau, radius, full_support, polarity)
        x, y, t, mask, chunk = check_raw_stream(xs, ys, ts, pixel_mask, chunk, (self.H, self.W))
        n = x.shape[0]
        p = check_event_polarity(ps, n, polarity)
        keep, weights, support = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint8)
        for i0, i1 in chunk_walk(n, chunk):
            self._check_data(self._lib.eincm_event_filter(
                self._ctx, x.ctypes.data + 2 * i0, y.ctypes.data + 2 * i0, t.ctypes.data + 8 * i0, None if p is None else p.ctypes.data + i0,
                i1 - i0, refractory, tau, radius, full_support, flags, None if mask is None else mask.ctypes.data, int(i0 == 0),
                keep.ctypes.data + i0, weights.ctypes.data + 4 * i0, support.ctypes.data + i0))
        keep = keep.view(np.bool_)
        return (keep, weights, support) if return_support else (keep, weights)

    def remap_cubic(self, src, mapping):
        """cv.remap(src, mapping, None, INTER_CUBIC) under the contract of DESIGN.md section 16 (map_image_to_rect_event,
        dsec_loader.py:243-245).  src: (n, Hs, Ws) or (Hs, Ws) uint8, any size up to 32766; mapping (H, W, 2) float32 of the engine's
        sensor size, one for the stack.  Returns (n, H, W) or (H, W) uint8."""
        a, m, single = check_remap_args(src, mapping)
        if m.shape[:2] != (self.H, self.W):
            raise ValueError(f'mapping must be ({self.H}, {self.W}, 2), got {m.shape}')
        tab = remap_cubic_table()
        out = np.empty((a.shape[0], self.H, self.W), dtype=np.uint8)
        self._check(self._lib.eincm_remap_cubic(self._ctx, a.ctypes.data, a.shape[0], a.shape[1], a.shape[2], m.ctypes.data,
                                                tab.ctypes.data, out.ctypes.data))
        return out[0] if single else out

    def flow_decode(self, flow_16bit):
        """DSECDataLoader.flow_16bit_to_float (dsec_loader.py:247-266) for (B, H, W, 3) or (H, W, 3) uint16: returns (flow float64
        (..., H, W, 2), valid2D bool (..., H, W)).  ValueError: a pixel whose third channel is neither 0 nor 1 (the reference asserts)."""
        a, single = check_flow_16bit(flow_16bit)
        if a.shape[1:3] != (self.H, self.W):
            raise ValueError(f'16-bit flow must be ({self.H}, {self.W}, 3) per image, got {a.shape[1:]}')
        flow = np.empty(a.shape[:3] + (2,), dtype=np.float64)
        valid = np.empty(a.shape[:3], dtype=np.uint8)
        bad = C.c_int64(0)
        self._check_data(self._lib.eincm_flow_decode(self._ctx, a.ctypes.data, a.shape[0], flow.ctypes.data, valid.ctypes.data, C.byref(bad)))
        valid = valid.view(np.bool_)
        return (flow[0], valid[0]) if single else (flow, valid)

    def flow_encode(self, theta, valid=None):
        """dsec_npz_to_png.py:84-96: theta (B, h, w, 2) or (h, w, 2), scaled to the sensor with the bilinear scale_and_translate and
        coded as uint16(trunc(v * 128 + 2^15)), in one kernel.  Channel 2 is 0, or ``valid`` (B, H, W) where given.  Returns
        (..., H, W, 3) uint16.  ValueError: a value that is not finite or codes outside [0, 65536)."""
        t, v, single = check_theta_batch(theta, valid, (self.H, self.W))
        out = np.empty((t.shape[0], self.H, self.W, 3), dtype=np.uint16)
        bad = C.c_int64(0)
        self._check_data(self._lib.eincm_flow_encode(self._ctx, t.ctypes.data, t.shape[0], t.shape[1], t.shape[2],
                                                     None if v is None else v.ctypes.data, out.ctypes.data, C.byref(bad)))
        return out[0] if single else out

    # -- flow errors of solved thetas -----------------------------------------
    def flow_eval_stage(self, gt_flows, events, eval_masks=None):
        """Stage the ground truth of a batch of evaluation windows once: gt_flows (n, H, W, 2) float32 or float64, events a list of
        (xs, ys) per window (the evaluation events: per_pix_theta_to_flow's mask), eval_masks None or (n, H, W) (sparse_flow_error's
        event_mask).  Independent of set_windows; replaced by the next flow_eval_stage.  ValueError: a shape or dtype that does not
        fit (before the library is touched), an event outside the sensor (the engine then has no staged flow evaluation)."""
        g, n_events, xs, ys, m = check_flow_eval_batch(gt_flows, events, eval_masks, (self.H, self.W))
        rc = self._lib.eincm_flow_eval_stage(self._ctx, g.shape[0], g.ctypes.data, n_events.ctypes.data, xs.ctypes.data, ys.ctypes.data,
                                             None if m is None else m.ctypes.data)
        if rc != L.ERR_STATE:              # (refused for an evaluation in flight: what was staged is still there)
            self.flow_eval_windows = g.shape[0] if rc == L.OK else 0
        self._check_data(rc)

    def flow_errors(self, thetas, method='bilinear', ee_map=False):
        """sparse_flow_error(per_pix_theta_to_flow(Theta_b, events_b), gt_b, mask_b) of every staged window in one kernel, Theta_b =
        thetas[b] scaled to the sensor with ``method`` (thetas (n, h, w, 2) at any pyramid level up to the sensor's size).  Returns a
        list of {'errors': {AEE, AREE, A1PE, ...}, 'counts': {n_ee, n_pred, n_gt}}, sparse_flow_error's keys and types; with
        ee_map=True also the (n, H, W) float64 map of the endpoint error (NaN outside the intersection of the masks)."""
        n = self.flow_eval_windows
        if n < 1:
            raise EincmError(L.ERR_STATE, 'flow_errors called before flow_eval_stage')
        t, code = check_flow_eval_thetas(thetas, n, (self.H, self.W), method)
        out = (L.FlowErrorOut * n)()
        emap = np.empty((n, self.H, self.W), dtype=np.float64) if ee_map else None
        self._check(self._lib.eincm_flow_errors(self._ctx, t.ctypes.data, t.shape[1], t.shape[2], code, out,
                                                None if emap is None else emap.ctypes.data))
        res = []
        for o in out:
            errs = {'AEE': float(o.aee), 'AREE': float(o.aree)}
            for k, thr in enumerate(L.FLOW_ERROR_THRESHOLDS):
                errs[f'A{thr}PE'] = float(o.anpe[k])
            res.append({'errors': errs, 'counts': {'n_ee': int(o.n_ee), 'n_pred': int(o.n_pred), 'n_gt': int(o.n_gt)}})
        return (res, emap) if ee_map else res

    # -- a solved theta carried to the next window -----------------------------
    def advect_theta(self, thetas, tau=1.0, gain=1.0, method='bilinear', fill='source', min_coverage=0.5, return_dense=False,
                     return_coverage=False):
        """The prior of the next window from a solved theta: every field (thetas (n, h, w, 2) or (h, w, 2), any pyramid level up to the
        sensor's size) is scaled to the sensor with ``method``, forward-splatted along itself over ``tau`` (the time to the next
        window's start in units of this window's normalised duration) with integer bilinear weights, resolved per pixel (a pixel with
        coverage below ``min_coverage`` keeps its own value with fill='source', or gets 0 with fill='zero'), and the DIFFERENCE to the
        source field is resampled back to (h, w) and added: returns gain * (theta + R(D)), so tau=0 returns gain * theta exactly.
        ``gain``: the ratio of the two windows' durations.  tau and gain are scalars or (n,).  With return_dense / return_coverage
        also the (n, H, W, 2) float64 dense field and the (n, H, W) float32 coverage, in that order.  The same bytes on every run
        and in both precisions; the staged batch and its last evaluation are not touched.  ValueError: an argument that does not
        fit, a theta value that is not finite or beyond the fixed-point range (511 px at the sensor)."""
        t, tau, gain, mcode, fcode, mc, single = check_theta_advect_args(thetas, tau, gain, method, fill, min_coverage, (self.H, self.W))
        n = t.shape[0]
        out = np.empty_like(t)
        dense = np.empty((n, self.H, self.W, 2), dtype=np.float64) if return_dense else None
        cov = np.empty((n, self.H, self.W), dtype=np.float32) if return_coverage else None
        self._check_data(self._lib.eincm_theta_advect(self._ctx, t.ctypes.data, n, t.shape[1], t.shape[2], mcode, tau.ctypes.data,
                                                      gain.ctypes.data, fcode, mc, out.ctypes.data,
                                                      None if dense is None else dense.ctypes.data,
                                                      None if cov is None else cov.ctypes.data))
        res = [out] + [a for a in (dense, cov) if a is not None]
        res = [a[0] for a in res] if single else res
        return res[0] if len(res) == 1 else tuple(res)

    # -- device images ----------------------------------------------------------------------------
    def iwes(self):
        if self.precision == 'fp64':
            a = np.empty((self.B, self.R, self.H, self.W), dtype=np.float64)
            self._check(self._lib.eincm_get_iwes_f64(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double))))
            return a
        a = np.empty((self.B, self.R, self.H, self.W), dtype=np.float32)
        self._check(self._lib.eincm_get_iwes(self._ctx, a.ctypes.data_as(C.POINTER(C.c_float))))
        return a

    def zero_iwe(self):
        if self.precision == 'fp64':
            a = np.empty((self.B, self.H, self.W), dtype=np.float64)
            self._check(self._lib.eincm_get_zero_iwe_f64(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double))))
            return a
        a = np.empty((self.B, self.H, self.W), dtype=np.float32)
        self._check(self._lib.eincm_get_zero_iwe(self._ctx, a.ctypes.data_as(C.POINTER(C.c_float))))
        return a

    def image_grad(self):
        if self.precision == 'fp64':
            a = np.empty((self.B, self.R, self.H, self.W), dtype=np.float64)
            self._check(self._lib.eincm_get_image_grad_f64(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double))))
            return a
        a = np.empty((self.B, self.R, self.H, self.W), dtype=np.float32)
        self._check(self._lib.eincm_get_image_grad(self._ctx, a.ctypes.data_as(C.POINTER(C.c_float))))
        return a

    def count_images(self):
        """(B,R,H,W) uint32 histogram of the rounded warped coordinates under the last evaluation's Theta."""
        a = np.empty((self.B, self.R, self.H, self.W), dtype=np.uint32)
        self._check(self._lib.eincm_get_count_images(self._ctx, a.ctypes.data_as(C.POINTER(C.c_uint32))))
        return a

    def warped_events(self, window=0):
        """(warped_xs, warped_ys), (R, n_events) float64 each: per_pix_warp of one window's events (caller's order) at every reference
        time under the last evaluation's Theta - the two per-event entries of compute_loss_objectives (losses.py:58,90-91)."""
        n = int(self.n_events[window]) if 0 <= window < self.B else 0        # (the library reports a bad index)
        wx = np.empty((self.R, n), dtype=np.float64)
        wy = np.empty((self.R, n), dtype=np.float64)
        self._check(self._lib.eincm_get_warped_events(self._ctx, int(window), _dp(wx), _dp(wy)))
        return wx, wy

    def event_scores(self, images=None, ref_weights=None, exclude_self=False, theta=None, params=None):
        """Per-event scores: an image stack sampled at every staged event's warped position under the last
        evaluation's Theta, with the splat's nine tap weights - how much image lies under the event once it is warped.
        images: (B,R,H,W), or (R,H,W) when B == 1; None takes the IWEs of the last evaluation (read on the device).
        ref_weights: None gives one (R, n_b) float32 array per window; (R,) finite numbers give (n_b,), the weighted sum over the
        reference times.  exclude_self: subtract the event's own share w_e * sum_d k(d)^2, the leave-one-out score against the IWE;
        w is what ``set_windows`` was handed, or ones (a keep-order batch: ``staged_weights()``).  theta with params: ``loss_grad(theta, params, want_grad=False)`` runs first.
        Returns the list of the B arrays, events in the order they were staged."""
        if (theta is None) != (params is None):
            raise ValueError('theta and params go together: both, or neither (the last evaluation)')
        imgs = check_score_images(images, self.B, self.R, (self.H, self.W))
        rw = check_ref_weights(ref_weights, self.R)
        ws = self._self_weights() if exclude_self else None
        if theta is not None:
            self.loss_grad(theta, params, want_grad=False)
        off, length, total = event_scores_layout(self.n_events if self.B else [], self.R, rw is not None)
        scores = np.empty(total, dtype=np.float32)
        selfs = np.empty(total, dtype=np.float32) if exclude_self else None
        self._check(self._lib.eincm_event_scores(self._ctx, None if imgs is None else imgs.ctypes.data, None if rw is None else rw.ctypes.data,
                                                 scores.ctypes.data, None if selfs is None else selfs.ctypes.data))
        out = []
        for b in range(self.B):
            n = int(self.n_events[b])
            shape = (n,) if rw is not None else (self.R, n)
            s = scores[off[b]:off[b] + length[b]].reshape(shape)
            if exclude_self:
                q = selfs[off[b]:off[b] + length[b]].reshape(shape)
                s = s - q if ws[b] is None else s - ws[b] * q
            out.append(np.ascontiguousarray(s, dtype=np.float32))
        return out

    def event_responsibilities(self, n_models, images=None, ref_weights=None, prior=None, exclude_self=True,
                               want=('weights', 'labels', 'mass')):
        """The E-step of a segmentation into ``n_models`` motions, one device operation: the staged batch is
        G = B / n_models groups of n_models consecutive windows that hold the same events under different motions (and complementary
        weights); every event's combined scores (event_scores with ref_weights) under the last evaluation are normalised over the
        models of its group.  images as event_scores.  ref_weights: (R,) finite, default multi_ref_weights(R).  prior: None (ones) or
        (B,) numbers >= 0, positive in sum per group.  exclude_self: the leave-one-out score, with the weights ``set_windows`` was
        handed.  want: which of RS_OUTPUTS to fetch.  Returns a dict of those: 'weights' a list of B float32 (n_b,) arrays, what
        set_windows takes back; 'labels' a list of G uint8 (n_g,) arrays, the lowest model with the largest share; 'mass' (G,
        n_models) float64, each window's sum of weights; 'n_unsupported' (G,) int64, the events no model supports (they get the
        prior's shares).  A keep-order batch's leave-one-out score reads the staged weights on the device (EINCM_RS_STAGED_WEIGHTS)."""
        return self._responsibilities(n_models, images, ref_weights, prior, exclude_self, want, False)

    def apply_responsibilities(self, n_models, images=None, ref_weights=None, prior=None, exclude_self=True, want=('labels', 'mass')):
        """event_responsibilities whose result becomes the staged weights of all B windows, in place (EINCM_RS_APPLY, DESIGN.md section
        29): after the responsibilities are formed on the device they are gathered into the staged layouts as set_weights would, with
        no host round trip in between.  The batch must have been staged with keep_order=True.  ``want`` may leave 'weights' out, so that
        nothing per-event is downloaded, or be empty; what it names are the bytes event_responsibilities returns, and the engine is
        left as event_responsibilities followed by a set_windows with its 'weights' would leave it.  Returns the dict of ``want``."""
        self._need_keep_order('apply_responsibilities')
        return self._responsibilities(n_models, images, ref_weights, prior, exclude_self, want, True)

    def _responsibilities(self, n_models, images, ref_weights, prior, exclude_self, want, apply, spatial=False, prior_images=None):
        if apply and isinstance(want, (tuple, list)) and len(want) == 0:
            K, pi, _ = check_responsibility_args(n_models, self.n_events if self.B else [], prior, RS_OUTPUTS)
            want = ()
        else:
            K, pi, want = check_responsibility_args(n_models, self.n_events if self.B else [], prior, want)
        imgs = check_score_images(images, self.B, self.R, (self.H, self.W))
        rw = check_ref_weights(multi_ref_weights(self.R) if ref_weights is None else ref_weights, self.R)
        ws = None if (self.keep_order or not exclude_self) else self._self_weights()
        flags = (L.RS_EXCLUDE_SELF if exclude_self else 0) | (L.RS_APPLY if apply else 0)
        if self.keep_order and exclude_self:
            flags |= L.RS_STAGED_WEIGHTS
        B, G = self.B, self.B // K
        w_off, w_total, lab_off, lab_len, lab_total = event_responsibilities_layout(self.n_events if B else [], K)
        weights = np.empty(w_total, dtype=np.float32) if 'weights' in want else None
        labels = np.empty(lab_total, dtype=np.uint8) if 'labels' in want else None
        mass = np.zeros(B, dtype=np.float64) if 'mass' in want else None                # (a batch without events writes nothing)
        n_uns = np.zeros(G, dtype=np.int64) if 'n_unsupported' in want else None
        addr = lambda a: None if a is None else a.ctypes.data
        if spatial:
            pimg = check_prior_images(prior_images, B, (self.H, self.W))
            if pimg is None:
                flags |= L.RS_PRIOR_STAGED
            self._check(self._lib.eincm_event_responsibilities_spatial(self._ctx, K, addr(imgs), addr(rw), per_window_ptrs(ws), addr(pi),
                                                                       addr(pimg), flags, addr(weights), addr(labels), addr(mass), addr(n_uns)))
        else:
            self._check(self._lib.eincm_event_responsibilities(self._ctx, K, addr(imgs), addr(rw), per_window_ptrs(ws), addr(pi), flags,
                                                               addr(weights), addr(labels), addr(mass), addr(n_uns)))
        if apply:
            self._staged_weights = None     # (they are the device's now: staged_weights())
        out = {}
        if weights is not None:
            out['weights'] = [weights[w_off[b]:w_off[b] + int(self.n_events[b])] for b in range(B)]
        if labels is not None:
            out['labels'] = [labels[lab_off[g]:lab_off[g] + lab_len[g]] for g in range(G)]
        if mass is not None:
            out['mass'] = mass.reshape(G, K)
        if n_uns is not None:
            out['n_unsupported'] = n_uns
        return out

    def label_prior(self, n_models, radius, floor_mass=4096, want=('prior',)):
        """The per-pixel label prior of the E-step, one device operation.  The staged batch is G = B / n_models
        groups of n_models consecutive windows, as compose_motions reads it, and 'mass' is that operator's: the staged weights quantised
        to 1/4096 and summed per pixel and model.  Per pixel every model's mass is summed over the (2 radius + 1)^2 box around it,
        clipped to the sensor; floor_mass (4096 is one event of weight 1) is added to every model's sum, which keeps a model alive where
        it has no mass yet; the prior is the model's share of the K sums, 1 where they are all 0.  Returns a dict of ``want``: 'prior'
        (B, H, W) float32, what event_responsibilities_spatial takes; 'smoothed' (G, n_models, H, W) uint64, the box sums.  want=() only
        stages: whatever is downloaded, the prior stays on the device as the staged prior, which event_responsibilities_spatial reads in
        place; set_windows drops it, set_weights and apply_responsibilities keep it.  Needs staged windows, no model and no evaluation.
        Exact: equal to tests/_label_prior_witness.py byte for byte, and the same bytes on every run."""
        K, r, floor, want = check_label_prior_args(n_models, radius, floor_mass, want)
        lay = label_prior_layout(self.B // K, K, (self.H, self.W))
        out = {name: np.zeros(lay[name][0], dtype=lay[name][1]) for name in want}
        addr = lambda name: out[name].ctypes.data if name in out else None
        self._check(self._lib.eincm_label_prior(self._ctx, K, r, floor, 0, addr('prior'), addr('smoothed')))
        return out

    def staged_prior(self):
        """The staged prior, downloaded: (B, H, W) float32, what the last label_prior left.  For tests and tools."""
        p = np.zeros((self.B, self.H, self.W), dtype=np.float32)
        self._check(self._lib.eincm_get_staged_prior(self._ctx, p.ctypes.data))
        return p

    def carry_label_prior(self, n_models, coeffs, tau=1.0, radius=2, floor_mass=4096, want=('prior',)):
        """The label prior of the staged segmentation carried to the next window, one device operation.  The
        staged batch, n_models and coeffs (B, K_c) are compose_motions'.  Every model's mass image is pushed along that model's own
        field by tau (a number, or (G,): one per group; the displacement is model.field(coeffs) * tau pixels), split over the four
        pixels around where it lands with weights that sum to 2^20, summed in uint64 and rounded back to uint32 masses, half up and
        saturating at 2^32 - 1; label_prior's box sum and shares (radius, floor_mass) run on those.  Mass that leaves the sensor, or
        whose landing is not finite, is dropped.  Returns a dict of ``want``: 'prior' (B, H, W) float32, what
        event_responsibilities_spatial takes; 'carried' (G, n_models, H, W) uint32, the masses that arrived; 'accum' (G, n_models, H, W)
        uint64, the sums before rounding; 'dropped' (G, n_models) uint64, in the units of 'accum': accum.sum() + dropped is 2^20 times
        the model's mass.  want=() only carries: whatever is downloaded, the prior stays on the device as the carried prior, which
        set_windows leaves alone and adopt_carried_prior makes the staged prior of the next batch.  The staged prior of this batch is
        not touched.  Needs staged windows and a motion model, no evaluation; fp32 engines only, no sharded staging, no theta-grid
        fields.  Exact: equal to tests/_label_carry_witness.py byte for byte, and the same bytes on every run."""
        K, c, t, r, floor, want = check_label_carry_args(n_models, coeffs, self.B,
                                                         None if self.motion_model is None else self.motion_model.n_coeffs, tau, radius,
                                                         floor_mass, want)
        t = np.ascontiguousarray(np.broadcast_to(t, (max(self.B // K, 1),)) if t.ndim == 0 else t)
        lay = label_carry_layout(self.B // K, K, (self.H, self.W))
        out = {name: np.zeros(lay[name][0], dtype=lay[name][1]) for name in want}
        addr = lambda name: out[name].ctypes.data if name in out else None
        self._check(self._lib.eincm_carry_label_prior(self._ctx, K, c.ctypes.data, c.shape[1], t.ctypes.data, r, floor, 0, addr('prior'),
                                                      addr('carried'), addr('accum'), addr('dropped')))
        self._carried_windows = self.B
        return out

    def adopt_carried_prior(self, n_models):
        """The carried prior of carry_label_prior becomes the staged prior of the batch staged now, on the device: the next
        event_responsibilities_spatial / apply_responsibilities_spatial without prior_images reads it.  The batch must have the B and
        the n_models the prior was carried with.  The carried prior stays, so it can be adopted again after another staging."""
        if isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer)) or not 1 <= int(n_models) <= L.RS_MAX_MODELS:
            raise ValueError(f'n_models must be an integer within 1 .. {L.RS_MAX_MODELS}, got {n_models!r}')
        self._check(self._lib.eincm_adopt_carried_prior(self._ctx, int(n_models)))

    def carried_prior(self):
        """The carried prior, downloaded: (B, H, W) float32 of the batch it was formed on.  For tests and tools."""
        p = np.zeros((max(self._carried_windows, 1), self.H, self.W), dtype=np.float32)     # (none carried: the library refuses)
        self._check(self._lib.eincm_get_carried_prior(self._ctx, p.ctypes.data))
        return p

    def event_responsibilities_spatial(self, n_models, prior_images=None, images=None, ref_weights=None, prior=None, exclude_self=True,
                                       want=('weights', 'labels', 'mass')):
        """event_responsibilities with a prior image: model l's mixing weight for an event is prior[b] times
        prior_images[b] at the event's own pixel, so that an event is told what its neighbourhood belongs to.  prior_images: (B, H, W)
        numbers, finite and >= 0, or (H, W) when B == 1; None reads the staged prior of label_prior on the device.  An event that no
        model supports takes the shares of prior * prior_images, and those of prior alone where that product has no positive sum; it
        is counted unsupported once.  Everything else is event_responsibilities'; with prior_images of ones, so are the bytes."""
        return self._responsibilities(n_models, images, ref_weights, prior, exclude_self, want, False, True, prior_images)

    def apply_responsibilities_spatial(self, n_models, prior_images=None, images=None, ref_weights=None, prior=None, exclude_self=True,
                                       want=('labels', 'mass')):
        """event_responsibilities_spatial whose result becomes the staged weights of all B windows, in place, as apply_responsibilities
        does it.  The batch must have been staged with keep_order=True.  The staged prior stays as it is."""
        self._need_keep_order('apply_responsibilities_spatial')
        return self._responsibilities(n_models, images, ref_weights, prior, exclude_self, want, True, True, prior_images)

    def contrast_landscape(self, coeffs, t_ref=None, cell=1, keep=None, want=('sumsq', 'n_in')):
        """The contrast landscape over motion coefficients, one device operation: every staged window's raw
        events are warped to ``t_ref`` by the engine's motion model at each of V candidate coefficient vectors, dropped where they leave
        the sensor, and counted in cells of ``cell`` x ``cell`` pixels.  coeffs: (B, V, K), or (V, K) when B == 1.  t_ref: None (0.5), a
        number or (B,).  keep: None, or B entries, each None or a mask over the window's events as they were staged: only those take
        part.  Returns a dict of ``want``: 'sumsq' (B, V) uint64, the sum of squared cell counts - the integer the search ranks by;
        'n_in' (B, V) uint32, the events inside the sensor.  Staged weights are ignored.  Exact: equal to
        tests/_contrast_landscape_witness.py integer for integer, and the same bytes on every run."""
        c, t, cell, masks, want = check_contrast_landscape_args(coeffs, self.n_events if self.B else [],
                                                                None if self.motion_model is None else self.motion_model.n_coeffs,
                                                                t_ref, cell, keep, want)
        B, V = c.shape[:2]
        sumsq = np.zeros((B, V), dtype=np.uint64) if 'sumsq' in want else None
        n_in = np.zeros((B, V), dtype=np.uint32) if 'n_in' in want else None
        addr = lambda a: None if a is None else a.ctypes.data
        self._check(self._lib.eincm_contrast_landscape(self._ctx, V, c.ctypes.data, t.ctypes.data, cell, per_window_ptrs(masks), addr(sumsq), addr(n_in)))
        out = {}
        if sumsq is not None:
            out['sumsq'] = sumsq
        if n_in is not None:
            out['n_in'] = n_in
        return out

    def compose_motions(self, n_models, coeffs, mode='hard', fill='zero', want=('theta', 'labels')):
        """A motion segmentation composed into one flow field and a label image, one device operation.  The
        staged batch is G = B / n_models groups of n_models consecutive windows that hold the same events with complementary
        weights, as event_responsibilities reads it; coeffs (B, K_c) are the models' coefficients, window g * n_models + l model l of
        group g.  Per sensor pixel the staged weights of the events that fired there are quantised to 1/4096 and summed per model.
        Returns a dict of ``want``: 'mass' (G, n_models, H, W) uint32, those sums; 'total' (G, n_models) uint64, their sums over the
        pixels; 'labels' (G, H, W) uint8, the lowest model with the largest mass, ML_NO_LABEL (255) where no mass lies; 'theta'
        (G, H, W, 2) float64, what flow_errors, advect_theta and loss_grad take: mode 'hard' writes the label's field
        (model.field(coeffs) there, bit for bit), 'soft' the mass-weighted blend of the models' fields; a pixel without mass takes
        fill 'zero', (0, 0), or 'dominant', the field of the group's model of the largest total.  Needs staged windows and a motion
        model, no evaluation.  Exact: equal to tests/_motion_layers_witness.py byte for byte, and the same bytes on every run."""
        K, c, flags, want = check_compose_args(n_models, coeffs, self.B, None if self.motion_model is None else self.motion_model.n_coeffs,
                                               mode, fill, want)
        lay = compose_motions_layout(self.B // K, K, (self.H, self.W))
        out = {name: np.zeros(lay[name][0], dtype=lay[name][1]) for name in want}
        addr = lambda name: out[name].ctypes.data if name in out else None
        self._check(self._lib.eincm_compose_motions(self._ctx, K, c.ctypes.data, flags, addr('theta'), addr('labels'), addr('mass'), addr('total')))
        return out

    def densify_motions(self, n_models, coeffs, mode='hard', fallback='dominant', min_site_mass=1, max_distance=None,
                        want=('theta', 'labels')):
        """compose_motions made dense, one device operation: a pixel is a site if its summed mass reaches
        min_site_mass (4096 is one event of weight 1), and every pixel within max_distance pixels of a site (None: any distance) takes
        the label of its nearest site - equal distances go to the lowest row, then the lowest column - and is composed from that
        site's masses and the models' fields at the pixel itself.  A pixel no site reaches keeps ML_NO_LABEL and takes fallback
        'zero' or 'dominant', compose_motions' fill.  The staged batch, n_models, coeffs and mode are compose_motions'.  Returns a
        dict of ``want``: 'theta' (G, H, W, 2) float64, 'labels' (G, H, W) uint8, 'dist2' (G, H, W) uint32, the squared distance to
        the nearest site (MD_NONE in a group without one), 'nearest' (G, H, W) int32, that site as y * W + x (-1), 'n_sites' (G,)
        uint32.  With min_site_mass=1 and max_distance=0 'theta' and 'labels' are compose_motions' bytes.  Exact: equal to
        tests/_motion_fill_witness.py byte for byte, and the same bytes on every run."""
        K, c, flags, site_mass, max_dist2, want = check_densify_args(
            n_models, coeffs, self.B, None if self.motion_model is None else self.motion_model.n_coeffs, mode, fallback, min_site_mass,
            max_distance, want)
        lay = densify_motions_layout(self.B // K, (self.H, self.W))
        out = {name: np.zeros(lay[name][0], dtype=lay[name][1]) for name in want}
        addr = lambda name: out[name].ctypes.data if name in out else None
        self._check(self._lib.eincm_densify_motions(self._ctx, K, c.ctypes.data, flags, site_mass, max_dist2, addr('theta'), addr('labels'),
                                                    addr('dist2'), addr('nearest'), addr('n_sites')))
        return out

    def scaled_theta(self):
        a = np.empty((self.B, self.H, self.W, 2), dtype=np.float64)
        self._check(self._lib.eincm_get_scaled_theta(self._ctx, _dp(a)))
        return a

    def timings_total(self, reset=False):
        """(dict of per-stage ms summed over the evaluations since the last reset, number of evaluations)."""
        t = L.Timings(); n = C.c_int64(0)
        self._check(self._lib.eincm_get_timings_total(self._ctx, C.byref(t), C.byref(n), 1 if reset else 0))
        d = {name: float(t.ms[i]) for i, name in enumerate(L.STAGE_NAMES)}
        d['total'] = float(t.total_ms)
        return d, int(n.value)

    def host_profile(self, reset=False):
        """(dict of host-side microseconds per evaluation phase summed since the last reset, number of evaluations)."""
        us = (C.c_double * 4)(); n = C.c_int64(0)
        self._check(self._lib.eincm_get_host_profile(self._ctx, us, C.byref(n), 1 if reset else 0))
        return dict(zip(('begin', 'launch', 'wait', 'collect'), (float(v) for v in us))), int(n.value)

    LAUNCH_POLICY_NAMES = ('seg_gather', 'seg_splat', 'seg_gather_2dof', 'seg_splat_short', 'pitch_policy', 'span_splat', 'span_gather',
                           'span_gather_2dof', 'cap_splat', 'cap_gather', 'cap_gather_2dof', 'pitch_aligned', 'splat_short')

    def launch_policy(self):
        """Diagnostic (eincm_get_launch_policy): segment lengths and pitch regime of the staged batch, window capacities of the last
        evaluation.  No counterpart in the reference."""
        out = (C.c_double * len(self.LAUNCH_POLICY_NAMES))()
        self._check(self._lib.eincm_get_launch_policy(self._ctx, out))
        return dict(zip(self.LAUNCH_POLICY_NAMES, (float(v) for v in out)))

    def memory(self):
        """Diagnostic (eincm_get_memory): the context's live device and pinned bytes, its allocations and its scratch block.  Equal
        before and after a call: the call allocated nothing.  No HIP call."""
        out = (C.c_int64 * 4)()
        self._check(self._lib.eincm_get_memory(self._ctx, out))
        return Memory(*(int(v) for v in out))

    def set_timed_kernels(self, splat=True, gather=True):
        """timing='dominant' contexts: which event kernels carry HIP timing events from the next evaluation on."""
        self._check(self._lib.eincm_set_timed_kernels(self._ctx, 1 if splat else 0, 1 if gather else 0))

    def set_timing_period(self, period):
        """timing='dominant' contexts: timing events on every ``period``-th evaluation only."""
        self._check(self._lib.eincm_set_timing_period(self._ctx, int(period)))

    def timings(self):
        t = L.Timings()
        self._check(self._lib.eincm_get_timings(self._ctx, C.byref(t)))
        d = {n: float(t.ms[i]) for i, n in enumerate(L.STAGE_NAMES)}
        d['total'] = float(t.total_ms)
        return d


def per_window_ptrs(arrays):
    """The C form of one optional host array per window: a (void* x B) list with NULL for a missing or empty entry, or None for the
    whole list when no entry has data (or ``arrays`` is None).  The arrays must outlive the call that takes the list."""
    if arrays is None or not any(a is not None and a.size for a in arrays):
        return None
    return (C.c_void_p * len(arrays))(*[None if (a is None or not a.size) else a.ctypes.data for a in arrays])


def multi_ref_weights(n_refs):
    w = np.empty(n_refs)
    rc = L.load().eincm_multi_ref_weights(int(n_refs), _dp(w))
    if rc:
        raise EincmError(rc, 'eincm_multi_ref_weights')
    return w


def resample_matrix(n_in, n_out, method='bilinear'):
    A = np.empty((n_out, n_in))
    rc = L.load().eincm_resample_matrix(int(n_in), int(n_out), L.METHODS[method], _dp(A))
    if rc:
        raise EincmError(rc, 'eincm_resample_matrix')
    return A


class EngineGroup:
    """A batch of independent windows spread over ``n_groups`` contexts of one GPU (one HIP stream each).  ``loss_grad`` enqueues
    every group's evaluation before waiting for any, so the latency-bound small kernels of one group overlap the event kernels of
    another: on MI355X the 8-window / 10^6-event batch gains 18 % (2 groups) to 25 % (4 groups) over a single context.
    Same call shapes as ``Engine`` for set_windows / loss_grad; results are concatenated in window order."""

    def __init__(self, sensor_size, max_events_total, max_refs=8, max_windows=1, n_groups=2, device=0, timing=False, precision='fp32'):
        self.precision = check_precision(precision)
        self.n_groups = max(1, min(int(n_groups), int(max_windows)))
        per = -(-int(max_windows) // self.n_groups)
        self.engines = [Engine(sensor_size, max_events_total, max_refs=max_refs, max_windows=per, device=device, timing=timing,
                               precision=precision)
                        for _ in range(self.n_groups)]
        self.H, self.W = self.engines[0].H, self.engines[0].W
        self.B = 0
        self._slices = []

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_windows(self, windows):
        B = len(windows)
        per = -(-B // self.n_groups)
        self._slices = [slice(i, min(i + per, B)) for i in range(0, B, per)]
        for e, sl in zip(self.engines, self._slices):
            e.set_windows(windows[sl])
        self.B = B
        self.R = self.engines[0].R

    def loss_grad(self, theta, params, want_grad=True, want_aux=False, allow_nonfinite=True):
        th = np.asarray(theta, dtype=np.float64)
        if th.ndim == 3:
            th = th[None]
        if th.shape[0] != self.B:
            raise ValueError(f'theta must be ({self.B},h,w,2), got {th.shape}')
        # Every context that was launched is waited for before anything is raised: a context left in flight would refuse
        # every later call (EINCM_ERR_STATE) and the group has no other drain.  The first error wins.
        launched, outs, first_err = [], [], None
        try:
            for e, sl in zip(self.engines, self._slices):
                e.loss_grad_async(th[sl], params, want_grad)
                launched.append(e)
        except Exception as err:          # noqa: BLE001 - re-raised below, after the drain
            first_err = err
        for e in launched:
            try:
                outs.append(e.loss_grad_wait(want_aux, allow_nonfinite))
            except Exception as err:      # noqa: BLE001
                outs.append(None)
                if first_err is None:
                    first_err = err
        if first_err is not None:
            raise first_err
        value = np.concatenate([o[0] for o in outs])
        grad = np.concatenate([o[1] for o in outs]) if want_grad else None
        aux = [a for o in outs for a in o[2]] if want_aux else None
        return value, grad, aux

    def timings(self):
        """Per-stage device times summed over the groups (they overlap on the GPU: the sum exceeds the wall time)."""
        acc = {}
        for e in self.engines[:len(self._slices)]:
            for k, v in e.timings().items():
                acc[k] = acc.get(k, 0.0) + v
        return acc
