"""Plain restatement of the event kernels' launch policy (DESIGN.md 4.2 "where those rules hold"): from the tile populations of a
staged batch, its shape (H, W, R, B), the splat radius and max|theta|, the thirteen fields of eincm_get_launch_policy.

Test helper only: numpy and the standard library, no GPU.  Restated from the rules, not from the library's code paths:
- staging: the segment lengths of the four lists from x_wg and per_tile, whether the short splat list exists, the pitch policy
  (EINCM_PITCH_ALIGNED as the argument `pitch_env`), each list's time span (the span all but 3 % of the events' segments stay within);
- evaluation: the LDS capacity class of every list from max|theta| * span (fit_window with its floor class and pitch argument and the
  margin 2 * (radius + 1)), the short-list decision of a 2-DoF splat, the theta-grid gather's rule (sized on the unrounded side) and
  the 2-DoF gather's.
Not covered: the float64 mode (it has no launch policy), a pinned capacity (EINCM_WINCAP), EINCM_SEG* and the theta transport.
"""
import math

import numpy as np

TS = 32                                # source tile edge
CAPS = (2304, 3072, 4608, 6912)        # LDS capacity classes, words
SEG_LONG, SEG_SHORT, SEG_MIN = 16384, 8192, 4096
SPAN_CLASSES = 64                      # spans 1, 1/2, ... 1/64
ALLOWANCE = 0.03                       # share of the events whose segments may span more than the list's span

FIELDS = ('seg_gather', 'seg_splat', 'seg_gather_2dof', 'seg_splat_short', 'pitch_policy', 'span_splat', 'span_gather',
          'span_gather_2dof', 'cap_splat', 'cap_gather', 'cap_gather_2dof', 'pitch_aligned', 'splat_short')


def tiles_of(H, W):
    """(tilesY, tilesX) of an H x W sensor."""
    return (H + TS - 1) // TS, (W + TS - 1) // TS


def tile_counts(xs, ys, H, W):
    """Events per 32 x 32 source tile of one window, row-major (ntiles,)."""
    ty, tx = tiles_of(H, W)
    idx = (np.asarray(ys, dtype=np.int64) // TS) * tx + np.asarray(xs, dtype=np.int64) // TS
    return np.bincount(idx, minlength=ty * tx).astype(np.int64)


def balanced_seg_len(count, seg):
    """Length of the equal segments a tile of `count` events is cut into: as many as ceil(count / seg), rounded up to 256 events."""
    nseg = -(-count // seg)
    if nseg <= 1:
        return seg
    per = -(-count // nseg)
    return min(-(-per // 256) * 256, seg)


def segment_lengths(counts, seg):
    """Lengths of the segments of every (window, tile) bin, in bin order."""
    out = []
    for c in np.asarray(counts).reshape(-1):
        c, ln = int(c), balanced_seg_len(int(c), seg)
        out.extend(min(ln, c - s) for s in range(0, c, ln))
    return out


def list_span(counts, seg):
    """Time span (fraction of the window) a list's LDS windows are sized for: a tile of n events is cut into k = ceil(n / seg)
    segments of about 1 / k of the time each; the largest span 1 / k such that the events in tiles of fewer segments (longer
    spans) are at most 3 % of all events."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n_total = int(counts.sum())
    by_nseg = np.zeros(SPAN_CLASSES + 1, dtype=np.int64)
    for c in counts[counts > 0]:
        by_nseg[min(-(-int(c) // seg), SPAN_CLASSES)] += c
    allow = int(ALLOWANCE * n_total)
    beyond = 0
    for k in range(1, SPAN_CLASSES + 1):
        beyond += int(by_nseg[k])
        if beyond > allow:
            return 1.0 / k
    return 1.0 / SPAN_CLASSES


def stage_policy(counts, H, W, R, B, pitch_env=None):
    """The staging half.  counts: (B, ntiles) events per window and tile.  pitch_env: the value of EINCM_PITCH_ALIGNED, or None."""
    counts = np.asarray(counts, dtype=np.int64).reshape(B, -1)
    ty, tx = tiles_of(H, W)
    ntiles = ty * tx
    assert counts.shape[1] == ntiles
    N = int(counts.sum())
    x_wg = (N / 8192.0 + 0.5 * B * ntiles) * R          # workgroups of a launch at 8192-event segments
    per_tile = N / (B * ntiles)
    resident = per_tile < SEG_LONG                      # about one long segment per tile
    seg_gather = SEG_LONG
    seg_2 = SEG_LONG if (x_wg >= 4000.0 and resident) else (SEG_MIN if x_wg < 1000.0 else SEG_SHORT)
    seg_s = SEG_LONG if (x_wg >= 3000.0 and resident) else (SEG_SHORT if x_wg >= 400.0 else SEG_MIN)
    short = seg_s > SEG_SHORT and N > 0
    pitch = 1 if (x_wg >= 3000.0 and resident) else 0
    if pitch_env is not None:
        pitch = max(0, min(2, int(pitch_env)))
    return dict(seg_gather=seg_gather, seg_splat=seg_s, seg_gather_2dof=seg_2, seg_splat_short=SEG_SHORT if short else 0,
                pitch_policy=pitch, span_splat=list_span(counts, seg_s), span_gather=list_span(counts, seg_gather),
                span_gather_2dof=list_span(counts, seg_2), span_splat_short=list_span(counts, SEG_SHORT) if short else None,
                x_wg=x_wg, per_tile=per_tile, n_events=N)


def win_maxw(cap):
    """Largest width of a window of `cap` words."""
    return max(40, int(math.floor(math.sqrt(cap * 1.4) + 0.5)))


def window_side(vmax, span, rad=1):
    """Side in pixels of the window a segment of time span `span` needs: the tile, the displacement spread, the margin."""
    return TS + 2.0 * (rad + 1) + vmax * span


def fit_window(vmax, span, margin, floor_k, pitch):
    """Capacity class of one list in one evaluation.  floor_k: index of the smallest class the list takes.  pitch: 1 = take the
    bank-aligned pitch (width rounded up to 32 words) where the padded window stays in the class, 0 = pitch is the width, -1 = too,
    and the class is sized on the unrounded side.  Returns dict(cap, maxw, aligned, fits)."""
    side = TS + margin + vmax * span
    sd = math.ceil(side)
    need = side * side if pitch < 0 else float(sd) * sd
    cap = CAPS[-1]
    for k in range(floor_k, len(CAPS)):
        if need <= CAPS[k]:
            cap = CAPS[k]
            break
    aligned = pitch > 0 and math.ceil(sd / 32.0) * 32.0 * sd <= cap
    return dict(cap=cap, maxw=win_maxw(cap), aligned=bool(aligned), fits=need <= CAPS[-1], side=sd)


def eval_policy(stage, vmax, two_dof, rad=1):
    """The evaluation half on a staged batch (stage_policy's result).  two_dof: a (1, 1) theta, else a theta grid or a dense theta.
    Returns the evaluation's fields and, under 'splat' / 'gather' / 'gather_2dof', the fit of each list."""
    margin = 2.0 * (rad + 1)
    floor_s = 2 if two_dof else 0                       # the 2-DoF kernels hold only the window in LDS: 4608 words cost no residency
    pitch_s = 1 if stage['pitch_policy'] != 0 else 0
    s = fit_window(vmax, stage['span_splat'], margin, floor_s, pitch_s)
    long_fits = s['fits']
    short = bool(two_dof and stage['seg_splat_short'] and not s['fits'])
    if short:
        s = fit_window(vmax, stage['span_splat_short'], margin, floor_s, pitch_s)
    a = fit_window(vmax, stage['span_gather'], margin, 2, -1)
    g2 = fit_window(vmax, stage['span_gather_2dof'], margin, 2, 1 if stage['pitch_policy'] >= 2 else 0)
    return dict(cap_splat=s['cap'], cap_gather=a['cap'], cap_gather_2dof=g2['cap'],
                pitch_aligned=(1 if s['aligned'] else 0) | (2 if g2['aligned'] else 0), splat_short=1 if short else 0,
                splat=s, gather=a, gather_2dof=g2, long_fits=long_fits)


def launch_policy(counts, H, W, R, B, rad=1, vmax=None, two_dof=True, pitch_env=None):
    """The thirteen fields of eincm_get_launch_policy, as floats.  vmax None: staged, not evaluated (the evaluation's fields are 0;
    a staging evaluates theta = 0 for the window constants, which does not count)."""
    st = stage_policy(counts, H, W, R, B, pitch_env)
    out = {k: float(st[k]) for k in FIELDS[:8]}
    if vmax is None:
        out.update({k: 0.0 for k in FIELDS[8:]})
    else:
        ev = eval_policy(st, float(vmax), two_dof, rad)
        out.update({k: float(ev[k]) for k in FIELDS[8:]})
    return out
