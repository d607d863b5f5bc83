"""The contrast landscape (eincm_contrast_landscape in include/eincm.h) stated in numpy, the peel rule of
segmentation.seed_motions beside it, and the scenes the tests of both share.

The contract is written here a second time, on purpose, from MotionModel.field alone: Theta at the event's own pixel, dt = t - t_ref,
w = x - Theta * dt (numpy rounds the product, then the difference), r = rint(w) (half to even), the in-sensor test on the floats, the
cell by an integer shift, a histogram of the cells and the sum of its squares in Python-sized integers.  Events outside the sensor are
dropped; nothing wraps."""
import numpy as np

MAX_CANDIDATES = 4096
CELLS = (1, 2, 4, 8)


def warp(model, c, xs, ys, ts, t_ref):
    """(r_x, r_y) float64 and the in-sensor mask of one window's events under the coefficients c (K,)"""
    H, W = model.sensor_size
    x, y = np.asarray(xs).astype(np.int64), np.asarray(ys).astype(np.int64)
    with np.errstate(over='ignore', invalid='ignore'):
        theta = model.field(np.asarray(c, dtype=np.float64))[y, x]
        dt = np.asarray(ts, dtype=np.float64) - np.float64(t_ref)
        px, py = theta[:, 0] * dt, theta[:, 1] * dt                       # the products, rounded
        rx, ry = np.rint(x.astype(np.float64) - px), np.rint(y.astype(np.float64) - py)
        inside = (rx >= 0.0) & (rx < float(W)) & (ry >= 0.0) & (ry < float(H))
    return rx, ry, inside


def cell_image(rx, ry, part, sensor, cell):
    """The ceil(H / cell) x ceil(W / cell) image of counts, int64, of the warped events that take part"""
    H, W = sensor
    Hc, Wc = -(-H // cell), -(-W // cell)
    shift = CELLS.index(cell)
    cy, cx = ry[part].astype(np.int64) >> shift, rx[part].astype(np.int64) >> shift
    return np.bincount(cy * Wc + cx, minlength=Hc * Wc).reshape(Hc, Wc)


def counts(model, c, xs, ys, ts, t_ref, cell, keep=None):
    rx, ry, inside = warp(model, c, xs, ys, ts, t_ref)
    return cell_image(rx, ry, inside if keep is None else inside & (np.asarray(keep) != 0), model.sensor_size, cell)


def landscapes(model, events, coeffs, t_ref, cells, keep=None):
    """events: B (xs, ys, ts) triples; coeffs (B, V, K); t_ref (B,); keep None or B entries, each None or a mask.
    Returns {cell: (sumsq (B, V) uint64, n_in (B, V) uint32)}; every candidate is warped once for all the cells."""
    coeffs = np.asarray(coeffs, dtype=np.float64)
    B, V = coeffs.shape[:2]
    out = {cell: (np.zeros((B, V), dtype=np.uint64), np.zeros((B, V), dtype=np.uint32)) for cell in cells}
    for b, (xs, ys, ts) in enumerate(events):
        assert len(xs) < 2 ** 31                                            # sum count^2 <= n^2 < 2^62: int64 holds it
        k = None if keep is None or keep[b] is None else np.asarray(keep[b]) != 0
        for j in range(V):
            rx, ry, inside = warp(model, coeffs[b, j], xs, ys, ts, t_ref[b])
            for cell in cells:
                img = cell_image(rx, ry, inside if k is None else inside & k, model.sensor_size, cell)
                out[cell][0][b, j] = int((img * img).sum())
                out[cell][1][b, j] = int(img.sum())
    return out


def landscape(model, events, coeffs, t_ref, cell, keep=None):
    """(sumsq (B, V) uint64, n_in (B, V) uint32) at one cell size"""
    return landscapes(model, events, coeffs, t_ref, (cell,), keep)[cell]


def explained(model, c, xs, ys, ts, t_ref, keep, peel_min_count):
    """The peel rule: an event is explained when it is kept, in-sensor, and the cell-1 count of the kept in-sensor events under it,
    minus its own 1, is >= peel_min_count."""
    img = counts(model, c, xs, ys, ts, t_ref, 1, keep)
    rx, ry, inside = warp(model, c, xs, ys, ts, t_ref)
    out = np.zeros(len(xs), dtype=bool)
    for e in np.flatnonzero(inside & (np.asarray(keep) != 0)):
        out[e] = img[int(ry[e]), int(rx[e])] - 1 >= peel_min_count
    return out


def landscape_callable(model, windows):
    """What segmentation.seed_motions takes as ``landscape``: the witness on these windows."""
    events = [w[:3] for w in windows]

    def call(coeffs, t_ref, cell, keep):
        return landscape(model, events, coeffs, t_ref, cell, keep)[0]
    return call


# ---- the two-layer scenes of the search tests, built as examples/motion_segmentation.py builds its own ---------------------------------
SCENES = {1: ((64, 96), 3000, (1, 2), ((12.0, 3.0), (-6.0, -9.0))),
          2: ((64, 96), 3000, (3, 4), ((-10.0, 5.0), (7.0, 8.0))),
          3: ((96, 128), 5000, (5, 6), ((4.0, -12.0), (-9.0, 2.0)))}
SCENE_R = 2


def layered_window(synth, sensor, n_layer, seeds, flows):
    """One window of len(seeds) transparent layers merged by time: ((xs, ys, ts, edges, edge_ts), truth)"""
    H, W = sensor
    layers = [synth.make_window(seed, (H, W), n_layer, SCENE_R, flow=np.broadcast_to(np.array(v), (H, W, 2)).copy(), n_segments=8,
                                n_circles=2, jitter_px=0.3, noise_frac=0) for seed, v in zip(seeds, flows)]
    ts = np.concatenate([l['ts'] for l in layers])
    order = np.argsort(ts, kind='stable')
    xs = np.concatenate([l['xs'] for l in layers])[order]
    ys = np.concatenate([l['ys'] for l in layers])[order]
    edges = layers[0]['edges']
    for l in layers[1:]:
        edges = np.maximum(edges, l['edges'])
    return (xs, ys, ts[order], edges, layers[0]['edge_ts']), (order // n_layer).astype(np.uint8)


def scene(synth, k):
    sensor, n_layer, seeds, flows = SCENES[k]
    return layered_window(synth, sensor, n_layer, seeds, flows)[0], np.array(flows), sensor


def exact_layer(sensor, n_pix, flow, seed):
    """One layer whose stop is known by construction: n_pix distinct pixels, each seen at the five times 0, 1/4 .. 1 at exactly
    x0 + flow * (t - 1/2) (flow a multiple of 4: integers).  At the true flow, and at any candidate within 1 px of it (|dv| * |dt| <
    1/2 leaves every rint where it was), the five events of a pixel coincide at t_ref = 1/2: every count is 5, every event is explained
    and none remains.  Returns the 5-tuple window."""
    H, W = sensor
    vx, vy = flow
    assert vx % 4 == 0 and vy % 4 == 0
    mx, my = abs(vx) // 2, abs(vy) // 2
    pix = np.random.default_rng(seed).choice((H - 2 * my) * (W - 2 * mx), n_pix, replace=False)
    y0, x0 = pix // (W - 2 * mx) + my, pix % (W - 2 * mx) + mx
    t = np.repeat(np.arange(5) / 4.0, n_pix)
    xs = (np.tile(x0, 5) + vx * (t - 0.5)).astype(np.int16)
    ys = (np.tile(y0, 5) + vy * (t - 0.5)).astype(np.int16)
    return xs, ys, t, np.zeros((SCENE_R, H, W)), np.array([0.0, 1.0])
