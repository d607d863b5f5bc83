"""numpy witness of MVSEC's ground-truth flow: MVSECDataLoader.estimate_gt_flow / _prop_flow (src/dataloaders/mvsec_loader.py:322-433),
restated with the reference's dtypes under numpy >= 2.

The reference's cv.remap(flow, x, y, INTER_NEAREST) on float32 maps is here np.rint (round half to even, as cvRound) plus a range
check with a constant 0 border; a NaN coordinate reads 0.  Everything else keeps the reference's types: float32 pixel coordinates,
the remapped flow in the stack's own dtype, the scaled flow added to the float32 coordinates in float64 (numpy's in-place ``+=``
with a float64 operand) and cast back, the middle steps scaled by the Python float 1.0, the shift a float32 difference.  The
index arithmetic is written here independently of evaluation.gt_flow_plan."""
import numpy as np


def remap_nearest(src, cx, cy):
    """cv.remap(src, cx, cy, INTER_NEAREST), BORDER_CONSTANT 0: the output has src's dtype."""
    H, W = src.shape
    rx, ry = np.rint(cx), np.rint(cy)
    with np.errstate(invalid='ignore'):
        inside = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    out = np.zeros(cx.shape, dtype=src.dtype)
    out[inside] = src[ry[inside].astype(np.int64), rx[inside].astype(np.int64)]
    return out


def prop_flow(fx, fy, cx, cy, mx, my, scale):
    """_prop_flow: in-place update of the float32 coordinates and the two masks."""
    ix = remap_nearest(fx, cx, cy)
    iy = remap_nearest(fy, cx, cy)
    mx[ix == 0] = False
    my[iy == 0] = False
    cx += ix * scale
    cy += iy * scale


def estimate_gt_flow(gt_x, gt_y, gt_ts, t_start, t_end):
    """(H,W,2) float64 ground-truth flow of the window [t_start, t_end]; valid windows only (the reference's own behaviour)."""
    gt_ts = np.asarray(gt_ts, dtype=np.float64)
    t_start, t_end = np.float64(t_start), np.float64(t_end)
    i = np.searchsorted(gt_ts, t_start, side='right') - 1
    assert i >= 0
    interval = gt_ts[i + 1] - gt_ts[i]
    span = t_end - t_start
    lead = gt_ts[i + 1] - t_start
    if interval >= span and lead >= span:
        u = gt_x[i] * span / interval
        v = gt_y[i] * span / interval
        return np.stack([u, v], axis=-1).astype(np.float64)
    H, W = gt_x.shape[1:]
    cx, cy = np.meshgrid(np.arange(W), np.arange(H), indexing='xy')
    cx, cy = cx.astype(np.float32), cy.astype(np.float32)
    x0, y0 = cx.copy(), cy.copy()
    mx = np.ones((H, W), dtype=bool)
    my = np.ones((H, W), dtype=bool)
    prop_flow(gt_x[i], gt_y[i], cx, cy, mx, my, lead / interval)
    i += 1
    while gt_ts[i + 1] < t_end:
        prop_flow(gt_x[i], gt_y[i], cx, cy, mx, my, 1.0)
        i += 1
    prop_flow(gt_x[i], gt_y[i], cx, cy, mx, my, (t_end - gt_ts[i]) / (gt_ts[i + 1] - gt_ts[i]))
    u = cx - x0
    v = cy - y0
    u[~mx] = 0
    v[~my] = 0
    return np.stack([u, v], axis=-1).astype(np.float64)


def estimate_batch(gt_x, gt_y, gt_ts, t_starts, t_ends):
    return np.stack([estimate_gt_flow(gt_x, gt_y, gt_ts, a, b) for a, b in zip(t_starts, t_ends)])


def flow_from_plan(gt_x, gt_y, plan):
    """The (H,W,2) float64 flow of one evaluation.gt_flow_plan plan, walked with the functions above (every scale a numpy float64)."""
    mode, steps = plan
    if mode == 'direct':
        (f, num, den), = steps
        return np.stack([gt_x[f] * np.float64(num) / np.float64(den), gt_y[f] * np.float64(num) / np.float64(den)],
                        axis=-1).astype(np.float64)
    H, W = gt_x.shape[1:]
    cx, cy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    x0, y0 = cx.copy(), cy.copy()
    mx = np.ones((H, W), dtype=bool)
    my = np.ones((H, W), dtype=bool)
    for f, num, _ in steps:
        prop_flow(gt_x[f], gt_y[f], cx, cy, mx, my, np.float64(num))
    u = np.where(mx, cx - x0, np.float32(0))
    v = np.where(my, cy - y0, np.float32(0))
    return np.stack([u, v], axis=-1).astype(np.float64)


def random_sequence(seed, H, W, n_gt=40, nan_inf=False, big=False):
    """(gt_ts, gx, gy): non-uniform GT timestamps and float32 flows with zeros, half-integer ties, optionally NaN / inf and, with
    big, flows of a third of the sensor, which carry many pixels out of the frame."""
    rng = np.random.default_rng(seed)
    gt_ts = 1.5 + np.cumsum(rng.uniform(0.02, 0.08, n_gt))
    sigma = max(H, W) / 3.0 if big else 2.5
    gx = rng.normal(0, sigma, (n_gt, H, W)).astype(np.float32)
    gy = rng.normal(0, sigma, (n_gt, H, W)).astype(np.float32)
    gx[rng.random(gx.shape) < 0.05] = 0.0
    gy[rng.random(gy.shape) < 0.05] = 0.0
    ties = rng.random(gx.shape) < 0.03
    gx[ties] = 0.5 * rng.integers(-20, 20, int(ties.sum()))
    if nan_inf:
        gx[rng.random(gx.shape) < 0.002] = np.nan
        gy[rng.random(gy.shape) < 0.002] = np.inf
        gx[rng.random(gx.shape) < 0.002] = -np.inf
    return gt_ts, gx, gy


def random_windows(seed, gt_ts, n, dt_img):
    """n windows [img_ts[i], img_ts[i + dt_img]] of image timestamps denser than the GT's, inside the GT's span."""
    rng = np.random.default_rng(seed + 99)
    img_ts = np.cumsum(rng.uniform(0.02, 0.05, 4 * len(gt_ts))) + gt_ts[0]
    img_ts = img_ts[img_ts < gt_ts[-1]]
    i = rng.integers(0, len(img_ts) - dt_img, n)
    return img_ts[i], img_ts[i + dt_img]


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class FakeEngine:
    """Stands in for an Engine in the CPU tests: gt_flow(gt_x, gt_y, plans) walked by flow_from_plan; records every call's plans."""

    def __init__(self):
        self.calls = []

    def gt_flow(self, gt_x, gt_y, plans):
        self.calls.append(list(plans))
        return np.stack([flow_from_plan(np.asarray(gt_x), np.asarray(gt_y), p) for p in plans])
