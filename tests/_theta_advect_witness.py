"""Numpy and Python-int witness of the theta transport between windows, written for this repository.  It
restates the contract step by step, every float64 operation in the kernels' order, so the GPU result is compared byte for byte:

  expand    Theta = theta at the sensor's size: theta itself when dense, else ``_flow_error_witness.upsample`` (the tap order of
            k_flow_error) with the matrices of resample_matrix(h -> H) and (w -> W)
  splat     source (x, y) lands at q = (x + Theta_x tau, y + Theta_y tau), product and sum each rounded; nothing is deposited unless
            -1 < qx < W and -1 < qy < H.  x0 = floor(qx), ix = rint((qx - x0) 2^K) in [0, 2^K], likewise y; the four taps carry the
            integer weights (2^K - ix | ix) (2^K - iy | iy), which sum to 2^2K; taps outside the sensor are dropped.  Each adds
            (w, w Qx, w Qy), Q = rint(Theta 2^S), to the int64 planes Wacc, Uacc, Vacc
  resolve   c = Wacc 2^-2K.  Where c >= min_coverage: D = (float64(Uacc) / float64(Wacc)) 2^-S - Q(Theta) 2^-S; elsewhere D = 0
            ('source') or -Theta ('zero').  dense = Theta + D, coverage = float32(c)
  reduce    out = gain (theta + R(D)); R = ``upsample`` again with the matrices of resample_matrix(H -> h) and (W -> w): columns, then
            rows, ordered sums from +0.0.  For a dense theta R is the identity and is skipped: out = gain dense
``advect_exact`` is the unquantised float64 form of splat and resolve (real-valued weights and values, no difference trick).
The module also builds the fields the CPU and the GPU tests share (``case_fields``, ``converging_field``)."""
import importlib

import numpy as np

from _flow_error_witness import upsample

K, S = 10, 13                      # TA_K, TA_S of csrc/eincm_theta_advect.h
ONE = 1 << K
FULL = ONE * ONE
VALUE_STEP = 2.0 ** -S
COVERAGE_STEP = 2.0 ** -(2 * K)
THETA_MAX = 511.0
MAX_PIXELS = 1 << 21


def matrices(h, w, H, W, method):
    """(A_H (H, h), A_W (W, w), R_H (h, H), R_W (w, W)) from the library's own eincm_resample_matrix (host code: no GPU)."""
    E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    return (E.resample_matrix(h, H, method), E.resample_matrix(w, W, method), E.resample_matrix(H, h, method),
            E.resample_matrix(W, w, method))


def expand(theta, sensor, method):
    theta = np.asarray(theta, dtype=np.float64)
    H, W = sensor
    if theta.shape[:2] == (H, W):
        return theta.copy()
    A_H, A_W, _, _ = matrices(theta.shape[0], theta.shape[1], H, W, method)
    return upsample(theta, A_H, A_W)


def quantise(v):
    return np.rint(np.asarray(v, dtype=np.float64) * 2.0 ** S).astype(np.int64)


def landing(Theta, tau):
    """(ok (H, W), x0, y0, ix, iy) of every source pixel; the last four are meaningful where ok."""
    H, W = Theta.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all='ignore'):
        px, py = Theta[..., 0] * np.float64(tau), Theta[..., 1] * np.float64(tau)
        qx, qy = xs.astype(np.float64) + px, ys.astype(np.float64) + py
        ok = (qx > -1.0) & (qx < float(W)) & (qy > -1.0) & (qy < float(H))
        qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
    fx, fy = np.floor(qx), np.floor(qy)
    ix = np.rint((qx - fx) * float(ONE)).astype(np.int64)
    iy = np.rint((qy - fy) * float(ONE)).astype(np.int64)
    return ok, fx.astype(np.int64), fy.astype(np.int64), ix, iy


def splat(Theta, tau):
    """The three int64 planes, and the bookkeeping the case-property tests read: 'dropped' (taps of positive weight that fell outside
    the sensor), 'sources' (per pixel, the sources that added a positive weight), 'rejected' (sources that deposited nothing)."""
    H, W = Theta.shape[:2]
    ok, x0, y0, ix, iy = landing(Theta, tau)
    Q = quantise(Theta)
    Wacc, Uacc, Vacc = (np.zeros(H * W, dtype=np.int64) for _ in range(3))
    sources = np.zeros(H * W, dtype=np.int64)
    dropped = 0
    for dy in (0, 1):
        for dx in (0, 1):
            wt = (ix if dx else ONE - ix) * (iy if dy else ONE - iy)
            tx, ty = x0 + dx, y0 + dy
            live = ok & (wt > 0)
            inside = live & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            dropped += int((live & ~inside).sum())
            at = (ty * W + tx)[inside]
            np.add.at(Wacc, at, wt[inside])
            np.add.at(Uacc, at, (wt * Q[..., 0])[inside])
            np.add.at(Vacc, at, (wt * Q[..., 1])[inside])
            np.add.at(sources, at, 1)
    shape = (H, W)
    return {'W': Wacc.reshape(shape), 'U': Uacc.reshape(shape), 'V': Vacc.reshape(shape), 'dropped': dropped,
            'sources': sources.reshape(shape), 'rejected': int((~ok).sum()), 'Q': Q}


def resolve(Theta, acc, fill, min_coverage):
    """(D, dense, coverage float32, holes bool)."""
    c = acc['W'].astype(np.float64) * COVERAGE_STEP
    covered = c >= np.float64(min_coverage)
    dw = np.where(covered, acc['W'], 1).astype(np.float64)
    D = np.zeros_like(Theta)
    for k, plane in enumerate((acc['U'], acc['V'])):
        moved = plane.astype(np.float64) / dw * VALUE_STEP - acc['Q'][..., k].astype(np.float64) * VALUE_STEP
        hole = -Theta[..., k] if fill == 'zero' else np.zeros(Theta.shape[:2])
        D[..., k] = np.where(covered, moved, hole)
    return D, Theta + D, c.astype(np.float32), ~covered


def advect(theta, sensor, tau=1.0, gain=1.0, method='bilinear', fill='source', min_coverage=0.5):
    """One field.  Returns {'theta': (h, w, 2), 'dense': (H, W, 2), 'coverage': (H, W) float32, 'holes', 'acc', 'Theta'}."""
    theta = np.asarray(theta, dtype=np.float64)
    H, W = sensor
    Theta = expand(theta, sensor, method)
    acc = splat(Theta, tau)
    D, dense, cov, holes = resolve(Theta, acc, fill, min_coverage)
    if theta.shape[:2] == (H, W):
        out = np.float64(gain) * dense
    else:
        _, _, R_H, R_W = matrices(theta.shape[0], theta.shape[1], H, W, method)
        out = np.float64(gain) * (theta + upsample(D, R_H, R_W))
    return {'theta': out, 'dense': dense, 'coverage': cov, 'holes': holes, 'acc': acc, 'Theta': Theta}


def advect_batch(thetas, sensor, tau, gain, **kw):
    n = len(thetas)
    tau, gain = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(gain, dtype=np.float64), (n,))
    return [advect(thetas[b], sensor, tau[b], gain[b], **kw) for b in range(n)]


def advect_exact(Theta, tau, fill='source', min_coverage=0.5):
    """Steps 2 and 3 without any quantisation: float64 positions, weights and values.  Returns (dense (H, W, 2), coverage float64,
    spread (H, W): max - min of the values meeting at each pixel, per component the larger; n (H, W): the taps meeting there, those of
    weight 0 included)."""
    H, W = Theta.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    qx, qy = xs + Theta[..., 0] * tau, ys + Theta[..., 1] * tau
    ok = (qx > -1.0) & (qx < W) & (qy > -1.0) & (qy < H)
    qx, qy = np.where(ok, qx, 0.0), np.where(ok, qy, 0.0)
    fx, fy = np.floor(qx), np.floor(qy)
    ax, ay = qx - fx, qy - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    Wa, Ua, Va = (np.zeros(H * W) for _ in range(3))
    hi = np.full((H * W, 2), -np.inf)
    lo = np.full((H * W, 2), np.inf)
    n = np.zeros(H * W, dtype=np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            wt = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
            tx, ty = x0 + dx, y0 + dy
            inside = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            at = (ty * W + tx)[inside]
            np.add.at(n, at, 1)
            np.add.at(Wa, at, wt[inside])
            np.add.at(Ua, at, (wt * Theta[..., 0])[inside])
            np.add.at(Va, at, (wt * Theta[..., 1])[inside])
            np.maximum.at(hi, at, Theta[inside])
            np.minimum.at(lo, at, Theta[inside])
    c = Wa.reshape(H, W)
    covered = c >= min_coverage
    safe = np.where(covered, c, 1.0)
    hole = np.zeros_like(Theta) if fill == 'zero' else Theta
    dense = np.where(covered[..., None], np.stack([Ua.reshape(H, W) / safe, Va.reshape(H, W) / safe], axis=-1), hole)
    with np.errstate(invalid='ignore'):
        spread = np.where(np.isfinite(hi - lo), hi - lo, 0.0).max(axis=1).reshape(H, W)
    return dense, c, spread, n.reshape(H, W)


# -- fields the tests share ------------------------------------------------------------------------------------------------------------
SENSORS = ((37, 53), (70, 90))
SHAPES = ((1, 1), (2, 2), (3, 5), (16, 16), 'dense')
TAUS, GAINS = (1.0, 0.0, -0.75), (1.0, 1.0, 1.25)


def case_fields(sensor, shape, seed=0):
    """Three (h, w, 2) fields for one parity case (shape 'dense': the sensor's), to run with TAUS and GAINS.  Field 0: a translation
    (holes along two borders, taps dropped over the other two), a radial bump that spreads the middle apart (holes) and squeezes the
    ring around it (coverage above 1.5), one cell that flies further than 32 px, and noise.  Field 1: noise (it runs with tau = 0).
    Field 2: another translation and the same bump, which the negative tau turns into a sink (many sources on few pixels).  A 1x1 or
    2x2 theta has room for little more than the translations; the bump and the far cell need 3x5 cells or more."""
    H, W = sensor
    h, w = sensor if shape == 'dense' else shape
    rng = np.random.default_rng(1000 * seed + 37 * h + w)
    ys, xs = np.mgrid[0:h, 0:w]
    u = (xs + 0.5) / w - 0.5                      # cell centres in [-0.5, 0.5]
    v = (ys + 0.5) / h - 0.5
    bump = np.exp(-((u - 0.08) ** 2 + (v + 0.06) ** 2) / (2 * 0.15 ** 2))
    radial = np.stack([W * (u - 0.08) * bump, H * (v + 0.06) * bump], axis=-1)
    out = np.empty((3, h, w, 2))
    out[0] = np.array([5.25, -3.5]) + 1.5 * radial + rng.normal(0.0, 0.2, (h, w, 2))
    out[1] = rng.normal(0.0, 6.0, (h, w, 2))
    out[2] = np.array([-4.5, 6.25]) + 1.0 * radial + rng.normal(0.0, 0.2, (h, w, 2))
    if h * w >= 15:
        out[0, h // 4, w // 5] = (41.0, 3.0)      # (the far cell)
    return out


def converging_field(sensor, target=None):
    """A dense field whose every source lands, with tau = 1, inside the 2x2 block at ``target`` (x, y): H W sources on four pixels."""
    H, W = sensor
    tx, ty = (W // 2 + 0.25, H // 2 + 0.5) if target is None else target
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([tx - xs, ty - ys], axis=-1).astype(np.float64)


def smooth_random_field(sensor, seed, mag=6.0, cells=5):
    """A smooth random dense field: a (cells, cells) normal grid scaled up bilinearly by hand (no library call)."""
    H, W = sensor
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, mag, (cells, cells, 2))
    y = np.linspace(0, cells - 1, H)
    x = np.linspace(0, cells - 1, W)
    y0, x0 = np.minimum(y.astype(int), cells - 2), np.minimum(x.astype(int), cells - 2)
    fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
    return ((1 - fy) * (1 - fx) * g[y0][:, x0] + (1 - fy) * fx * g[y0][:, x0 + 1] + fy * (1 - fx) * g[y0 + 1][:, x0]
            + fy * fx * g[y0 + 1][:, x0 + 1])
