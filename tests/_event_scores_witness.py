"""The per-event scores (eincm_event_scores in include/eincm.h) stated in numpy float64, with the image stack F
taken as an input:

    s[r, e]    = sum over d in {-1,0,1}^2 of  k_{e,r}(d) * F_r[ wrap_drop(round(x'_{e,r}) + d) ]
    self[r, e] = sum over the undropped d of  k_{e,r}(d)^2

The warp, the rounding and the index rule are the oracle's (per_pix_warp, _round_i, _tap_index), the tap weight is the one of its
events_to_pdf_frame.  Beside the two outputs the witness returns, per output cell, the magnitude the tolerance of
tests/test_gpu_event_scores.py is relative to: M = sum_d k |F| for the scores, sum_d k^2 for selfs (each weighted by |omega_r| and
summed over r in the combined form), and how many of the nine taps were wrapped and dropped.

It also holds the case generators of tests/test_gpu_event_scores.py; tests/test_event_scores_interface.py asserts on the CPU that
every generated case exercises wrapped and dropped taps, positive scores and a theta that matters."""
import math

import numpy as np

from oracle import eincm_oracle as O

TOL = 1e-5              # |gpu - witness| <= TOL * M per cell: the project's standing fp32 bar (DESIGN.md sections 2 and 6)
NT = 256                # csrc/eincm_types.h: the block size of k_event_scores


def event_scores(F, Theta, xs, ys, ts, edge_ts, ref_weights=None):
    """F (R,H,W), Theta (H,W,2) at sensor size, the window's events, edge_ts (R,), ref_weights None or (R,).
    Returns a dict of (R, n) float64 arrays - or (n,) with ref_weights - 'scores', 'selfs', 'M', 'M_self', and the per-(r, e) integer
    arrays 'wrapped', 'dropped' (taps of the nine), 'ksum' (sum of k over all nine taps, dropped ones included), always (R, n)."""
    F = np.asarray(F, dtype=np.float64)
    R, H, W = F.shape
    edge_ts = np.atleast_1d(np.asarray(edge_ts, dtype=np.float64))
    assert edge_ts.shape == (R,)
    n = len(xs)
    s, q, M = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R, n))
    ksum = np.zeros((R, n))
    wrapped, dropped = np.zeros((R, n), dtype=np.int64), np.zeros((R, n), dtype=np.int64)
    for r in range(R):
        wx, wy = O.per_pix_warp(np.asarray(Theta, dtype=np.float64), xs, ys, ts, edge_ts[r], 1.0)
        rx, ry = O._round_i(wx), O._round_i(wy)
        for dy in (-1, 0, 1):              # the summation order the header states: rows, then columns within a row
            for dx in (-1, 0, 1):
                qx, qy = (rx + dx) - wx, (ry + dy) - wy
                k = np.exp(-0.5 * (qx * qx + qy * qy) - math.log(2.0 * math.pi))
                cs, vx = O._tap_index(rx, dx, W)
                rs, vy = O._tap_index(ry, dy, H)
                v = vx & vy
                f = np.zeros(n)
                f[v] = F[r][rs[v], cs[v]]
                s[r] += np.where(v, k * f, 0.0)
                M[r] += np.where(v, k * np.abs(f), 0.0)
                q[r] += np.where(v, k * k, 0.0)
                ksum[r] += k
                dropped[r] += ~v
                wrapped[r] += v & (((rx + dx) < 0) | ((ry + dy) < 0))
    out = {'wrapped': wrapped, 'dropped': dropped, 'ksum': ksum}
    if ref_weights is None:
        out.update(scores=s, selfs=q, M=M, M_self=q.copy())
        return out
    # (float)omega_r, as the kernel takes them
    w = np.asarray(ref_weights, dtype=np.float64).astype(np.float32).astype(np.float64)
    assert w.shape == (R,)
    out.update(scores=w @ s, selfs=w @ q, M=np.abs(w) @ M, M_self=np.abs(w) @ q)
    return out


def within(got, ref, M, tol=TOL):
    """(ok, largest |got - ref| / M over the cells with M > 0); cells with M == 0 must be exactly 0"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    zero = M == 0
    exact = bool(np.all(got[zero] == 0.0))
    ratio = float((np.abs(got - ref)[~zero] / M[~zero]).max()) if (~zero).any() else 0.0
    return exact and ratio <= tol, ratio


# ---- the generated cases --------------------------------------------------------------------------------------------------------------
# name -> (sensor, theta grid or None for a dense theta, R, n, seed).  The event counts straddle 64 (a wave) and NT (the block).
GENERATED = {
    '33x65-grid-r3': ((33, 65), (3, 5), 3, 300, 11),
    '33x65-grid-r1': ((33, 65), (3, 5), 1, 300, 12),
    '60x80-dense-r3': ((60, 80), None, 3, 700, 13),
    '60x80-dense-r1': ((60, 80), None, 1, 700, 14),
    '60x80-n1': ((60, 80), None, 3, 1, 15),
    '60x80-n63': ((60, 80), None, 3, 63, 16),
    '60x80-n64': ((60, 80), None, 3, 64, 17),
    '60x80-n65': ((60, 80), None, 3, 65, 18),
    '60x80-n255': ((60, 80), None, 1, NT - 1, 19),
    '60x80-n256': ((60, 80), None, 3, NT, 20),
    '60x80-n257': ((60, 80), None, 3, NT + 1, 21),
}
_cache = {}


def window(shape, n, R, seed, border=0.25):
    """A window of n time-sorted events, the first of every four (``border``) on the sensor's outermost rows and columns, and an edge
    stack in [0, 1]: (xs, ys, ts, edges, edge_ts)"""
    H, W = shape
    rng = np.random.default_rng(seed)
    xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
    nb = max(1, int(math.ceil(border * n)))
    side = rng.integers(0, 4, nb)
    xs[:nb] = np.where(side == 0, 0, np.where(side == 1, W - 1, xs[:nb]))
    ys[:nb] = np.where(side == 2, 0, np.where(side == 3, H - 1, ys[:nb]))
    perm = rng.permutation(n)
    xs, ys = xs[perm].astype(np.int16), ys[perm].astype(np.int16)
    ts = np.sort(rng.uniform(0.05, 0.95, n))
    edge_ts = np.linspace(0.0, 1.0, R) + 0.013 if R > 1 else np.array([0.013])
    edges = rng.uniform(0.0, 1.0, (R, H, W))
    edges[:, 0, 0], edges[:, -1, -1] = 0.0, 1.0          # (already min-max normalised)
    return xs, ys, ts, edges, edge_ts


def generated(name):
    """dict(shape, R, xs, ys, ts, edges, edge_ts, theta (h,w,2), stack (R,H,W) float32 signed random), read-only, made once"""
    if name not in _cache:
        shape, grid, R, n, seed = GENERATED[name]
        H, W = shape
        xs, ys, ts, edges, edge_ts = window(shape, n, R, seed)
        rng = np.random.default_rng(seed + 1000)
        theta = rng.uniform(-9.0, 9.0, (grid or shape) + (2,))
        stack = rng.uniform(-0.5, 1.0, (R, H, W)).astype(np.float32)          # signed, more often positive than not
        c = dict(shape=shape, R=R, xs=xs, ys=ys, ts=ts, edges=edges, edge_ts=edge_ts, theta=theta, stack=stack)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def sensor_theta(theta, shape, method='bilinear'):
    """theta at the sensor's size, as the oracle scales it"""
    theta = np.asarray(theta, dtype=np.float64)
    return theta if theta.shape[:2] == tuple(shape) else O.scale_theta_to_sensor_size(theta, tuple(shape), method)


def oracle_iwes(Theta, xs, ys, ts, edge_ts, shape):
    """(R,H,W) float64: the oracle's splat of the window under a sensor-size Theta"""
    return np.stack([O.events_to_pdf_frame(*O.per_pix_warp(Theta, xs, ys, ts, tau, 1.0), shape) for tau in np.atleast_1d(edge_ts)])


# ---- the example's window: signal events on moving edges plus a known set of uniform noise events, merged by time -----------------------
def noisy_window(synth, shape, n_signal, n_noise, R, seed=0, flow_mag=20.0):
    """(window dict as synth.make_window's with the noise merged in, is_noise bool (n,))"""
    win = synth.make_window(seed, shape, n_signal, R, flow='constant', flow_mag=flow_mag, noise_frac=0)
    H, W = shape
    rng = np.random.default_rng(seed + 4242)
    nx, ny = rng.integers(0, W, n_noise).astype(np.int16), rng.integers(0, H, n_noise).astype(np.int16)
    nt = rng.uniform(0.0, 1.0, n_noise)
    ts = np.concatenate([win['ts'], nt])
    order = np.argsort(ts, kind='stable')
    out = dict(win)
    out['xs'] = np.concatenate([win['xs'], nx])[order]
    out['ys'] = np.concatenate([win['ys'], ny])[order]
    out['ts'] = ts[order]
    is_noise = np.concatenate([np.zeros(n_signal, bool), np.ones(n_noise, bool)])[order]
    return out, is_noise
