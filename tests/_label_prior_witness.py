"""The numpy witness of eincm_label_prior and of the E-step with a prior image, following the contract line by
line: the mass images are _motion_layers_witness's, the box sum a summed-area table in uint64, lp_prior one float64 division and one
rounding to float32, and the spatial E-step _responsibilities_witness.responsibilities_f32's rule with the two changes of the
contract, every operation one numpy float32 operation in the stated order.  Every function returns what the device must return byte
for byte."""
import numpy as np

import _motion_layers_witness as ML

MAX_RADIUS = 8


def box_sum(mass, r):
    """mass (..., H, W) uint32 -> (..., H, W) uint64: the sum over the sensor pixels within r in both axes, by a summed-area table in
    uint64 (a sum of at most H * W masses below 2^32 each: exact while H * W < 2^32)."""
    m = np.asarray(mass).astype(np.uint64)
    H, W = m.shape[-2:]
    sat = np.zeros(m.shape[:-2] + (H + 1, W + 1), dtype=np.uint64)
    sat[..., 1:, 1:] = m.cumsum(axis=-2, dtype=np.uint64).cumsum(axis=-1, dtype=np.uint64)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r + 1, H)
    x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r + 1, W)
    a = sat[..., y1[:, None], x1[None, :]]
    b = sat[..., y0[:, None], x1[None, :]]
    c = sat[..., y1[:, None], x0[None, :]]
    d = sat[..., y0[:, None], x0[None, :]]
    return (a - b) - (c - d)                                     # (both differences are >= 0 and so is theirs: no wrap in uint64)


def lp_prior(S, floor_mass):
    """S (K, ...) uint64 -> (K, ...) float32: n_l = S_l + floor_mass, T = sum_l n_l, T == 0 ? 1 : float32(float64(n_l) / float64(T))."""
    n = np.asarray(S, dtype=np.uint64) + np.uint64(floor_mass)
    T = n.sum(axis=0, dtype=np.uint64)
    assert int(T.max(initial=0)) < 2 ** 53
    with np.errstate(invalid='ignore', divide='ignore'):
        p = (n.astype(np.float64) / T.astype(np.float64)[None]).astype(np.float32)
    return np.where((T == 0)[None], np.float32(1.0), p).astype(np.float32)


def label_prior(groups, sensor_size, radius, floor_mass):
    """groups: G entries (xs, ys, [K weight arrays or None]).  Returns dict(prior (G * K, H, W) float32, smoothed (G, K, H, W) uint64,
    mass (G, K, H, W) uint32)."""
    H, W = sensor_size
    mass = np.stack([ML.mass_images(xs, ys, ws, (H, W)) for xs, ys, ws in groups])
    smoothed = box_sum(mass, radius)
    prior = np.stack([lp_prior(smoothed[g], floor_mass) for g in range(len(groups))]).reshape(-1, H, W)
    return dict(prior=prior, smoothed=smoothed, mass=mass)


def responsibilities_spatial_f32(s, q, w, pi, P, exclude_self):
    """_responsibilities_witness.responsibilities_f32 with a prior per event and model.  s, q (K, n) float32; w (K, n) float32 or None
    (ones); pi (K,) numbers or None (ones); P (K, n) float32: the prior stack at each window's own event pixels.  Returns
    dict(weights (K, n) float32, labels (n,) uint8, unsupported (n,) bool, fallback (n,) uint8: 0 none, 1 the c_l shares, 2 the pi_l)."""
    f = np.float32
    s, q, P = np.asarray(s, dtype=f), np.asarray(q, dtype=f), np.asarray(P, dtype=f)
    K, n = s.shape
    pi32 = np.ones(K, dtype=f) if pi is None else np.asarray(pi, dtype=np.float64).astype(f)

    def total(p):
        T = np.zeros(n, dtype=f)
        for l in range(K):
            T = np.add(T, p[l], dtype=f)
        return T

    def bad(T):
        return ~(T > f(0)) | ~np.isfinite(T)

    with np.errstate(all='ignore'):
        if exclude_self:
            wq = q.copy() if w is None else np.multiply(np.asarray(w, dtype=f), q, dtype=f)
            a = np.subtract(s, wq, dtype=f)
        else:
            a = s.copy()
        a = np.where(a > f(0), a, f(0)).astype(f)
        c = np.multiply(pi32[:, None], P, dtype=f)
        p = np.multiply(c, a, dtype=f)
        T = total(p)
        uns = bad(T)
        p = np.where(uns[None, :], c, p).astype(f)
        T = np.where(uns, total(p), T).astype(f)
        second = uns & bad(T)
        p = np.where(second[None, :], np.broadcast_to(pi32[:, None], (K, n)), p).astype(f)
        T = np.where(second, total(p), T).astype(f)
        labels = np.zeros(n, dtype=np.uint8)
        best = p[0].copy()
        for l in range(1, K):
            up = p[l] > best
            best = np.where(up, p[l], best)
            labels[up] = l
        weights = np.divide(p, T[None, :], dtype=f)
    return dict(weights=weights, labels=labels, unsupported=uns, fallback=uns.astype(np.uint8) + second.astype(np.uint8))


def prior_at_events(prior, windows):
    """prior (K, H, W), windows: K (xs, ys) pairs of equal length -> (K, n) float32: P[l, y_e, x_e] at each window's own events."""
    return np.stack([np.asarray(prior[l], dtype=np.float32)[np.asarray(ys).astype(np.int64), np.asarray(xs).astype(np.int64)]
                     for l, (xs, ys) in enumerate(windows)])
