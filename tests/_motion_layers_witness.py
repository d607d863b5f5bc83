"""The numpy witness of eincm_compose_motions, following the contract line by line: the quantised weight, the
mass images by np.add.at on uint32, the totals, the label, MotionModel.field for the models' flows, and the soft blend written out in
its order.  Every function returns what the device must return byte for byte."""
import numpy as np

NO_LABEL = 255
Q_ONE = 4096


def q(w):
    """(uint32) rintf(w * 4096.0f): float32 product (exact: a power of two), half to even."""
    w = np.asarray(w, dtype=np.float32)
    return np.rint(w * np.float32(4096.0)).astype(np.uint32)


def label(mass):
    """mass (K, ...) uint32 -> the lowest l with the largest mass where that is > 0, else 255; uint8."""
    mass = np.asarray(mass)
    lab = np.argmax(mass, axis=0).astype(np.uint8)            # (the first of equal maxima: the lowest l)
    return np.where(mass.max(axis=0) > 0, lab, np.uint8(NO_LABEL)).astype(np.uint8)


def dominant(total):
    """total (K,) uint64 -> the lowest l with the largest total, or -1 if that total is 0."""
    total = np.asarray(total, dtype=np.uint64)
    d = int(np.argmax(total))
    return d if int(total[d]) > 0 else -1


def soft_blend(mass, f):
    """mass (K, ...) uint32 with a positive sum everywhere, f (K, ..., 2) -> Theta (..., 2): a_0 f_0, then + a_l f_l in order."""
    mass = np.asarray(mass)
    S = mass.astype(np.uint64).sum(axis=0).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        out = (mass[0].astype(np.float64) / S)[..., None] * f[0]
        for l in range(1, mass.shape[0]):
            out = out + (mass[l].astype(np.float64) / S)[..., None] * f[l]
    return out


def mass_images(xs, ys, weights, sensor_size):
    """One group: the events' pixels (n,), weights a list of K entries, each (n,) float32 or None (ones) -> (K, H, W) uint32."""
    H, W = sensor_size
    out = np.zeros((len(weights), H, W), dtype=np.uint32)
    y, x = np.asarray(ys).astype(np.int64), np.asarray(xs).astype(np.int64)
    for l, w in enumerate(weights):
        ql = np.full(len(x), Q_ONE, dtype=np.uint32) if w is None else q(w)
        np.add.at(out[l], (y, x), ql)
    return out


def compose(model, groups, coeffs, mode='hard', fill='zero'):
    """groups: G entries (xs, ys, [K weight arrays or None]); coeffs (G * K, K_c).  Returns the dict of all four outputs."""
    H, W = model.sensor_size
    G, K = len(groups), len(groups[0][2])
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(G, K, -1)
    mass = np.stack([mass_images(xs, ys, ws, (H, W)) for xs, ys, ws in groups])
    total = mass.astype(np.uint64).sum(axis=(2, 3), dtype=np.uint64)
    labels = np.stack([label(mass[g]) for g in range(G)])
    theta = np.zeros((G, H, W, 2), dtype=np.float64)
    for g in range(G):
        f = model.field(coeffs[g])                             # (K, H, W, 2)
        has = labels[g] != NO_LABEL
        if mode == 'hard':
            pick = np.where(has, labels[g], 0).astype(np.int64)
            comp = np.take_along_axis(f, pick[None, :, :, None], axis=0)[0]
        else:
            comp = soft_blend(np.where(has[None], mass[g], np.uint32(1)), f)     # (a pixel without mass: any positive sum, it is filled)
        d = dominant(total[g]) if fill == 'dominant' else -1
        hole = f[d] if d >= 0 else np.zeros((H, W, 2))
        theta[g] = np.where(has[..., None], comp, hole)
    return dict(theta=theta, labels=labels, mass=mass, total=total)
