"""The numpy witness of eincm_densify_motions, following the contract line by line: the sites from the summed
masses, the nearest site of every pixel by brute force over all sites with the key (d2, y', x'), the reach test, and the composition
from the site's masses and the models' fields at the pixel.  The mass, label, dominant and blend rules are
tests/_motion_layers_witness.py's, imported, not restated.  Every function returns what the device must return byte for byte."""
import numpy as np

import _motion_layers_witness as ML

NO_LABEL = ML.NO_LABEL
MD_NONE = 0xFFFFFFFF
MD_UNBOUNDED = 0xFFFFFFFF


def sites(mass, min_site_mass):
    """mass (K, H, W) uint32 -> (H, W) bool: the uint64 sum over the models reaches min_site_mass."""
    return mass.astype(np.uint64).sum(axis=0, dtype=np.uint64) >= np.uint64(min_site_mass)


def feature_transform(site):
    """site (H, W) bool -> (nearest (H, W) int32, dist2 (H, W) uint32): for every pixel the site of the smallest key
    d2 << 32 | y' << 16 | x' - the distance, then the lowest row, then the lowest column - over ALL sites; -1 and MD_NONE without one."""
    H, W = site.shape
    ys, xs = np.nonzero(site)
    if len(ys) == 0:
        return np.full((H, W), -1, dtype=np.int32), np.full((H, W), MD_NONE, dtype=np.uint32)
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    # key = d2 << 32 | y' << 16 | x' as int64: d2 < 2^31, so the signed order is the unsigned one.  One row of pixels at a time, every
    # site against every pixel; the part of the key that does not depend on the row, (x - x')^2 << 32 | y' << 16 | x', is made once.
    x_part = (((np.arange(W, dtype=np.int64)[:, None] - xs) ** 2) << 32) | (ys << 16) | xs                 # (W, n_sites)
    nearest, dist2 = np.empty((H, W), dtype=np.int32), np.empty((H, W), dtype=np.uint32)
    for y in range(H):
        k = (x_part + (((y - ys) ** 2) << 32)).min(axis=1)   # (the two squares add below bit 32's carry: the low half is untouched)
        dist2[y] = k >> 32
        nearest[y] = ((k >> 16) & 0xFFFF) * W + (k & 0xFFFF)
    return nearest, dist2


def densify(model, groups, coeffs, mode='hard', fallback='zero', min_site_mass=1, max_dist2=MD_UNBOUNDED, transforms=None):
    """groups: G entries (xs, ys, [K weight arrays or None]); coeffs (G * K, K_c).  Returns the dict of all five outputs, and 'mass'
    and 'total' beside them.  transforms: a dict the feature transforms are kept in between calls, keyed by (group, min_site_mass) -
    they do not depend on mode, fallback or max_dist2."""
    H, W = model.sensor_size
    G, K = len(groups), len(groups[0][2])
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(G, K, -1)
    mass = np.stack([ML.mass_images(xs, ys, ws, (H, W)) for xs, ys, ws in groups])
    total = mass.astype(np.uint64).sum(axis=(2, 3), dtype=np.uint64)
    theta = np.zeros((G, H, W, 2), dtype=np.float64)
    labels = np.zeros((G, H, W), dtype=np.uint8)
    nearest, dist2 = np.zeros((G, H, W), dtype=np.int32), np.zeros((G, H, W), dtype=np.uint32)
    n_sites = np.zeros(G, dtype=np.uint32)
    for g in range(G):
        site = sites(mass[g], min_site_mass)
        n_sites[g] = site.sum()
        if transforms is not None and (g, min_site_mass) in transforms:
            nearest[g], dist2[g] = transforms[(g, min_site_mass)]
        else:
            nearest[g], dist2[g] = feature_transform(site)
            if transforms is not None:
                transforms[(g, min_site_mass)] = (nearest[g].copy(), dist2[g].copy())
        reached = (nearest[g] >= 0) & (dist2[g].astype(np.int64) <= int(max_dist2))
        at = np.where(reached, nearest[g], 0).astype(np.int64)
        m_site = mass[g].reshape(K, H * W)[:, at.reshape(-1)].reshape(K, H, W)       # the mass vector of every pixel's nearest site
        labels[g] = np.where(reached, ML.label(m_site), np.uint8(NO_LABEL))
        f = model.field(coeffs[g])                             # (K, H, W, 2): the fields at the pixel itself
        if mode == 'hard':
            pick = np.where(reached, labels[g], 0).astype(np.int64)
            comp = np.take_along_axis(f, pick[None, :, :, None], axis=0)[0]
        else:
            comp = ML.soft_blend(np.where(reached[None], m_site, np.uint32(1)), f)
        d = ML.dominant(total[g]) if fallback == 'dominant' else -1
        hole = f[d] if d >= 0 else np.zeros((H, W, 2))
        theta[g] = np.where(reached[..., None], comp, hole)
    return dict(theta=theta, labels=labels, dist2=dist2, nearest=nearest, n_sites=n_sites, mass=mass, total=total)
