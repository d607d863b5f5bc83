"""The numpy witness of eincm_carry_label_prior, following the contract line by line: the mass images are
_motion_layers_witness's, every model's displacement MotionModel.field of its own coefficients, the landing and the four integer tap
weights _theta_advect_witness.landing's, the deposit np.add.at on uint64, the resolve rule written out in uint64, and the prior
_label_prior_witness's box sum and lp_prior on what arrived.  Every function returns what the device must return byte for byte."""
import numpy as np

import _label_prior_witness as LP
import _motion_layers_witness as ML
import _theta_advect_witness as TA

SHIFT = 2 * TA.K                   # LC_SHIFT of csrc/eincm_label_carry.h
FULL = TA.FULL                     # LC_FULL: what the four taps of a source sum to
HALF = FULL >> 1
CARRIED_MAX = 2 ** 32 - 1
EVENTS_MAX = 2 ** 32 - 1           # LC_EVENTS_MAX: the largest n with FULL * 4096 * n < 2^64


def resolve(accum):
    """uint64 -> uint32: min((A + 2^19) >> 20, 2^32 - 1) in uint64.  Where the sum would wrap (A > 2^64 - 1 - 2^19, far above the
    first saturating value) the result is the saturated one, so the rule holds for every uint64."""
    a = np.asarray(accum, dtype=np.uint64)
    wraps = a > np.uint64(2 ** 64 - 1 - HALF)
    c = (np.where(wraps, np.uint64(0), a) + np.uint64(HALF)) >> np.uint64(SHIFT)
    return np.where(wraps, np.uint64(CARRIED_MAX), np.minimum(c, np.uint64(CARRIED_MAX))).astype(np.uint32)


def splat(mass, Theta, tau):
    """One (group, model): mass (H, W) uint32, Theta (H, W, 2) -> dict(accum (H, W) uint64, dropped (Python int), and the bookkeeping
    the case-property tests read: 'sources' (H, W), how many sources added to a pixel; 'partial', the sources with mass that landed in
    row or column -1 and still deposited; 'taps_dropped', the taps of positive weight and mass that fell off the sensor; 'rejected',
    the sources with mass that deposited nothing)."""
    H, W = mass.shape
    ok, x0, y0, ix, iy = TA.landing(Theta, tau)
    m = mass.astype(np.uint64)
    has = mass > 0
    accum = np.zeros(H * W, dtype=np.uint64)
    sources = np.zeros(H * W, dtype=np.int64)
    rejected = has & ~ok
    dropped = int(m[rejected].sum(dtype=np.uint64)) * FULL
    taps_dropped, deposited = 0, np.zeros((H, W), dtype=bool)
    for dy in (0, 1):
        for dx in (0, 1):
            wt = (ix if dx else TA.ONE - ix) * (iy if dy else TA.ONE - iy)
            tx, ty = x0 + dx, y0 + dy
            live = ok & has & (wt > 0)
            inside = live & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            d = m * wt.astype(np.uint64)
            dropped += sum(int(v) for v in d[live & ~inside])
            taps_dropped += int((live & ~inside).sum())
            deposited |= inside
            at = (ty * W + tx)[inside]
            np.add.at(accum, at, d[inside])
            np.add.at(sources, at, 1)
    partial = int((deposited & ok & has & ((x0 == -1) | (y0 == -1))).sum())
    return dict(accum=accum.reshape(H, W), dropped=dropped, sources=sources.reshape(H, W), partial=partial, taps_dropped=taps_dropped,
                rejected=int(rejected.sum()))


def carry(model, groups, coeffs, tau, radius, floor_mass):
    """groups: G entries (xs, ys, [K weight arrays or None]); coeffs (G * K, K_c); tau a number or (G,).  Returns dict(prior
    (G * K, H, W) float32, carried (G, K, H, W) uint32, accum (G, K, H, W) uint64, dropped (G, K) uint64, mass (G, K, H, W) uint32,
    info: G lists of K splat() dicts)."""
    H, W = model.sensor_size
    G, K = len(groups), len(groups[0][2])
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(G, K, -1)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (G,))
    mass = np.stack([ML.mass_images(xs, ys, ws, (H, W)) for xs, ys, ws in groups])
    accum = np.zeros((G, K, H, W), dtype=np.uint64)
    dropped = np.zeros((G, K), dtype=np.uint64)
    info = []
    for g in range(G):
        with np.errstate(all='ignore'):
            f = model.field(coeffs[g])                         # (K, H, W, 2)
        info.append([splat(mass[g, l], f[l], tau[g]) for l in range(K)])
        for l in range(K):
            accum[g, l] = info[g][l]['accum']
            dropped[g, l] = np.uint64(info[g][l]['dropped'])
    carried = resolve(accum)
    return dict(prior=prior_of(carried, radius, floor_mass), carried=carried, accum=accum, dropped=dropped, mass=mass, info=info)


def prior_of(carried, radius, floor_mass):
    """carried (G, K, H, W) uint32 -> (G * K, H, W) float32: the label prior's box sum and shares on the masses that arrived."""
    G, _, H, W = carried.shape
    return np.stack([LP.lp_prior(LP.box_sum(carried[g], radius), floor_mass) for g in range(G)]).reshape(-1, H, W)


# ---- the saturation case the CPU and the GPU tests share ----
SAT_SENSOR, SAT_TARGET, SAT_PER_TILE = (40, 72), (36, 20), 600000


def saturation_case(motion):
    """One group of one model: 2 x 600 000 unit-weight events in two source tiles (each below the 2^20 a tile may hold), and a zoom
    field that takes every pixel of the sensor exactly onto SAT_TARGET after tau = 1: with the centre on the target pixel and a scale
    of 32, u = (x - cx) / 32 is exact, so is f_x = -32 u = cx - x, and x + f_x = cx with both fractions 0.  Returns (model, window
    (xs, ys, ts, edges, edge_ts), coeffs (1, 4), tau)."""
    H, W = SAT_SENSOR
    model = motion.MotionModel('similarity', SAT_SENSOR, centre=SAT_TARGET, scale=32.0)
    rng = np.random.default_rng(77)
    n = SAT_PER_TILE
    xs = np.concatenate([rng.integers(0, 32, n), rng.integers(32, 64, n)]).astype(np.int16)
    ys = np.concatenate([rng.integers(0, 32, n), rng.integers(0, 32, n)]).astype(np.int16)
    window = (xs, ys, np.linspace(0.0, 1.0, 2 * n), np.ones((1, H, W)), np.array([0.5]))
    return model, window, np.array([[0.0, 0.0, -32.0, 0.0]]), 1.0
