"""Randomised sweeps of the HIP loss/grad path against fp64 references (dev script; run on the GPU box).

Draws sensor sizes, event counts, reference counts, theta shapes, resampling methods, weights, pyramid levels, contrast kinds
and flow magnitudes (including flows that throw most events out of the frame), batches windows of different sizes in one
context, and reports the worst relative errors.  Five sweeps:
  default   draw_case        the fp32 engine against the fp64 oracle
  --fp64    draw_case_fp64   the float64 mode against the oracle: value, gradient, IWE and dL/dIWE at 1e-10 / 1e-9 / 1e-11 / 1e-10
  --kinds   draw_case_kinds  the selectable objective kinds and tile sizes against the fp64 autograd witness
                             (tests/_objective_kinds_witness.py): value, gradient, dL/dIWE and the two mean relative terms at 1e-5
  --motion  draw_case_motion  the motion models (every kind, custom matrices, drawn centres and scales, fields of 0..200 px, ragged and
                             many source tiles, masks) on the expanded path against fp64 at 1e-5, and the fused path against the
                             expanded one: value and IWE stack bit for bit, the gradient within tests/_motion_bounds.py's bound
  --weights draw_case_weights per-event weights (None, ones, {0} u [1/8, 1], k/4, all zero, mixed in a batch) on every theta kind,
                             resampling method and objective kind against tests/_event_weights_witness.py: value, gradient, IWE
                             stack and dL/dIWE at 1e-5, count images bit for bit, ones = None and all-zero = empty
usage: python tests/dev/fuzz_gpu.py [n_cases] [seed] [--fp64 | --kinds | --motion | --weights]
"""
import argparse
import importlib
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
from oracle import eincm_oracle as O    # noqa: E402
import _event_weights_witness as EW     # noqa: E402
import _motion_bounds as MB             # noqa: E402
import _objective_kinds_witness as WIT  # noqa: E402
import _splat_window_witness as SW      # noqa: E402

pkg = 'edge-informed-contrast-maximization_amd'
synth = importlib.import_module(pkg + '.synth')
engine = importlib.import_module(pkg + '.engine')
motion = importlib.import_module(pkg + '.motion')

METHODS = ['bilinear', 'lanczos3', 'lanczos5', 'cubic']
N_CHOICES = [0, 1, 7, 300, 5000, 40000]
# per sweep: the tolerance of each measured error (max-norm relative; the value and gradient after the conditioning rules of run_case)
TOLS = {'fp32': dict(value=1e-5, grad=1e-5),
        'fp64': dict(value=1e-10, grad=1e-9, iwe=1e-11, G=1e-10),
        'kinds': dict(value=1e-5, grad=1e-5, G=1e-5, corr=1e-5, contrast=1e-5),
        'motion': dict(value=1e-5, grad=1e-5),
        'weights': dict(value=1e-5, grad=1e-5, iwe=1e-5, G=1e-5)}
# the relative rounding unit of the engine's images, on which the gradient's conditioning floor is built
IMAGE_EPS = {'fp32': 6e-8, 'fp64': 2.2e-16}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def draw_case(rng):
    lo, hi_h, hi_w = (3, 9, 9) if os.environ.get('EINCM_FUZZ_TINY') else (6, 200, 260)      # EINCM_FUZZ_TINY=1: 3..8 px sensors
    H = int(rng.integers(lo, hi_h)); W = int(rng.integers(lo, hi_w))
    R = int(rng.integers(1, 7))
    B = int(rng.integers(1, 4))
    kind = rng.choice(['2dof', 'coarse', 'coarse', 'dense'])
    if kind == '2dof':
        hw = (1, 1)
    elif kind == 'coarse':
        hw = (int(rng.integers(1, min(H, 17) + 1)), int(rng.integers(1, min(W, 17) + 1)))
    else:
        hw = (H, W)
    method = 'bilinear' if kind == 'dense' else str(rng.choice(['bilinear', 'lanczos3', 'lanczos5', 'cubic']))
    mag = float(rng.choice([0.0, 2.0, 10.0, 40.0, 200.0]))
    return dict(H=H, W=W, R=R, B=B, hw=hw, method=method, mag=mag,
                N=[int(rng.choice([0, 1, 7, 300, 5000, 40000])) for _ in range(B)],
                alpha=float(rng.choice([0.0, 20.0, 1.0])), beta=float(rng.choice([0.0, 35.0, 1.0])),
                gamma=float(rng.choice([0.0, 2.5e-4, 0.1])), delta=float(rng.choice([0.0, 0.0, 0.5])),
                lvl=int(rng.choice([0, 0, 2, 4])), ck=int(rng.integers(0, 2)), flow=str(rng.choice(['constant', 'smooth', 'zero'])))


def _loss_terms(rng):
    return dict(alpha=float(rng.choice([0.0, 20.0, 1.0])), beta=float(rng.choice([0.0, 35.0, 1.0])),
                gamma=float(rng.choice([0.0, 2.5e-4, 0.1])), delta=float(rng.choice([0.0, 0.0, 0.5])),
                lvl=int(rng.choice([0, 0, 2, 4])), mag=float(rng.choice([0.0, 2.0, 10.0, 40.0, 200.0])),
                flow=str(rng.choice(['constant', 'smooth', 'zero'])))


def _theta_shape(rng, H, W, kinds):
    """(theta kind, (h, w), method): 'finer' is a grid finer than the sensor in one axis (at most H * W cells)"""
    kind = str(rng.choice(kinds))
    if kind == '2dof':
        hw = (1, 1)
    elif kind == 'coarse':
        hw = (int(rng.integers(1, min(H, 17) + 1)), int(rng.integers(1, min(W, 17) + 1)))
    elif kind == 'dense':
        hw = (H, W)
    else:
        if rng.random() < 0.5:
            h = H + int(rng.integers(1, 5))
            hw = (h, int(rng.integers(1, max(1, min(W - 1, H * W // h)) + 1)))
        else:
            w = W + int(rng.integers(1, 5))
            hw = (int(rng.integers(1, max(1, min(H - 1, H * W // w)) + 1)), w)
    method = 'bilinear' if kind == 'dense' else str(rng.choice(METHODS))
    return kind, hw, method


def draw_case_fp64(rng):
    """A case of the float64 sweep: sensors 3..200 px (a third of them 3..8 px), 1..16 reference times, 1..5 windows of
    0..40000 events, 2-DoF / coarse / dense / finer-than-sensor theta, every resampling method and loss term, ck 0 or 1."""
    hi = 9 if rng.random() < 1.0 / 3.0 else 201
    H = int(rng.integers(3, hi)); W = int(rng.integers(3, hi))
    R = int(rng.integers(1, 17))
    B = int(rng.integers(1, 6))
    kind, hw, method = _theta_shape(rng, H, W, ['2dof', 'coarse', 'coarse', 'dense', 'finer'])
    c = dict(H=H, W=W, R=R, B=B, theta=kind, hw=hw, method=method, N=[int(rng.choice(N_CHOICES)) for _ in range(B)],
             ck=int(rng.integers(0, 2)))
    c.update(_loss_terms(rng))
    return c


TILE_KINDS = ['ragged', 'ragged', 'side1', 'side2', 'sensor', 'many', 'any']


def _ragged(rng, n):
    """a tile side in 1..n that leaves a remainder when there is one to leave"""
    sides = [t for t in range(1, n + 1) if n % t] or list(range(1, n + 1))
    return int(rng.choice(sides))


def _tile_of(rng, tk, H, W):
    """a (tile_h, tile_w) of kind tk (one of TILE_KINDS) on an H x W sensor; 'many' needs H, W >= 9"""
    if tk == 'ragged':
        return (_ragged(rng, H), _ragged(rng, W))
    if tk in ('side1', 'side2'):
        s = 1 if tk == 'side1' else 2
        return (s, _ragged(rng, W)) if rng.random() < 0.5 else (_ragged(rng, H), s)
    if tk == 'sensor':
        return (H, W)
    if tk == 'many':            # at least 9 x 9 whole tiles
        return (int(rng.integers(1, H // 9 + 1)), int(rng.integers(1, W // 9 + 1)))
    return (int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1)))


def draw_case_kinds(rng):
    """A case of the objective-kinds sweep: ck 0..3 and rk 0..3 (at least one of them not a default kind), a tile of one of
    TILE_KINDS (ragged remainders, a side of 1 or 2, tile = sensor, more than 64 cells), sensors 6..260 px, 1..16 reference times,
    1..5 windows."""
    tk = str(rng.choice(TILE_KINDS))
    lo = 24 if tk == 'many' else 6
    H = int(rng.integers(lo, 200)); W = int(rng.integers(lo, 261))
    R = int(rng.integers(1, 17))
    B = int(rng.integers(1, 6))
    ck, rk = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    if ck < 2 and rk == 0:
        rk = int(rng.integers(1, 4))
    tile = _tile_of(rng, tk, H, W)
    kind, hw, method = _theta_shape(rng, H, W, ['2dof', 'coarse', 'coarse', 'dense'])
    c = dict(H=H, W=W, R=R, B=B, theta=kind, hw=hw, method=method, N=[int(rng.choice(N_CHOICES)) for _ in range(B)],
             ck=ck, rk=rk, tile=tile, tile_kind=tk)
    c.update(_loss_terms(rng))
    return c


def n_cells(c):
    return (c['H'] // c['tile'][0]) * (c['W'] // c['tile'][1])


def _rel_img(a, b):
    """max-norm relative error of an image stack; 0 when both are zero, and 0 for a non-finite reference (the handling of
    non-finite references: the value and gradient checks see those cases)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.all(np.isfinite(b)):
        return 0.0
    if np.abs(b).max(initial=0.0) == 0.0:
        return 0.0 if np.abs(a).max(initial=0.0) == 0.0 else np.inf
    return rel(a, b)


def _rel_scalar(a, b):
    if not np.isfinite(b):
        return 0.0 if not np.isfinite(a) else np.inf
    return abs(a - b) / max(abs(b), 1e-300) if b != 0.0 else abs(a)


def loss_term_sizes(c, aux):
    """the four terms of the value, each with its weight (a reference's aux / terms dict)"""
    return [c['alpha'] * aux.get('mean_rel_contrast', 0.0), c['beta'] * aux.get('mean_rel_corr', 0.0),
            c['gamma'] * aux.get('theta_total_variation', 0.0), c['delta'] * aux.get('mean_rel_iwe_divergence', 0.0)]


def value_error(v, v_ref, terms):
    """The error of a value in units of its conditioning scale (every sweep's rule).
    The value is a signed sum of terms (-alpha*contrast - beta*corr + gamma*TV + delta*div) that can cancel (tiny sensor, one event:
    -0.18152 + 0.18121); its error is measured against the size of the terms, each of which carries the images' accuracy.  A
    non-finite reference asks for a non-finite value."""
    vscale = max(abs(v_ref), sum(abs(t) for t in terms if np.isfinite(t))) if np.isfinite(v_ref) else 1.0
    ev = abs(v - v_ref) / max(vscale, 1e-300) if np.isfinite(v_ref) else (0.0 if not np.isfinite(v) else np.inf)
    if np.isfinite(v_ref) and vscale < 1e-12:
        ev = abs(v - v_ref)
    return ev


def grad_is_checked(g_ref):
    """whether grad_error compares a gradient with this reference at all: a finite reference that is not zero"""
    return bool(np.all(np.isfinite(g_ref)) and np.abs(g_ref).max() > 1e-200)


def grad_error(g, g_ref, G_ref, n, R, tol_g, image_eps, amp=1.0):
    """The max-norm relative error of a gradient in units of max(1, its conditioning floor / tol_g) (every sweep's rule).  n: the
    window's events (of weight > 0); G_ref: the reference's dL/dIWE; image_eps: the rounding unit of the engine's images.
    amp: the largest factor between an event's term in dL/dTheta and its term in this gradient (1 for a theta grid, whose resampling
    weights are at most ~1; for the coefficients of a motion model max_k sum_j |M_jk| max|m_j|, since dL/dc_k = sum_e sum_j M_jk
    m_j(p_e) dL/dTheta(p_e)) - it carries kappa and the floor, both built on the size of the cancelling terms, into the units of g."""
    gmax = np.abs(g_ref).max()
    eg = rel(g, g_ref) if (np.all(np.isfinite(g_ref)) and gmax > 1e-200) else (0.0 if gmax <= 1e-200 and np.abs(g).max() < 1e-12 else
                                                                            (0.0 if not np.all(np.isfinite(g_ref)) else np.inf))
    # Conditioning of the gradient: every event contributes terms of size ~ max|dL/dIWE| that cancel down to max|g_ref|.  With a
    # handful of events the arg-max term of the normalisation can make that ratio 1e13 (one event: max|G| 8.5e11, max|g| 0.036), and
    # then fp64 itself - the reference included - resolves the gradient only to ratio * 2.2e-16.  The error is reported in units of
    # max(the usual tolerance scale, that floor).
    if np.all(np.isfinite(g_ref)) and gmax > 1e-200 and np.all(np.isfinite(G_ref)):
        kappa = 2.15 * np.abs(G_ref).max() * max(n, 1) * R / gmax * amp
        # the engine stores dL/dIWE as an image of its precision (fp32: 6e-8 per pixel; fp64: 2.2e-16): with a handful of events
        # nothing averages that out (one event on a 5x6 sensor: max|g| 6.7e-4 under max|G| ~ 0.1); with many events the pixel
        # errors add incoherently
        nb = max(n, 1)
        g_level = np.abs(G_ref).max() if nb <= 16 else np.sqrt(np.mean(np.square(G_ref))) * np.sqrt(nb)
        floor = 2.15 * image_eps * np.sqrt(9.0 * R) * g_level / gmax * amp
        eg = eg / max(1.0, kappa * 2.2e-16 / tol_g, floor / tol_g)
    return eg


def run_case(c, seed, precision='fp32', kinds=None):
    """Evaluate case c (a draw_case* dict) on the engine and compare every window with its fp64 reference.
    precision 'fp32' / 'fp64'; kinds None (the oracle) or (ck, rk, tile) (the objective-kinds witness; fp32 only).
    Returns (value err, grad err, counts bit-exact) for the default sweep, else a dict of the worst errors
    (value, grad, and iwe / G for fp64, G / corr / contrast for kinds) and 'counts' (bool)."""
    H, W, R, B = c['H'], c['W'], c['R'], c['B']
    rng = np.random.default_rng(seed)
    wins, thetas = [], []
    for b in range(B):
        n = c['N'][b]
        win = synth.make_window(seed + b, (H, W), max(n, 1), R, flow=c['flow'], flow_mag=max(c['mag'], 1e-3))
        for k in ('xs', 'ys', 'ts'):
            win[k] = win[k][:n]
        wins.append(win)
        h, w = c['hw']
        base = win['flow_gt'] if (h, w) == (H, W) else np.broadcast_to(win['flow_gt'].mean(axis=(0, 1)), (h, w, 2))
        thetas.append(base * rng.uniform(0.5, 1.5, (h, w, 2)) + rng.normal(0, 0.5, (h, w, 2)))
    thetas = np.stack(thetas)
    value_only = c['mag'] == 0.0 and c['flow'] == 'zero'      # theta = 0 exactly: the gradient cancels by symmetry (ill-conditioned)
    if value_only:
        thetas[:] = 0.0
    args = lambda w: (w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts'])   # noqa: E731
    mode = 'kinds' if kinds is not None else precision
    ck, rk, tile = kinds if kinds is not None else (c['ck'], 0, None)
    with engine.Engine((H, W), max(sum(c['N']), 1), max_refs=R, max_windows=B, precision=precision) as eng:
        eng.set_windows([args(w) for w in wins])
        if tile is not None:
            eng.set_objective_tiles(tile)
        p = engine.make_params(c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'], c['method'], ck, correlation_kind=rk)
        v, g, aux_e = eng.loss_grad(thetas, p, want_aux=mode == 'kinds')
        iwes = eng.iwes() if mode == 'fp64' else None
        G_e = eng.image_grad() if mode != 'fp32' else None      # (before count_images, which reuses the fp32 dL/dIWE buffer)
        counts = eng.count_images() if hasattr(eng, 'count_images') else None
    worst = dict(value=0.0, grad=0.0, counts=True)
    worst.update({'fp64': dict(iwe=0.0, G=0.0), 'kinds': dict(G=0.0, corr=0.0, contrast=0.0)}.get(mode, {}))
    tol_g = TOLS[mode]['grad']
    for b in range(B):
        if mode == 'kinds':
            h, w = c['hw']
            AH = O.resample_matrix(h, H, H / h, c['method'])
            AW = O.resample_matrix(w, W, W / w, c['method'])
            v_ref, g_ref, G_ref, aux = WIT.loss_and_grad(thetas[b], *args(wins[b]), c['alpha'], c['beta'], c['gamma'], c['delta'],
                                                         c['lvl'], AH, AW, ck, rk, tile)
        else:
            v_ref, g_ref, aux = O.loss_and_grad(thetas[b], *args(wins[b]), c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'], 5,
                                                (H, W), c['method'], contrast_kind=c['ck'], return_intermediates=True)
            G_ref = aux['_G']
        ev = value_error(v[b], v_ref, loss_term_sizes(c, aux))
        eg = grad_error(g[b], g_ref, G_ref, c['N'][b], R, tol_g, IMAGE_EPS[precision])
        errs = dict(value=ev, grad=0.0 if value_only else eg)
        # at theta = 0 the IWE is mirror-symmetric about each event, so |div n| sits at exact zeros whose sign (its subgradient in
        # dL/dIWE) follows the last bit of the summation order: dL/dIWE is not defined there by more than that sign
        e_G = 0.0 if (value_only and c['delta'] != 0.0) else _rel_img(G_e[b], G_ref) if G_e is not None else 0.0
        if mode == 'fp64':
            errs.update(iwe=_rel_img(iwes[b], aux['_iwes']), G=e_G)
        elif mode == 'kinds':
            errs.update(G=e_G, corr=_rel_scalar(aux_e[b]['mean_rel_corr'], aux['mean_rel_corr']),
                        contrast=_rel_scalar(aux_e[b]['mean_rel_contrast'], aux['mean_rel_contrast']))
        ok_cnt = True
        if counts is not None:
            Theta = O.scale_theta_to_sensor_size(thetas[b], (H, W), c['method'])
            for r in range(R):
                wx, wy = O.per_pix_warp(Theta, wins[b]['xs'], wins[b]['ys'], wins[b]['ts'], wins[b]['edge_ts'][r])
                ok_cnt &= np.array_equal(counts[b, r], O.rounded_count_image(wx, wy, (H, W)))
        if os.environ.get('EINCM_FUZZ_VERBOSE'):
            print(f'   window {b}: N {c["N"][b]} ' + ' '.join(f'{k} err {e:.2e}' for k, e in errs.items())
                  + f' max|g_ref| {np.abs(g_ref).max():.3e} max|g - g_ref| {np.abs(g[b] - g_ref).max():.3e}')
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
        worst['counts'] = worst['counts'] and bool(ok_cnt)
    if mode == 'fp32':
        return worst['value'], worst['grad'], worst['counts']
    return worst


# ---- the motion-model sweep (DESIGN.md sections 20 and 21) ------------------------------------------------------------------------
MOTION_KINDS = list(motion.KINDS)
MOTION_MAGS = [0.0, 2.0, 10.0, 40.0, 200.0]
MOTION_N = [n for n in N_CHOICES if n != 40000]            # the 40000-event window is placed, once per sweep
# a window without events, or with none of weight > 0, checks no gradient: such windows are drawn, but less often than the others
P_MOTION_N = [0.08, 0.23, 0.23, 0.23, 0.23]
P_N_CHOICES = [0.08, 0.184, 0.184, 0.184, 0.184, 0.184]
# sensors by the case's index in its sweep: a third 3..8 px, and the shapes the fused kernels' tile code can go wrong at
SENSOR_STRATA = ['tiny', 'ragged4x4', 'narrow', 'tiny', 'mult32', 'two_segments', 'tiny', 'any', 'any', 'tiny', 'any', 'any']
_REFS = {}                                                  # (sweep, seed, case) -> the fp64 references of the case, once per process


def _motion_sensor(rng, stratum):
    if stratum == 'tiny':
        return int(rng.integers(3, 9)), int(rng.integers(3, 9))
    if stratum == 'ragged4x4':                              # at least 4 x 4 source tiles of 32 px, a remainder in both axes
        return tuple(int(rng.choice([n for n in range(97, 201) if n % 32])) for _ in range(2))
    if stratum == 'narrow':                                 # one row of tiles, shorter than a tile: H < 32 <= W
        return int(rng.integers(9, 32)), int(rng.integers(32, 201))
    if stratum == 'mult32':                                 # no ragged tile in one axis
        H, W = 32 * int(rng.integers(1, 7)), int(rng.integers(9, 201))
        return (H, W) if rng.random() < 0.5 else (W, H)
    if stratum == 'two_segments':                           # small enough for 40000 events to make a tile of two gather segments
        return int(rng.integers(9, 33)), int(rng.integers(9, 41))
    return int(rng.integers(9, 201)), int(rng.integers(9, 201))


def draw_case_motion(rng, k=None):
    """A case of the motion-model sweep.  k: the case's index in its sweep - it places the model kind (every key of motion.KINDS in
    turn; the first custom case has K = 12, the second K = 1), the sensor's stratum (SENSOR_STRATA) and the one 40000-event window
    (k = 5); without k all of it is drawn.  Half the cases have a drawn centre (anywhere in the sensor grown by 50 %) and scale
    ([0.3, 2] max(H, W)); R 1..16 (up to 6 above 64 x 64 px); 1..5 windows of different sizes, one sometimes masked; every loss term,
    contrast and correlation kind with a drawn tile; the field's bound model.abs_bound(c) about one of MOTION_MAGS (0: value only -
    drawn less often than the others, since a value-only case checks no gradient)."""
    kind = MOTION_KINDS[k % len(MOTION_KINDS)] if k is not None else str(rng.choice(MOTION_KINDS))
    K = motion.KINDS[kind]
    if kind == 'custom':
        K = {0: 12, 1: 1}.get(k // len(MOTION_KINDS)) if k is not None else None
        K = K or int(rng.integers(1, 13))
    stratum = SENSOR_STRATA[k % len(SENSOR_STRATA)] if k is not None else str(rng.choice(SENSOR_STRATA))
    H, W = _motion_sensor(rng, stratum)
    R = int(rng.integers(1, 17 if H * W <= 64 * 64 else 7))
    B = int(rng.integers(1, 6))
    N = [int(n) for n in rng.choice(MOTION_N, size=B, replace=False, p=P_MOTION_N)]
    if stratum == 'two_segments' and (k == 5 if k is not None else rng.random() < 0.2):
        N[int(rng.integers(B))] = 40000
    masked = int(rng.integers(B)) if B >= 2 and rng.random() < 0.5 else None
    centre = scale = None
    if rng.random() < 0.5:
        centre = ((W - 1) / 2.0 + float(rng.uniform(-0.75, 0.75)) * (W - 1), (H - 1) / 2.0 + float(rng.uniform(-0.75, 0.75)) * (H - 1))
        scale = float(rng.uniform(0.3, 2.0)) * max(H, W)
    tk = str(rng.choice(TILE_KINDS))
    if tk == 'many' and min(H, W) < 24:
        tk = 'any'
    c = dict(H=H, W=W, R=R, B=B, kind=kind, K=K, matrix_seed=int(rng.integers(1 << 31)), centre=centre, scale=scale, stratum=stratum,
             N=N, masked=masked, ck=int(rng.integers(0, 4)), rk=int(rng.integers(0, 4)), tile=_tile_of(rng, tk, H, W), tile_kind=tk,
             method='bilinear')
    c.update(_loss_terms(rng))
    c['mag'] = float(rng.choice(MOTION_MAGS, p=[0.08, 0.27, 0.25, 0.2, 0.2]))
    return c


def motion_model_of(c):
    matrix = np.random.default_rng(c['matrix_seed']).normal(size=(motion.NQ, c['K'])) if c['kind'] == 'custom' else None
    return motion.MotionModel(c['kind'], (c['H'], c['W']), centre=c['centre'], scale=c['scale'], matrix=matrix)


def motion_amp(model):
    """max_k sum_j |M_jk| max|m_j|: grad_error's amp of a model's coefficients"""
    mm = model.monomial_bounds()
    return float((np.abs(model.matrix) * np.concatenate([mm, mm])[:, None]).sum(axis=0).max())


def _scaled_coeffs(model, c, mag):
    """c scaled so that model.abs_bound(c) is mag (the bound is homogeneous in c)"""
    bound = model.abs_bound(c)
    return c * (mag / bound) if mag > 0.0 and bound > 0.0 else np.zeros_like(c)


def motion_inputs(c, seed):
    """(model, window dicts, coefficients (B, K)) of a motion case: every window's ground-truth flow is the field of drawn
    coefficients at the case's magnitude, the test coefficients are those times U(0.5, 1.5) at the same magnitude."""
    model = motion_model_of(c)
    rng = np.random.default_rng(seed)
    K = model.n_coeffs
    wins, coeffs = [], []
    for b in range(c['B']):
        n = c['N'][b]
        ct = _scaled_coeffs(model, rng.uniform(0.3, 1.0, K) * rng.choice([-1.0, 1.0], K), c['mag'])
        win = synth.make_window(seed + b, (c['H'], c['W']), max(n, 1), c['R'], flow=model.field(ct))
        for k in ('xs', 'ys', 'ts'):
            win[k] = win[k][:n]
        wins.append(win)
        coeffs.append(_scaled_coeffs(model, ct * rng.uniform(0.5, 1.5, K), c['mag']))
    return model, wins, np.stack(coeffs)


def _win_args(w):
    return (w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts'])


def _key(sweep, c, seed):
    return (sweep, seed, repr(sorted(c.items())))


def motion_reference(c, seed):
    """Per window dict(v, g (K,), G, terms) by fp64: the oracle on model.field(c) with identity resampling - the fp64 autograd witness
    where the kinds are outside the oracle (ck >= 2 or rk >= 1) - projected by model.project.  Once per process."""
    key = _key('motion', c, seed)
    if key not in _REFS:
        model, wins, coeffs = motion_inputs(c, seed)
        H, W = c['H'], c['W']
        out = []
        for b in range(c['B']):
            F = model.field(coeffs[b])
            if c['ck'] >= 2 or c['rk'] >= 1:
                v, gT, G, _, terms = SW.loss_and_grad(F, *_win_args(wins[b]), c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'],
                                                      np.eye(H), np.eye(W), window_size=3, contrast_kind=c['ck'],
                                                      correlation_kind=c['rk'], tile=c['tile'])
            else:
                v, gT, terms = O.loss_and_grad(F, *_win_args(wins[b]), c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'], 5, (H, W),
                                               'bilinear', contrast_kind=c['ck'], return_intermediates=True)
                G = terms['_G']
            out.append(dict(v=float(v), g=model.project(gT), G=G, terms=terms))
        _REFS[key] = out
    return _REFS[key]


def is_value_only(c):
    """a case whose theta is exactly 0: the gradient cancels by symmetry, so only the value is compared"""
    return c['mag'] == 0.0 and ('kind' in c or c['flow'] == 'zero')         # ('kind': a motion case, whose field is 0 at mag 0)


def vacuous_windows(c, refs):
    """(windows whose gradient check says nothing, windows): a value-only case, or a non-finite or zero reference gradient"""
    return sum(1 for r in refs if is_value_only(c) or not np.isfinite(r['v']) or not grad_is_checked(r['g'])), len(refs)


def run_case_motion(c, seed):
    """Evaluate a draw_case_motion case on both motion paths and compare every window (module docstring; the issue's list):
    expanded against fp64, fused against expanded (value and IWE stack bit for bit), against the exact moments of the same build's
    dense gradient (tests/_motion_bounds.py) and against fp64; the mask; scaled_theta; the refusal where the fused path does not apply.
    Returns the worst errors: value, grad (expanded), fused_grad, moment (|fused gradient - exact moments M| / bound) and the flags
    theta_bits, fused_bits, mask_bits, refusal."""
    import torch
    H, W, R, B = c['H'], c['W'], c['R'], c['B']
    model, wins, coeffs = motion_inputs(c, seed)
    refs = motion_reference(c, seed)
    value_only = is_value_only(c)                           # c = 0 exactly: the gradient cancels by symmetry (ill-conditioned)
    p = engine.make_params(c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'], 'bilinear', c['ck'], correlation_kind=c['rk'])
    why = engine.motion_fused_refusal('fp32', 3, p)
    act = None
    if c['masked'] is not None:
        act = np.ones(B, dtype=np.uint8)
        act[c['masked']] = 0
    on = [b for b in range(B) if b != c['masked']]
    worst = dict(value=0.0, grad=0.0, fused_grad=0.0, moment=0.0, theta_bits=True, fused_bits=True, mask_bits=True, refusal=True)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)      # noqa: E731

    def masked_ok(vm, gm, v, g):
        return bool(np.isnan(vm[c['masked']]) and same(gm[c['masked']], np.zeros(model.n_coeffs)) and same(vm[on], v[on]) and same(gm[on], g[on]))

    with engine.Engine((H, W), max(sum(c['N']), 1), max_refs=R, max_windows=B) as eng:
        eng.set_windows([_win_args(w) for w in wins])
        eng.set_objective_tiles(c['tile'])
        eng.set_motion_model(model)
        eng.set_motion_path('expanded')
        ve, ge, _ = eng.loss_grad_motion(coeffs, p)
        worst['theta_bits'] = bool(np.array_equal(eng.scaled_theta(), model.field(coeffs).reshape(B, H, W, 2)))
        iwe_e = eng.iwes()
        if act is not None:
            worst['mask_bits'] &= masked_ok(*eng.loss_grad_motion(coeffs, p, active=act)[:2], ve, ge)
        gf = None
        if why is None:
            eng.set_motion_path('fused')
            vf, gf, _ = eng.loss_grad_motion(coeffs, p)
            worst['fused_bits'] = bool(same(vf, ve) and np.array_equal(eng.iwes(), iwe_e))
            if act is not None:
                worst['mask_bits'] &= masked_ok(*eng.loss_grad_motion(coeffs, p, active=act)[:2], vf, gf)
            _, gd, _ = eng.loss_grad_device(torch.from_numpy(model.field(coeffs).reshape(B, H, W, 2)).cuda(), p, theta_abs_max=model.abs_bound(coeffs))
            gd = gd.cpu().numpy().reshape(B, H, W, 2)
        else:                                               # level-0 TV: 'fused' raises with the library's reason, 'auto' is the expanded path
            eng.set_motion_path('fused')
            try:
                eng.loss_grad_motion(coeffs, p)
                worst['refusal'] = False
            except ValueError as exc:
                worst['refusal'] = str(exc) == why and 'TV term' in why
            eng.set_motion_path('auto')
            va, ga, _ = eng.loss_grad_motion(coeffs, p)
            worst['refusal'] &= bool(same(va, ve) and same(ga, ge))
    if gf is not None:
        want, bound = MB.moment_bound(model, gd, MB.slots_per_window(wins, (H, W), R)[0])
    amp = motion_amp(model)
    tol_g = TOLS['motion']['grad']
    for b in range(B):
        r = refs[b]
        errs = dict(value=value_error(ve[b], r['v'], loss_term_sizes(c, r['terms'])),
                    grad=0.0 if value_only else grad_error(ge[b], r['g'], r['G'], c['N'][b], R, tol_g, IMAGE_EPS['fp32'], amp))
        if gf is not None:
            errs['fused_grad'] = 0.0 if value_only else grad_error(gf[b], r['g'], r['G'], c['N'][b], R, tol_g, IMAGE_EPS['fp32'], amp)
            if np.all(np.isfinite(gd[b])):
                err = np.abs(gf[b] - want[b])
                errs['moment'] = float(np.max(np.where(err <= bound[b], err / np.maximum(bound[b], 1e-300), np.inf)))
            else:                                           # no finite dense gradient to take moments of: the fused one is not finite either
                errs['moment'] = 0.0 if not np.all(np.isfinite(gf[b])) else np.inf
        if os.environ.get('EINCM_FUZZ_VERBOSE'):
            print(f'   window {b}: N {c["N"][b]} ' + ' '.join(f'{k} {e:.2e}' for k, e in errs.items())
                  + f' max|g_ref| {np.abs(r["g"]).max():.3e} max|g - g_ref| {np.abs(ge[b] - r["g"]).max():.3e}')
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
    return worst


# ---- the per-event weights sweep ----------------------------------------------------------------------------
WEIGHT_THETAS = ['2dof', 'coarse', 'dense', 'motion']
WEIGHT_KINDS = ['none', 'ones', 'eighth', 'quarters', 'zero']
P_WEIGHT_KINDS = [0.2, 0.2, 0.25, 0.25, 0.1]
WEIGHT_MODELS = [k for k in MOTION_KINDS if k != 'custom']


def draw_case_weights(rng, k=None):
    """A case of the weights sweep.  k: the case's index in its sweep - it places the theta kind (WEIGHT_THETAS in turn) and, at
    k = 3, a batch that is all None but one window; without k all of it is drawn.  Sensors as draw_case_fp64 (3..200 px, a third of
    them 3..8 px), R 1..16 (up to 6 above 64 x 64 px), 1..4 windows, every resampling method for the coarse grids, every loss term and
    level, ck and rk 0..3 with a drawn tile, and per window a weight kind of WEIGHT_KINDS: None, all ones, {0} u [1/8, 1] (about a
    fifth zero), k/4 with k = 0..4, all zero."""
    hi = 9 if rng.random() < 1.0 / 3.0 else 201
    H = int(rng.integers(3, hi)); W = int(rng.integers(3, hi))
    R = int(rng.integers(1, 17 if H * W <= 64 * 64 else 7))
    B = int(rng.integers(1, 5))
    theta = WEIGHT_THETAS[k % len(WEIGHT_THETAS)] if k is not None else str(rng.choice(WEIGHT_THETAS))
    if theta == 'motion':
        hw, method = (H, W), 'bilinear'
    else:
        _, hw, method = _theta_shape(rng, H, W, [theta])
    tk = str(rng.choice(TILE_KINDS))
    if tk == 'many' and min(H, W) < 24:
        tk = 'any'
    wk = [str(rng.choice(WEIGHT_KINDS, p=P_WEIGHT_KINDS)) for _ in range(B)]
    if k == 3:
        B = max(B, 2)
        wk = ['none'] * B
        wk[int(rng.integers(B))] = str(rng.choice(['eighth', 'quarters']))
    c = dict(H=H, W=W, R=R, B=B, theta=theta, hw=hw, method=method, model=str(rng.choice(WEIGHT_MODELS)),
             N=[int(rng.choice(N_CHOICES, p=P_N_CHOICES) if H * W <= 64 * 64 else rng.choice(MOTION_N, p=P_MOTION_N)) for _ in range(B)], wk=wk,
             ck=int(rng.integers(0, 4)), rk=int(rng.integers(0, 4)), tile=_tile_of(rng, tk, H, W), tile_kind=tk)
    c.update(_loss_terms(rng))
    return c


def _weights_of(rng, kind, n):
    """the weights of one window (float32, as staged) or None"""
    if kind == 'none':
        return None
    if kind == 'ones':
        return np.ones(n, dtype=np.float32)
    if kind == 'zero':
        return np.zeros(n, dtype=np.float32)
    if kind == 'eighth':                                    # tests/test_gpu_event_weights.py: draw_weights
        w = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.125, 1.0, n))
    else:
        w = rng.integers(0, 5, n) / 4.0
    if n and not w.any():
        w[0] = 1.0 if kind == 'quarters' else rng.uniform(0.125, 1.0)
    return w.astype(np.float32)


def weights_inputs(c, seed):
    """(window dicts, thetas (B, h, w, 2) or coefficients (B, K), weights per window, model or None) of a weights case"""
    H, W, R, B = c['H'], c['W'], c['R'], c['B']
    rng = np.random.default_rng(seed)
    value_only = c['mag'] == 0.0 and c['flow'] == 'zero'
    model = motion.MotionModel(c['model'], (H, W)) if c['theta'] == 'motion' else None
    wins, thetas, ws = [], [], []
    for b in range(B):
        n = c['N'][b]
        win = synth.make_window(seed + b, (H, W), max(n, 1), R, flow=c['flow'], flow_mag=max(c['mag'], 1e-3))
        for k in ('xs', 'ys', 'ts'):
            win[k] = win[k][:n]
        wins.append(win)
        if model is not None:
            # (as the grids below, whose noise of 0.5 px keeps them off theta = 0 unless the case is value-only)
            thetas.append(_scaled_coeffs(model, rng.normal(size=model.n_coeffs), max(c['mag'], 0.5) * rng.uniform(0.5, 1.0)))
        else:
            h, w = c['hw']
            base = win['flow_gt'] if (h, w) == (H, W) else np.broadcast_to(win['flow_gt'].mean(axis=(0, 1)), (h, w, 2))
            thetas.append(base * rng.uniform(0.5, 1.5, (h, w, 2)) + rng.normal(0, 0.5, (h, w, 2)))
        ws.append(_weights_of(rng, c['wk'][b], n))
    thetas = np.stack(thetas)
    if value_only:
        thetas[:] = 0.0
    return wins, thetas, ws, model


def _n_present(w, n):
    return n if w is None else int(np.count_nonzero(w))


def weights_reference(c, seed):
    """Per window dict(v, g, G, I, terms, Theta) by tests/_event_weights_witness.py (fp64 autograd).  Once per process."""
    key = _key('weights', c, seed)
    if key not in _REFS:
        wins, thetas, ws, model = weights_inputs(c, seed)
        H, W = c['H'], c['W']
        kw = dict(weights=None, contrast_kind=c['ck'], correlation_kind=c['rk'], tile=c['tile'])
        terms5 = (c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'])
        out = []
        for b in range(c['B']):
            kw['weights'] = ws[b]
            if c['theta'] in ('dense', 'motion'):
                Theta = model.field(thetas[b]) if model is not None else thetas[b]
                v, g, G, I, terms = EW.loss_and_grad_Theta(Theta, *_win_args(wins[b]), *terms5, full=True, **kw)
                g = model.project(g) if model is not None else g
            else:
                h, w = c['hw']
                v, g, G, I, terms = EW.loss_and_grad(thetas[b], *_win_args(wins[b]), *terms5, O.resample_matrix(h, H, H / h, c['method']),
                                                     O.resample_matrix(w, W, W / w, c['method']), **kw)
                Theta = O.scale_theta_to_sensor_size(thetas[b], (H, W), c['method'])
            out.append(dict(v=float(v), g=g, G=G, I=I, terms=terms, Theta=Theta))
        _REFS[key] = out
    return _REFS[key]


def run_case_weights(c, seed):
    """Evaluate a draw_case_weights case and compare every window with the weighted witness: value, gradient, IWE stack and dL/dIWE
    at TOLS['weights'] (the conditioning rules with N = the events of weight > 0), the count images bit for bit; an all-ones window
    has the bits of the batch staged with None in its place; an all-zero window behaves as the same window staged without events, and
    every other window has the bits it has then; a weighted batch on the motion model refuses 'fused' and takes 'expanded' for 'auto'.
    Returns the worst errors (value, grad, iwe, G) and the flags counts, ones_bits, zero_as_empty, others_bits, refusal."""
    H, W, R, B = c['H'], c['W'], c['R'], c['B']
    wins, thetas, ws, model = weights_inputs(c, seed)
    refs = weights_reference(c, seed)
    value_only = c['mag'] == 0.0 and c['flow'] == 'zero'
    p = engine.make_params(c['alpha'], c['beta'], c['gamma'], c['delta'], c['lvl'], c['method'], c['ck'], correlation_kind=c['rk'])
    worst = dict(value=0.0, grad=0.0, iwe=0.0, G=0.0, counts=True, ones_bits=True, zero_as_empty=True, others_bits=True, refusal=True)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)      # noqa: E731

    def evaluate(batch, probe=False):
        """(value, gradient, IWE stack, dL/dIWE, count images) of a staged batch"""
        with engine.Engine((H, W), max(sum(c['N']), 1), max_refs=R, max_windows=B) as eng:
            eng.set_windows(batch)
            eng.set_objective_tiles(c['tile'])
            if model is not None:
                eng.set_motion_model(model)
                v, g, _ = eng.loss_grad_motion(thetas, p)
            else:
                v, g, _ = eng.loss_grad(thetas, p)
            out = (v, g, eng.iwes(), eng.image_grad(), eng.count_images())       # (dL/dIWE before count_images, which reuses its buffer)
            if probe and model is not None and eng.weighted:
                eng.set_motion_path('fused')
                try:
                    eng.loss_grad_motion(thetas, p)
                    worst['refusal'] = False
                except ValueError as exc:
                    worst['refusal'] = str(exc) == engine.motion_fused_refusal('fp32', 3, p, weighted=True) and 'weight' in str(exc)
                eng.set_motion_path('auto')
                va, ga, _ = eng.loss_grad_motion(thetas, p)
                worst['refusal'] &= bool(same(va, v) and same(ga, g))
        return out

    v, g, iwes, G_e, counts = evaluate([_win_args(w) + (ws[b],) for b, w in enumerate(wins)], probe=True)
    ones = [b for b in range(B) if c['wk'][b] == 'ones' and c['N'][b] > 0]
    zeros = [b for b in range(B) if c['wk'][b] == 'zero' and c['N'][b] > 0]
    if ones:
        alt = evaluate([_win_args(w) + (None if b in ones else ws[b],) for b, w in enumerate(wins)])
        worst['ones_bits'] = all(same(x[b], y[b]) for x, y in zip((v, g, iwes, G_e), alt) for b in ones)
    if zeros:
        # how a window without events behaves is read from the engine: the all-zero window staged empty, in the same batch
        empty = lambda w: (w['xs'][:0], w['ys'][:0], w['ts'][:0], w['edges'], w['edge_ts'], None)      # noqa: E731
        ve, ge, _, _, _ = evaluate([empty(w) if b in zeros else _win_args(w) + (ws[b],) for b, w in enumerate(wins)])
        for b in range(B):
            if b not in zeros:
                worst['others_bits'] &= bool(same(v[b], ve[b]) and same(g[b], ge[b]))
            elif not (np.isfinite(ve[b]) and np.all(np.isfinite(ge[b]))):
                worst['zero_as_empty'] &= bool(np.isfinite(v[b]) == np.isfinite(ve[b]) and same(np.isfinite(g[b]), np.isfinite(ge[b])))
            else:
                e_v = value_error(v[b], ve[b], loss_term_sizes(c, refs[b]['terms']))
                e_g = rel(g[b], ge[b]) if np.abs(ge[b]).max() > 1e-200 else (0.0 if np.abs(g[b]).max() < 1e-12 else np.inf)
                worst['zero_as_empty'] &= bool(e_v <= TOLS['weights']['value'] and e_g <= TOLS['weights']['grad'])
    amp = motion_amp(model) if model is not None else 1.0
    for b in range(B):
        r = refs[b]
        n = _n_present(ws[b], c['N'][b])
        errs = dict(value=value_error(v[b], r['v'], loss_term_sizes(c, r['terms'])),
                    grad=0.0 if value_only else grad_error(g[b], r['g'], r['G'], n, R, TOLS['weights']['grad'], IMAGE_EPS['fp32'], amp),
                    iwe=_rel_img(iwes[b], r['I']),
                    # (at theta = 0 the sign of |div n|'s subgradient follows the last bit of the summation order: run_case)
                    G=0.0 if (value_only and c['delta'] != 0.0) else _rel_img(G_e[b], r['G']))
        ok_cnt = np.array_equal(counts[b], EW.count_images(r['Theta'], wins[b]['xs'], wins[b]['ys'], wins[b]['ts'], wins[b]['edge_ts'], ws[b]))
        if os.environ.get('EINCM_FUZZ_VERBOSE'):
            print(f'   window {b}: N {c["N"][b]} ({n} present, {c["wk"][b]}) ' + ' '.join(f'{k} {e:.2e}' for k, e in errs.items())
                  + f' counts {ok_cnt} max|g_ref| {np.abs(r["g"]).max():.3e}')
        for k, e in errs.items():
            worst[k] = max(worst[k], e)
        worst['counts'] = worst['counts'] and bool(ok_cnt)
    return worst


# per sweep: bounds that are no tolerance (the fused gradient against fp64 at the gradient's; the moment bound in its own units),
# and the flags that must hold
EXTRA_BOUNDS = {'motion': dict(fused_grad=TOLS['motion']['grad'], moment=1.0)}
FLAGS = {'motion': ['theta_bits', 'fused_bits', 'mask_bits', 'refusal'],
         'weights': ['counts', 'ones_bits', 'zero_as_empty', 'others_bits', 'refusal']}


def failures(worst, mode):
    """the measures of a run_case* result dict that exceed the sweep's tolerance, and the flags that do not hold ('counts': the count
    images differ)"""
    bad = [k for k, t in list(TOLS[mode].items()) + list(EXTRA_BOUNDS.get(mode, {}).items()) if not worst[k] <= t]
    return bad + [k for k in FLAGS.get(mode, ['counts']) if not worst[k]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('n', nargs='?', type=int, default=60)
    ap.add_argument('seed', nargs='?', type=int, default=0)
    g = ap.add_mutually_exclusive_group()
    g.add_argument('--fp64', action='store_true', help='the float64 mode against the oracle (draw_case_fp64)')
    g.add_argument('--kinds', action='store_true', help='the objective kinds against the witness (draw_case_kinds)')
    g.add_argument('--motion', action='store_true', help='the motion models, expanded and fused (draw_case_motion)')
    g.add_argument('--weights', action='store_true', help='per-event weights against the weighted witness (draw_case_weights)')
    a = ap.parse_args()
    mode = 'fp64' if a.fp64 else 'kinds' if a.kinds else 'motion' if a.motion else 'weights' if a.weights else 'fp32'
    draw = {'fp32': draw_case, 'fp64': draw_case_fp64, 'kinds': draw_case_kinds, 'motion': draw_case_motion,
            'weights': draw_case_weights}[mode]
    rng = np.random.default_rng(a.seed)
    bad = 0
    worst_all = {k: 0.0 for k in list(TOLS[mode]) + list(EXTRA_BOUNDS.get(mode, {}))}
    flags = FLAGS.get(mode, ['counts'])
    for i in range(a.n):
        c = draw(rng, i) if mode in ('motion', 'weights') else draw(rng)
        try:
            if mode == 'fp32':
                ev, eg, okc = run_case(c, 1000 * a.seed + i)
                res = dict(value=ev, grad=eg, counts=okc)
            elif mode == 'fp64':
                res = run_case(c, 1000 * a.seed + i, precision='fp64')
            elif mode in ('motion', 'weights'):
                res = {'motion': run_case_motion, 'weights': run_case_weights}[mode](c, 1000 * a.seed + i)
            else:
                res = run_case(c, 1000 * a.seed + i, kinds=(c['ck'], c['rk'], c['tile']))
        except Exception as exc:      # noqa: BLE001
            print(f'case {i} EXC {type(exc).__name__}: {exc}\n   {c}', flush=True)
            bad += 1
            continue
        for k in worst_all:
            worst_all[k] = max(worst_all[k], res[k])
        fail = failures(res, mode)
        bad += bool(fail)
        print(f'case {i:3d} ' + ' '.join(f'{k} {res[k]:.2e}' for k in worst_all) + ''.join(f' {k} {"ok" if res[k] else "DIFF"}' for k in flags)
              + (f'   <-- FAIL {fail}\n   {c}' if fail else ''), flush=True)
    print('worst ' + ', '.join(f'{k} err {e:.2e}' for k, e in worst_all.items()) + f', failures {bad}/{a.n}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
