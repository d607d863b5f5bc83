"""Randomised sweeps of the HIP loss/grad path against fp64 references (dev script; run on the GPU box).

Draws sensor sizes, event counts, reference counts, theta shapes, resampling methods, weights, pyramid levels, contrast kinds
and flow magnitudes (including flows that throw most events out of the frame), batches windows of different sizes in one
context, and reports the worst relative errors.  Six sweeps:
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
  --segmentation draw_case_segmentation  the per-event and segmentation operators (event_scores, event_responsibilities, set_weights and
                             apply_responsibilities on keep-order batches, compose_motions, contrast_landscape) on batches of groups of
                             windows, each against its own witness at the bar of its own test module (run_case_segmentation)
usage: python tests/dev/fuzz_gpu.py [n_cases] [seed] [--fp64 | --kinds | --motion | --weights | --segmentation]
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
import _contrast_landscape_witness as CL    # noqa: E402
import _event_scores_witness as ES      # noqa: E402
import _event_weights_witness as EW     # noqa: E402
import _motion_layers_witness as ML     # noqa: E402
import _motion_bounds as MB             # noqa: E402
import _objective_kinds_witness as WIT  # noqa: E402
import _responsibilities_witness as RW  # noqa: E402
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


# ---- the per-event and segmentation operators (DESIGN.md sections 25, 27, 28, 29 and 30) ------------------------------------------------
SEG_N = [0, 1, 63, 64, 65, 255, 256, 257, 300, 5000]        # events per group; the 40000-event group is placed, once per sweep
SEG_SMALL_N = [0, 1, 63]                                    # ... where the field throws most events out of the sensor (draw_case_segmentation)
SEG_EVALS = ['2dof', 'coarse', 'dense', 'motion-expanded', 'motion-fused']
SEG_WAYS = ['set_windows', 'set_weights', 'apply']
SEG_V = [1, 7, 64]
SEG_T_REF = ['none', 'scalar', 'window']
FAR = RW.FAR
SEG_ALL_RS = ('weights', 'labels', 'mass', 'n_unsupported')
SEG_ALL_ML = ('theta', 'labels', 'mass', 'total')
SEG_SENTINEL = np.float32(-777.0)


def far_coeffs(model):
    """Coefficients whose field is at least FAR px in one component at every pixel, so that every tap of every event is dropped; None
    for a custom matrix whose field has no such multiple within 4 FAR."""
    c = np.zeros(model.n_coeffs)
    if model.kind == 'rotation':
        c[0] = FAR / model.scale                            # Theta_y = s (1 + v v) c0
    elif model.kind == 'polynomial2':
        c[0] = c[6] = FAR
    elif model.kind != 'custom':
        c[0] = c[1] = FAR                                   # every other model starts with the translation
    else:
        c = np.ones(model.n_coeffs)
        least = float(np.abs(model.field(c)).max(axis=-1).min())
        if not least > 0.0:
            return None
        c = c * (FAR / least)
        if model.abs_bound(c) > 4.0 * FAR:
            return None
    return c


def draw_case_segmentation(rng, k=None):
    """A case of the segmentation sweep: one fp32 engine with a motion model, a batch of G groups of K consecutive windows, and the
    arguments of every operator of the chain run_case_segmentation runs.  k: the case's index in its sweep - it places the model kind
    (every key of motion.KINDS in turn, custom matrices as draw_case_motion), the sensor's stratum (SENSOR_STRATA), the last
    evaluation's kind (SEG_EVALS in turn; the coarse grids take every resampling method in turn), the way (SEG_WAYS), K = 1 (k = 2) and
    K = 8 (k = 7), the batch of three groups with an empty one in the middle (k = 9) and the one 40000-event group (k = 5, the
    two_segments stratum: R <= 2 and K = 2..3 there, for the witnesses' time); without k all of it is drawn.
    The 40000-event group has no window at FAR: a third of the sweep's score cells would have M == 0.  The fused path runs where the
    evaluation is motion-fused, the way set_windows and k even: those batches carry no weights and sit above level 0.
    The field's magnitude is one of MOTION_MAGS.  A field of more than half the sensor's shorter side throws most events out of the
    sensor under every model, and no stack makes such events supported: those cases take their group sizes from SEG_SMALL_N, so that
    every group of 64 events and more can meet the conditions of tests/test_fuzz_segmentation_interface.py.  The window at FAR and the
    zero entry of the prior lie in the case's largest group (the one the stack's lower bound is chosen on) and leave two models live."""
    kind = MOTION_KINDS[k % len(MOTION_KINDS)] if k is not None else str(rng.choice(MOTION_KINDS))
    Kc = motion.KINDS[kind]
    if kind == 'custom':
        Kc = {0: 12, 1: 1}.get(k // len(MOTION_KINDS)) if k is not None else None
        Kc = Kc or int(rng.integers(1, 13))
    stratum = SENSOR_STRATA[k % len(SENSOR_STRATA)] if k is not None else str(rng.choice(SENSOR_STRATA))
    H, W = _motion_sensor(rng, stratum)
    big = stratum == 'two_segments' and (k == 5 if k is not None else rng.random() < 0.2)
    R = int(rng.integers(1, 17 if H * W <= 64 * 64 else 7))
    K = {2: 1, 7: 8}.get(k) or int(rng.integers(1, 9))
    empty_mid = k == 9 if k is not None else rng.random() < 0.1
    if empty_mid:
        K = min(K, 5)
    if big:
        R, K = min(R, 2), min(max(K, 2), 3)
    G = 3 if empty_mid else int(rng.integers(1, min(3, 16 // K) + 1))
    mag = float(rng.choice([2.0, 10.0])) if big else float(rng.choice(MOTION_MAGS, p=[0.1, 0.3, 0.3, 0.15, 0.15]))
    pool = SEG_N if mag <= min(H, W) / 2.0 else SEG_SMALL_N
    p_pool = np.array([0.4 if n == 0 else 1.0 for n in pool])
    N = [int(n) for n in rng.choice(pool, size=G, replace=False, p=p_pool / p_pool.sum())]
    if empty_mid:
        a, b = rng.choice(pool[1:], size=2, replace=False)
        N = [int(a), 0, int(b)]
    if big:
        N[int(rng.integers(G))] = 40000
    centre = scale = None
    if rng.random() < 0.5:
        centre = ((W - 1) / 2.0 + float(rng.uniform(-0.75, 0.75)) * (W - 1), (H - 1) / 2.0 + float(rng.uniform(-0.75, 0.75)) * (H - 1))
        scale = float(rng.uniform(0.3, 2.0)) * max(H, W)
    ev = SEG_EVALS[k % len(SEG_EVALS)] if k is not None else str(rng.choice(SEG_EVALS))
    hw, method = (1, 1), 'bilinear'
    if ev == 'coarse':
        hw = (int(rng.integers(1, min(H, 17) + 1)), int(rng.integers(1, min(W, 17) + 1)))
        method = METHODS[(k // len(SEG_EVALS)) % len(METHODS)] if k is not None else str(rng.choice(METHODS))
    elif ev == 'dense':
        hw = (H, W)
    c = dict(H=H, W=W, R=R, K=K, G=G, B=G * K, N=N, kind=kind, K_c=Kc, matrix_seed=int(rng.integers(1 << 31)), centre=centre, scale=scale,
             stratum=stratum, mag=mag, eval=ev, hw=hw, method=method)
    largest = int(np.argmax(N))
    far = zero_prior = None
    if K >= 3 and N[largest] > 0 and not big and rng.random() < 0.5 and far_coeffs(seg_model_of(c)) is not None:
        far = largest * K + int(rng.integers(K))
    prior = bool(rng.random() < 0.5)
    if prior and K - (far is not None) >= 3:
        zero_prior = largest * K + int(rng.choice([l for l in range(K) if largest * K + l != far]))
    way = SEG_WAYS[(k + k // 3) % len(SEG_WAYS)] if k is not None else str(rng.choice(SEG_WAYS))
    wk = [str(rng.choice(WEIGHT_KINDS, p=P_WEIGHT_KINDS)) for _ in range(G * K)]
    lvl = int(rng.choice([0, 1]))
    if ev == 'motion-fused' and way == 'set_windows' and (k % 2 == 0 if k is not None else rng.random() < 0.5):
        wk, lvl = ['none'] * (G * K), 1                     # an unweighted batch above level 0: the fused path runs
    c.update(far=far, prior=prior, zero_prior=zero_prior, way=way, shared=bool(rng.random() < 0.5), wk=wk,
             wk2=[str(rng.choice(WEIGHT_KINDS, p=P_WEIGHT_KINDS)) for _ in range(G * K)],
             host_binning=bool(rng.random() < 0.5), exclude_self=bool(rng.random() < 0.5), omega=bool(rng.random() < 0.5),
             apply_source=str(rng.choice(['iwe', 'stack'])), mode=str(rng.choice(['hard', 'soft'])), fill=str(rng.choice(['zero', 'dominant'])),
             cell=int(rng.choice(CL.CELLS)), V=int(rng.choice(SEG_V)), t_ref=str(rng.choice(SEG_T_REF)), keep=bool(rng.random() < 0.5),
             gamma=float(rng.choice([0.0, 2.5e-4])), lvl=lvl)
    return c


def seg_model_of(c):
    """the motion model of a segmentation case (its K is the models of a group, K_c the model's coefficients)"""
    return motion_model_of(dict(c, K=c['K_c']))


def seg_params(c):
    return engine.make_params(20.0, 35.0, c['gamma'], 0.0, c['lvl'], c['method'])


def _seg_f64(inp, c, g, F, exclude_self=None):
    """RW.responsibilities_f64 of group g on the image stack F (B, R, H, W), with the weights staged when the chain scores"""
    K = c['K']
    b0 = g * K
    ws = inp['wins'][b0:b0 + K]
    return RW.responsibilities_f64(F[b0:b0 + K], inp['Theta'][b0:b0 + K], [(w['xs'], w['ys'], w['ts']) for w in ws], [w['edge_ts'] for w in ws],
                                   inp['omega_eff'], inp['w_eval'][b0:b0 + K], None if inp['prior'] is None else inp['prior'][b0:b0 + K],
                                   c['exclude_self'] if exclude_self is None else exclude_self)


def _seg_stack(U, lo):
    return (lo + (1.0 - lo) * U).astype(np.float32)


def segmentation_inputs(c, seed):
    """Everything a segmentation case is run on, made once per process and read-only: model, wins (B dicts xs, ys, ts, edges, edge_ts),
    w1 / w2 (the weights handed at staging / to set_weights; None or float32), w_eval (what is staged when the chain scores), theta
    ((B, h, w, 2), the grid kinds) and coeffs (B, K_c), Theta (B, H, W, 2) at the sensor's size by the oracle's resampling or
    model.field, prior (B,) or None, omega (R,) or None and omega_eff, the signed stack (B, R, H, W) float32 uniform in [lo, 1) with
    lo, its share and the steps of the bisection, and the landscape's candidates cl_coeffs (B, V, K_c) with the indices j_zero and
    j_far, t_ref (what the call takes) and t_ref_b (B,), keep."""
    key = _key('segmentation', c, seed)
    if key in _REFS:
        return _REFS[key]
    H, W, R, K, G, B = c['H'], c['W'], c['R'], c['K'], c['G'], c['B']
    shape = (H, W)
    model = seg_model_of(c)
    rng = np.random.default_rng(seed)
    wins = []
    for g, n in enumerate(c['N']):
        for l in range(K):
            if l == 0 or not c['shared']:
                if n:
                    xs, ys, ts, edges, edge_ts = ES.window(shape, n, R, seed * 64 + g * 8 + l)
                else:
                    xs, ys, ts = np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0)
                    edges, edge_ts = rng.uniform(0.0, 1.0, (R, H, W)), np.linspace(0.0, 1.0, R) + 0.013 if R > 1 else np.array([0.013])
            wins.append(dict(xs=xs, ys=ys, ts=ts, edges=edges, edge_ts=np.atleast_1d(edge_ts)))
    ns = [len(w['xs']) for w in wins]
    w1 = [_weights_of(rng, c['wk'][b], ns[b]) for b in range(B)]
    w2 = [_weights_of(rng, c['wk2'][b], ns[b]) for b in range(B)]
    Kc = model.n_coeffs
    coeffs = np.stack([_scaled_coeffs(model, rng.uniform(0.3, 1.0, Kc) * rng.choice([-1.0, 1.0], Kc), c['mag'] * rng.uniform(0.5, 1.0))
                       for _ in range(B)])
    theta = rng.uniform(-c['mag'], c['mag'], (B,) + tuple(c['hw']) + (2,)) if c['mag'] > 0.0 else np.zeros((B,) + tuple(c['hw']) + (2,))
    if c['far'] is not None:
        coeffs[c['far']] = far_coeffs(model)
        theta[c['far']] = FAR
    if c['eval'].startswith('motion'):
        Theta = model.field(coeffs).reshape(B, H, W, 2)
    else:
        Theta = np.stack([np.broadcast_to(theta[b, 0, 0], (H, W, 2)) if tuple(c['hw']) == (1, 1) else ES.sensor_theta(theta[b], shape, c['method'])
                          for b in range(B)])
    prior = None
    if c['prior']:
        prior = rng.uniform(0.2, 2.0, B)
        if c['zero_prior'] is not None:
            prior[c['zero_prior']] = 0.0
    omega = rng.uniform(0.2, 1.0, R) if c['omega'] else None
    inp = dict(model=model, wins=wins, ns=ns, w1=w1, w2=w2, w_eval=w2 if c['way'] == 'set_weights' else w1, theta=theta, coeffs=coeffs,
               Theta=Theta, prior=prior, omega=omega,
               omega_eff=omega if omega is not None else np.asarray(O.compute_weights_for_multi_reference(R), dtype=np.float64))
    # the stack's lower bound: bisection on the fp64 witness alone, on the largest group of 64 events and more
    U = rng.random((B, R, H, W))
    lo, share, steps = -0.9, None, 0
    cand = [g for g, n in enumerate(c['N']) if n >= 64]
    if cand:
        g = max(cand, key=lambda g: c['N'][g])
        lo_a, lo_b = -8.0, 0.95
        for steps in range(1, 25):
            share = float(_seg_f64(inp, c, g, _seg_stack(U, lo))['unsupported'].mean())
            if 0.15 <= share <= 0.35:
                break
            lo_a, lo_b = (lo, lo_b) if share > 0.35 else (lo_a, lo)
            lo = 0.5 * (lo_a + lo_b)
    inp.update(stack=_seg_stack(U, lo), lo=lo, lo_share=share, lo_steps=steps)
    # the landscape's candidates, at the case's magnitude within [10 px, the sensor's longer side]: a smaller field moves no event out
    # of the sensor and a larger one all of them - the zero and the FAR candidate again, which the list holds anyway
    V = c['V']
    cl_mag = min(max(c['mag'], 10.0), float(max(H, W)))
    cl = np.stack([[_scaled_coeffs(model, rng.uniform(0.3, 1.0, Kc) * rng.choice([-1.0, 1.0], Kc), cl_mag * rng.uniform(0.5, 1.0))
                    for _ in range(V)] for _ in range(B)])
    j_zero = j_far = None
    if V > 1:                                               # (one candidate cannot be both: it is at the magnitude)
        j_zero, j_far = (int(j) for j in rng.choice(V, size=2, replace=False))
        cl[:, j_zero] = 0.0
        if far_coeffs(model) is not None:
            cl[:, j_far] = far_coeffs(model)
        else:
            j_far = None
    t_ref = {'none': None, 'scalar': float(rng.uniform(0.2, 0.8)), 'window': rng.uniform(0.0, 1.0, B)}[c['t_ref']]
    keep = [None if b % 2 == 0 else rng.random(ns[b]) < 0.6 for b in range(B)] if c['keep'] else None
    inp.update(cl_coeffs=cl, j_zero=j_zero, j_far=j_far, t_ref=t_ref, keep=keep,
               t_ref_b=np.full(B, 0.5) if t_ref is None else np.broadcast_to(np.asarray(t_ref, dtype=np.float64), (B,)).copy())
    for v in list(inp.values()) + [a for w in wins for a in w.values()] + w1 + w2 + (keep or []):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REFS[key] = inp
    return inp


def seg_score_refs(inp, F):
    """Per window the fp64 witness of the scores on the stack F (B, R, H, W): dict(per: ES.event_scores' dict in the per-reference
    form, comb: its combined form under omega_eff, formed as ES.event_scores forms it)"""
    w32 = np.asarray(inp['omega_eff'], dtype=np.float64).astype(np.float32).astype(np.float64)
    out = []
    for b, w in enumerate(inp['wins']):
        per = ES.event_scores(F[b], inp['Theta'][b], w['xs'], w['ys'], w['ts'], w['edge_ts'])
        out.append(dict(per=per, comb=dict(scores=w32 @ per['scores'], selfs=w32 @ per['selfs'], M=np.abs(w32) @ per['M'],
                                           M_self=np.abs(w32) @ per['M_self'])))
    return out


def seg_compose(model, wins, K, weights, coeffs, mode='hard', fill='zero'):
    """ML.compose for groups of K windows that may hold their own events: every window's mass image comes from its own events, as
    the device walks every window's own bins; with shared events this is ML.compose itself (tests/test_fuzz_segmentation_interface.py)."""
    H, W = model.sensor_size
    G = len(wins) // K
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(G, K, -1)
    mass = np.stack([np.concatenate([ML.mass_images(wins[g * K + l]['xs'], wins[g * K + l]['ys'], [weights[g * K + l]], (H, W)) for l in range(K)])
                     for g in range(G)])
    total = mass.astype(np.uint64).sum(axis=(2, 3), dtype=np.uint64)
    labels = np.stack([ML.label(mass[g]) for g in range(G)])
    theta = np.zeros((G, H, W, 2), dtype=np.float64)
    for g in range(G):
        f = model.field(coeffs[g])
        has = labels[g] != ML.NO_LABEL
        if mode == 'hard':
            comp = np.take_along_axis(f, np.where(has, labels[g], 0).astype(np.int64)[None, :, :, None], axis=0)[0]
        else:
            comp = ML.soft_blend(np.where(has[None], mass[g], np.uint32(1)), f)
        d = ML.dominant(total[g]) if fill == 'dominant' else -1
        theta[g] = np.where(has[..., None], comp, f[d] if d >= 0 else np.zeros((H, W, 2)))
    return dict(theta=theta, labels=labels, mass=mass, total=total)


def seg_landscape_by_hand(c, inp, sumsq, n_in):
    """Whether a landscape (B, V) holds the two answers known without a warp.  The zero candidate moves nothing: n_in is the window's
    kept events.  The FAR candidate moves an event by at least FAR |t - t_ref| px in one axis, so no event further than
    (max(H, W) + 1) / FAR from t_ref stays in the sensor: n_in is at most the kept events that close to t_ref (none, in most windows),
    and sumsq is 0 where n_in is."""
    keep = [np.ones(n, dtype=bool) if inp['keep'] is None or inp['keep'][b] is None else np.asarray(inp['keep'][b]) != 0
            for b, n in enumerate(inp['ns'])]
    ok = True
    if inp['j_zero'] is not None:
        ok &= bool(np.array_equal(n_in[:, inp['j_zero']], [int(k.sum()) for k in keep]))
    if inp['j_far'] is not None:
        close = (max(c['H'], c['W']) + 1.0) / FAR
        near = [int((k & (np.abs(w['ts'] - t) < close)).sum()) for k, w, t in zip(keep, inp['wins'], inp['t_ref_b'])]
        ok &= bool(np.all(n_in[:, inp['j_far']] <= near) and np.array_equal(sumsq[:, inp['j_far']] == 0, n_in[:, inp['j_far']] == 0))
    return ok


def segmentation_reference(c, seed):
    """What the fp64 witnesses alone say about a case, for tests/test_fuzz_segmentation_interface.py; once per process.  dict(cells,
    zero_cells: the score cells of both sources and those with M == 0; wrapped, dropped: some tap is; groups: per group with K >= 2 and
    n >= 64 dict(unsupported, two, clear: shares of its events, self_changes); compose: dict(two_models, tied, holes, zero_total);
    landscape: (candidates with 0 < n_in < n of the windows of 64 events and more, those candidates); landscape_by_hand: the witness
    holds seg_landscape_by_hand's answers; far_empties: (windows the FAR candidate leaves without an event, windows) or None)."""
    key = _key('segmentation-ref', c, seed)
    if key in _REFS:
        return _REFS[key]
    inp = segmentation_inputs(c, seed)
    K, B, shape = c['K'], c['B'], (c['H'], c['W'])
    wins = inp['wins']
    iwe = np.stack([RW.weighted_iwes(inp['Theta'][b], w['xs'], w['ys'], w['ts'], w['edge_ts'], shape, inp['w_eval'][b]) for b, w in enumerate(wins)])
    out = dict(cells=0, zero_cells=0, wrapped=False, dropped=False, groups=[])
    for F in (iwe, inp['stack']):
        for r in seg_score_refs(inp, F):
            out['cells'] += r['per']['M'].size + r['comb']['M'].size
            out['zero_cells'] += int((r['per']['M'] == 0).sum() + (r['comb']['M'] == 0).sum())
            out['wrapped'] |= bool((r['per']['wrapped'] > 0).any())
            out['dropped'] |= bool((r['per']['dropped'] > 0).any())
    w_seg = list(inp['w_eval'])
    for g, n in enumerate(c['N']):
        if n == 0:
            continue
        r = _seg_f64(inp, c, g, inp['stack'])
        if c['way'] == 'apply':                             # (the weights compose_motions finds: the E-step's, in fp64 here)
            ra = r if c['apply_source'] == 'stack' else _seg_f64(inp, c, g, iwe)
            w_seg[g * K:(g + 1) * K] = list(ra['weights'].astype(np.float32))
        if K >= 2 and n >= 64:
            pi = np.ones(K) if inp['prior'] is None else inp['prior'][g * K:(g + 1) * K]
            live = (pi[:, None] * np.maximum(r['a'], 0.0)) > 0
            clear = ((np.abs(r['a']) > 1e-4 * r['M']) | (r['M'] == 0)).all(axis=0) & ~r['unsupported']      # (tests/test_gpu_responsibilities.py's rule)
            flip = _seg_f64(inp, c, g, inp['stack'], exclude_self=not c['exclude_self'])
            out['groups'].append(dict(g=g, n=n, unsupported=float(r['unsupported'].mean()), two=float((live.sum(axis=0) >= 2).mean()),
                                      clear=float(clear.mean()), self_changes=bool((flip['a'] != r['a']).any())))
    comp = seg_compose(inp['model'], wins, K, w_seg, inp['coeffs'], 'soft', 'dominant')
    mass = comp['mass']
    top = mass.max(axis=1)
    out['compose'] = dict(two_models=bool(((mass > 0).sum(axis=1) >= 2).any()), tied=bool((((mass == top[:, None]).sum(axis=1) >= 2) & (top > 0)).any()),
                          holes=bool((comp['labels'] == ML.NO_LABEL).any()), zero_total=bool((comp['total'].sum(axis=1) == 0).any()))
    big = [b for b in range(B) if inp['ns'][b] >= 64]
    sumsq, n_in = CL.landscape(inp['model'], [(w['xs'], w['ys'], w['ts']) for w in wins], inp['cl_coeffs'], inp['t_ref_b'], c['cell'], inp['keep'])
    out['landscape_by_hand'] = seg_landscape_by_hand(c, inp, sumsq, n_in)
    out['far_empties'] = None if inp['j_far'] is None else (int((n_in[:, inp['j_far']] == 0).sum()), B)
    kept = np.array([inp['ns'][b] if inp['keep'] is None or inp['keep'][b] is None else int(inp['keep'][b].sum()) for b in range(B)])
    part = (n_in > 0) & (n_in < kept[:, None])
    out['landscape'] = (int(part[big].sum()), int(part[big].size))
    _REFS[key] = out
    return out


def _seg_raw_scores(eng, images, omega, want_selfs=True):
    """eincm_event_scores itself on sentinel-filled outputs one cell longer than their layout: ([scores per window], [selfs per window]
    or None, whether the cell past every block is untouched)"""
    off, length, total = engine.event_scores_layout(eng.n_events, eng.R, omega is not None)
    flat = [np.full(total + 1, SEG_SENTINEL, dtype=np.float32) for _ in range(2 if want_selfs else 1)]
    img = None if images is None else np.ascontiguousarray(images, dtype=np.float32)
    rw = None if omega is None else np.ascontiguousarray(omega, dtype=np.float64)
    rc = eng._lib.eincm_event_scores(eng._ctx, None if img is None else img.ctypes.data, None if rw is None else rw.ctypes.data,
                                     flat[0].ctypes.data, flat[1].ctypes.data if want_selfs else None)
    if rc:
        raise engine.EincmError(rc, eng._lib.eincm_last_error(eng._ctx).decode())
    shape = (lambda n: (n,)) if omega is not None else (lambda n: (eng.R, n))
    split = [[a[off[b]:off[b] + length[b]].reshape(shape(int(eng.n_events[b]))) for b in range(eng.B)] for a in flat]
    return split[0], (split[1] if want_selfs else None), all(a[total] == SEG_SENTINEL for a in flat)


def _bytes_of(*arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def run_case_segmentation(c, seed, monkeypatch=None):
    """Run a draw_case_segmentation case through the chain - stage (the case's way), evaluate, event_scores, event_responsibilities,
    the re-weighting, compose_motions, contrast_landscape - and compare every operator with its witness at the bar of the operator's
    own test module.  monkeypatch: pytest's, for EINCM_HOST_BINNING (without it the variable is set here and put back).
    Returns the worst measures - scores, selfs (|gpu - witness| / M per cell), iwe (the GPU IWE against RW.weighted_iwes, of its
    maximum), sum_one (| sum_l w - 1 | / (K 2^-23)), mass (relative to RW.ordered_mass), w_f64 (|w - fp64 form| on the clear events) -
    and the flags: zero_cells (a cell with M == 0 is exactly 0), sentinels, resp_bits (weights and labels = RW.responsibilities_f32 on
    the GPU's own combined scores), n_unsupported, prior_shares, resp_repeat, order_perm, staged_bits, reweight_bits (value, gradient,
    iwes(), count_images() = a fresh keep-order engine's), none_bits (an all-None keep-order batch = the unweighted batch),
    compose_bits (all four outputs, the drawn mode / fill and the opposite one), hard_field, landscape (= CL.landscape), cl_zero_far
    (seg_landscape_by_hand), cl_repeat, cl_weights."""
    H, W, R, K, G, B = c['H'], c['W'], c['R'], c['K'], c['G'], c['B']
    shape = (H, W)
    inp = segmentation_inputs(c, seed)
    model, wins, ns = inp['model'], inp['wins'], inp['ns']
    p = seg_params(c)
    worst = dict(scores=0.0, selfs=0.0, iwe=0.0, sum_one=0.0, mass=0.0, w_f64=0.0, zero_cells=True, sentinels=True, resp_bits=True,
                 n_unsupported=True, prior_shares=True, resp_repeat=True, order_perm=True, staged_bits=True, reweight_bits=True,
                 none_bits=True, compose_bits=True, hard_field=True, landscape=True, cl_zero_far=True, cl_repeat=True, cl_weights=True)
    old_env = os.environ.get('EINCM_HOST_BINNING')
    if monkeypatch is not None:
        monkeypatch.setenv('EINCM_HOST_BINNING', '1') if c['host_binning'] else monkeypatch.delenv('EINCM_HOST_BINNING', raising=False)
    elif c['host_binning']:
        os.environ['EINCM_HOST_BINNING'] = '1'
    else:
        os.environ.pop('EINCM_HOST_BINNING', None)

    def new_engine():
        eng = engine.Engine(shape, max(sum(ns), 1), max_refs=R, max_windows=B)
        eng.set_motion_model(model)
        return eng

    def stage(eng, ws, keep_order):
        eng.set_windows([_win_args(w) + (ws[b],) for b, w in enumerate(wins)], keep_order=keep_order)

    def evaluate(eng, fused_ok=True):
        """(value, gradient, iwes(), count_images()) of the case's last evaluation on the staged batch"""
        if c['eval'].startswith('motion'):
            fused = c['eval'] == 'motion-fused' and fused_ok and engine.motion_fused_refusal('fp32', 3, p, weighted=eng.weighted) is None
            eng.set_motion_path('fused' if fused else 'expanded')
            v, g, _ = eng.loss_grad_motion(inp['coeffs'], p)
        else:
            v, g, _ = eng.loss_grad(inp['theta'], p)
        return v, g

    def images_of(eng):
        iw = eng.iwes()
        return iw, eng.count_images()

    def landscape(eng):
        return eng.contrast_landscape(inp['cl_coeffs'], t_ref=inp['t_ref'], cell=c['cell'], keep=inp['keep'])

    def ones(ws):
        return [np.ones(ns[b], np.float32) if w is None else w for b, w in enumerate(ws)]

    omega_eff = inp['omega'] if inp['omega'] is not None else engine.multi_ref_weights(R)
    way = c['way']
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    eng = new_engine()
    try:
        # ---- staging, by the case's way -----------------------------------------------------------------------------------------
        stage(eng, inp['w1'], way != 'set_windows')
        w_cur = inp['w1']
        cl_first = landscape(eng)
        if way != 'set_windows':
            for o in eng.staged_order():
                worst['order_perm'] &= bool(o.shape == (sum(ns),) and all(np.array_equal(np.sort(o[off[b]:off[b + 1]]), np.arange(off[b], off[b + 1]))
                                                                          for b in range(B)))
        if way == 'set_weights':
            eng.set_weights(inp['w2'])
            w_cur = inp['w2']
            worst['staged_bits'] &= _bytes_of(*eng.staged_weights()) == _bytes_of(*ones(w_cur))
        v, g = evaluate(eng)
        # ---- 1. scores ------------------------------------------------------------------------------------------------------------------
        gpu_comb = {}
        got_scores = {}
        for source in ('iwe', 'stack'):
            images = None if source == 'iwe' else inp['stack']
            for form, om in (('per', None), ('comb', omega_eff)):
                s, q, ok = _seg_raw_scores(eng, images, om, True)
                s2, _, ok2 = _seg_raw_scores(eng, images, om, False)
                worst['sentinels'] &= bool(ok and ok2)
                got_scores[source, form] = (s, q, s2)
                if form == 'comb':
                    gpu_comb[source] = (s, q)
        Theta = eng.scaled_theta()                          # (after the scores, which build the image where the evaluation left none)
        iwes = eng.iwes()
        gin = dict(inp, Theta=Theta, omega_eff=omega_eff, w_eval=w_cur)
        for b, w in enumerate(wins):
            ref = RW.weighted_iwes(Theta[b], w['xs'], w['ys'], w['ts'], w['edge_ts'], shape, w_cur[b])
            worst['iwe'] = max(worst['iwe'], _rel_img(iwes[b], ref))
        F_of = dict(iwe=iwes, stack=inp['stack'])
        for source in ('iwe', 'stack'):
            refs = seg_score_refs(gin, F_of[source])
            for form in ('per', 'comb'):
                s, q, s2 = got_scores[source, form]
                for b in range(B):
                    r = refs[b][form]
                    for got, want, M, name in ((s[b], r['scores'], r['M'], 'scores'), (s2[b], r['scores'], r['M'], 'scores'),
                                               (q[b], r['selfs'], r['M_self'], 'selfs')):
                        zero = M == 0
                        worst['zero_cells'] &= bool(np.all(got[zero] == 0.0))
                        worst[name] = max(worst[name], ES.within(got, want, M)[1])
        # ---- 2. responsibilities ------------------------------------------------------------------------------------------------------
        kw = dict(ref_weights=inp['omega'], prior=inp['prior'], exclude_self=c['exclude_self'])
        wk = ones(w_cur)
        rs = {}
        for source in ('iwe', 'stack'):
            images = None if source == 'iwe' else inp['stack']
            r = eng.event_responsibilities(K, images=images, want=SEG_ALL_RS, **kw)
            again = eng.event_responsibilities(K, images=images, want=SEG_ALL_RS, **kw)
            worst['resp_repeat'] &= all(_bytes_of(*r[k]) == _bytes_of(*again[k]) for k in ('weights', 'labels')) and \
                _bytes_of(r['mass'], r['n_unsupported']) == _bytes_of(again['mass'], again['n_unsupported'])
            rs[source] = r
            s, q = gpu_comb[source]
            for gi in range(G):
                n, b0 = c['N'][gi], gi * K
                gw = np.stack(r['weights'][b0:b0 + K])
                pi = None if inp['prior'] is None else inp['prior'][b0:b0 + K]
                ref = RW.responsibilities_f32(np.stack(s[b0:b0 + K]), np.stack(q[b0:b0 + K]), np.stack(wk[b0:b0 + K]), pi, c['exclude_self'])
                worst['resp_bits'] &= bool(gw.tobytes() == ref['weights'].tobytes() and np.array_equal(r['labels'][gi], ref['labels']))
                worst['n_unsupported'] &= int(r['n_unsupported'][gi]) == int(ref['unsupported'].sum())
                want_mass = RW.ordered_mass(gw)
                some = want_mass != 0
                worst['mass'] = max(worst['mass'], float((np.abs(r['mass'][gi] - want_mass)[some] / np.abs(want_mass[some])).max(initial=0.0)),
                                    0.0 if np.all(r['mass'][gi][~some] == 0.0) else np.inf)
                if not n:
                    continue
                worst['sum_one'] = max(worst['sum_one'], float(np.abs(gw.astype(np.float64).sum(axis=0) - 1.0).max() / (K * 2.0 ** -23)))
                pi32 = np.ones(K, np.float32) if pi is None else np.asarray(pi, dtype=np.float64).astype(np.float32)
                T = np.float32(0)
                for x in pi32:
                    T = np.float32(T + x)
                worst['prior_shares'] &= bool(np.all(gw[:, ref['unsupported']] == (pi32 / T).astype(np.float32)[:, None]))
                r64 = _seg_f64(gin, c, gi, F_of[source])
                clear = ((np.abs(r64['a']) > 1e-4 * r64['M']) | (r64['M'] == 0)).all(axis=0) & ~r64['unsupported'] & ~ref['unsupported']
                if clear.any():
                    worst['w_f64'] = max(worst['w_f64'], float(np.abs(gw[:, clear] - r64['weights'][:, clear]).max()))
        # ---- 3. the keep-order ways ---------------------------------------------------------------------------------------------------
        if way == 'apply':
            src = c['apply_source']
            ra = eng.apply_responsibilities(K, images=None if src == 'iwe' else inp['stack'], want=SEG_ALL_RS, **kw)
            worst['resp_repeat'] &= all(_bytes_of(*ra[k]) == _bytes_of(*rs[src][k]) for k in ('weights', 'labels')) and \
                _bytes_of(ra['mass'], ra['n_unsupported']) == _bytes_of(rs[src]['mass'], rs[src]['n_unsupported'])
            w_cur = [np.array(w) for w in ra['weights']]
            worst['staged_bits'] &= _bytes_of(*eng.staged_weights()) == _bytes_of(*w_cur)
            v, g = evaluate(eng)
            iwes = eng.iwes()
            for b, w in enumerate(wins):                    # (the IWE under the weights the E-step left, against the witness again)
                ref = RW.weighted_iwes(Theta[b], w['xs'], w['ys'], w['ts'], w['edge_ts'], shape, w_cur[b])
                worst['iwe'] = max(worst['iwe'], _rel_img(iwes[b], ref))
        if way != 'set_windows':
            mine = _bytes_of(v, g, iwes, eng.count_images())
            with new_engine() as fresh:
                stage(fresh, w_cur, True)
                vf, gf = evaluate(fresh)
                worst['reweight_bits'] &= mine == _bytes_of(vf, gf, *images_of(fresh))
        with new_engine() as plain:
            plain.set_windows([_win_args(w) for w in wins])
            worst['cl_weights'] &= _bytes_of(*landscape(plain).values()) == _bytes_of(*cl_first.values())
            if way != 'set_windows':
                vp, gp = evaluate(plain, fused_ok=False)
                plain_bytes = _bytes_of(vp, gp, *images_of(plain))
                with new_engine() as none:
                    stage(none, [None] * B, True)
                    vn, gn = evaluate(none, fused_ok=False)
                    worst['none_bits'] &= plain_bytes == _bytes_of(vn, gn, *images_of(none))
        # ---- 4. compose_motions ---------------------------------------------------------------------------------------------------------
        other = dict(hard='soft', soft='hard', zero='dominant', dominant='zero')
        for mode, fill in ((c['mode'], c['fill']), (other[c['mode']], other[c['fill']])):
            got = eng.compose_motions(K, inp['coeffs'], mode=mode, fill=fill, want=SEG_ALL_ML)
            want = seg_compose(model, wins, K, w_cur, inp['coeffs'], mode, fill)
            worst['compose_bits'] &= all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes()
                                         for k in SEG_ALL_ML)
            if mode == 'hard':
                f = model.field(inp['coeffs']).reshape(G, K, H, W, 2)
                has = got['labels'] != ML.NO_LABEL
                pick = np.take_along_axis(f, np.where(has, got['labels'], 0).astype(np.int64)[:, None, :, :, None], axis=1)[:, 0]
                worst['hard_field'] &= bool(np.array_equal(got['theta'][has], pick[has]))
        # ---- 5. contrast_landscape (after the re-weighting: staged weights do not change it) -------------------------------------------
        cl = landscape(eng)
        worst['cl_repeat'] &= _bytes_of(*landscape(eng).values()) == _bytes_of(*cl.values())
        worst['cl_weights'] &= _bytes_of(*cl.values()) == _bytes_of(*cl_first.values())
        sumsq, n_in = CL.landscape(model, [(w['xs'], w['ys'], w['ts']) for w in wins], inp['cl_coeffs'], inp['t_ref_b'], c['cell'], inp['keep'])
        worst['landscape'] &= bool(np.array_equal(cl['sumsq'], sumsq) and np.array_equal(cl['n_in'], n_in)
                                   and cl['sumsq'].dtype == np.uint64 and cl['n_in'].dtype == np.uint32)
        worst['cl_zero_far'] &= seg_landscape_by_hand(c, inp, cl['sumsq'], cl['n_in'])
    finally:
        eng.close()
        if monkeypatch is None:
            if old_env is None:
                os.environ.pop('EINCM_HOST_BINNING', None)
            else:
                os.environ['EINCM_HOST_BINNING'] = old_env
    return worst


# per sweep: bounds that are no tolerance (the fused gradient against fp64 at the gradient's; the moment bound in its own units; the
# responsibilities' sum in units of K 2^-23), and the flags that must hold
TOLS['segmentation'] = dict(scores=ES.TOL, selfs=ES.TOL, iwe=1e-5, mass=1e-12, w_f64=1e-4)
EXTRA_BOUNDS = {'motion': dict(fused_grad=TOLS['motion']['grad'], moment=1.0), 'segmentation': dict(sum_one=1.0)}
FLAGS = {'motion': ['theta_bits', 'fused_bits', 'mask_bits', 'refusal'],
         'weights': ['counts', 'ones_bits', 'zero_as_empty', 'others_bits', 'refusal'],
         'segmentation': ['zero_cells', 'sentinels', 'resp_bits', 'n_unsupported', 'prior_shares', 'resp_repeat', 'order_perm', 'staged_bits',
                          'reweight_bits', 'none_bits', 'compose_bits', 'hard_field', 'landscape', 'cl_zero_far', 'cl_repeat', 'cl_weights']}


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
    g.add_argument('--segmentation', action='store_true', help='the per-event and segmentation operators against their witnesses '
                                                                 '(draw_case_segmentation)')
    a = ap.parse_args()
    mode = 'fp64' if a.fp64 else 'kinds' if a.kinds else 'motion' if a.motion else 'weights' if a.weights else \
        'segmentation' if a.segmentation else 'fp32'
    draw = {'fp32': draw_case, 'fp64': draw_case_fp64, 'kinds': draw_case_kinds, 'motion': draw_case_motion,
            'weights': draw_case_weights, 'segmentation': draw_case_segmentation}[mode]
    rng = np.random.default_rng(a.seed)
    bad = 0
    worst_all = {k: 0.0 for k in list(TOLS[mode]) + list(EXTRA_BOUNDS.get(mode, {}))}
    flags = FLAGS.get(mode, ['counts'])
    for i in range(a.n):
        c = draw(rng, i) if mode in ('motion', 'weights', 'segmentation') else draw(rng)
        try:
            if mode == 'fp32':
                ev, eg, okc = run_case(c, 1000 * a.seed + i)
                res = dict(value=ev, grad=eg, counts=okc)
            elif mode == 'fp64':
                res = run_case(c, 1000 * a.seed + i, precision='fp64')
            elif mode in ('motion', 'weights', 'segmentation'):
                res = {'motion': run_case_motion, 'weights': run_case_weights, 'segmentation': run_case_segmentation}[mode](c, 1000 * a.seed + i)
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
