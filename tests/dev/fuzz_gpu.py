"""Randomised sweeps of the HIP loss/grad path against fp64 references (dev script; run on the GPU box).

Draws sensor sizes, event counts, reference counts, theta shapes, resampling methods, weights, pyramid levels, contrast kinds
and flow magnitudes (including flows that throw most events out of the frame), batches windows of different sizes in one
context, and reports the worst relative errors.  Three sweeps:
  default   draw_case        the fp32 engine against the fp64 oracle
  --fp64    draw_case_fp64   the float64 mode against the oracle: value, gradient, IWE and dL/dIWE at 1e-10 / 1e-9 / 1e-11 / 1e-10
  --kinds   draw_case_kinds  the selectable objective kinds and tile sizes against the fp64 autograd witness
                             (tests/_objective_kinds_witness.py): value, gradient, dL/dIWE and the two mean relative terms at 1e-5
usage: python tests/dev/fuzz_gpu.py [n_cases] [seed] [--fp64 | --kinds]
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
import _objective_kinds_witness as WIT  # noqa: E402

pkg = 'edge-informed-contrast-maximization_amd'
synth = importlib.import_module(pkg + '.synth')
engine = importlib.import_module(pkg + '.engine')

METHODS = ['bilinear', 'lanczos3', 'lanczos5', 'cubic']
N_CHOICES = [0, 1, 7, 300, 5000, 40000]
# per sweep: the tolerance of each measured error (max-norm relative; the value and gradient after the conditioning rules of run_case)
TOLS = {'fp32': dict(value=1e-5, grad=1e-5),
        'fp64': dict(value=1e-10, grad=1e-9, iwe=1e-11, G=1e-10),
        'kinds': dict(value=1e-5, grad=1e-5, G=1e-5, corr=1e-5, contrast=1e-5)}
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
    if tk == 'ragged':
        tile = (_ragged(rng, H), _ragged(rng, W))
    elif tk in ('side1', 'side2'):
        s = 1 if tk == 'side1' else 2
        tile = (s, _ragged(rng, W)) if rng.random() < 0.5 else (_ragged(rng, H), s)
    elif tk == 'sensor':
        tile = (H, W)
    elif tk == 'many':          # at least 9 x 9 whole tiles
        tile = (int(rng.integers(1, H // 9 + 1)), int(rng.integers(1, W // 9 + 1)))
    else:
        tile = (int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1)))
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
        # the value is a signed sum of terms (-alpha*contrast - beta*corr + gamma*TV + delta*div) that can cancel (tiny sensor, one event:
        # -0.18152 + 0.18121); its error is measured against the size of the terms, each of which carries the images' accuracy
        terms = [c['alpha'] * aux.get('mean_rel_contrast', 0.0), c['beta'] * aux.get('mean_rel_corr', 0.0),
                 c['gamma'] * aux.get('theta_total_variation', 0.0), c['delta'] * aux.get('mean_rel_iwe_divergence', 0.0)]
        vscale = max(abs(v_ref), sum(abs(t) for t in terms if np.isfinite(t))) if np.isfinite(v_ref) else 1.0
        ev = abs(v[b] - v_ref) / max(vscale, 1e-300) if np.isfinite(v_ref) else (0.0 if not np.isfinite(v[b]) else np.inf)
        if np.isfinite(v_ref) and vscale < 1e-12:
            ev = abs(v[b] - v_ref)
        gmax = np.abs(g_ref).max()
        eg = rel(g[b], g_ref) if (np.all(np.isfinite(g_ref)) and gmax > 1e-200) else (0.0 if gmax <= 1e-200 and np.abs(g[b]).max() < 1e-12 else
                                                                                  (0.0 if not np.all(np.isfinite(g_ref)) else np.inf))
        # Conditioning of the gradient: every event contributes terms of size ~ max|dL/dIWE| that cancel down to max|g_ref|.  With a
        # handful of events the arg-max term of the normalisation can make that ratio 1e13 (one event: max|G| 8.5e11, max|g| 0.036), and
        # then fp64 itself - the reference included - resolves the gradient only to ratio * 2.2e-16.  The error is reported in units of
        # max(the usual tolerance scale, that floor).
        if np.all(np.isfinite(g_ref)) and gmax > 1e-200 and np.all(np.isfinite(G_ref)):
            kappa = 2.15 * np.abs(G_ref).max() * max(c['N'][b], 1) * R / gmax
            # the engine stores dL/dIWE as an image of its precision (fp32: 6e-8 per pixel; fp64: 2.2e-16): with a handful of events
            # nothing averages that out (one event on a 5x6 sensor: max|g| 6.7e-4 under max|G| ~ 0.1); with many events the pixel
            # errors add incoherently
            nb = max(c['N'][b], 1)
            g_level = np.abs(G_ref).max() if nb <= 16 else np.sqrt(np.mean(np.square(G_ref))) * np.sqrt(nb)
            floor = 2.15 * IMAGE_EPS[precision] * np.sqrt(9.0 * R) * g_level / gmax
            eg = eg / max(1.0, kappa * 2.2e-16 / tol_g, floor / tol_g)
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


def failures(worst, mode):
    """the measures of run_case's result dict that exceed the sweep's tolerance (and 'counts' if the count images differ)"""
    bad = [k for k, t in TOLS[mode].items() if not worst[k] <= t]
    return bad + ([] if worst['counts'] else ['counts'])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('n', nargs='?', type=int, default=60)
    ap.add_argument('seed', nargs='?', type=int, default=0)
    g = ap.add_mutually_exclusive_group()
    g.add_argument('--fp64', action='store_true', help='the float64 mode against the oracle (draw_case_fp64)')
    g.add_argument('--kinds', action='store_true', help='the objective kinds against the witness (draw_case_kinds)')
    a = ap.parse_args()
    mode = 'fp64' if a.fp64 else 'kinds' if a.kinds else 'fp32'
    draw = {'fp32': draw_case, 'fp64': draw_case_fp64, 'kinds': draw_case_kinds}[mode]
    rng = np.random.default_rng(a.seed)
    bad = 0
    worst_all = {k: 0.0 for k in TOLS[mode]}
    for i in range(a.n):
        c = draw(rng)
        try:
            if mode == 'fp32':
                ev, eg, okc = run_case(c, 1000 * a.seed + i)
                res = dict(value=ev, grad=eg, counts=okc)
            elif mode == 'fp64':
                res = run_case(c, 1000 * a.seed + i, precision='fp64')
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
        print(f'case {i:3d} ' + ' '.join(f'{k} {res[k]:.2e}' for k in TOLS[mode]) + f' counts {"ok" if res["counts"] else "DIFF"}'
              + (f'   <-- FAIL {fail}\n   {c}' if fail else ''), flush=True)
    print('worst ' + ', '.join(f'{k} err {e:.2e}' for k, e in worst_all.items()) + f', failures {bad}/{a.n}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
