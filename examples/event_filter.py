"""The refractory and polarity-aware event filter in front of the solver: a synthetic window of a few moving
edges with uniform noise, random polarity and one chattering pixel beside an edge is filtered, staged and solved with and without the
filter's weights.

    python3 examples/event_filter.py [--events 30000] [--noise 0.6] [--refractory-us 100] [--tau-us 3000]

Raw times are integer microseconds, as a recording has them; ``refractory`` and ``tau`` are in that unit.  The chattering pixel fires
every 25 us: the support filter (examples/event_denoise.py) would let each of its events vouch for the noise around it, and would
need a hot-pixel mask to silence it.  Here the refractory rule keeps the first event of the chatter and drops the rest, support counts
kept events of the event's own polarity only, and stage_datasample takes the weights as they are (dropped events weigh 0; the staged
lists keep their length, index with ``keep`` to shorten them).  The flow error of both solves is printed."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'edge-informed-contrast-maximization_amd'
synth, engine, bsol, staging = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine', 'batch_solver', 'staging'))

ap = argparse.ArgumentParser()
ap.add_argument('--events', type=int, default=30000, help='events of the moving edges')
ap.add_argument('--noise', type=float, default=0.6, help='uniform noise events per edge event')
ap.add_argument('--refractory-us', type=float, default=100.0,
                help='longer than the chatter\'s period, shorter than the gap between an edge\'s own events on one pixel')
ap.add_argument('--tau-us', type=float, default=3000.0, help='random polarity halves the neighbours that count: twice event_denoise.py\'s')
ap.add_argument('--radius', type=int, default=1)
ap.add_argument('--full-support', type=int, default=2)
a = ap.parse_args()

H, W, R, WINDOW_US, CHATTER_US = 96, 128, 3, 50_000, 25
rng = np.random.default_rng(0)
win = synth.make_window(0, (H, W), a.events, R, flow='constant', flow_mag=8.0, noise_frac=0.0, n_segments=12, n_circles=2)
n_noise, n_chatter = int(a.noise * a.events), WINDOW_US // CHATTER_US
cy, cx = int(win['ys'][0]), int(min(W - 1, win['xs'][0] + 1))                 # beside a pixel that an edge crosses
xs = np.concatenate([win['xs'], rng.integers(0, W, n_noise), np.full(n_chatter, cx)])
ys = np.concatenate([win['ys'], rng.integers(0, H, n_noise), np.full(n_chatter, cy)])
t01 = np.concatenate([win['ts'], rng.random(n_noise), np.arange(n_chatter) * (CHATTER_US / WINDOW_US)])
order = np.argsort(t01, kind='stable')
n = len(order)
events = dict(x=xs[order].astype(np.int16), y=ys[order].astype(np.int16), t=np.floor(t01[order] * WINDOW_US).astype(np.int64) + 1_000_000,
              p=rng.integers(0, 2, n).astype(np.int8) * 2 - 1)                # random polarity, as {-1, +1}

keep, weights, support = staging.event_filter_weights(events, (H, W), refractory=a.refractory_us, tau=a.tau_us, radius=a.radius,
                                                      full_support=a.full_support, polarity=True, return_support=True)
is_edge, is_chatter = order < a.events, order >= a.events + n_noise
print(f'{n} events: {a.events} on the edges, {n_noise} noise, {n_chatter} on the chattering pixel ({cx}, {cy})')
print(f'kept: {int(keep.sum())} of {n}; of the chatter {int(keep[is_chatter].sum())} of {n_chatter}')
print(f'mean weight: edge events {weights[is_edge].mean():.3f}, noise {weights[~is_edge & ~is_chatter].mean():.3f}, '
      f'chatter {weights[is_chatter].mean():.3f}; {int((weights == 1).sum())} events at weight 1')

ds = dict(events=events, image_ts=1_000_000 + win['edge_ts'] * WINDOW_US, eval_ts=(1_000_000, 1_000_000 + WINDOW_US))
weighted = staging.stage_datasample(ds, edges=win['edges'], event_weights=weights)
plain = staging.stage_datasample(ds, edges=win['edges'])
params = engine.make_params(20.0, 35.0, 0.0, 0.0, 1)
with engine.Engine((H, W), 2 * n, max_refs=R, max_windows=2) as eng:
    eng.set_windows([weighted, plain])                                        # one batch: the filtered window and the same events as they are
    results = bsol.minimize_thetas(eng, np.zeros((2, 1, 1, 2)), params, maxiter=60, gtol=1e-6)
truth = win['flow_gt'][0, 0]
print(f'true flow ({truth[0]:+.2f}, {truth[1]:+.2f}) px per window')
for name, r in zip(('with the filter\'s weights', 'without'), results):
    th = np.asarray(r.x).reshape(2)
    print(f'{name}: theta ({th[0]:+.2f}, {th[1]:+.2f}), score {float(r.fun):.6f}, flow error {np.linalg.norm(th - truth):.3f} px '
          f'after {r.nit} iterations')
