"""The event-support filter in front of the solver: a synthetic window of a few moving edges, uniform noise
and two hot pixels is masked, filtered, staged and solved with and without the filter's weights.

    python3 examples/event_denoise.py [--events 30000] [--noise 0.6] [--tau-us 1500]

Raw times are integer microseconds, as a recording has them; ``tau`` is in that unit.  staging.hot_pixel_mask marks the pixels that
fire far more often than any edge makes them; staging.event_support_weights gives every event the weight min(support, k) / k from its
neighbours' recent events, 0 for the lone ones; stage_datasample takes the weights as they are, beside the normalised times.  Isolated
noise flattens the IWE's contrast and hot pixels plant peaks that no warp moves: the flow error of both solves is printed."""
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
ap.add_argument('--tau-us', type=float, default=1500.0)
ap.add_argument('--radius', type=int, default=1)
ap.add_argument('--full-support', type=int, default=2)
a = ap.parse_args()

H, W, R, WINDOW_US = 96, 128, 3, 50_000
rng = np.random.default_rng(0)
win = synth.make_window(0, (H, W), a.events, R, flow='constant', flow_mag=8.0, noise_frac=0.0, n_segments=12, n_circles=2)
n_noise, n_hot = int(a.noise * a.events), a.events // 20
hot = [(17, 23), (60, 101)]                                                   # (y, x), each firing n_hot times at a steady rate
xs = np.concatenate([win['xs'], rng.integers(0, W, n_noise)] + [np.full(n_hot, x) for _, x in hot])
ys = np.concatenate([win['ys'], rng.integers(0, H, n_noise)] + [np.full(n_hot, y) for y, _ in hot])
t01 = np.concatenate([win['ts'], rng.random(n_noise)] + [np.linspace(0.0, 1.0, n_hot, endpoint=False)] * len(hot))
order = np.argsort(t01, kind='stable')
events = dict(x=xs[order].astype(np.int16), y=ys[order].astype(np.int16), t=np.floor(t01[order] * WINDOW_US).astype(np.int64) + 1_000_000)
n = len(events['x'])

mask = staging.hot_pixel_mask(events['x'], events['y'], (H, W), max_count=n_hot // 2)
weights, support = staging.event_support_weights(events, (H, W), a.tau_us, radius=a.radius, full_support=a.full_support, pixel_mask=mask,
                                                 return_support=True)
is_edge = order < a.events
print(f'{n} events: {a.events} on the edges, {n_noise} noise, {len(hot) * n_hot} on {len(hot)} hot pixels; {int(mask.sum())} pixels masked')
print(f'mean weight: edge events {weights[is_edge].mean():.3f}, the others {weights[~is_edge].mean():.3f}; '
      f'{int((weights == 0).sum())} events at weight 0, {int((weights == 1).sum())} at weight 1')

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
    print(f'{name}: theta ({th[0]:+.2f}, {th[1]:+.2f}), flow error {np.linalg.norm(th - truth):.3f} px after {r.nit} iterations')
