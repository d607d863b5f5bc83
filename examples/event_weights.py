"""Per-event weights: stage one synthetic window whose events carry a time taper and a region mask, and
solve it with the lockstep solver beside the same window without weights.

    python3 examples/event_weights.py [--events 30000] [--grid 4]

The taper gives the first and last tenth of the window (the events a loader borrows from its neighbours when it pads a short window,
mvsec_loader.py:276-283) a weight that falls linearly to 0 at the borders; the mask gives the lowest fifth of the sensor (a car bonnet,
say) the weight 0.  A weight-0 event behaves as an absent one - in the IWEs, the gradient and the TV mask - and the event arrays are
staged as they are: no new event list, no new n_events."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'edge-informed-contrast-maximization_amd'
synth, engine, bsol = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine', 'batch_solver'))

ap = argparse.ArgumentParser()
ap.add_argument('--events', type=int, default=30000)
ap.add_argument('--grid', type=int, default=4, help='theta is (grid, grid, 2)')
a = ap.parse_args()

H, W, R = 96, 128, 3
win = synth.make_window(0, (H, W), a.events, R, flow='smooth', flow_mag=8.0)
xs, ys, ts = win['xs'], win['ys'], win['ts']

t01 = (ts - ts.min()) / (ts.max() - ts.min())
taper = np.clip(np.minimum(t01, 1.0 - t01) / 0.1, 0.0, 1.0)          # 0 at the time borders, 1 from a tenth of the window on
inside = ys < int(0.8 * H)                                            # the lowest fifth of the sensor is masked out
weights = engine.check_event_weights(taper * inside, len(xs))
print(f'{len(xs)} events: {int((weights == 0).sum())} masked, {int(((weights > 0) & (weights < 1)).sum())} tapered')

params = engine.make_params(20.0, 35.0, 2.5e-4, 0.0, 0)
theta0 = np.zeros((2, a.grid, a.grid, 2))
with engine.Engine((H, W), 2 * a.events, max_refs=R, max_windows=2) as eng:
    # one batch, two windows: the weighted one and the same events without weights
    eng.set_windows([(xs, ys, ts, win['edges'], win['edge_ts'], weights), (xs, ys, ts, win['edges'], win['edge_ts'], None)])
    assert eng.weighted
    stats = {}
    results = bsol.minimize_thetas(eng, theta0, params, maxiter=60, gtol=1e-6, stats=stats)
print(f'{stats["n_batch_evals"]} engine calls for {stats["n_window_evals"]} window evaluations')
truth = synth.theta_near_truth(0, win, (a.grid, a.grid))
for name, r in zip(('weighted', 'unweighted'), results):
    th = r.x.reshape(a.grid, a.grid, 2)
    print(f'{name}: loss {r.fun:.4f} after {r.nit} iterations, mean |theta - near-truth| {np.abs(th - truth).mean():.3f} px')
