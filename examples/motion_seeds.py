"""Start a motion segmentation without knowing the motions: the scene of examples/motion_segmentation.py - two
transparent layers of moving edges merged by time into one event list - but the EM's starting coefficients come from
segmentation.seed_motions, a coarse-to-fine search on the contrast landscape (Engine.contrast_landscape: one device operation per
grid) that finds the best motion, peels off the events it explains and searches the rest.  The EM of section 27 then runs from
those seeds.

    python3 examples/motion_seeds.py [--events 3000] [--iters 3] [--span 16]

The seeds with their distance from the layers' true flows are printed, then the label accuracy and the solved velocities per
iteration."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'edge-informed-contrast-maximization_amd'
synth, engine, motion, segmentation = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine', 'motion', 'segmentation'))

ap = argparse.ArgumentParser()
ap.add_argument('--events', type=int, default=3000, help='events of each layer')
ap.add_argument('--iters', type=int, default=3, help='EM iterations')
ap.add_argument('--span', type=float, default=16.0, help='half-range of the search in px per window')
a = ap.parse_args()

H, W, R = 64, 96, 2
flows = np.array([[12.0, 3.0], [-6.0, -9.0]])                                  # px per window, one per layer
layers = [synth.make_window(seed, (H, W), a.events, R, flow=np.broadcast_to(v, (H, W, 2)).copy(), n_segments=8, n_circles=2,
                            jitter_px=0.3, noise_frac=0) for seed, v in zip((1, 2), flows)]
ts = np.concatenate([l['ts'] for l in layers])
order = np.argsort(ts, kind='stable')                                          # the two layers merged by time
xs = np.concatenate([l['xs'] for l in layers])[order]
ys = np.concatenate([l['ys'] for l in layers])[order]
truth = (order >= a.events).astype(np.uint8)
edges = np.maximum(layers[0]['edges'], layers[1]['edges'])
window = (xs, ys, ts[order], edges, layers[0]['edge_ts'])

model = motion.MotionModel('translation', (H, W))
params = engine.make_params(1.0, 0.0, 0.0, 0.0, 1)                             # contrast alone: the edges of two layers overlap


def report(it, rec):
    v = rec['coeffs'][0]
    match = int(np.abs(v[0] - flows[0]).max() > np.abs(v[0] - flows[1]).max())  # the seeds come in the order they were found
    acc = float(((rec['labels'][0] ^ match) == truth).mean())
    print(f'iteration {it}: label accuracy {acc:.3f}; velocity ({v[0, 0]:+.2f}, {v[0, 1]:+.2f}) and ({v[1, 0]:+.2f}, {v[1, 1]:+.2f}); '
          f'mass {rec["mass"][0].round(1).tolist()}, {int(rec["n_unsupported"][0])} unsupported events')


print(f'{2 * a.events} events of two layers moving at {flows[0].tolist()} and {flows[1].tolist()} px per window')
with engine.Engine((H, W), 4 * a.events, max_refs=R, max_windows=2) as eng:
    seeds = segmentation.seed_motions(eng, [window], model, 2, a.span)
    for m in range(int(seeds['n_found'][0])):
        c = seeds['coeffs0'][0, m]
        err = np.abs(flows - c).max(axis=1)
        print(f'seed {m}: ({c[0]:+.3f}, {c[1]:+.3f}) from {int(seeds["n_kept"][0, m])} events, sum of squared counts {int(seeds["sumsq"][0, m])}; '
              f'{err.min():.3f} px from layer {int(err.argmin())}')
    if seeds['n_found'][0] < 2:
        sys.exit('fewer than two motions found')
    history = segmentation.segment_motions(eng, [window], model, seeds['coeffs0'], params, n_iters=a.iters, prior='uniform', callback=report)
v = history[-1]['coeffs'][0]
err = max(np.abs(v - f).max(axis=1).min() for f in flows)
print(f'largest velocity error {err:.3f} px')
