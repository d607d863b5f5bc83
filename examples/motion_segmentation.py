"""Segment one window into two motions: two transparent layers of moving edges, each with its own constant flow,
are merged by time into one event list; expectation-maximisation then alternates between solving one translation per layer on the
events weighted by their responsibilities (the M-step, batch_solver.minimize_motion) and scoring every event under both motions, the
event's own share left out (the E-step, Engine.event_responsibilities, one device operation).

    python3 examples/motion_segmentation.py [--events 3000] [--iters 3] [--in-place]

--in-place stages the two windows once with keep_order=True and lets every E-step write its responsibilities straight into the staged
events (segmentation.segment_motions_in_place) instead of staging the batch again in every iteration: the same
numbers, byte for byte.  The label accuracy against the layer every event came from and the solved velocities are printed per iteration."""
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
ap.add_argument('--in-place', action='store_true', help='stage once and re-weight the staged events in place')
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
coeffs0 = (flows * np.array([[0.6], [1.4]]))[None]                             # (1 window, 2 models, 2 coefficients), off the truths


def report(it, rec):
    acc = float((rec['labels'][0] == truth).mean())
    v = rec['coeffs'][0]
    print(f'iteration {it}: label accuracy {acc:.3f}; velocity ({v[0, 0]:+.2f}, {v[0, 1]:+.2f}) and ({v[1, 0]:+.2f}, {v[1, 1]:+.2f}); '
          f'mass {rec["mass"][0].round(1).tolist()}, {int(rec["n_unsupported"][0])} unsupported events')


print(f'{2 * a.events} events of two layers moving at {flows[0].tolist()} and {flows[1].tolist()} px per window')
with engine.Engine((H, W), 4 * a.events, max_refs=R, max_windows=2) as eng:
    drive = segmentation.segment_motions_in_place if a.in_place else segmentation.segment_motions
    history = drive(eng, [window], model, coeffs0, params, n_iters=a.iters, prior='uniform', callback=report)
err = np.abs(history[-1]['coeffs'][0] - flows).max()
print(f'largest velocity error {err:.3f} px')
