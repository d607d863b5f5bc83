"""A spatially coherent E-step: the two-region scene of examples/segmented_flow.py - the left and the right half
move with different translations - with uniformly random noise events added.  The scene is segmented twice from the same seeds
(segmentation.seed_motions): by segmentation.segment_motions_in_place, whose E-step decides every event on its own, and by
segmentation.segment_motions_spatial, whose E-step multiplies every model's mixing weight by that model's share of the mass around
the event's pixel (Engine.label_prior, formed on the device from the weights the E-step is about to replace).  For each it prints the
share of the non-noise events whose label matches their region (up to the permutation of the labels) and the dense AEE over all pixels
of the true flow after Engine.densify_motions.

    python3 examples/spatial_segmentation.py [--events 6000] [--noise 0.25] [--iters 3] [--span 16] [--radius 2] [--floor-mass 4096]
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'edge-informed-contrast-maximization_amd'
synth, engine, motion, segmentation = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine', 'motion', 'segmentation'))

ap = argparse.ArgumentParser()
ap.add_argument('--events', type=int, default=6000, help='events of the scene itself')
ap.add_argument('--noise', type=float, default=0.25, help='uniformly random events added, as a share of --events')
ap.add_argument('--iters', type=int, default=3, help='EM iterations')
ap.add_argument('--span', type=float, default=16.0, help='half-range of the seed search in px per window')
ap.add_argument('--radius', type=int, default=2, help='half-width of the label prior\'s box, 0 .. 8')
ap.add_argument('--floor-mass', type=int, default=4096, help='added to every model\'s box sum (4096 = one whole event)')
a = ap.parse_args()

H, W, R = 64, 96, 2
flows = np.array([[10.0, 2.0], [-7.0, -5.0]])                                  # px per window: the left half, the right half
left = np.broadcast_to(np.arange(W) < W // 2, (H, W))
flow_gt = np.where(left[..., None], flows[0], flows[1])
win = synth.make_window(3, (H, W), a.events, R, flow=flow_gt.copy(), n_segments=24, n_circles=6, jitter_px=0.3, noise_frac=0)
rng = np.random.default_rng(7)
n_noise = int(round(a.noise * a.events))
xs = np.concatenate([win['xs'], rng.integers(0, W, n_noise).astype(np.int16)])
ys = np.concatenate([win['ys'], rng.integers(0, H, n_noise).astype(np.int16)])
ts = np.concatenate([win['ts'], rng.uniform(win['ts'].min(), win['ts'].max(), n_noise)])
order = np.argsort(ts, kind='stable')
xs, ys, ts = xs[order], ys[order], ts[order]
scene = (order < a.events)                                                     # not noise
truth = (~left[ys, xs]).astype(np.uint8)                                       # the region every event fired in
window = (xs, ys, ts, win['edges'], win['edge_ts'])
n = len(xs)

model = motion.MotionModel('translation', (H, W))
params = engine.make_params(1.0, 0.0, 0.0, 0.0, 1)                             # contrast alone
K = 2

print(f'{a.events} events and {n_noise} noise events; the left half moves at {flows[0].tolist()}, the right half at {flows[1].tolist()} px per window')
with engine.Engine((H, W), 2 * K * n, max_refs=R, max_windows=K) as eng:
    seeds = segmentation.seed_motions(eng, [window], model, K, a.span)
    if seeds['n_found'][0] < K:
        sys.exit('fewer than two motions found')

    def report(name, rec):
        v = rec['coeffs'][0]
        swap = int(np.abs(v[0] - flows[0]).max() > np.abs(v[0] - flows[1]).max())     # the seeds come in the order they were found
        acc = float(((rec['labels'][0] ^ swap) == truth)[scene].mean())
        # the engine still holds the final weights in its staged layouts: the dense field needs no staging
        dense = eng.densify_motions(K, v.reshape(K, -1), mode='hard', fallback='dominant', want=('theta', 'labels'))
        aee = float(np.linalg.norm(dense['theta'][0] - flow_gt, axis=-1).mean())
        pix = float(((dense['labels'][0] ^ swap) == (~left).astype(np.uint8)).mean())
        print(f'{name}: velocities ({v[0, 0]:+.2f}, {v[0, 1]:+.2f}) and ({v[1, 0]:+.2f}, {v[1, 1]:+.2f}); label accuracy on the {int(scene.sum())} '
              f'non-noise events {acc:.4f}; dense pixel label accuracy {pix:.4f}; dense AEE over all {H * W} pixels {aee:.3f} px')

    plain = segmentation.segment_motions_in_place(eng, [window], model, seeds['coeffs0'], params, n_iters=a.iters, prior='uniform',
                                                  record_weights=False)
    report('per-event E-step (segment_motions_in_place)', plain[-1])
    spatial = segmentation.segment_motions_spatial(eng, [window], model, seeds['coeffs0'], params, radius=a.radius, floor_mass=a.floor_mass,
                                                   n_iters=a.iters, prior='uniform', record_weights=False)
    report(f'spatial E-step, radius {a.radius} (segment_motions_spatial)', spatial[-1])
