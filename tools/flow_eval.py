"""Cost of the batched flow-error evaluation against the per-window path it stands beside, for the two batch
shapes of the lockstep solver: 8 windows of 260x346 and 64 windows of 256x336, theta (16, 16), bilinear, synthetic windows
(synth.make_window, 20000 events, 3 reference times).  Every timed call is synchronous (it returns with the stream drained), so the host
clock around it is the call's time.  Per shape, one JSON line with medians and (min, max) over the repeats, in ms per BATCH:
  stage_ms        BatchThetaEvaluator(...): set_windows + flow_eval_stage (once per batch, not per iterate)
  flow_errors_ms  BatchThetaEvaluator.flow_errors(thetas): thetas up, one kernel, 32 partials per window down
  evaluate_ms     BatchThetaEvaluator.evaluate(thetas): host up-sampling + one Engine.objectives call + flow_errors
  host_flow_ms    the per-window path for the flow errors alone: up-sampling (two matrix products) + per_pix_theta_to_flow + sparse_flow_error, B times
  host_eval_ms    the per-window path for everything: up-sampling + evaluate_theta_array (which stages the window again), B times
The two paths' figures are compared on the way (counts and A{N}PE equal, AEE within n_ee 2^-52 relative, the loss within 1e-5);
'paths_differ' lists what did not agree.
    python3 tools/flow_eval.py [--repeats N] [--host-repeats N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, evaluation as ev, synth  # noqa: E402

PARAMS = (20.0, 35.0, 2.5e-4, 0.0)
SHAPES = [(8, (260, 346)), (64, (256, 336))]
THETA_HW = (16, 16)
N_EVENTS, N_REFS = 20000, 3


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        out = fn()
    t = []
    for _ in range(repeats):
        s = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - s))
    return out, [round(float(np.median(t)), 3), round(min(t), 3), round(max(t), 3)]


def main():
    arg = lambda name, d: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else d      # noqa: E731
    repeats, host_repeats = arg('--repeats', 30), arg('--host-repeats', 5)
    for B, (H, W) in SHAPES:
        wins = [synth.make_window(b, (H, W), N_EVENTS, N_REFS, flow='smooth', flow_mag=10.0) for b in range(B)]
        windows = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]
        gts = np.stack([w['flow_gt'] for w in wins])
        thetas = np.stack([synth.theta_near_truth(b, w, THETA_HW) for b, w in enumerate(wins)])

        def stage():
            ev.BatchThetaEvaluator((H, W), windows, gts, *PARAMS).close()
        print(f'# {B} x {(H, W)}: windows made', file=sys.stderr, flush=True)
        _, stage_ms = timed(stage, max(3, host_repeats), warmup=1)
        with ev.BatchThetaEvaluator((H, W), windows, gts, *PARAMS) as be:
            fe, fe_ms = timed(lambda: be.flow_errors(thetas), repeats)
            res, eval_ms = timed(lambda: be.evaluate(thetas), repeats)

        A_H, A_W = E.resample_matrix(THETA_HW[0], H, 'bilinear'), E.resample_matrix(THETA_HW[1], W, 'bilinear')

        def scale(theta):                                    # A_H theta A_W^T as two matrix products
            return np.stack([A_H @ theta[..., c] @ A_W.T for c in range(2)], axis=-1)

        def host_flow():
            out = []
            for b in range(B):
                Theta = scale(thetas[b])
                out.append(ev.sparse_flow_error(ev.per_pix_theta_to_flow(Theta, windows[b][0], windows[b][1]), gts[b]))
            return out

        def host_eval():
            out = []
            for b in range(B):
                Theta = scale(thetas[b])
                out.append(ev.evaluate_theta_array(Theta, *windows[b], gts[b], *PARAMS, (H, W)))
            return out
        print('# device path timed', file=sys.stderr, flush=True)
        hf, hf_ms = timed(host_flow, host_repeats, warmup=1)
        print('# host flow path timed', file=sys.stderr, flush=True)
        he, he_ms = timed(host_eval, host_repeats, warmup=1)
        differ = []                                          # the two paths agree (reported, not fatal: this is a timing tool)
        for b in range(B):
            if fe[b]['counts'] != hf[b]['counts']:
                differ.append((b, 'counts'))
            for k, v in hf[b]['errors'].items():
                tol = 0.0 if k.endswith('PE') else fe[b]['counts']['n_ee'] * 2.0 ** -52 + 1e-12      # 1e-12: the up-sampling's tap order
                if not abs(fe[b]['errors'][k] - v) <= tol * abs(v):
                    differ.append((b, k))
            if not abs(res[b][0]['loss'] - he[b][0]['loss']) <= 1e-5 * abs(he[b][0]['loss']):
                differ.append((b, 'loss'))
        print(json.dumps({'windows': B, 'sensor': [H, W], 'theta': list(THETA_HW), 'events_per_window': N_EVENTS, 'refs': N_REFS,
                          'repeats': repeats, 'host_repeats': host_repeats, 'paths_differ': differ, 'median_min_max_ms': {
                              'stage_ms': stage_ms, 'flow_errors_ms': fe_ms, 'evaluate_ms': eval_ms, 'host_flow_ms': hf_ms,
                              'host_eval_ms': he_ms}}), flush=True)


if __name__ == '__main__':
    main()
