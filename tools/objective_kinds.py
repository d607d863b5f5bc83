"""Cost of the selectable objective kinds against the default kinds: ms per evaluation, the kinds alternating
evaluation by evaluation in one run (so that clocks and heat treat them alike), median of host-clock timings after a synchronise.
    python3 tools/objective_kinds.py [--steps N]        (one JSON line per workload and kind on stdout)
    python3 tools/objective_kinds.py --profile          (bench batch 2-DoF, adaptive_variance + joint_contrast only: for
                                                         rocprofv3 --kernel-trace --stats)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, synth  # noqa: E402

A, BETA = 20.0, 35.0
KINDS = [('grad_mag', 'mse'), ('adaptive_grad_mag', 'mse'), ('adaptive_variance', 'mse'), ('grad_mag', 'adaptive_mse'),
         ('grad_mag', 'hadamard'), ('grad_mag', 'joint_contrast'), ('adaptive_variance', 'joint_contrast')]


def measure(wins, theta, kinds, steps, warmup, lvl=1):
    H, W = wins[0]['sensor_size']
    R = len(wins[0]['edge_ts'])
    with E.Engine((H, W), sum(len(w['xs']) for w in wins), max_refs=R, max_windows=len(wins)) as eng:
        eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
        ps = [E.make_params(A, BETA, 0.0, 0.0, lvl, 'bilinear', ck, correlation_kind=rk) for ck, rk in kinds]
        for _ in range(warmup):
            for p in ps:
                eng.loss_grad(theta, p)
        ts = [[] for _ in ps]
        for _ in range(steps):
            for i, p in enumerate(ps):
                t0 = time.perf_counter()
                eng.loss_grad(theta, p)          # synchronous: returns after the stream has drained
                ts[i].append(time.perf_counter() - t0)
        return [float(np.median(t)) * 1e3 for t in ts]


def main():
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 50
    bench = [synth.make_window(1000 + b, (260, 346), 1_000_000, 5, flow='constant', flow_mag=20.0) for b in range(8)]
    if '--profile' in sys.argv:
        theta = np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)])
        ms = measure(bench, theta, [('adaptive_variance', 'joint_contrast')], 30, 5, 4)
        print(json.dumps({'workload': 'bench_batch_2dof', 'kinds': 'adaptive_variance+joint_contrast', 'ms_per_eval': round(ms[0], 4)}))
        return
    mv = synth.make_window(7, (256, 336), 30_000, 5, flow='smooth', flow_mag=10.0)
    for name, wins, theta, lvl in (
            ('bench_batch_2dof', bench, np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)]), 4),
            ('bench_batch_16x16', bench, np.stack([synth.theta_near_truth(b, w, (16, 16)) for b, w in enumerate(bench)]), 1),
            ('mvsec_256x336_3e4_R5_2dof', [mv], synth.theta_near_truth(0, mv, (1, 1))[None], 4)):
        ms = measure(wins, theta, KINDS, steps, 10, lvl)
        for (ck, rk), t in zip(KINDS, ms):
            print(json.dumps({'workload': name, 'contrast_kind': ck, 'correlation_kind': rk, 'ms_per_eval': round(t, 4),
                              'vs_default': round(t / ms[0], 3)}), flush=True)


if __name__ == '__main__':
    main()
