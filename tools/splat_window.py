"""Cost of the selectable splat window size against the default 3x3 splat: ms per evaluation, the sizes
alternating evaluation by evaluation in one run (one context per size, so that clocks and heat treat them alike), median of
host-clock timings of a synchronous loss_grad.
    python3 tools/splat_window.py [--steps N]        (one JSON line per workload and size on stdout)
    python3 tools/splat_window.py --profile SIZE     (bench batch 2-DoF at one size only: for rocprofv3 --kernel-trace --stats)"""
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
SIZES = (3, 1, 5, 7)


def measure(wins, theta, sizes, steps, warmup, lvl=1):
    H, W = wins[0]['sensor_size']
    R = len(wins[0]['edge_ts'])
    engs = []
    try:
        for s in sizes:
            eng = E.Engine((H, W), sum(len(w['xs']) for w in wins), max_refs=R, max_windows=len(wins))
            engs.append(eng)
            eng.set_splat_window(s)
            eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
        p = E.make_params(A, BETA, 0.0, 0.0, lvl, 'bilinear')
        for _ in range(warmup):
            for eng in engs:
                eng.loss_grad(theta, p)
        ts = [[] for _ in engs]
        for _ in range(steps):
            for i, eng in enumerate(engs):
                t0 = time.perf_counter()
                eng.loss_grad(theta, p)          # synchronous: returns after the stream has drained
                ts[i].append(time.perf_counter() - t0)
        return [float(np.median(t)) * 1e3 for t in ts]
    finally:
        for eng in engs:
            eng.close()


def main():
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 50
    bench = [synth.make_window(1000 + b, (260, 346), 1_000_000, 5, flow='constant', flow_mag=20.0) for b in range(8)]
    if '--profile' in sys.argv:
        s = int(sys.argv[sys.argv.index('--profile') + 1])
        theta = np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)])
        ms = measure(bench, theta, [s], 30, 5, 4)
        print(json.dumps({'workload': 'bench_batch_2dof', 'window_size': s, 'ms_per_eval': round(ms[0], 4)}))
        return
    mv = synth.make_window(7, (256, 336), 30_000, 5, flow='smooth', flow_mag=10.0)
    for name, wins, theta, lvl in (
            ('bench_batch_2dof', bench, np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)]), 4),
            ('bench_batch_16x16', bench, np.stack([synth.theta_near_truth(b, w, (16, 16)) for b, w in enumerate(bench)]), 1),
            ('mvsec_256x336_3e4_R5_2dof', [mv], synth.theta_near_truth(0, mv, (1, 1))[None], 4)):
        ms = measure(wins, theta, SIZES, steps, 10, lvl)
        for s, t in zip(SIZES, ms):
            print(json.dumps({'workload': name, 'window_size': s, 'ms_per_eval': round(t, 4), 'vs_default': round(t / ms[0], 3)}), flush=True)


if __name__ == '__main__':
    main()
