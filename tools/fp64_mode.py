"""Cost of the float64 mode (Engine(..., precision='fp64')) against the default fp32 path: time per evaluation of the workloads DESIGN.md
section 10 reports, the fp64 C port beside one of them, and BFGS engine calls / wall time at pyramid levels 4 and 3 of one window.
    python3 tools/fp64_mode.py [--quick]            (one JSON line per measurement on stdout)
    python3 tools/fp64_mode.py --profile            (fp64 bench batch only: what rocprofv3 --kernel-trace --stats runs)"""
import json
import os
import sys
import time
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, losses, solver as sol, synth  # noqa: E402

A, BETA = 20.0, 35.0


def time_eval(wins, theta, precision, steps, warmup, gamma=0.0, lvl=1):
    H, W = wins[0]['sensor_size']
    R = len(wins[0]['edge_ts'])
    with E.Engine((H, W), sum(len(w['xs']) for w in wins), max_refs=R, max_windows=len(wins), precision=precision) as eng:
        eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
        p = E.make_params(A, BETA, gamma, 0.0, lvl)
        for _ in range(warmup):
            eng.loss_grad(theta, p)
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.loss_grad(theta, p)
        return (time.perf_counter() - t0) / steps * 1e3


def profile():
    """--profile: only fp64 evaluations of the bench batch (2-DoF), for a kernel trace of the mode"""
    bench = [synth.make_window(1000 + b, (260, 346), 1_000_000, 5, flow='constant', flow_mag=20.0) for b in range(8)]
    theta = np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)])
    print(json.dumps({'workload': 'bench_batch_2dof', 'precision': 'fp64', 'ms_per_eval': round(time_eval(bench, theta, 'fp64', 20, 3, 0.0, 4), 4)}))


def main():
    if '--profile' in sys.argv:
        return profile()
    quick = '--quick' in sys.argv
    steps, warmup = (5, 2) if quick else (30, 5)
    rows = []
    bench = [synth.make_window(1000 + b, (260, 346), 1_000_000, 5, flow='constant', flow_mag=20.0) for b in range(8)]
    for name, wins, theta, gamma, lvl in (
            ('bench_batch_2dof', bench, np.stack([synth.theta_near_truth(b, w, (1, 1)) for b, w in enumerate(bench)]), 0.0, 4),
            ('bench_batch_16x16', bench, np.stack([synth.theta_near_truth(b, w, (16, 16)) for b, w in enumerate(bench)]), 0.0, 1),
            ('one_1e6_window_2dof', bench[:1], synth.theta_near_truth(0, bench[0], (1, 1))[None], 0.0, 4)):
        for prec in ('fp32', 'fp64'):
            rows.append({'workload': name, 'precision': prec, 'ms_per_eval': round(time_eval(wins, theta, prec, steps, warmup, gamma, lvl), 4)})
            print(json.dumps(rows[-1]), flush=True)
    mv = synth.make_window(7, (256, 336), 30_000, 5, flow='smooth', flow_mag=10.0)
    dn = synth.make_window(8, (480, 640), 1_000_000, 3, flow='smooth', flow_mag=15.0)
    for name, wins, theta in (('mvsec_256x336_3e4_R5_16x16', [mv], synth.theta_near_truth(0, mv, (16, 16))[None]),
                              ('dense_480x640_1e6_R3', [dn], (dn['flow_gt'] * 0.9)[None])):
        for prec in ('fp32', 'fp64'):
            rows.append({'workload': name, 'precision': prec, 'ms_per_eval': round(time_eval(wins, theta, prec, steps, warmup), 4)})
            print(json.dumps(rows[-1]), flush=True)
    from oracle import eincm_c_port as CP            # the fp64 C/OpenMP port, beside the one-window figure
    w0 = bench[0]
    th0 = synth.theta_near_truth(0, w0, (1, 1))
    args = (w0['xs'], w0['ys'], w0['ts'], w0['edges'], w0['edge_ts'])
    CP.loss_and_grad(th0, *args, A, BETA, (260, 346))
    t0 = time.perf_counter()
    n = 3 if quick else 10
    for _ in range(n):
        CP.loss_and_grad(th0, *args, A, BETA, (260, 346))
    print(json.dumps({'workload': 'one_1e6_window_2dof', 'precision': 'fp64 C port', 'threads': CP.max_threads(),
                      'ms_per_eval': round((time.perf_counter() - t0) / n * 1e3, 3)}), flush=True)
    # BFGS at pyramid levels 4 and 3 of one C4-like window: engine calls and wall time
    H, W = 260, 346

    def port_vg(theta, xs, ys, ts, edges, edge_ts, cur_pyr_lvl):
        v, g = CP.loss_and_grad(theta, xs, ys, ts, edges, edge_ts, A, BETA, (H, W))
        return (v, {}), g
    fns = {p: partial(losses.value_and_grad_loss_func, alpha=A, beta=BETA, gamma=0.0, delta=0.0, n_pyr_lvls=5, sensor_size=(H, W),
                      precision=p) for p in ('fp32', 'fp64')}
    fns['fp64 C port'] = port_vg
    for name, f in fns.items():
        start = np.zeros((1, 1, 2))
        for lvl, hw, maxiter in ((4, (1, 1), 8), (3, (2, 2), 11)):
            cnt = [0]

            def counted(theta, *a, _f=f, **k):
                cnt[0] += 1
                return _f(theta, *a, **k)
            s = sol.ScipyMinimize(fun=partial(counted, cur_pyr_lvl=lvl), method='BFGS', maxiter=maxiter, has_aux=True, options={'gtol': 1e-7})
            x0 = np.repeat(np.repeat(start, hw[0] // start.shape[0], 0), hw[1] // start.shape[1], 1)
            f(x0, *args, cur_pyr_lvl=lvl)                   # stage the window outside the timed solve
            t0 = time.perf_counter()
            th, st = s.run(x0, *args)
            dt = time.perf_counter() - t0
            print(json.dumps({'bfgs': name, 'level': lvl, 'status': int(st.status), 'nit': int(st.iter_num), 'calls': cnt[0],
                              'wall_ms': round(dt * 1e3, 2), 'theta00': [round(float(v), 6) for v in th[0, 0]]}), flush=True)
            start = th
    losses.clear_engine_cache()


if __name__ == '__main__':
    main()
