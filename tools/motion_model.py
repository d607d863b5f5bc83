"""Time per loss_grad_motion beside the dense device-resident evaluation it is built on, at the bench's batch
(8 x [260x346, 1e6 events, R = 5]) and at one 480x640 window of 1e6 events; affine model, level 1, no TV term.

    python3 tools/motion_model.py [--runs 5] [--calls 200] [--events 1000000] [--dense-root TREE] [--out profiles/motion_model.md]
    python3 tools/motion_model.py --cell batch|dense480 --what motion|dense ...     one cell in this process, one JSON line

Every cell runs in a process of its own, started by the driver one after the other: stage, 20 warm-up calls, then --runs timed runs of
--calls calls each; a call is synchronous (it returns with the stream drained), so a host clock around a run measures it.  The figure
of a run is its mean time per call; the table has the median and the range of the runs.  The 'dense' cells call loss_grad_device on
the same field as a dense theta with the same bound of |theta|; --dense-root names the tree whose package they import (a checkout of
the parent commit with its library built: the yardstick is the parent's dense evaluation), default this tree.  They use nothing the
parent lacks.  The two kernels' own times come from a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/motion_model.py --cell batch --what motion"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = {'batch': ((260, 346), 8), 'dense480': ((480, 640), 1)}          # name: (sensor, windows)
R = 5
PKG = 'edge-informed-contrast-maximization_amd'

ap = argparse.ArgumentParser()
ap.add_argument('--cell', default=None, choices=list(CELLS))
ap.add_argument('--what', default='motion', choices=['motion', 'dense'])
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--calls', type=int, default=200)
ap.add_argument('--events', type=int, default=1_000_000)
ap.add_argument('--dense-root', default=ROOT)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'motion_model.md'))
a = ap.parse_args()


def affine_field(sensor, c):
    """The affine model's field in plain numpy (the 'dense' cells run on trees without motion.py)."""
    H, W = sensor
    s = max(H, W) / 2.0
    u = ((np.arange(W, dtype=np.float64) - (W - 1) / 2.0) / s)[None, :]
    v = ((np.arange(H, dtype=np.float64) - (H - 1) / 2.0) / s)[:, None]
    return np.ascontiguousarray(np.stack([c[0] + c[2] * u + c[3] * v, c[1] + c[4] * u + c[5] * v], axis=-1))


def cell(name, what):
    if what == 'dense':
        import torch                       # before the first Engine: the HIP runtime loaded first serves both
    sys.path.insert(0, a.dense_root if what == 'dense' else ROOT)
    synth, engine = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine'))
    sensor, B = CELLS[name]
    rng = np.random.default_rng(3)
    c_true = rng.uniform(0.4, 1.0, (B, 6)) * rng.choice([-1.0, 1.0], (B, 6)) * np.array([12.0, 12.0, 6.0, 6.0, 6.0, 6.0])
    wins = []
    for b in range(B):                     # (the scene's flow is constant: the parent's make_window takes no array; the timing does not need more)
        wins.append(synth.make_window(b, sensor, a.events, R, flow='constant', flow_mag=20.0))
        c_true[b, :2] = wins[b]['flow_gt'][0, 0]
    c = c_true * rng.uniform(0.8, 1.2, (B, 6))
    params = engine.make_params(20.0, 35.0, 0.0, 0.0, 1, 'bilinear')
    fields = np.stack([affine_field(sensor, c[b]) for b in range(B)])
    with engine.Engine(sensor, B * a.events, max_refs=R, max_windows=B) as eng:
        eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
        if what == 'motion':
            motion = importlib.import_module(f'{PKG}.motion')
            model = motion.MotionModel('affine', sensor)
            assert np.array_equal(model.field(c), fields)
            eng.set_motion_model(model)
            call = lambda: eng.loss_grad_motion(c, params)
        else:
            th = torch.from_numpy(fields).cuda()
            bound = float(np.abs(fields).max())
            call = lambda: eng.loss_grad_device(th, params, theta_abs_max=bound)
        for _ in range(20):
            v = call()[0]
        assert np.all(np.isfinite(v))
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call()
            runs.append((time.perf_counter() - t0) / a.calls * 1e6)
    print(json.dumps({'cell': name, 'what': what, 'us_per_call': runs, 'value0': float(v[0])}))


def fmt(runs):
    return f'{np.median(runs):.1f} ({min(runs):.1f} … {max(runs):.1f})'


def driver():
    rows = {}
    for name in CELLS:
        for what in ('dense', 'motion'):
            cmd = [sys.executable, os.path.abspath(__file__), '--cell', name, '--what', what, '--runs', str(a.runs), '--calls', str(a.calls),
                   '--events', str(a.events), '--dense-root', a.dense_root]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:          # a cell that failed ends the measurement: nothing more is started on the GPU
                sys.exit(f'cell {name} / {what} failed (exit {r.returncode}):\n{r.stderr[-3000:]}')
            rows[(name, what)] = json.loads(r.stdout.strip().splitlines()[-1])
            print(r.stdout.strip().splitlines()[-1], flush=True)
    lines = ['| | dense device evaluation, µs | loss_grad_motion, µs | difference of the medians, µs |', '|---|---|---|---|']
    for name, (sensor, B) in CELLS.items():
        d, m = rows[(name, 'dense')]['us_per_call'], rows[(name, 'motion')]['us_per_call']
        lines.append(f'| {B} × [{sensor[0]}×{sensor[1]}, {a.events} events, R = {R}] | {fmt(d)} | {fmt(m)} | {np.median(m) - np.median(d):+.1f} |')
    table = '\n'.join(lines)
    print(table)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(f'\n<!-- tools/motion_model.py --runs {a.runs} --calls {a.calls} --events {a.events} -->\n{table}\n')


if __name__ == '__main__':
    cell(a.cell, a.what) if a.cell else driver()
