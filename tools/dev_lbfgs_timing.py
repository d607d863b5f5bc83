"""Time per lockstep tick and per accept of the limited-memory BFGS state, device state against host state, on the
bench's windows (8 x [260x346, 1e6 events, R = 5]) at theta 32x32 and 64x64, on a dense 480x640 theta (8 windows of 1e6 events, level 0
with the TV term), and the dense-matrix device form beside the limited one at 16x16.

    python3 tools/dev_lbfgs_timing.py [--columns NAME,NAME,...] [--runs 5] [--history 10] [--events 1000000] [--out profiles/lbfgs.md]
    python3 tools/dev_lbfgs_timing.py --column NAME ...        one column in this process, one JSON line (what the driver starts)

Every column runs in a process of its own, started by the driver one after the other.  A run is: begin, the first evaluation, INIT,
then history + 5 times [one evaluation at a small fixed step (a tick), one UPDATE accept]; the figure of a run is the median over its
last five ticks / accepts (the ring is full by then).  One warm-up run, then --runs timed ones: the table has their median and range.
Beside each accept stands its floor: the bytes of two sweeps of the basis, 2 B (2 m + 1) n 8, at the 6 TB/s the microarchitecture guide
measured for streaming reads."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = {                     # name: (sensor, theta shape, level, gamma, state, hessian)
    '16x16 device dense': ((260, 346), (16, 16), 1, 0.0, 'device', 'dense'),
    '16x16 device limited': ((260, 346), (16, 16), 1, 0.0, 'device', 'limited'),
    '32x32 device': ((260, 346), (32, 32), 1, 0.0, 'device', 'limited'),
    '32x32 host': ((260, 346), (32, 32), 1, 0.0, 'host', 'limited'),
    '64x64 device': ((260, 346), (64, 64), 1, 0.0, 'device', 'limited'),
    '64x64 host': ((260, 346), (64, 64), 1, 0.0, 'host', 'limited'),
    'dense 480x640 device': ((480, 640), (480, 640), 0, 2.5e-4, 'device', 'limited'),
    'dense 480x640 host': ((480, 640), (480, 640), 0, 2.5e-4, 'host', 'limited'),
}
HBM_BYTES_PER_S = 6e12
B, R = 8, 5

ap = argparse.ArgumentParser()
ap.add_argument('--column', default=None)
ap.add_argument('--columns', default=','.join(COLUMNS))
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--history', type=int, default=10)
ap.add_argument('--events', type=int, default=1_000_000)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lbfgs.md'))
a = ap.parse_args()


def column(name):
    sys.path.insert(0, ROOT)
    PKG = 'edge-informed-contrast-maximization_amd'
    synth, engine, bsol = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine', 'batch_solver'))
    L = engine.L
    sensor, shape, lvl, gamma, where, hessian = COLUMNS[name]
    m = a.history
    wins = [synth.make_window(b, sensor, a.events, R, flow='constant', flow_mag=20.0) for b in range(B)]
    params = engine.make_params(20.0, 35.0, gamma, 0.0, lvl, 'bilinear')
    n = 2 * shape[0] * shape[1]
    with engine.Engine(sensor, B * a.events, max_refs=R, max_windows=B) as eng:
        eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])

        def fun_batch(X, mask):
            v, g, _ = eng.loss_grad(X.reshape((B,) + shape + (2,)), params, active=mask)
            return v, g.reshape(B, -1)
        if where == 'device':
            state = bsol.DeviceBFGSState(eng, shape + (2,), params) if hessian == 'dense' else bsol.DeviceLBFGSState(eng, shape + (2,), params, m)
        else:
            state = bsol.NumpyLBFGSState(fun_batch, m)
        everyone = np.ones(B, bool)

        def one_run():
            state.begin(np.zeros((B, n)), everyone)
            state.eval(np.zeros(B), everyone)
            sc = state.accept(np.zeros(B), np.full(B, L.BFGS_INIT, np.uint8))
            ticks, accepts = [], []
            for _ in range(m + 5):
                alpha = 0.05 / np.maximum(sc[:, L.BFGS_S_PMAX], 1e-300)          # a step of 0.05 px at the largest entry
                t0 = time.perf_counter()
                state.eval(alpha, everyone)
                t1 = time.perf_counter()
                sc = state.accept(alpha, np.full(B, L.BFGS_UPDATE, np.uint8))
                t2 = time.perf_counter()
                ticks.append(t1 - t0); accepts.append(t2 - t1)
            return float(np.median(ticks[-5:])), float(np.median(accepts[-5:]))
        one_run()
        runs = [one_run() for _ in range(a.runs)]
    basis = (2 * m + 1) if hessian == 'limited' else n          # the dense form reads and writes H: 3 n^2 doubles per accept
    floor = (2 * B * basis * n * 8 if hessian == 'limited' else 3 * B * n * n * 8) / HBM_BYTES_PER_S
    return {'column': name, 'n': n, 'history': m if hessian == 'limited' else None, 'tick_s': [r[0] for r in runs],
            'accept_s': [r[1] for r in runs], 'accept_floor_s': floor}


def fmt(v):
    return f'{1e6 * np.median(v):.1f} ({1e6 * min(v):.1f} .. {1e6 * max(v):.1f})'


if a.column is not None:
    print(json.dumps(column(a.column)))
    sys.exit(0)

rows = []
for name in [c.strip() for c in a.columns.split(',') if c.strip()]:
    if name not in COLUMNS:
        sys.exit(f'unknown column {name!r}: one of {sorted(COLUMNS)}')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--column', name, '--runs', str(a.runs), '--history', str(a.history),
                        '--events', str(a.events)], capture_output=True, text=True)
    if r.returncode != 0:                       # nothing more is started after a failure
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f'column {name!r} failed with status {r.returncode}')
    rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(rows[-1], flush=True)
lines = ['# Limited-memory lockstep BFGS: time per tick and per accept', '',
         f'B = {B} windows of {a.events} events, R = {R}, history {a.history}; microseconds, median (min .. max) of {a.runs} runs after a warm-up,',
         'one process per row (tools/dev_lbfgs_timing.py).  Floor: the bytes of two sweeps of the basis (the dense form: two reads and one',
         'write of H) at 6 TB/s.', '',
         '| column | n | tick | accept | accept floor | accept / floor |', '|---|---|---|---|---|---|']
for r in rows:
    ratio = np.median(r['accept_s']) / r['accept_floor_s']
    lines.append(f"| {r['column']} | {r['n']} | {fmt(r['tick_s'])} | {fmt(r['accept_s'])} | {1e6 * r['accept_floor_s']:.2f} | {ratio:.1f} |")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('\n'.join(lines))
