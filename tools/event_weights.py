"""What per-event weights cost and what they do to the accuracy; writes profiles/event_weights.md.

Timing.  Two batches - the bench batch (8 x [260x346, 10^6 events, R = 5]) and one such window - each at a 2-DoF theta and a 16x16
theta, evaluated by loss_grad (theta changes every call, as bench.py does) with: the PARENT commit's library and package (unweighted),
this tree unweighted, this tree with all-ones weights, this tree with random weights ({0} u [1/8, 1], a fifth zero).  Every (batch,
what) runs in a process of its own, started by the driver one after the other, the parent and this tree's unweighted form twice,
alternating, so that the table shows the spread between two processes of the same code beside the differences.  In a process: stage
(timed: median of 3 set_windows calls), 20 warm-up calls, then --runs timed runs of --calls synchronous calls each; the figure of a run
is its mean time per call, the table has the median and the range of the runs.

Accuracy.  (260, 346), 10^5 events, R = 5, 16x16 theta, gamma = 2.5e-4 at level 0: relative error of value and gradient (max-norm)
against the fp64 witness (tests/_event_weights_witness.py) for weights drawn from [1/64, 1], [1/8, 1] and {1}.

    python3 tools/event_weights.py --parent-root TREE [--runs 5] [--calls 100] [--out profiles/event_weights.md]
    python3 tools/event_weights.py --cell bench|win1m --what parent|plain|ones|random ...     one cell in this process, one JSON line
    python3 tools/event_weights.py --accuracy                                                  the accuracy rows, one JSON line

--parent-root names a checkout of the parent commit with its library built."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'edge-informed-contrast-maximization_amd'
SENSOR, R, EVENTS = (260, 346), 5, 1_000_000
CELLS = {'bench': 8, 'win1m': 1}          # windows
THETAS = {'2dof': (1, 1), '16x16': (16, 16)}
WHATS = ('parent', 'plain', 'ones', 'random')

ap = argparse.ArgumentParser()
ap.add_argument('--cell', default=None, choices=list(CELLS))
ap.add_argument('--what', default='plain', choices=WHATS)
ap.add_argument('--accuracy', action='store_true')
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--calls', type=int, default=100)
ap.add_argument('--parent-root', default=None)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'event_weights.md'))
a = ap.parse_args()
if a.parent_root:
    a.parent_root = os.path.abspath(a.parent_root)


def draw(n, seed, lo):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.2, 0.0, rng.uniform(lo, 1.0, n)).astype(np.float32)


def cell(name, what):
    sys.path.insert(0, a.parent_root if what == 'parent' else ROOT)
    synth, engine = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine'))
    B = CELLS[name]
    wins = [synth.make_window(1000 + b, SENSOR, EVENTS, R, flow='constant', flow_mag=20.0) for b in range(B)]
    tup = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]
    if what == 'ones':
        tup = [t + (np.ones(EVENTS, dtype=np.float32),) for t in tup]
    elif what == 'random':
        tup = [t + (draw(EVENTS, 50 + b, 0.125),) for b, t in enumerate(tup)]
    p = engine.make_params(20.0, 35.0, 0.0, 0.0, 1)
    out = {'cell': name, 'what': what}
    with engine.Engine(SENSOR, B * EVENTS, max_refs=R, max_windows=B) as eng:
        st = []
        for _ in range(4):
            t0 = time.perf_counter()
            eng.set_windows(tup)
            st.append((time.perf_counter() - t0) * 1e3)
        out['set_windows_ms'] = float(np.median(st[1:]))          # (the first staging of a weighted batch allocates its two buffers)
        for tname, hw in THETAS.items():
            base = np.stack([synth.theta_near_truth(1000 + b, w, hw) for b, w in enumerate(wins)])
            thetas = [base * (1.0 + 0.01 * k) for k in range(5)]
            for k in range(20):
                v, g, _ = eng.loss_grad(thetas[k % 5], p)
            assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
            runs = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                for k in range(a.calls):
                    eng.loss_grad(thetas[k % 5], p)
                runs.append((time.perf_counter() - t0) / a.calls * 1e6)
            v, g, _ = eng.loss_grad(thetas[0], p)
            out[tname] = {'us': [float(np.median(runs)), float(min(runs)), float(max(runs))], 'value0': float(v[0]),
                          'gmax0': float(np.abs(g[0]).max())}
    print(json.dumps(out))


def accuracy():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    synth, engine = (importlib.import_module(f'{PKG}.{m}') for m in ('synth', 'engine'))
    from oracle import eincm_oracle as O
    import _event_weights_witness as EW
    (H, W), N, hw = SENSOR, 100_000, (16, 16)
    win = synth.make_window(11, SENSOR, N, R, flow='smooth', flow_mag=20.0)
    args = (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])
    th = synth.theta_near_truth(11, win, hw)
    AH, AW = O.resample_matrix(hw[0], H, H / hw[0], 'bilinear'), O.resample_matrix(hw[1], W, W / hw[1], 'bilinear')
    rng = np.random.default_rng(4)
    rows = []
    for label, w in (('[1/64, 1]', rng.uniform(1.0 / 64.0, 1.0, N)), ('[1/8, 1]', rng.uniform(0.125, 1.0, N)), ('{1}', np.ones(N))):
        v_w, g_w, _, I_w, _ = EW.loss_and_grad(th, *args, 20.0, 35.0, 2.5e-4, 0.0, 0, AH, AW, weights=w)
        with engine.Engine(SENSOR, N, max_refs=R) as eng:
            eng.set_window(*args, weights=w)
            v, g, _ = eng.loss_grad(th, engine.make_params(20.0, 35.0, 2.5e-4, 0.0, 0))
            iw = eng.iwes()[0]
        rows.append({'weights': label, 'value': abs(v[0] - v_w) / abs(v_w), 'grad': float(np.abs(g[0] - g_w).max() / np.abs(g_w).max()),
                     'iwe': float(np.abs(iw - I_w).max() / np.abs(I_w).max())})
    print(json.dumps({'accuracy': rows}))


def child(args):
    cmd = [sys.executable, os.path.abspath(__file__), '--runs', str(a.runs), '--calls', str(a.calls)] + args
    if a.parent_root:
        cmd += ['--parent-root', a.parent_root]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f'{" ".join(args)} ended with {r.returncode}:\n{r.stderr[-2000:]}')       # nothing more is started on the GPU
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def driver():
    if not a.parent_root:
        sys.exit('--parent-root TREE: a checkout of the parent commit with its library built')
    res = {}
    for name in CELLS:
        for what in ('parent', 'plain', 'ones', 'random', 'parent', 'plain'):
            res.setdefault((name, what), []).append(child(['--cell', name, '--what', what]))
    acc = child(['--accuracy'])['accuracy']
    fmt = lambda u: f'{u[0]:.1f} ({u[1]:.1f} … {u[2]:.1f})'
    lines = ['# Per-event weights: cost and accuracy (MI355X)', '',
             f'`python3 tools/event_weights.py --parent-root PARENT --runs {a.runs} --calls {a.calls}`; the protocol is in the tool\'s docstring.',
             'Times are µs per `loss_grad` call (median of the runs, their range in brackets); a row marked 2 is a second process of the',
             'same code, started after the others.', '']
    for name, B in CELLS.items():
        lines += [f'## {B} × [260×346, 10⁶ events, R = 5]', '', '| | 2-DoF θ | 16×16 θ | `set_windows` ms |', '|---|---|---|---|']
        label = {'parent': 'parent commit, unweighted', 'plain': 'this commit, unweighted', 'ones': 'this commit, all-ones weights',
                 'random': 'this commit, random weights'}
        for what in WHATS:
            for i, r in enumerate(res[(name, what)]):
                lines.append(f'| {label[what]}{" 2" if i else ""} | {fmt(r["2dof"]["us"])} | {fmt(r["16x16"]["us"])} | {r["set_windows_ms"]:.2f} |')
        par, pl, on = res[(name, 'parent')], res[(name, 'plain')], res[(name, 'ones')][0]
        for t in THETAS:
            same = all(r[t]['value0'] == par[0][t]['value0'] and r[t]['gmax0'] == par[0][t]['gmax0'] for r in par + pl + [on])
            lines.append(f'')
            lines.append(f'{t}: value and max|gradient| of window 0 at the first theta are {"the same bits" if same else "NOT the same bits"} in the parent, '
                         f'this commit unweighted and this commit with all-ones weights.')
        lines.append('')
    lines += ['## Error against the fp64 witness: (260, 346), 10⁵ events, R = 5, 16×16 θ, γ = 2.5·10⁻⁴ at level 0', '',
              '| weights drawn from | value | gradient (max-norm) | IWE stack (max-norm) |', '|---|---|---|---|']
    lines += [f'| {r["weights"]} | {r["value"]:.2e} | {r["grad"]:.2e} | {r["iwe"]:.2e} |' for r in acc]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if a.accuracy:
    accuracy()
elif a.cell:
    cell(a.cell, a.what)
else:
    driver()
