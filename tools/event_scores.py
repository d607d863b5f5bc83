"""What the per-event scores cost; writes profiles/event_scores.md.

Batches: the bench batch (8 windows of 10^6 events, 260x346, R = 5), 64 windows of 3 10^4 events on 256x336 (R = 3) and one 480x640
window of 10^7 events (R = 3).  Events are uniform over the sensor with sorted uniform times in [0, 1), as a recording hands them
over: in time order, not by pixel.  theta is a random (4, 4) grid within +-10 px, the caller's stack uniform in [-0.5, 1).

Forms: the per-reference and the combined output, each on the IWEs of the last evaluation (read on the device) and on a caller's
stack (uploaded by the call).  Beside them: one loss_grad (value and gradient) of the same batch on the
same context; the numpy route the call replaces - Engine.warped_events per window, then the witness's arithmetic in float32 on the
host - timed in the rounds on the small batch and once on the two large ones; and the floor of the bytes the call must move, over
PCIe (the scores down, a caller's stack up) and in HBM (12 bytes of event, 16 of Theta, 9 taps of 4 bytes per event and reference time
if no tap were shared or cached, 4 bytes of score per cell).

Per batch, in one process, on one context: 3 warm-up calls of every form; then --repeats rounds, each timing one call of every form in
turn, so that drift of the machine falls on all alike.  A call ends synchronised (its results are on the host), so the host clock
around it is the call's time: upload, kernel, download.  Each figure is the median of the rounds with their range.  The kernel's own
time comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/event_scores.py --case NAME --no-numpy

    python3 tools/event_scores.py [--repeats 7] [--out profiles/event_scores.md]
    python3 tools/event_scores.py --case NAME        one batch in this process, one JSON line"""
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
CASES = {                      # name: (sensor, windows, events per window, R, numpy route in every round)
    '8 x 1e6 on 260x346, R=5': ((260, 346), 8, 1_000_000, 5, False),
    '64 x 3e4 on 256x336, R=3': ((256, 336), 64, 30_000, 3, True),
    '1 x 1e7 on 480x640, R=3': ((480, 640), 1, 10_000_000, 3, False),
}
FORMS = ('per-r, IWE', 'combined, IWE', 'per-r, stack', 'combined, stack')
OTHERS = ('loss_grad', 'numpy route')

ap = argparse.ArgumentParser()
ap.add_argument('--case', default=None, choices=list(CASES))
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--no-numpy', action='store_true', help='leave the numpy route out (a run under the profiler)')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'event_scores.md'))
a = ap.parse_args()


def numpy_scores(wx, wy, F):
    """The witness's arithmetic (tests/_event_scores_witness.py) in float32 after the float64 rounding: (R, n) from the warped
    coordinates (R, n) and F (R, H, W)"""
    R, H, W = F.shape
    rx, ry = np.rint(wx), np.rint(wy)
    fx, fy = (wx - rx).astype(np.float32), (wy - ry).astype(np.float32)
    rx, ry = rx.astype(np.int64), ry.astype(np.int64)
    rows = np.arange(R)[:, None]
    s = np.zeros(wx.shape, dtype=np.float32)
    for dy in (-1, 0, 1):
        py = ry + dy
        py = np.where(py < 0, py + H, py)
        ky = np.exp(np.float32(-0.5) * (dy - fy) ** 2)
        for dx in (-1, 0, 1):
            px = rx + dx
            px = np.where(px < 0, px + W, px)
            ok = (py >= 0) & (py < H) & (px >= 0) & (px < W)
            k = ky * np.exp(np.float32(-0.5) * (dx - fx) ** 2) * np.float32(0.15915494309189535)
            s += np.where(ok, k * F[rows, np.clip(py, 0, H - 1), np.clip(px, 0, W - 1)], np.float32(0))
    return s


def case(name):
    sys.path.insert(0, ROOT)
    engine = importlib.import_module(f'{PKG}.engine')
    (H, W), B, n, R, numpy_every_round = CASES[name]
    rng = np.random.default_rng(len(name) + n)
    edge_ts = np.linspace(0.0, 1.0, R)
    wins = []
    for _ in range(B):
        wins.append((rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16), np.sort(rng.random(n)),
                     rng.random((R, H, W)), edge_ts))
    theta = rng.uniform(-10.0, 10.0, (B, 4, 4, 2))
    stack = rng.uniform(-0.5, 1.0, (B, R, H, W)).astype(np.float32)
    omega = engine.multi_ref_weights(R)
    p = engine.make_params(20.0, 35.0, 2.5e-4, 0.0, 1)
    cells = B * n * R
    out = {'case': name, 'events': B * n, 'R': R,
           'pcie_mb': {'per-r': cells * 4 / 1e6, 'combined': B * n * 4 / 1e6, 'stack up': stack.nbytes / 1e6},
           'hbm_mb': {'per-r': (B * n * 28 + cells * 40) / 1e6, 'combined': (B * n * 32 + cells * 36) / 1e6}}
    with engine.Engine((H, W), B * n, max_refs=R, max_windows=B) as eng:
        eng.set_windows(wins)
        eng.loss_grad(theta, p)

        def numpy_route():
            F = eng.iwes()
            return [numpy_scores(*eng.warped_events(b), F[b]) for b in range(B)]

        calls = {
            FORMS[0]: lambda: eng.event_scores(), FORMS[1]: lambda: eng.event_scores(ref_weights=omega),
            FORMS[2]: lambda: eng.event_scores(images=stack), FORMS[3]: lambda: eng.event_scores(images=stack, ref_weights=omega),
            OTHERS[0]: lambda: eng.loss_grad(theta, p),
        }
        for f in calls.values():
            for _ in range(3):
                f()
        ms = {k: [] for k in calls}
        if not a.no_numpy:
            ms[OTHERS[1]] = []
            if numpy_every_round:
                calls[OTHERS[1]] = numpy_route
            else:
                t0 = time.perf_counter()
                got = numpy_route()
                ms[OTHERS[1]].append((time.perf_counter() - t0) * 1e3)
                gpu = calls[FORMS[0]]()
                out['numpy_vs_gpu'] = float(max(np.abs(x - y).max() for x, y in zip(got, gpu)))
                del got, gpu
        for _ in range(a.repeats):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        out['ms'] = {k: [float(np.median(v)), float(min(v)), float(max(v)), len(v)] for k, v in ms.items()}
    print(json.dumps(out))


def driver():
    results = []
    for name in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--repeats', str(a.repeats)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f'{name} ended with {r.returncode}:\n{r.stderr[-2000:]}')          # nothing more is started on the GPU
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    cols = FORMS + OTHERS
    lines = ['# Per-event scores: what a call costs (MI355X)', '',
             f'`python3 tools/event_scores.py --repeats {a.repeats}`; the protocol and the batches are in the tool\'s docstring.',
             'Times in ms, host clock around a call that ends synchronised (upload, kernel and download), median of the rounds with their',
             'range in brackets, 3 warm-up calls of every form before them, the forms timed in turn within a round.  `numpy route` is',
             '`warped_events` per window and the same arithmetic in float32 on the host; where it shows no range it ran once.  The floors',
             'are bytes, not times: PCIe the scores down (and a caller\'s stack up), HBM the events, Theta, nine uncached taps and the',
             'scores.  Nothing here is asserted by a test.', '',
             '| batch | ' + ' | '.join(f'`{c}` ms' for c in cols) + ' | PCIe floor MB: per-r / combined / stack up | HBM floor MB: per-r / combined |',
             '|---|' + '---|' * (len(cols) + 2)]
    for r in results:
        def cell(k):
            if k not in r['ms']:
                return '-'
            med, lo, hi, cnt = r['ms'][k]
            return f'{med:.2f}' + (f' ({lo:.2f} … {hi:.2f})' if cnt > 1 else '')
        pc, hb = r['pcie_mb'], r['hbm_mb']
        lines.append(f'| {r["case"]} | ' + ' | '.join(cell(k) for k in cols) +
                     f' | {pc["per-r"]:.0f} / {pc["combined"]:.0f} / {pc["stack up"]:.1f} | {hb["per-r"]:.0f} / {hb["combined"]:.0f} |')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if a.case:
    case(a.case)
else:
    driver()
