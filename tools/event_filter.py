"""What the refractory and polarity-aware event filter costs beside the event-support filter; writes
profiles/event_filter.md.

Cases: 10^6 events on 260x346 (one call, one chunk) and 10^7 on 480x640 (three chunks of 2^22, the default; the figure is per chunk:
the call's time over its number of chunks).  Events are uniform over the sensor with sorted uniform times in [0, 1) and random
polarity; tau is set so that a pixel's 3x3 neighbourhood holds two earlier events inside tau on average, radius 1, full_support 2,
as tools/event_support.py sets them.  Three forms of the filter are timed: refractory 0 without the polarity flag (the bytes of
event_support: asserted here), refractory tau / 4 without the flag, and refractory tau / 4 with it.

Per case, in one process, on one context: 3 warm-up calls of each operator; then --repeats rounds, each timing one call of
Engine.event_support and one of every form of Engine.event_filter on the same stream, in turn, so that drift of the machine falls on
all alike.  A call ends synchronised (its results are on the host), so the host clock around it is the call's time: upload, kernels,
download.  Each figure is the median of the rounds with their range.  The per-kernel split comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/event_filter.py --case NAME

    python3 tools/event_filter.py [--repeats 7] [--out profiles/event_filter.md]
    python3 tools/event_filter.py --case NAME        one case in this process, one JSON line"""
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
CASES = {                      # name: (sensor, events)
    '1e6 on 260x346': ((260, 346), 1_000_000),
    '1e7 on 480x640': ((480, 640), 10_000_000),
}
RADIUS, FULL_SUPPORT, CHUNK = 1, 2, 1 << 22
FORMS = ('event_support', 'event_filter rho=0', 'event_filter rho=tau/4', 'event_filter rho=tau/4 polarity')

ap = argparse.ArgumentParser()
ap.add_argument('--case', default=None, choices=list(CASES))
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'event_filter.md'))
a = ap.parse_args()


def stream(name):
    (H, W), n = CASES[name]
    rng = np.random.default_rng(len(name) + n)
    xs, ys = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
    ts = np.sort(rng.random(n))
    ps = rng.integers(0, 2, n).astype(np.int8)
    tau = 2.0 * H * W / (8.0 * n)              # 8 neighbours see n / (H W) * 8 * tau events inside tau: two
    return xs, ys, ts, ps, tau


def case(name):
    sys.path.insert(0, ROOT)
    engine = importlib.import_module(f'{PKG}.engine')
    (H, W), n = CASES[name]
    xs, ys, ts, ps, tau = stream(name)
    kw = dict(radius=RADIUS, full_support=FULL_SUPPORT, chunk=CHUNK)
    out = {'case': name, 'chunks': -(-n // CHUNK)}
    with engine.Engine((H, W), max_events_total=1, max_refs=1) as eng:
        calls = {
            FORMS[0]: lambda: eng.event_support(xs, ys, ts, tau, **kw),
            FORMS[1]: lambda: eng.event_filter(xs, ys, ts, ps, refractory=0.0, tau=tau, **kw),
            FORMS[2]: lambda: eng.event_filter(xs, ys, ts, ps, refractory=tau / 4.0, tau=tau, **kw),
            FORMS[3]: lambda: eng.event_filter(xs, ys, ts, ps, refractory=tau / 4.0, tau=tau, polarity=True, **kw),
        }
        w_es = calls[FORMS[0]]()
        keep, w = calls[FORMS[1]]()
        if w.tobytes() != w_es.tobytes() or not keep.all():
            sys.exit('event_filter at refractory 0 without the flag does not give the bytes of event_support')
        keep, w = calls[FORMS[3]]()
        out['kept'] = float(keep.mean())
        out['weights'] = [float((w == 0).mean()), float(((w > 0) & (w < 1)).mean()), float((w == 1).mean())]
        for f in calls.values():
            for _ in range(3):
                f()
        ms = {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        out['ms'] = {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in ms.items()}
    print(json.dumps(out))


def driver():
    rows = []
    for name in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', name, '--repeats', str(a.repeats)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f'{name} ended with {r.returncode}:\n{r.stderr[-2000:]}')          # nothing more is started on the GPU
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    lines = ['# The refractory and polarity-aware event filter: what a call costs beside `event_support` (MI355X)', '',
             f'`python3 tools/event_filter.py --repeats {a.repeats}`; the protocol and the streams are in the tool\'s docstring.',
             f'radius {RADIUS}, full_support {FULL_SUPPORT}, chunk 2^22; times in ms, host clock around a call that ends synchronised (upload,',
             'kernels and download), median of the rounds with their range in brackets, 3 warm-up calls of every form before them, the',
             'forms timed in turn within a round.  Where a call walks several chunks the figure is per chunk.  `kept` and the weights are',
             'those of the last form.  Nothing here is asserted by a test.', '',
             '| stream | chunks | ' + ' | '.join(f'`{f}` ms' for f in FORMS) + ' | rho=0 over `event_support` | kept | weights 0 / between / 1 |',
             '|---|---|' + '---|' * (len(FORMS) + 3)]
    for r in rows:
        c = r['chunks']
        cells = ' | '.join(f'{r["ms"][f][0] / c:.2f} ({r["ms"][f][1] / c:.2f} … {r["ms"][f][2] / c:.2f})' for f in FORMS)
        wz = ' / '.join(f'{100 * v:.0f} %' for v in r['weights'])
        lines.append(f'| {r["case"]} | {c} | {cells} | {r["ms"][FORMS[1]][0] / r["ms"][FORMS[0]][0]:.2f} | {100 * r["kept"]:.0f} % | {wz} |')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if a.case:
    case(a.case)
else:
    driver()
