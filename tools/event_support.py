"""What the event-support filter costs; writes profiles/event_support.md.

Cases: 3*10^4 and 10^6 events on 260x346, 10^6 and 10^7 on 480x640, and 10^6 events that all sit on two adjacent pixels of
260x346 (every search runs in a list of 5*10^5 indices).  Events of the four spread cases are uniform over the sensor with sorted
uniform times in [0, 1); tau is set so that a pixel's 3x3 neighbourhood holds two earlier events inside tau on average, radius 1,
full_support 2.  The two-pixel stream alternates between its pixels at steps of tau / 4.

Per case, in one process: one context for the sensor; 3 warm-up calls; then --repeats timed calls of Engine.event_support on the
whole stream with the default chunk.  A call ends synchronised (its results are on the host), so the host clock around it is the
call's time: upload, kernels, download.  Beside it, in the same process: Engine.set_windows of the same events as one window with
R = 2 edge images (times normalised to [0, 1]), the project's nearest comparable pass over an event stream, timed the same way on a
context sized for it.  Each figure is the median of the repeats with their range.

The floor is what the bytes cost that the passes must move (nothing was measured to get it):
  device   per event: validate 12 in + 4 out; per sort pass 4 (histogram) + 8 in + 8 out (the first pass reads no values: 4 less);
           bounds 4; support 12 in + 5 out; at the 6.3 TB/s a copy kernel reaches (MI355X_MICROARCH.md).  The searches' reads are left
           out: they hit lists that the caches hold.
  link     12 bytes per event up, 5 down, at the 63 GB/s of PCIe Gen5 x16.

    python3 tools/event_support.py [--repeats 7] [--out profiles/event_support.md]
    python3 tools/event_support.py --case NAME        one case in this process, one JSON line"""
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
CASES = {                      # name: (sensor, events, two adjacent pixels only)
    '3e4 on 260x346': ((260, 346), 30_000, False),
    '1e6 on 260x346': ((260, 346), 1_000_000, False),
    '1e6 on 480x640': ((480, 640), 1_000_000, False),
    '1e7 on 480x640': ((480, 640), 10_000_000, False),
    '1e6 on two adjacent pixels of 260x346': ((260, 346), 1_000_000, True),
}
RADIUS, FULL_SUPPORT = 1, 2
HBM_BPS, LINK_BPS = 6.3e12, 63e9

ap = argparse.ArgumentParser()
ap.add_argument('--case', default=None, choices=list(CASES))
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'event_support.md'))
a = ap.parse_args()


def stream(name):
    (H, W), n, two = CASES[name]
    rng = np.random.default_rng(len(name) + n)
    if two:
        tau = 1.0
        xs, ys = (100 + np.arange(n) % 2).astype(np.int16), np.full(n, 100, dtype=np.int16)
        ts = np.arange(n) * (tau / 4.0)
    else:
        xs, ys = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
        ts = np.sort(rng.random(n))
        tau = 2.0 * H * W / (8.0 * n)          # 8 neighbours see n / (H W) * 8 * tau events inside tau: two
    return xs, ys, ts, tau


def floors(name):
    (H, W), n, _ = CASES[name]
    passes = -(-max(1, int(np.ceil(np.log2(H * W)))) // 8)
    device = n * (16 + passes * 20 - 4 + 4 + 17) + 2 * 4 * H * W * 2
    link = n * 17
    return passes, device / HBM_BPS * 1e3, link / LINK_BPS * 1e3


def timed(f, repeats, warm=3):
    for _ in range(warm):
        f()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(out)), float(min(out)), float(max(out))]


def case(name):
    sys.path.insert(0, ROOT)
    engine = importlib.import_module(f'{PKG}.engine')
    (H, W), n, _ = CASES[name]
    xs, ys, ts, tau = stream(name)
    out = {'case': name}
    with engine.Engine((H, W), max_events_total=1, max_refs=1) as eng:
        w, sup = eng.event_support(xs, ys, ts, tau, radius=RADIUS, full_support=FULL_SUPPORT, return_support=True)
        out['weights'] = [float((w == 0).mean()), float(((w > 0) & (w < 1)).mean()), float((w == 1).mean())]
        out['filter_ms'] = timed(lambda: eng.event_support(xs, ys, ts, tau, radius=RADIUS, full_support=FULL_SUPPORT), a.repeats)
    tn = (ts - ts[0]) / max(ts[-1] - ts[0], 1e-300)
    edges = np.random.default_rng(1).random((2, H, W))
    with engine.Engine((H, W), n, max_refs=2) as eng:
        out['staging_ms'] = timed(lambda: eng.set_windows([(xs, ys, tn, edges, np.array([0.0, 1.0]))]), a.repeats)
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
    fmt = lambda u: f'{u[0]:.2f} ({u[1]:.2f} … {u[2]:.2f})'
    lines = ['# The event-support filter: what a call costs (MI355X)', '',
             f'`python3 tools/event_support.py --repeats {a.repeats}`; the protocol, the streams and the floor are in the tool\'s docstring.',
             f'radius {RADIUS}, full_support {FULL_SUPPORT}; times in ms per call, host clock around a call that ends synchronised (upload,',
             'kernels and download), median of the repeats with their range in brackets, 3 warm-up calls before them.  `set_windows` is the',
             'staging of the same events as one window with two edge images, on the same commit, timed the same way.  Nothing here is',
             'asserted by a test.', '',
             '| stream | `event_support` ms | `set_windows` ms | sort passes | floor: device bytes ms | floor: host link ms | weights 0 / between / 1 |',
             '|---|---|---|---|---|---|---|']
    for r in rows:
        passes, dev, link = floors(r['case'])
        wz = ' / '.join(f'{100 * v:.0f} %' for v in r['weights'])
        lines.append(f'| {r["case"]} | {fmt(r["filter_ms"])} | {fmt(r["staging_ms"])} | {passes} | {dev:.3f} | {link:.3f} | {wz} |')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if a.case:
    case(a.case)
else:
    driver()
