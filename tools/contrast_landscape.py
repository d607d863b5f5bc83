"""What the contrast landscape costs as one call, against the only route there was before it; writes
profiles/contrast_landscape.md.

Batches: one 256x336 window of 3 10^4 events; 16 such windows; one 260x346 window of 10^6 events.  Events are uniform over the sensor
less a margin of 10 px, with sorted uniform times in [0, 1), so that no candidate warps an event out of the sensor and the two routes
count the same events.  Per batch two grids of the seeding schedule, 'translation' model: 17 x 17 candidates of half-range 16 px at
cell 2, and 9 x 9 candidates of half-range 2 px around (4, -2) at cell 1; t_ref = 0.5, which is the middle of R = 3 reference times.

Routes: `one call` is Engine.contrast_landscape on the staged windows.  `evaluate + count images` is what a caller had before: the
batch staged so that one evaluation covers as many candidates as the engine holds windows (a single window is staged 16 times, the
10^6-event one 4 times; 16 windows take one candidate each per evaluation), then per batch of candidates
Engine.loss_grad_motion(coeffs, want_grad=False) on the engine's default path, Engine.count_images(), the image of reference time 0.5
binned to the cell size and squared in numpy.  Staging is outside the clock for both.  The two routes' integers are compared.

In one process: 3 warm-up calls of every route; then --repeats rounds, each timing one call of every route in turn.  A call ends
synchronised, so the host clock around it is its time.  Each figure is the median of the rounds with their range.  The whole
segmentation.seed_motions on the scene of examples/motion_seeds.py is timed the same way.  The kernel's resource line is taken from
hipcc's -Rpass-analysis=kernel-resource-usage on the kernel's header; where the measurement ran without the compiler, --resources
fills that block of an existing file in from a machine that has it (no GPU needed).  Nothing here is asserted by a test.

    python3 tools/contrast_landscape.py [--repeats 7] [--out profiles/contrast_landscape.md]
    python3 tools/contrast_landscape.py --resources [--out profiles/contrast_landscape.md]"""
import argparse
import importlib
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'edge-informed-contrast-maximization_amd'
sys.path.insert(0, ROOT)
engine, motion, segmentation, synth = (importlib.import_module(f'{PKG}.{m}') for m in ('engine', 'motion', 'segmentation', 'synth'))

R, MARGIN = 3, 10
CASES = {                      # name: (sensor, windows, events per window, copies of a window the old route stages)
    '1 x [256x336, 3e4 events]': ((256, 336), 1, 30_000, 16),
    '16 x [256x336, 3e4 events]': ((256, 336), 16, 30_000, 1),
    '1 x [260x346, 1e6 events]': ((260, 346), 1, 1_000_000, 4),
}
GRIDS = {'17 x 17, cell 2': (np.zeros(2), 16.0, 17, 2), '9 x 9, cell 1': (np.array([4.0, -2.0]), 2.0, 9, 1)}
ROUTES = ('one call', 'evaluate + count images')

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=7)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'contrast_landscape.md'))
ap.add_argument('--resources', action='store_true', help='only rewrite the resource block of --out')
a = ap.parse_args()
NO_HIPCC = '    (no hipcc where the tool ran)'
P = engine.make_params(1.0, 0.0, 0.0, 0.0, 1)


def timed(calls, repeats):
    for f in calls.values():
        for _ in range(3):
            f()
    ms = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def case(name):
    (H, W), B, n, copies = CASES[name]
    rng = np.random.default_rng(len(name) + n)
    edge_ts = np.linspace(0.0, 1.0, R)
    wins = [(rng.integers(MARGIN, W - MARGIN, n).astype(np.int16), rng.integers(MARGIN, H - MARGIN, n).astype(np.int16), np.sort(rng.random(n)),
             rng.random((R, H, W)), edge_ts) for _ in range(B)]
    model = motion.MotionModel('translation', (H, W))
    rows = []
    with engine.Engine((H, W), B * n, max_refs=R, max_windows=B) as new, engine.Engine((H, W), B * copies * n, max_refs=R, max_windows=B * copies) as old:
        new.set_windows(wins)
        new.set_motion_model(model)
        old.set_windows([w for w in wins for _ in range(copies)])
        old.set_motion_model(model)
        for gname, (centre, span, count, cell) in GRIDS.items():
            cands = motion.coefficient_grid(model, centre, (0, 1), span, count)
            V = len(cands)
            coeffs = np.ascontiguousarray(np.broadcast_to(cands, (B, V, 2)))

            def one_call():
                return new.contrast_landscape(coeffs, cell=cell, want='sumsq')['sumsq']

            def old_route():
                out = np.zeros((B, V), dtype=np.uint64)
                for v0 in range(0, V, copies):
                    idx = np.minimum(np.arange(v0, v0 + copies), V - 1)                          # (the last batch repeats its last candidate)
                    old.loss_grad_motion(coeffs[:, idx].reshape(B * copies, 2), P, want_grad=False)
                    cnt = old.count_images()[:, R // 2].reshape(B, copies, H // cell, cell, W // cell, cell).sum(axis=(3, 5), dtype=np.uint64)
                    out[:, idx] = (cnt * cnt).sum(axis=(2, 3))
                return out

            equal = bool(np.array_equal(one_call(), old_route()))
            ms = timed({ROUTES[0]: one_call, ROUTES[1]: old_route}, a.repeats)
            rows.append((name, gname, ms, equal, B * copies * R * H * W * 4 * -(-V // copies) / 1e6))
            print(name, gname, ms, 'equal' if equal else 'DIFFERENT', flush=True)
    return rows


def seeding():
    H, W, n_layer = 64, 96, 3000
    flows = np.array([[12.0, 3.0], [-6.0, -9.0]])
    layers = [synth.make_window(seed, (H, W), n_layer, 2, flow=np.broadcast_to(v, (H, W, 2)).copy(), n_segments=8, n_circles=2, jitter_px=0.3,
                                noise_frac=0) for seed, v in zip((1, 2), flows)]
    ts = np.concatenate([l['ts'] for l in layers])
    order = np.argsort(ts, kind='stable')
    window = (np.concatenate([l['xs'] for l in layers])[order], np.concatenate([l['ys'] for l in layers])[order], ts[order],
              np.maximum(layers[0]['edges'], layers[1]['edges']), layers[0]['edge_ts'])
    model = motion.MotionModel('translation', (H, W))
    with engine.Engine((H, W), 4 * n_layer, max_refs=2, max_windows=2) as eng:
        out = segmentation.seed_motions(eng, [window], model, 2, 16)
        ms = timed({'seed_motions': lambda: segmentation.seed_motions(eng, [window], model, 2, 16)}, a.repeats)['seed_motions']
    err = [float(np.abs(out['coeffs0'][0] - f).max(axis=1).min()) for f in flows]
    print('seed_motions', ms, out['coeffs0'][0].tolist(), err, flush=True)
    return ms, out['coeffs0'][0], err


def resource_lines():
    """hipcc's resource remarks of k_contrast_landscape, or None where there is no hipcc"""
    hipcc = os.environ.get('HIPCC', 'hipcc')
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'tu.hip')
        with open(src, 'w') as f:
            f.write('#include "eincm_contrast_landscape.hip.h"\n')
        cmd = [hipcc, '-O3', '--offload-arch=gfx950', '-std=c++17', '-fno-slp-vectorize', '--offload-device-only', '-c', '-o', os.path.join(d, 'tu.o'),
               '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, PKG, 'csrc'), '-Rpass-analysis=kernel-resource-usage', src]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        except (OSError, subprocess.TimeoutExpired):
            return None
    got, on = [], False
    for line in r.stderr.splitlines():
        m = re.search(r'remark: +(?:\S+:\d+:\d+: +)?(.*?) \[-Rpass-analysis', line)        # (the location stands before or after the word)
        if not m:
            continue
        if 'Function Name' in m.group(1):
            on = 'k_contrast_landscape' in m.group(1)
        elif on:
            got.append(m.group(1).strip())
    return got or None


def main():
    rows = [r for name in CASES for r in case(name)]
    seed_ms, seeds, seed_err = seeding()
    res = resource_lines()
    fmt = lambda t: f'{t[0]:.2f} ({t[1]:.2f} … {t[2]:.2f})'
    lines = ['# The contrast landscape as one call: what it costs against evaluating candidate by candidate (MI355X)', '',
             f'`python3 tools/contrast_landscape.py --repeats {a.repeats}`; the protocol, the batches and the two routes are in the tool\'s docstring.',
             'Times in ms, host clock around a route that ends with its integers on the host, median of the rounds with their range in',
             'brackets, 3 warm-up calls of every route before them, the routes timed in turn within a round, staging outside the clock.',
             'The download column is what `evaluate + count images` fetches per grid (the count images of every reference time); the',
             'call fetches 8 bytes per window and candidate.  Nothing here is asserted by a test.', '',
             '| batch | grid | ' + ' | '.join(f'`{c}` ms' for c in ROUTES) + ' | ratio of the medians | count images fetched, MB | the two routes\' integers |',
             '|---|---|---|---|---|---|---|']
    for name, gname, ms, equal, mb in rows:
        lines.append(f'| {name} | {gname} | {fmt(ms[ROUTES[0]])} | {fmt(ms[ROUTES[1]])} | {ms[ROUTES[1]][0] / ms[ROUTES[0]][0]:.0f}x | {mb:.0f} | '
                     f'{"equal" if equal else "DIFFERENT"} |')
    lines += ['', f'`segmentation.seed_motions` on the scene of examples/motion_seeds.py (64x96, 6000 events of two layers, two motions, three levels each:',
              f'six calls of the operator and two peels on the host): {fmt(seed_ms)} ms; seeds ({seeds[0, 0]:+.3f}, {seeds[0, 1]:+.3f}) and '
              f'({seeds[1, 0]:+.3f}, {seeds[1, 1]:+.3f}), {seed_err[0]:.3f} and {seed_err[1]:.3f} px from the layers\' flows.', '',
              '`k_contrast_landscape`, `-Rpass-analysis=kernel-resource-usage` (gfx950; the LDS is dynamic, sized per launch by `cl_bands`, 64 KiB at the most):',
              '']
    lines += ['    ' + l for l in res] if res else [NO_HIPCC]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


def resources_only():
    res = resource_lines()
    if not res:
        sys.exit('no resource remarks: is hipcc here?')
    text = open(a.out).read()
    head, mark, _ = text.partition('`k_contrast_landscape`, `-Rpass-analysis')
    if not mark:
        sys.exit(f'{a.out} has no resource block')
    block = (mark + text[len(head) + len(mark):]).split('\n\n')[0]
    with open(a.out, 'w') as f:
        f.write(head + block + '\n\n' + '\n'.join('    ' + l for l in res) + '\n')
    print('wrote', a.out)


if a.resources:
    resources_only()
else:
    main()
