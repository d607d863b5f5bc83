"""What one call of the theta transport (Engine.advect_theta) costs on the GPU: B = 8 fields on a 480x640
sensor, from a 16x16 theta and from a dense theta, with a smooth flow of a few pixels per window.

    python3 tools/dev_theta_advect_timing.py [--runs 15] [--warmup 3] [--batch 8] [--sensor 480 640] [--outputs]
    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/dev_theta_advect_timing.py --runs 5      (the split per kernel)

A call uploads theta, zeroes the accumulators, runs k_ta_splat, k_ta_resolve and (for a coarse theta) the two reducers, downloads the
result and ends synchronised, so a host clock around it measures all of that.  --warmup calls of each form first, then the forms in
turn within a round, --runs rounds: the median and the range of each form are printed, one JSON line at the end.  --outputs also
asks for the dense field and the coverage (39 + 10 MB more over PCIe at the defaults).  Beside the times stand the bytes the splat
adds by atomics: taps that landed x 3 planes x 8 B, counted from the coverage of one extra call."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--runs', type=int, default=15)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--sensor', type=int, nargs=2, default=(480, 640))
ap.add_argument('--outputs', action='store_true')
a = ap.parse_args()

import __graft_entry__ as G      # noqa: E402
G.build()
E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')

H, W = a.sensor
B = a.batch
rng = np.random.default_rng(0)
coarse = rng.uniform(-12.0, 12.0, (B, 16, 16, 2))
dense = np.stack([synth._bilinear_field(coarse[b], H, W) for b in range(B)])
forms = {'16x16': coarse, 'dense': dense}
kw = dict(tau=1.0, gain=1.0, return_dense=a.outputs, return_coverage=a.outputs)
res = {'sensor': [H, W], 'batch': B, 'runs': a.runs, 'outputs': a.outputs}
with E.Engine((H, W), max_events_total=1, max_refs=1, max_windows=1) as eng:
    for name, th in forms.items():
        for _ in range(a.warmup):
            eng.advect_theta(th, **kw)
    times = {name: [] for name in forms}
    for _ in range(a.runs):
        for name, th in forms.items():
            t0 = time.perf_counter()
            eng.advect_theta(th, **kw)
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, th in forms.items():
        _, cov = eng.advect_theta(th, tau=1.0, return_coverage=True)
        t = np.array(times[name])
        # every landed tap adds three 8-byte words; the coverage sums the taps' weights, so it bounds them from below (4 taps a unit)
        landed = float(cov.astype(np.float64).sum())
        res[name] = {'ms_median': float(np.median(t)), 'ms_min': float(t.min()), 'ms_max': float(t.max()),
                     'theta_MB_up': th.nbytes / 1e6, 'covered_sources': landed, 'atomic_MB_at_4_taps': landed * 4 * 3 * 8 / 1e6,
                     'holes_percent': float(100.0 * (cov < 0.5).mean())}
        print(f'{name:>6}: {np.median(t):8.3f} ms ({t.min():.3f} ... {t.max():.3f}) per call of {B} fields on {H}x{W}; '
              f'{res[name]["atomic_MB_at_4_taps"]:.1f} MB of atomic adds, {res[name]["holes_percent"]:.1f} % holes')
print(json.dumps(res))
