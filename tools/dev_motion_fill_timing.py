"""What the dense composition of a motion segmentation costs on the GPU, against the route it replaces.

    python3 tools/dev_motion_fill_timing.py [--runs 5] [--warmup 2] [--cells small large corner] [--no-host-route]

Per cell the batch is staged once with keep_order=True and random weights (outside every clock), then two routes produce the hard
labels and Theta of every pixel of every group, each pixel from its nearest labelled one:

  one call     Engine.densify_motions(K, coeffs, mode='hard', fallback='dominant', want=('theta', 'labels')): the uploads of the bin
               offsets and q, six kernels (k_ml_mass, k_ml_total, k_mf_sites, k_mf_cols, k_mf_rows, k_mf_compose), the downloads of
               Theta and the labels.  Timed by a pair of HIP events recorded on the null stream around the call (the call ends
               synchronised) and by the host clock.
  host route   what a caller does without the operator: Engine.compose_motions(want=('labels', 'mass')), then per group
               scipy.ndimage.distance_transform_edt(no mass here, return_distances=False, return_indices=True), the labels taken at
               the indices, MotionModel.field of every model and a take along the labels.  Host clock.  scipy resolves equal
               distances by a rule of its own, so the two routes' labels are compared where they must agree - the squared distance to
               the chosen site is equal everywhere - and the share of pixels with another site of the same distance is printed.

The cells: small = 8 groups x 2 models of 3*10^4 events at 256x336; large = 1 group x 4 models of 10^6 events at 480x640; corner = one
event in the last pixel of 480x640, so that every row search runs its whole width.  --warmup calls of each route, then --runs timed
ones, the routes in turn.  Medians and ranges are printed, one JSON line at the end.  The kernels' own times come from a run with
--no-host-route under a kernel trace."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--cells', nargs='+', default=['small', 'large', 'corner'], choices=['small', 'large', 'corner'])
ap.add_argument('--no-host-route', action='store_true', help='time the call alone (a run under a kernel trace)')
a = ap.parse_args()

import __graft_entry__ as G      # noqa: E402
G.build()
PKG = 'edge-informed-contrast-maximization_amd'
E, synth, motion = (importlib.import_module(f'{PKG}.{m}') for m in ('engine', 'synth', 'motion'))


class HipEvents:
    """A pair of HIP events on the null stream, straight from the HIP runtime the engine's library runs on"""

    def __init__(self):
        self.hip = C.CDLL(os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'libamdhip64.so'))
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def record(self, i):
        assert self.hip.hipEventRecord(self.ev[i], None) == 0

    def elapsed_ms(self):
        ms = C.c_float(0.0)
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0 and self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return float(ms.value)


CELLS = {'small': ((256, 336), 8, 2, 30000), 'large': ((480, 640), 1, 4, 1000000), 'corner': ((480, 640), 1, 1, 1)}   # sensor, groups, models, events


def host_route(eng, model, coeffs, n_groups, K):
    from scipy.ndimage import distance_transform_edt
    H, W = model.sensor_size
    r = eng.compose_motions(K, coeffs, mode='hard', fill='dominant', want=('labels', 'mass'))
    theta, labels = np.empty((n_groups, H, W, 2)), np.empty((n_groups, H, W), dtype=np.uint8)
    d2 = np.empty((n_groups, H, W), dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for g in range(n_groups):
        hole = r['mass'][g].astype(np.uint64).sum(axis=0) == 0
        iy, ix = distance_transform_edt(hole, return_distances=False, return_indices=True)
        labels[g] = r['labels'][g][iy, ix]
        d2[g] = (iy - yy) ** 2 + (ix - xx) ** 2
        f = model.field(coeffs[g * K:(g + 1) * K])
        theta[g] = np.take_along_axis(f, labels[g].astype(np.int64)[None, :, :, None], axis=0)[0]
    return theta, labels, d2


def stats(t):
    t = np.asarray(t)
    return {'ms_median': float(np.median(t)), 'ms_min': float(t.min()), 'ms_max': float(t.max()), 'n': int(t.size)}


def show(s):
    return f'{s["ms_median"]:9.3f} ms ({s["ms_min"]:.3f} ... {s["ms_max"]:.3f}, n = {s["n"]})'


res = {'runs': a.runs, 'warmup': a.warmup}
for name in a.cells:
    (H, W), n_groups, K, n = CELLS[name]
    rng = np.random.default_rng(3)
    if name == 'corner':
        lists = [(np.array([W - 1], np.int16), np.array([H - 1], np.int16), np.array([0.5]), np.ones((1, H, W)), np.array([0.5]))]
    else:
        ws = [synth.make_window(700 + g, (H, W), n, 1, flow='constant', flow_mag=8.0) for g in range(n_groups)]
        lists = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in ws]
    weights = [rng.random(n, dtype=np.float32) * np.float32(0.5) + np.float32(0.5) for _ in range(n_groups * K)]
    model = motion.MotionModel('affine', (H, W))
    coeffs = rng.standard_normal((n_groups * K, model.n_coeffs)) * 4.0
    B, N = n_groups * K, n_groups * K * n
    out = res[name] = {'sensor': [H, W], 'groups': n_groups, 'models': K, 'events_per_group': n}
    print(f'== {name}: {n_groups} groups x {K} models of {n} events at {H}x{W}')
    with E.Engine((H, W), max(N, 1000), max_refs=1, max_windows=B) as eng:
        events = HipEvents()
        eng.set_motion_model(model)
        eng.set_windows([lists[g] for g in range(n_groups) for _ in range(K)], keep_order=True)
        eng.set_weights(weights)
        extra = eng.densify_motions(K, coeffs, want=('dist2', 'n_sites'))
        out['sites_share'] = float(extra['n_sites'].sum() / (n_groups * H * W))
        out['dist2_max'] = int(extra['dist2'].max())
        print(f'  sites: {out["sites_share"]:.3f} of the pixels; largest squared distance {out["dist2_max"]}')
        t_ev, t_host, t_route = [], [], []
        for k in range(a.warmup + a.runs):
            events.record(0)
            t0 = time.perf_counter()
            got = eng.densify_motions(K, coeffs, mode='hard', fallback='dominant', want=('theta', 'labels'))
            t1 = time.perf_counter()
            events.record(1)
            ms = events.elapsed_ms()
            if not a.no_host_route:
                t2 = time.perf_counter()
                theta, labels, d2 = host_route(eng, model, coeffs, n_groups, K)
                t3 = time.perf_counter()
                assert np.array_equal(d2, extra['dist2'].astype(np.int64)), 'the two routes differ in a distance'
                same = labels == got['labels']
                out['labels_equal_share'] = float(same.mean())
                assert theta[same].tobytes() == got['theta'][same].tobytes(), 'the two routes differ where their labels agree'
            if k >= a.warmup:
                t_host.append((t1 - t0) * 1e3)
                t_ev.append(ms)
                if not a.no_host_route:
                    t_route.append((t3 - t2) * 1e3)
        out['one_call_host_clock'] = stats(t_host)
        out['one_call_hip_events'] = stats(t_ev)
        print(f'  one call, host clock : {show(out["one_call_host_clock"])}')
        print(f'  one call, HIP events : {show(out["one_call_hip_events"])}')
        if t_route:
            out['host_route'] = stats(t_route)
            print(f'  host route           : {show(out["host_route"])}   (distances equal everywhere; labels equal on '
                  f'{out["labels_equal_share"]:.4f} of the pixels, the rest are ties scipy resolves otherwise)')
print(json.dumps(res))
