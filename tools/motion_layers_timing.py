"""What composing a motion segmentation into a flow field costs on the GPU, against the route it replaces.

    python3 tools/motion_layers_timing.py [--runs 5] [--warmup 2] [--cells small large] [--no-host-route]

Per cell the batch is staged once with keep_order=True and random weights (outside every clock), then two routes produce the hard
labels and the dominant-filled Theta of every group:

  one call     Engine.compose_motions(K, coeffs, mode='hard', fill='dominant', want=('theta', 'labels')): uploads of the bin offsets and
               q, three kernels, the downloads of Theta and the labels.  Timed twice: by a pair of HIP events recorded around the call
               (hipEventRecord on the null stream through ctypes; the call ends synchronised, so the pair brackets all of its device
               work, its copies and the host work between them) and by the host clock.
  host route   what a caller did before the operator existed: Engine.staged_weights() (one float per event and model comes down), the
               masses by numpy's add.at on uint32, the labels by argmax, MotionModel.field of every model and a take along the labels.
               Host clock.  Its bytes are compared with the call's.

The cells: small = 8 groups x 2 models of 3*10^4 events at 256x336; large = 1 group x 4 models of 10^6 events at 480x640.  --warmup
calls of each route, then --runs timed ones, the routes in turn.  Also printed: the bytes the three kernels move (events and weights
in, masses out and in again, Theta and labels out) and the time those bytes take at the HBM's measured copy rate, the floor under
the kernels.  Medians and ranges are printed, one JSON line at the end."""
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
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--warmup', type=int, default=2)
ap.add_argument('--cells', nargs='+', default=['small', 'large'], choices=['small', 'large'])
ap.add_argument('--no-host-route', action='store_true', help='time the call alone (a run under a kernel trace)')
a = ap.parse_args()

import __graft_entry__ as G      # noqa: E402
G.build()
PKG = 'edge-informed-contrast-maximization_amd'
E, synth, motion = (importlib.import_module(f'{PKG}.{m}') for m in ('engine', 'synth', 'motion'))
import ctypes as C      # noqa: E402


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

CELLS = {'small': ((256, 336), 8, 2, 30000), 'large': ((480, 640), 1, 4, 1000000)}      # sensor, groups, models, events per group
HBM_COPY_TBS = 6.29                                                                   # measured float4 copy rate of the MI355X's HBM3E (8.0 peak)


def host_route(eng, model, lists, coeffs, n_groups, K):
    H, W = model.sensor_size
    w = eng.staged_weights()
    theta, labels = np.empty((n_groups, H, W, 2)), np.empty((n_groups, H, W), dtype=np.uint8)
    for g in range(n_groups):
        y, x = lists[g][1].astype(np.int64), lists[g][0].astype(np.int64)
        mass = np.zeros((K, H, W), dtype=np.uint32)
        for l in range(K):
            np.add.at(mass[l], (y, x), np.rint(w[g * K + l] * np.float32(4096.0)).astype(np.uint32))
        f = model.field(coeffs[g * K:(g + 1) * K])
        lab = np.argmax(mass, axis=0)
        has = mass.max(axis=0) > 0
        d = int(np.argmax(mass.astype(np.uint64).sum(axis=(1, 2))))
        theta[g] = np.take_along_axis(f, np.where(has, lab, d)[None, :, :, None], axis=0)[0]
        labels[g] = np.where(has, lab, 255)
    return theta, labels


def stats(t):
    t = np.asarray(t)
    return {'ms_median': float(np.median(t)), 'ms_min': float(t.min()), 'ms_max': float(t.max()), 'n': int(t.size)}


def show(s):
    return f'{s["ms_median"]:9.3f} ms ({s["ms_min"]:.3f} ... {s["ms_max"]:.3f}, n = {s["n"]})'


res = {'runs': a.runs, 'warmup': a.warmup}
for name in a.cells:
    (H, W), n_groups, K, n = CELLS[name]
    ws = [synth.make_window(700 + g, (H, W), n, 1, flow='constant', flow_mag=8.0) for g in range(n_groups)]
    lists = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in ws]
    rng = np.random.default_rng(3)
    weights = [rng.random(n, dtype=np.float32) for _ in range(n_groups * K)]
    model = motion.MotionModel('affine', (H, W))
    coeffs = rng.standard_normal((n_groups * K, model.n_coeffs)) * 4.0
    B, N, npix = n_groups * K, n_groups * K * n, H * W
    moved = {'k_ml_mass': N * 8 + B * npix * 4, 'k_ml_compose': B * npix * 4 + n_groups * npix * 17}
    out = res[name] = {'sensor': [H, W], 'groups': n_groups, 'models': K, 'events_per_group': n, 'kernel_bytes': moved,
                       'hbm_floor_us': {k: v / (HBM_COPY_TBS * 1e6) for k, v in moved.items()},
                       'downloaded_bytes': {'one_call': n_groups * npix * 17, 'host_route': N * 4}}
    print(f'== {name}: {n_groups} groups x {K} models of {n} events at {H}x{W}')
    with E.Engine((H, W), N, max_refs=1, max_windows=B) as eng:
        events = HipEvents()
        eng.set_motion_model(model)
        eng.set_windows([lists[g] for g in range(n_groups) for _ in range(K)], keep_order=True)
        eng.set_weights(weights)
        t_ev, t_host, t_route = [], [], []
        for k in range(a.warmup + a.runs):
            events.record(0)
            t0 = time.perf_counter()
            got = eng.compose_motions(K, coeffs, mode='hard', fill='dominant', want=('theta', 'labels'))
            t1 = time.perf_counter()
            events.record(1)
            ms = events.elapsed_ms()
            if not a.no_host_route:
                t2 = time.perf_counter()
                theta, labels = host_route(eng, model, lists, coeffs, n_groups, K)
                t3 = time.perf_counter()
                assert theta.tobytes() == got['theta'].tobytes() and labels.tobytes() == got['labels'].tobytes(), 'the two routes differ'
            if k >= a.warmup:
                t_host.append((t1 - t0) * 1e3)
                t_ev.append(ms)
                if not a.no_host_route:
                    t_route.append((t3 - t2) * 1e3)
        out['one_call_host_clock'] = stats(t_host)
        print(f'  one call, host clock : {show(out["one_call_host_clock"])}')
        if t_ev:
            out['one_call_hip_events'] = stats(t_ev)
            print(f'  one call, HIP events : {show(out["one_call_hip_events"])}')
        if t_route:
            out['host_route'] = stats(t_route)
            out['routes_byte_equal'] = True
            print(f'  host route           : {show(out["host_route"])}   (bytes equal to the call\'s)')
        for kname, nbytes in moved.items():
            print(f'  {kname:>14}: {nbytes / 1e6:9.2f} MB moved, {out["hbm_floor_us"][kname]:8.2f} us at {HBM_COPY_TBS} TB/s')
print(json.dumps(res))
