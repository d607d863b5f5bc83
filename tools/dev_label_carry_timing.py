"""What carrying a segmentation's label prior to the next window costs on the GPU, against the only route there was before
(DESIGN.md section 33).

    python3 tools/dev_label_carry_timing.py [--runs 5] [--warmup 2] [--cells small large] [--no-host-route]

Per cell the batch is staged once with keep_order=True and random weights and evaluated once (outside every clock).  Then, in turn:

  device       Engine.carry_label_prior(K, coeffs, tau, radius, floor_mass, want=()) and Engine.adopt_carried_prior(K): the upload of
               the bin offsets, q and tau, one clear, four kernels (k_ml_mass, k_lc_splat, k_lc_resolve, k_label_prior) and one copy on
               the device; nothing comes down.  Each of the two calls is timed by a pair of HIP events recorded on the null stream
               around it (both end synchronised) and by the host clock.
  host route   what a caller did without the operator: Engine.staged_weights() brings the weights down, numpy forms the mass images
               (bincount), every model's field (MotionModel.field), the landing, the four integer tap weights and the uint64 deposit
               (np.add.at), the resolve rule, the box sums by a summed-area table and the division; the stack then goes up as
               prior_images of the E-step.  Host clock, up to the upload; the stack is compared with the carried prior, byte for byte.

and the E-step that follows, two ways, by HIP events and the host clock: Engine.event_responsibilities_spatial on the adopted prior,
and the same with the stack handed over from the host - the difference is what the upload costs the host route on top.

The cells are those of tools/dev_label_prior_timing.py: small = 8 groups x 2 models of 3*10^4 events at 256x336; large = 1 group x 4
models of 10^6 events at 480x640.  --warmup rounds, then --runs timed ones.  Medians and ranges are printed, one JSON line at the end.
--no-host-route times the device calls alone: the form to run under a kernel trace for the per-kernel split."""
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
ap.add_argument('--cells', nargs='+', default=['small', 'large'], choices=['small', 'large'])
ap.add_argument('--radius', type=int, default=2)
ap.add_argument('--tau', type=float, default=1.0)
ap.add_argument('--no-host-route', action='store_true', help='time the device calls alone (a run under a kernel trace)')
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


CELLS = {'small': ((256, 336), 8, 2, 30000), 'large': ((480, 640), 1, 4, 1000000)}   # sensor, groups, models, events
FLOOR = 4096


def host_carry(eng, model, lists, K, coeffs, tau, r, floor_mass):
    """The carried prior stack by the host route: the staged weights down, then the contract of DESIGN.md section 33 in numpy"""
    H, W = model.sensor_size
    npix = H * W
    w = eng.staged_weights()
    n_groups = len(lists)
    ys_, xs_ = np.mgrid[0:H, 0:W]
    carried = np.zeros((n_groups, K, H, W), dtype=np.uint32)
    for g in range(n_groups):
        pix = lists[g][1].astype(np.int64) * W + lists[g][0].astype(np.int64)
        with np.errstate(all='ignore'):
            f = model.field(coeffs[g * K:(g + 1) * K])
        for l in range(K):
            q = np.rint(np.asarray(w[g * K + l], dtype=np.float32) * np.float32(4096.0)).astype(np.float64)
            m = np.bincount(pix, weights=q, minlength=npix).astype(np.uint64).reshape(H, W)      # (sums below 2^53: exact)
            with np.errstate(all='ignore'):
                qx = xs_.astype(np.float64) + f[l, :, :, 0] * np.float64(tau)
                qy = ys_.astype(np.float64) + f[l, :, :, 1] * np.float64(tau)
                ok = (qx > -1.0) & (qx < float(W)) & (qy > -1.0) & (qy < float(H)) & (m > 0)
            qx, qy = qx[ok], qy[ok]
            fx, fy = np.floor(qx), np.floor(qy)
            ix, iy = np.rint((qx - fx) * 1024.0).astype(np.int64), np.rint((qy - fy) * 1024.0).astype(np.int64)
            x0, y0, mm = fx.astype(np.int64), fy.astype(np.int64), m[ok]
            acc = np.zeros(npix, dtype=np.uint64)
            for dy in (0, 1):
                for dx in (0, 1):
                    wt = ((ix if dx else 1024 - ix) * (iy if dy else 1024 - iy)).astype(np.uint64)
                    tx, ty = x0 + dx, y0 + dy
                    live = (wt > 0) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    np.add.at(acc, (ty * W + tx)[live], (mm * wt)[live])
            carried[g, l] = np.minimum((acc + np.uint64(1 << 19)) >> np.uint64(20), np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(H, W)
    mass = carried.astype(np.uint64)
    sat = np.zeros((n_groups, K, H + 1, W + 1), dtype=np.uint64)
    sat[:, :, 1:, 1:] = mass.cumsum(axis=2, dtype=np.uint64).cumsum(axis=3, dtype=np.uint64)
    y0, y1 = np.maximum(np.arange(H) - r, 0), np.minimum(np.arange(H) + r + 1, H)
    x0, x1 = np.maximum(np.arange(W) - r, 0), np.minimum(np.arange(W) + r + 1, W)
    S = (sat[:, :, y1[:, None], x1[None, :]] - sat[:, :, y0[:, None], x1[None, :]]) - \
        (sat[:, :, y1[:, None], x0[None, :]] - sat[:, :, y0[:, None], x0[None, :]])
    n = S + np.uint64(floor_mass)
    T = n.sum(axis=1, dtype=np.uint64)
    with np.errstate(invalid='ignore', divide='ignore'):
        p = (n.astype(np.float64) / T.astype(np.float64)[:, None]).astype(np.float32)
    return np.where((T == 0)[:, None], np.float32(1.0), p).astype(np.float32).reshape(n_groups * K, H, W)


def stats(t):
    t = np.asarray(t)
    return {'ms_median': float(np.median(t)), 'ms_min': float(t.min()), 'ms_max': float(t.max()), 'n': int(t.size)}


def show(s):
    return f'{s["ms_median"]:9.3f} ms ({s["ms_min"]:.3f} ... {s["ms_max"]:.3f}, n = {s["n"]})'


def timed(events, fn):
    events.record(0)
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    events.record(1)
    return out, events.elapsed_ms(), (t1 - t0) * 1e3


res = {'runs': a.runs, 'warmup': a.warmup, 'radius': a.radius, 'tau': a.tau}
for name in a.cells:
    (H, W), n_groups, K, n = CELLS[name]
    rng = np.random.default_rng(3)
    ws = [synth.make_window(700 + g, (H, W), n, 1, flow='constant', flow_mag=8.0) for g in range(n_groups)]
    lists = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in ws]
    weights = [rng.random(n, dtype=np.float32) * np.float32(0.5) + np.float32(0.5) for _ in range(n_groups * K)]
    model = motion.MotionModel('affine', (H, W))
    coeffs = rng.standard_normal((n_groups * K, model.n_coeffs)) * 4.0
    params = E.make_params(1.0, 0.0, 0.0, 0.0, 1)
    B, N = n_groups * K, n_groups * K * n
    out = res[name] = {'sensor': [H, W], 'groups': n_groups, 'models': K, 'events_per_group': n}
    print(f'== {name}: {n_groups} groups x {K} models of {n} events at {H}x{W}')
    with E.Engine((H, W), max(N, 1000), max_refs=1, max_windows=B) as eng:
        events = HipEvents()
        eng.set_motion_model(model)
        eng.set_motion_path('expanded')
        eng.set_windows([lists[g] for g in range(n_groups) for _ in range(K)], keep_order=True)
        eng.set_weights(weights)
        eng.loss_grad_motion(coeffs, params, want_grad=False, allow_nonfinite=True)
        t = {k: ([], []) for k in ('carry', 'adopt', 'e_step_adopted', 'e_step_host_stack')}
        t_route = []
        stack = None
        for k in range(a.warmup + a.runs):
            _, c_ms, c_host = timed(events, lambda: eng.carry_label_prior(K, coeffs, a.tau, a.radius, FLOOR, want=()))
            _, a_ms, a_host = timed(events, lambda: eng.adopt_carried_prior(K))
            _, e_ms, e_host = timed(events, lambda: eng.event_responsibilities_spatial(K, want=('labels', 'mass')))
            rounds = [('carry', c_ms, c_host), ('adopt', a_ms, a_host), ('e_step_adopted', e_ms, e_host)]
            if not a.no_host_route:
                t2 = time.perf_counter()
                stack = host_carry(eng, model, lists, K, coeffs, a.tau, a.radius, FLOOR)
                t3 = time.perf_counter()
                assert stack.tobytes() == eng.carried_prior().tobytes() == eng.staged_prior().tobytes(), 'the two routes differ'
                _, h_ms, h_host = timed(events, lambda: eng.event_responsibilities_spatial(K, stack, want=('labels', 'mass')))
                rounds.append(('e_step_host_stack', h_ms, h_host))
            if k >= a.warmup:
                for which, ms, host_ms in rounds:
                    t[which][0].append(ms)
                    t[which][1].append(host_ms)
                if not a.no_host_route:
                    t_route.append((t3 - t2) * 1e3)
        both = np.asarray(t['carry'][0]) + np.asarray(t['adopt'][0]), np.asarray(t['carry'][1]) + np.asarray(t['adopt'][1])
        out['carry_plus_adopt'] = {'hip_events': stats(both[0]), 'host_clock': stats(both[1])}
        print(f'  carry + adopt      : HIP events {show(out["carry_plus_adopt"]["hip_events"])}; host clock {show(out["carry_plus_adopt"]["host_clock"])}')
        for which in t:
            if t[which][0]:
                out[which] = {'hip_events': stats(t[which][0]), 'host_clock': stats(t[which][1])}
                print(f'  {which:19s}: HIP events {show(out[which]["hip_events"])}; host clock {show(out[which]["host_clock"])}')
        if t_route:
            out['host_route'] = stats(t_route)
            print(f'  host route         : {show(out["host_route"])}   (host clock, without the upload; the same bytes)')
print(json.dumps(res))
