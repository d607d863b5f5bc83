"""Cost of eincm_gt_flow: one call over 64 consecutive dt=4 windows at 256x336, float64 and float32 GT
stacks, against the numpy witness (tests/_gt_flow_witness.py) per window.  Synthetic MVSEC-like timestamps: GT at ~20 Hz, images at
~31 Hz.  Printed per stack type, one JSON line each:
  call_ms                 the whole synchronous Engine.gt_flow call (plans -> frames and steps up -> kernel -> (64,H,W,2)
                          float64 down) between HIP events, median over the steps; call_ms_host the same by the host clock
  upload_ms               the two frame stacks' pageable host-to-device copies alone (the same bytes, through torch), median
  download_ms             the (64,H,W,2) float64 result's pageable device-to-host copy alone (through torch), median
  rest_ms                 call_ms - upload_ms - download_ms: the kernel, the step tables and the launch
  witness_ms_per_window   the numpy witness, median over 8 windows (each checked bit-exact against the call's output)
The kernel's and each copy's own duration: run it under `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python3
tools/gt_flow.py --steps 5` (a run of its own).
    python3 tools/gt_flow.py [--steps N]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, evaluation as ev  # noqa: E402
import _gt_flow_witness as GW  # noqa: E402

H, W = 256, 336
N_WIN, DT = 64, 4


def sequence(seed=0):
    rng = np.random.default_rng(seed)
    gt_ts = 100.0 + np.cumsum(rng.uniform(0.048, 0.052, 60))
    image_ts = gt_ts[0] + 0.01 + np.cumsum(rng.uniform(0.030, 0.034, N_WIN + DT))
    yy, xx = np.mgrid[0:H, 0:W]
    gx = np.stack([1.5 * np.sin(xx / 40.0 + k) + 0.5 * rng.normal(0, 1, (H, W)) for k in range(len(gt_ts))])
    gy = np.stack([1.5 * np.cos(yy / 30.0 + k) + 0.5 * rng.normal(0, 1, (H, W)) for k in range(len(gt_ts))])
    gx[:, ::7, ::5] = 0.0
    return gt_ts, image_ts, gx, gy


def _event_ms(fn, steps):
    t = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def main():
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 20
    torch.cuda.init()
    gt_ts, image_ts, gx64, gy64 = sequence()
    t0, t1 = image_ts[:N_WIN], image_ts[DT:DT + N_WIN]
    plans = [ev.gt_flow_plan(gt_ts, a, b) for a, b in zip(t0, t1)]
    f_lo = min(f for p in plans for f, _, _ in p.steps)
    f_hi = max(f for p in plans for f, _, _ in p.steps)
    with E.Engine((H, W), max_events_total=1, max_refs=1) as eng:
        for name, dtype in (('float64', np.float64), ('float32', np.float32)):
            gx, gy = gx64.astype(dtype), gy64.astype(dtype)
            for _ in range(3):
                out = eng.gt_flow(gx, gy, plans)
            call = []
            for _ in range(steps):
                s = time.perf_counter()
                out = eng.gt_flow(gx, gy, plans)
                call.append(1e3 * (time.perf_counter() - s))
            full = _event_ms(lambda: eng.gt_flow(gx, gy, plans), steps)
            host = np.ascontiguousarray(gx[f_lo:f_hi + 1])
            tdt = torch.float64 if dtype == np.float64 else torch.float32
            dev = torch.empty(host.shape, dtype=tdt, device='cuda')
            src = torch.from_numpy(host)
            upload = 2 * _event_ms(lambda: dev.copy_(src), steps)
            dev_out = torch.zeros(out.shape, dtype=torch.float64, device='cuda')
            dst = torch.from_numpy(np.empty(out.shape))
            download = _event_ms(lambda: dst.copy_(dev_out), steps)
            wit = []
            for k in range(0, N_WIN, N_WIN // 8):
                s = time.perf_counter()
                w = GW.estimate_gt_flow(gx, gy, gt_ts, t0[k], t1[k])
                wit.append(1e3 * (time.perf_counter() - s))
                assert GW.same_bytes(w, out[k]), k
            print(json.dumps({
                'stack': name, 'shape': [H, W], 'windows': N_WIN, 'dt': DT, 'frames_uploaded': f_hi - f_lo + 1,
                'steps_per_window': [len(p.steps) for p in plans[:4]],
                'upload_bytes': int(2 * host.nbytes), 'download_bytes': int(out.nbytes),
                'call_ms': round(full, 3), 'call_ms_host': round(float(np.median(call)), 3), 'upload_ms': round(upload, 3),
                'download_ms': round(download, 3), 'rest_ms': round(full - upload - download, 3),
                'witness_ms_per_window': round(float(np.median(wit)), 3),
                'witness_ms_64_windows': round(64 * float(np.median(wit)), 1)}), flush=True)


if __name__ == '__main__':
    main()
