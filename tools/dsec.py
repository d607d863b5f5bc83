"""Cost of the DSEC data path on one GPU, each call beside the numpy witness (tests/_dsec_witness.py) on the
same machine's CPUs.  One JSON line per measurement:
  rectify   Engine.rectify_events over 1e7 and 1e8 random events (480x640, a map that sends ~9 % off the sensor): the whole call by the
            host clock (it ends in a device synchronise), median over the steps; the bytes that cross PCIe (4 per event up; 1 per
            event and 4 per kept event down) and the bytes its kernels move through HBM (k_rect_count: 4 in, 1 out; k_rect_scatter:
            4 in, 4 per kept event out; the 1.2 MB packed map is read through L2); the rate those PCIe bytes give over the call
  remap     Engine.remap_cubic of 5 frames 1080x1440 -> 480x640 through a homography
  encode    Engine.flow_encode of 64 theta at 16x16 (up-sampling and coding in one kernel; 118 MB of codes come down)
  every output is checked against the witness once (the encoder against the oracle's up-sampling, one code of slack at ties).
The kernels' own durations: `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/dsec.py --steps 2`, a
run of its own.
    python3 tools/dsec.py [--steps N] [--events 10000000,100000000]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, staging  # noqa: E402
from oracle import eincm_oracle as O  # noqa: E402
import _dsec_witness as DW  # noqa: E402

H, W = 480, 640


def _median_ms(fn, steps):
    t = []
    for _ in range(steps):
        s = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - s))
    return float(np.median(t))


def main():
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 5
    sizes = [int(float(v)) for v in sys.argv[sys.argv.index('--events') + 1].split(',')] if '--events' in sys.argv else [10**7, 10**8]
    rng = np.random.default_rng(0)
    m = DW.distortion_map(H, W)
    with E.Engine((H, W), max_events_total=1, max_refs=1) as eng:
        for n in sizes:
            x, y = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
            got = eng.rectify_events(x, y, m)                                     # warm-up: buffers, code objects
            s = time.perf_counter()
            want = DW.rectify_events(x, y, m)
            wit = 1e3 * (time.perf_counter() - s)
            assert got[3] == len(want[0]) and all(np.array_equal(a, b) for a, b in zip(got[:3], want))
            call = _median_ms(lambda: eng.rectify_events(x, y, m), steps)
            kept = got[3]
            pcie = 4 * n + n + 4 * kept
            print(json.dumps({'what': 'rectify', 'events': n, 'kept': kept, 'chunk': 1 << 22, 'call_ms': round(call, 2),
                              'pcie_bytes': pcie, 'pcie_GBps_over_call': round(pcie / call / 1e6, 2),
                              'hbm_bytes_kernels': 4 * n + n + 4 * n + 4 * kept, 'events_per_s': round(n / call * 1e3),
                              'witness_ms': round(wit, 1)}), flush=True)
            del x, y, got, want
        frames = rng.integers(0, 256, (5, 1080, 1440)).astype(np.uint8)
        mapping = staging.dsec_image_mapping(DW.dsec_like_calibration(3), (H, W))
        out = eng.remap_cubic(frames, mapping)
        s = time.perf_counter()
        want = DW.remap_cubic(frames, mapping)
        wit = 1e3 * (time.perf_counter() - s)
        assert np.array_equal(out, want)
        call = _median_ms(lambda: eng.remap_cubic(frames, mapping), steps)
        print(json.dumps({'what': 'remap', 'frames': list(frames.shape), 'out': list(out.shape), 'call_ms': round(call, 3),
                          'upload_bytes': int(frames.nbytes + mapping.nbytes + 65536), 'download_bytes': int(out.nbytes),
                          'witness_ms': round(wit, 1)}), flush=True)
        theta = rng.normal(0.0, 3.0, (64, 16, 16, 2))
        codes = eng.flow_encode(theta)
        s = time.perf_counter()
        scaled = np.stack([O.scale_theta_to_sensor_size(t, (H, W), 'bilinear') for t in theta])
        want = DW.flow_code(scaled)
        wit = 1e3 * (time.perf_counter() - s)
        d = np.abs(codes.astype(np.int64) - want.astype(np.int64))
        tie = np.abs(scaled * 128 - np.rint(scaled * 128)) < 1e-9
        assert d.max() <= 1 and np.all(d[..., :2][~tie] == 0)
        call = _median_ms(lambda: eng.flow_encode(theta), steps)
        print(json.dumps({'what': 'encode', 'theta': list(theta.shape), 'call_ms': round(call, 3), 'upload_bytes': int(theta.nbytes),
                          'download_bytes': int(codes.nbytes), 'f64_intermediate_bytes_avoided': int(scaled.nbytes),
                          'witness_ms': round(wit, 1)}), flush=True)


if __name__ == '__main__':
    main()
