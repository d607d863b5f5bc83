#!/usr/bin/env python3
"""Developer tool: record, or compare against, tests/golden/event_loop_edges/parent.npz - the bits a build computes on the cases of
tests/test_gpu_event_loop_edges.py and on the two bench batches (profiles/event_loop_trim.md).

  record (on the build whose bits are the yardstick; EINCM_LIB selects a variant of tools/build_variant.sh):
    python bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --no-latency --dump-outputs D1
    python bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --no-latency --theta 16x16 --dump-outputs D2
    python tools/record_event_loop_edges.py record OUT.npz D1 D2
  compare the bench dumps of another build with a recording (the small cases are compared by the test itself):
    python tools/record_event_loop_edges.py compare RECORDING.npz D1 D2
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def bench_arrays(d_default, d_16):
    out = {}
    for tag, d in (('bench_default', d_default), ('bench_16x16', d_16)):
        for what in ('loss', 'grad'):
            out[f'{tag}_{what}'] = np.load(os.path.join(d, what + '.npy'))
    return out


def main():
    mode, path, d1, d2 = sys.argv[1:5]
    bench = bench_arrays(d1, d2)
    if mode == 'record':
        import __graft_entry__ as ge
        ge.build()
        import _event_loop_edge_cases as E
        rec = E.record()
        rec.update(bench)
        np.savez_compressed(path, **rec)
        print(f'recorded {len(rec)} arrays, {os.path.getsize(path)} bytes')
        return 0
    ref = np.load(path, allow_pickle=False)
    bad = [k for k, v in bench.items() if not np.array_equal(v, ref[k])]
    for k, v in bench.items():
        print(f'{k}: shape {v.shape} float64 {"DIFFERS" if k in bad else "array_equal"}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
