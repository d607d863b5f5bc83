"""Cost of eincm_preprocess_image: ms per synchronous call for each stage alone and for the whole chain, at
260x346 and 480x640 for n = 1, 5 and 320 images, default parameters (the reference's), timed by HIP events around the call (uint8
copies in and out included), median over the steps.  Inputs: synth edge scenes plus noise.
    python3 tools/preprocess.py [--steps N]        (one JSON line per size, n and stage set on stdout)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eincm_amd  # noqa: E402,F401
from eincm_amd import engine as E, synth  # noqa: E402

STAGES = ['nlmeans', 'clahe', 'unsharp', 'bilateral', 'all']


def frames(shape, n, seed=0):
    rng = np.random.default_rng(seed)
    base = [synth.make_window(seed + k, shape, 10, 1, flow='zero')['edges'][0] for k in range(min(n, 5))]
    f = np.stack([40.0 + 170.0 * base[k % len(base)] for k in range(n)]) + rng.normal(0.0, 6.0, (n,) + shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def main():
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 20
    torch.cuda.init()
    for shape in ((260, 346), (480, 640)):
        with E.Engine(shape, max_events_total=1, max_refs=1) as eng:
            for n in (1, 5, 320):
                imgs = frames(shape, n)
                for stages in STAGES:
                    for _ in range(2):
                        eng.preprocess_image(imgs, stages)
                    t = []
                    for _ in range(steps):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        eng.preprocess_image(imgs, stages)     # synchronous: its stream has drained when it returns
                        b.record()
                        b.synchronize()
                        t.append(a.elapsed_time(b))
                    ms = float(np.median(t))
                    print(json.dumps({'shape': list(shape), 'n': n, 'stages': stages, 'ms_per_call': round(ms, 4),
                                      'us_per_image': round(1e3 * ms / n, 2)}), flush=True)


if __name__ == '__main__':
    main()
