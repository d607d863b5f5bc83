"""A window whose IWE has its maximum tied at several pixels (test helper)."""
import importlib

import numpy as np

synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')


def tied_window(H=24, W=32, R=2):
    """theta = 0 puts every event on its source pixel: six pixels, five apart, hold 3 events each (the maximum of every IWE, tied six
    ways, bit-exactly in any summation order), the rest of the events 1 or 2 per pixel"""
    win = synth.make_window(90, (H, W), 64, R, flow='constant', flow_mag=2.0)
    rng = np.random.default_rng(4)
    xs, ys = [], []
    for k, (y, x) in enumerate([(y, x) for y in range(2, H - 2, 5) for x in range(2, W - 2, 5)]):
        cnt = 3 if k % 3 == 0 and k < 18 else 1 + k % 2
        xs += [x] * cnt; ys += [y] * cnt
    win['xs'] = np.array(xs, dtype=np.int16); win['ys'] = np.array(ys, dtype=np.int16)
    win['ts'] = np.sort(rng.uniform(0.0, 1.0, len(xs)))
    return win
