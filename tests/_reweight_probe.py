"""Helper of tests/test_gpu_reweight.py: in THIS process (whose environment carries the launch switch under test) stage the batch of
tests/_reweight_scene.py with its first weight set and keep_order=True, set the second set in place, and evaluate at the 8 x 8 and the
dense theta; do the same on a fresh engine staged with the second set; write both results, the two indices and the environment to an
.npz.  Not a test module."""
import importlib
import json
import os
import sys

import numpy as np
import torch      # before the engine's library is loaded (tests/test_gpu_device_bfgs.py says why): mask_tensor hands out a torch view  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _reweight_scene as RS  # noqa: E402


def evaluate(eng, engine, c, res, tag):
    P = engine.make_params(RS.ALPHA, RS.BETA, RS.GAMMA, 0.0, 0)
    for name in ('theta8', 'dense'):
        v, g, aux = eng.loss_grad(c[name], P, want_aux=True)
        res[f'{tag}_{name}_v'], res[f'{tag}_{name}_g'] = v, g
        res[f'{tag}_{name}_aux'] = np.array([[a[k] for k in sorted(a)] for a in aux], dtype=np.float64)
        res[f'{tag}_{name}_iwe'] = eng.iwes()
    res[f'{tag}_mask'] = eng.mask_tensor().cpu().numpy()
    res[f'{tag}_zero'] = eng.zero_iwe()


def main(out_path):
    import __graft_entry__ as ge
    ge.build()
    engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
    c = RS.batch(synth)
    res = {'env': np.array(json.dumps({k: v for k, v in sorted(os.environ.items()) if k.startswith('EINCM_') and k != 'EINCM_LIB'}))}
    with engine.Engine((RS.H, RS.W), sum(RS.N), max_refs=RS.R, max_windows=RS.B) as eng:
        eng.set_windows(RS.staged(c, c['w1']), keep_order=True)
        eng.loss_grad(c['theta8'], engine.make_params(RS.ALPHA, RS.BETA, RS.GAMMA, 0.0, 0))       # (an evaluation that the re-weighting drops)
        eng.set_weights(c['w2'])
        res['order_splat'], res['order_gather'] = eng.staged_order()
        evaluate(eng, engine, c, res, 'inplace')
    with engine.Engine((RS.H, RS.W), sum(RS.N), max_refs=RS.R, max_windows=RS.B) as eng:
        eng.set_windows(RS.staged(c, c['w2']), keep_order=True)
        evaluate(eng, engine, c, res, 'fresh')
    np.savez(out_path, **res)


if __name__ == '__main__':
    main(sys.argv[1])
