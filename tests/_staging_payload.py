"""The cases of tests/test_gpu_staging_payload.py and of tools/record_staging_payload.py, and the child process that computes them.
Not a test module.

A record is what RS.answers() collects on the batch of tests/_reweight_scene.py in one of four payload situations - plain; weighted
with w1; keep-order with w1; keep-order with w1, then set_weights(w2) - and, for the keep-order ones, staged_order() and
staged_weights().  The four are computed in ONE process whose environment carries the launch setting under test:

    python tests/_staging_payload.py OUT.json

Every array is stored as dtype, shape and the SHA-256 of its bytes; a float scalar, and a float array of at most FULL elements (the
values, the aux blocks, the motion gradients), as C99 hex floats instead - exact, so equality of the text is equality of the bytes, and
a mismatch shows a number."""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch      # before the engine's library is loaded (tests/test_gpu_device_bfgs.py says why): mask_tensor hands out a torch view  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SITUATIONS = ('plain', 'weighted', 'keep_order', 'keep_order_reweighted')
SETTINGS = [('default', {}), ('host-binning', {'EINCM_HOST_BINNING': '1'}), ('no-segsort', {'EINCM_NO_SEGSORT': '1'}),
            ('no-spread', {'EINCM_NO_SPREAD': '1'})]
FULL = 32


def encode(x):
    if x is None or isinstance(x, (str, bool, int)):
        return x
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {str(k): encode(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    a = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, 'detach') else x)
    out = {'dtype': a.dtype.str, 'shape': list(a.shape)}
    if a.dtype.kind == 'f' and a.size <= FULL:
        out['hex'] = [float(v).hex() for v in a.ravel()]       # (float32 -> float is exact)
    else:
        out['sha256'] = hashlib.sha256(a.tobytes()).hexdigest()
    return out


def differences(got, want, path=''):
    """The paths at which two records differ, with both sides"""
    if isinstance(want, dict) and isinstance(got, dict) and 'dtype' not in want:
        for k in sorted(set(want) | set(got)):
            yield from differences(got.get(k, '<missing>'), want.get(k, '<missing>'), f'{path}/{k}')
    elif isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        for i, (g, w) in enumerate(zip(got, want)):
            yield from differences(g, w, f'{path}[{i}]')
    elif got != want:
        yield f'{path}: {got} != recorded {want}'


def compute():
    """situation -> record, on the library and under the launch setting of this process"""
    import _reweight_scene as RS
    engine = importlib.import_module(RS.PKG + '.engine')
    synth = importlib.import_module(RS.PKG + '.synth')
    c = RS.batch(synth)
    out = {}
    for name, w, keep, then in (('plain', None, False, None), ('weighted', c['w1'], False, None), ('keep_order', c['w1'], True, None),
                                ('keep_order_reweighted', c['w1'], True, c['w2'])):
        with engine.Engine((RS.H, RS.W), sum(RS.N), max_refs=RS.R, max_windows=RS.B) as eng:
            eng.set_windows(RS.staged(c, w), keep_order=keep)
            if then is not None:
                eng.set_weights(then)
            rec = {'answers': RS.answers(eng, c, encode)}
            if keep:
                rec['staged_order'] = encode(eng.staged_order())
                rec['staged_weights'] = encode(eng.staged_weights())
        out[name] = rec
    return out


def run_setting(env_extra, out_path):
    """compute() in a fresh child process whose environment carries env_extra and no other launch switch; the parsed result"""
    env = {k: v for k, v in os.environ.items() if not k.startswith('EINCM_') or k == 'EINCM_LIB'}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (env_extra, r.stdout[-2000:], r.stderr[-2000:])
    with open(out_path) as f:
        got = json.load(f)
    assert got['env'] == env_extra                  # the child saw this switch and no other
    return got['cases']


if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    import __graft_entry__ as ge
    ge.build()
    env = {k: v for k, v in sorted(os.environ.items()) if k.startswith('EINCM_') and k != 'EINCM_LIB'}
    with open(sys.argv[1], 'w') as f:
        json.dump({'env': env, 'cases': compute()}, f)
