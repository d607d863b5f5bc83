"""Host time per lockstep tick of the two BFGS drivers, no GPU: B = 8 windows over the Rosenbrock family of tests/_bfgs_cases.py (an
analytic objective that costs a few microseconds per window), maxiter = 30, gtol = 1e-7.

    python3 tools/dev_bfgs_tick.py [--root CHECKOUT] [--runs 5] [--out FILE.json]

* ``LockstepBFGS.run()`` at n = 2, 32 (SciPy's own update expression), 128 and 512 (the rank-two update)
* ``DeviceLockstepBFGS.run()`` on ``NumpyBFGSState`` at n = 128 and 512

Microseconds per tick = run time / n_batch_evals, objective included (it is the same on every side of a comparison).  --root: import
the package from another checkout, e.g. the parent commit; to compare two commits alternate the two invocations (one process each)
and take the median and the range per row over the alternations.  Prints one JSON line: {row: [us per tick of each run]}."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(HERE))
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--out', default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
bs = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
import _bfgs_cases as CASES   # noqa: E402

B, MAXITER, GTOL = 8, 30, 1e-7


def one(n, device):
    fun_batch = CASES.batch_of([CASES.rosen_like(0.5 + 0.25 * b) for b in range(B)])
    x0 = np.random.default_rng(n).uniform(-1.5, 1.5, (B, n))
    if device:
        drv = bs.DeviceLockstepBFGS(bs.NumpyBFGSState(fun_batch), x0, MAXITER, GTOL)
    else:
        drv = bs.LockstepBFGS(fun_batch, x0, MAXITER, GTOL)
    t0 = time.perf_counter()
    res = drv.run()
    t = time.perf_counter() - t0
    assert all(r.nit > 0 for r in res)
    return 1e6 * t / drv.n_batch_evals


rows = [(f'LockstepBFGS n={n}', n, False) for n in (2, 32, 128, 512)] + [(f'DeviceLockstepBFGS/NumpyBFGSState n={n}', n, True) for n in (128, 512)]
out = {}
for name, n, device in rows:
    one(n, device)                                           # warm-up
    out[name] = [round(one(n, device), 2) for _ in range(a.runs)]
line = json.dumps({'root': os.path.abspath(a.root), 'us_per_tick': out})
print(line)
if a.out:
    with open(a.out, 'w') as f:
        f.write(line + '\n')
