#!/usr/bin/env python3
"""Developer tool: record tests/golden/loss_assembly/parent.npz - the bits a build computes on the cases of
tests/test_gpu_loss_assembly.py (tests/_loss_assembly_cases.py).  Run it on the build whose bits are the yardstick (EINCM_LIB selects
a variant library):

    python tools/record_loss_assembly.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    path = sys.argv[1]
    import _loss_assembly_cases as A      # (imports torch before build() loads the engine's library)
    import __graft_entry__ as ge
    ge.build()
    rec = A.record()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **rec)
    print(f'recorded {len(rec)} arrays, {os.path.getsize(path)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
