#!/usr/bin/env python3
"""Developer tool: record tests/golden/staging_payload/parent.json - what a build answers on the batch of tests/_reweight_scene.py in
the four payload situations of staging (plain, weighted, keep-order, keep-order then set_weights) under the four launch settings
(default, EINCM_HOST_BINNING, EINCM_NO_SEGSORT, EINCM_NO_SPREAD); tests/_staging_payload.py says what a record holds and how it is
stored.  tests/test_gpu_staging_payload.py recomputes the same records with the tree's build and compares them for equality.

Run it on a GPU with a build of the commit whose bytes are the yardstick - the parent of a change to staging (EINCM_LIB selects a
library built elsewhere, tools/build_variant.sh) - and name that commit when the tree is no git checkout:

    python tools/record_staging_payload.py [--commit HASH] [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'staging_payload', 'parent.json')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', help='the commit whose build records (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=GOLDEN)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], check=True, capture_output=True, text=True).stdout.strip()
    import _staging_payload as SP
    rec = {'recorded_by': commit, 'scene': 'tests/_reweight_scene.py batch()', 'settings': dict(SP.SETTINGS), 'cases': {}}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env_extra in SP.SETTINGS:
            rec['cases'][tag] = SP.run_setting(env_extra, os.path.join(tmp, tag + '.json'))
            assert sorted(rec['cases'][tag]) == sorted(SP.SITUATIONS)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'recorded {sum(len(v) for v in rec["cases"].values())} cases at {commit}, {os.path.getsize(a.out)} bytes -> {a.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
