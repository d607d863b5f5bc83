"""Drawn configurations of the per-event and segmentation operators against their witnesses (tests/dev/fuzz_gpu.py:
draw_case_segmentation / run_case_segmentation; DESIGN.md sections 25, 27, 28, 29 and 30), one test per case.

24 cases: one fp32 engine with a motion model (every kind, custom matrices of 1 and 12 columns, drawn centres and scales) and a
batch of 1..3 unequal groups of 1..8 consecutive windows (an empty group in the middle, one 40000-event group on a sensor of at most
32 x 40), sensors of 3..200 px (a third of them 3..8 px, ragged 4 x 4 source tiles, H < 32 <= W, multiples of 32), 1..16 reference
times, weights None / ones / {0} u [1/8, 1] / k/4 / all zero mixed in a batch, fields of 0..200 px with one window sometimes at 1e5 px,
the last evaluation 2-DoF, coarse (every resampling method), dense, motion-expanded or motion-fused, the batch staged by set_windows
or with keep_order and then re-weighted by set_weights or apply_responsibilities, host binning on or off.  The chain and its bars, each
the operator's own module's:
  event_scores            both sources, both forms, with and without selfs: |gpu - witness| <= 1e-5 M per cell, 0 where M == 0, the
                          cell past every block untouched; the GPU IWE against the weighted fp64 splat at 1e-5 of its maximum
  event_responsibilities  weights and labels = the float32 restatement on the GPU's own scores bit for bit, n_unsupported exact,
                          sums within K 2^-23, the prior's shares, mass within 1e-12, 1e-4 of the fp64 form on the clear events, a
                          second call's bytes
  the keep-order ways     staged_order a permutation inside every window, staged_weights the bytes handed over, every answer the
                          bytes of a fresh keep-order engine, an all-None keep-order batch the unweighted batch's bytes
  compose_motions         all four outputs byte for byte in the drawn mode / fill and the opposite one
  contrast_landscape      sumsq and n_in integer for integer, the zero and the FAR candidate, a second call, no dependence on weights

What the draws cover and that the checks are not vacuous: tests/test_fuzz_segmentation_interface.py (no GPU)."""
import os
import signal
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dev'))
import fuzz_gpu  # noqa: E402

pytestmark = pytest.mark.gpu

N_CASES = 24
SEED = 245
TIME_LIMIT_S = 30


def case_seed(seed, k):
    return 1000 * seed + k


def sweep_cases(seed=None):
    rng = np.random.default_rng(SEED if seed is None else seed)
    return [fuzz_gpu.draw_case_segmentation(rng, k) for k in range(N_CASES)]


CASES = sweep_cases()

_WORST = {}
_SLOWEST = [0.0, None]


@pytest.fixture(scope='module', autouse=True)
def _worst_at_the_end(built_lib):
    yield
    if _WORST:
        print('\nsegmentation sweep, worst over its cases: ' + ', '.join(f'{m} {e:.2e}' for m, e in _WORST.items())
              + f'; slowest case {_SLOWEST[1]}: {_SLOWEST[0]:.1f} s')


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f'test exceeded {TIME_LIMIT_S} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TIME_LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.mark.parametrize('k', range(N_CASES))
def test_segmentation_case(k, monkeypatch):
    c = CASES[k]
    t0 = time.perf_counter()
    res = fuzz_gpu.run_case_segmentation(c, case_seed(SEED, k), monkeypatch=monkeypatch)
    dt = time.perf_counter() - t0
    measures = {m: e for m, e in res.items() if not isinstance(e, bool)}
    print(f'segmentation {k}: ' + ' '.join(f'{m} {e:.2e}' for m, e in measures.items())
          + ' ' + ' '.join(f'{m} {"ok" if e else "DIFF"}' for m, e in res.items() if isinstance(e, bool)) + f' ({dt:.1f} s)')
    for m, e in measures.items():
        _WORST[m] = max(_WORST.get(m, 0.0), e)
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, k]
    assert not fuzz_gpu.failures(res, 'segmentation'), (k, fuzz_gpu.failures(res, 'segmentation'), res, c)
