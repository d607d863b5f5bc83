"""Drawn configurations of the motion-model paths and of the weighted engine against fp64 (tests/dev/fuzz_gpu.py: draw_case_motion /
run_case_motion, draw_case_weights / run_case_weights; DESIGN.md sections 20 - 22), one test per case.

Motion, 24 cases: every model kind (custom matrices of 1..12 columns), drawn centres and scales, sensors of 3..200 px (ragged and
many source tiles, H < 32 <= W, multiples of 32), 1..16 reference times, 1..5 unequal windows with one sometimes masked, fields of
0..200 px, every loss term and objective kind.  The expanded path against the fp64 oracle projected by the model at 1e-5; the fused
path against the expanded one (value and IWE stack bit for bit), against the exact moments of the same build's dense gradient
(tests/_motion_bounds.py) and against fp64; the mask; scaled_theta; the refusal where the fused path does not apply.

Weights, 24 cases: 2-DoF, coarse (every resampling method), dense and motion-expanded theta, sensors down to 3 px, 1..16 reference
times, 1..4 windows whose weights are None, ones, {0} u [1/8, 1], k/4 or all zero, every loss term and objective kind.  Value,
gradient, IWE stack and dL/dIWE against tests/_event_weights_witness.py at 1e-5, count images bit for bit, all-ones = None, all-zero =
the window staged without events.

What the draws cover and how many of their gradient checks say something: tests/test_fuzz_cases_interface.py (no GPU)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dev'))
import fuzz_gpu  # noqa: E402

pytestmark = pytest.mark.gpu

N_CASES = 24
MOTION_SEED, WEIGHT_SEED = 23, 62


def sweep_cases(draw, seed):
    rng = np.random.default_rng(seed)
    return [draw(rng, k) for k in range(N_CASES)]


def case_seed(seed, k):
    return 1000 * seed + k


MOTION_CASES = sweep_cases(fuzz_gpu.draw_case_motion, MOTION_SEED)
WEIGHT_CASES = sweep_cases(fuzz_gpu.draw_case_weights, WEIGHT_SEED)

_WORST = {'motion': {}, 'weights': {}}
_SLOWEST = {'motion': (0.0, None), 'weights': (0.0, None)}


@pytest.fixture(scope='module', autouse=True)
def _worst_at_the_end(built_lib):
    yield
    for mode, worst in _WORST.items():
        if worst:
            t, k = _SLOWEST[mode]
            print(f'\n{mode} sweep, worst over its cases: ' + ', '.join(f'{m} {e:.2e}' for m, e in worst.items())
                  + f'; slowest case {k}: {t:.1f} s')


def _run(mode, run, name, c, seed):
    t0 = time.perf_counter()
    res = run(c, seed)
    dt = time.perf_counter() - t0
    measures = {m: e for m, e in res.items() if not isinstance(e, bool)}
    print(f'{mode} {name}: ' + ' '.join(f'{m} {e:.2e}' for m, e in measures.items())
          + ' ' + ' '.join(f'{m} {"ok" if e else "DIFF"}' for m, e in res.items() if isinstance(e, bool)) + f' ({dt:.1f} s)')
    for m, e in measures.items():
        _WORST[mode][m] = max(_WORST[mode].get(m, 0.0), e)
    if dt > _SLOWEST[mode][0]:
        _SLOWEST[mode] = (dt, name)
    assert not fuzz_gpu.failures(res, mode), (name, fuzz_gpu.failures(res, mode), res, c)


@pytest.mark.parametrize('k', range(N_CASES))
def test_motion_case(k):
    _run('motion', fuzz_gpu.run_case_motion, k, MOTION_CASES[k], case_seed(MOTION_SEED, k))


@pytest.mark.parametrize('k', range(N_CASES))
def test_weights_case(k):
    _run('weights', fuzz_gpu.run_case_weights, k, WEIGHT_CASES[k], case_seed(WEIGHT_SEED, k))

