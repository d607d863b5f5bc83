"""Randomised parity sweeps of the HIP loss/grad path (tests/dev/fuzz_gpu.py) as regression tests.

test_fuzz_against_oracle: 60 drawn configurations (sensor 6..260 px, 0..40000 events, 1..6 reference times, 2-DoF / coarse / dense
theta, four resampling kernels, every loss term on and off, flows up to 200 px, 1..3 windows per context).  Value and gradient within
1e-5 of the fp64 oracle, count images bit-exact.  Windows with only a handful of events have gradients that nearly cancel by symmetry;
with fp32 images their max-norm relative error is conditioned 10x worse, so those cases use 1e-4 (observed worst: 1.2e-5 for a single
event).

test_fuzz_fp64_against_oracle: the float64 mode (sensors 3..200 px, 1..16 reference times, 1..5 windows, finer-than-sensor theta
grids too) against the oracle at its own tolerances: value 1e-10, gradient 1e-9, IWE 1e-11, dL/dIWE 1e-10, count images bit-exact.

test_fuzz_objective_kinds_against_witness: every contrast x correlation kind with drawn tile sizes (ragged, a side of 1 or 2,
tile = sensor, more than 64 cells) against the fp64 autograd witness: value, gradient, dL/dIWE and the mean relative terms at 1e-5.

Each new sweep asserts that its drawn cases cover every category of its draw."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dev'))
import fuzz_gpu  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fuzz_against_oracle(built_lib):
    rng = np.random.default_rng(2)
    for i in range(60):
        c = fuzz_gpu.draw_case(rng)
        ev, eg, counts_ok = fuzz_gpu.run_case(c, 2000 + i)
        tol_g = 1e-5 if min(c['N']) >= 300 else 1e-4
        assert ev <= 1e-5 and eg <= tol_g and counts_ok, (i, ev, eg, counts_ok, c)


def _common_coverage(cases):
    """the categories both new draws share: (name, covered)"""
    nonzero = lambda k: any(c[k] != 0.0 for c in cases)      # noqa: E731
    return ([(f'N={n}', any(n in c['N'] for c in cases)) for n in fuzz_gpu.N_CHOICES]
            + [(f'theta {k}', any(c['theta'] == k for c in cases)) for k in ('2dof', 'coarse', 'dense')]
            + [(f'method {m}', any(c['method'] == m for c in cases)) for m in fuzz_gpu.METHODS]
            + [(f'{k} on', nonzero(k)) for k in ('alpha', 'beta', 'delta')]
            + [('gamma at level 0', any(c['gamma'] != 0.0 and c['lvl'] == 0 for c in cases)),
               ('R > 5', any(c['R'] > 5 for c in cases)), ('R = 16', any(c['R'] == 16 for c in cases)),
               ('B = 5', any(c['B'] == 5 for c in cases)),
               ('batch of windows of different sizes', any(len(set(c['N'])) > 1 for c in cases)),
               ('flow of 200 px', any(c['mag'] == 200.0 for c in cases))])


def fp64_coverage(cases):
    """the categories of draw_case_fp64 that no case of `cases` reaches"""
    cov = _common_coverage(cases) + [
        ('sensor of 3..8 px', any(max(c['H'], c['W']) <= 8 for c in cases)),
        ('sensor of 3 px', any(min(c['H'], c['W']) == 3 for c in cases)),
        ('theta finer than the sensor', any(c['theta'] == 'finer' for c in cases)),
        ('ck 0', any(c['ck'] == 0 for c in cases)), ('ck 1', any(c['ck'] == 1 for c in cases))]
    return [name for name, ok in cov if not ok]


def kinds_coverage(cases):
    """the categories of draw_case_kinds that no case of `cases` reaches"""
    cov = _common_coverage(cases) + [
        (f'ck {k}', any(c['ck'] == k for c in cases)) for k in range(4)] + [
        (f'rk {k}', any(c['rk'] == k for c in cases)) for k in range(4)] + [
        ('a default ck with a new rk', any(c['ck'] < 2 and c['rk'] > 0 for c in cases)),
        ('a new ck with rk 0', any(c['ck'] >= 2 and c['rk'] == 0 for c in cases))] + [
        (f'tile {k}', any(c['tile_kind'] == k for c in cases)) for k in fuzz_gpu.TILE_KINDS] + [
        ('ragged tile', any(c['H'] % c['tile'][0] and c['W'] % c['tile'][1] for c in cases)),
        ('tile side 1', any(1 in c['tile'] for c in cases)), ('tile side 2', any(2 in c['tile'] for c in cases)),
        ('tile = sensor', any(c['tile'] == (c['H'], c['W']) for c in cases)),
        ('more than 64 cells', any(fuzz_gpu.n_cells(c) > 64 for c in cases)),
        ('more than 128 cells', any(fuzz_gpu.n_cells(c) > 128 for c in cases))]
    return [name for name, ok in cov if not ok]


def _sweep(draw, n, seed, coverage, run):
    rng = np.random.default_rng(seed)
    cases = [draw(rng) for _ in range(n)]
    assert not coverage(cases), coverage(cases)
    worst = {}
    for i, c in enumerate(cases):
        res = run(c, 1000 * seed + i)
        for k, e in res.items():
            if k != 'counts':
                worst[k] = max(worst.get(k, 0.0), e)
        yield i, c, res
    print(f'worst over {n} cases: ' + ', '.join(f'{k} {e:.2e}' for k, e in worst.items()))


def test_fuzz_fp64_against_oracle(built_lib):
    for i, c, res in _sweep(fuzz_gpu.draw_case_fp64, 100, 5, fp64_coverage, lambda c, s: fuzz_gpu.run_case(c, s, precision='fp64')):
        assert not fuzz_gpu.failures(res, 'fp64'), (i, res, c)


def test_fuzz_objective_kinds_against_witness(built_lib):
    run = lambda c, s: fuzz_gpu.run_case(c, s, kinds=(c['ck'], c['rk'], c['tile']))      # noqa: E731
    for i, c, res in _sweep(fuzz_gpu.draw_case_kinds, 80, 6, kinds_coverage, run):
        assert not fuzz_gpu.failures(res, 'kinds'), (i, res, c)
