"""The HIP-free rules of a weighted staging (csrc/eincm_plan.h) on the CPU: which batches count as weighted
(batch_weighted, StagePlan.weighted from plan_staging), the first weight check_weights refuses, and the weights' way through the host
counting sort (bin_events: the order of sxy, ones for a window without weights, weight-0 events left out of cntmax).

tests/host/weights_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as tests/test_host_plan.py
builds plan_check, and run once, as a child process, over every case of this module; nothing is preloaded.  Its lines equal numpy."""
import numpy as np
import pytest

import _host_check as HC

TS = 32


@pytest.fixture(scope='session')
def weights_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'weights_check')


CASES, EXPECT = {}, {}


def _window(rng, n, H, W, weights):
    """(x, y, t, w | None): weights 'none' | 'ones' | 'mixed' (a third zero) | an array."""
    x, y, t = rng.integers(0, W, n), rng.integers(0, H, n), np.sort(rng.uniform(0.0, 1.0, n))
    if isinstance(weights, str):
        w = {'none': None, 'ones': np.ones(n, np.float32),
             'mixed': np.where(rng.random(n) < 0.33, 0.0, rng.uniform(0.125, 1.0, n)).astype(np.float32)}[weights]
    else:
        w = np.asarray(weights, dtype=np.float32)
    return x, y, t, w


def _case(name, H, W, wins, null_array=False, refused=(-1, 0)):
    B = len(wins)
    tokens = ['stage', H, W, B, int(null_array)] + [len(w[0]) for w in wins] + [int(w[3] is not None) for w in wins]
    for x, y, t, w in wins:
        tokens += list(x) + list(y) + list(t) + ([float(v) for v in w] if w is not None else [])
    HC.add_case(CASES, name, *tokens)
    weighted = (not null_array) and any(w[3] is not None and len(w[0]) for w in wins)
    sxy, sw, cntmax = [], [], []
    tilesX = (W + TS - 1) // TS
    for x, y, t, w in wins:
        order = np.argsort((y // TS) * tilesX + (x // TS), kind='stable')
        sxy += list((x[order].astype(np.uint32) | (y[order].astype(np.uint32) << 16)))
        wb = None if (null_array or w is None) else w
        sw += list((np.ones(len(x), np.float32) if wb is None else wb[order]).view(np.uint32))
        keep = np.ones(len(x), bool) if wb is None or not weighted else wb > 0
        cnt = np.bincount(y[keep] * W + x[keep], minlength=1)
        cntmax.append(int(cnt.max()) if keep.any() else 0)
    EXPECT[name] = (int(weighted), refused, sxy, sw if weighted else [], cntmax)
    return name


_rng = np.random.default_rng(5)
H0, W0 = 70, 100
_case('null-array', H0, W0, [_window(_rng, 40, H0, W0, 'mixed')], null_array=True)
_case('every-window-null', H0, W0, [_window(_rng, 40, H0, W0, 'none'), _window(_rng, 7, H0, W0, 'none')])
_case('weights-of-an-empty-window-only', H0, W0, [_window(_rng, 0, H0, W0, 'ones'), _window(_rng, 30, H0, W0, 'none')])
_case('one-weighted-window-of-three', H0, W0, [_window(_rng, 300, H0, W0, 'none'), _window(_rng, 500, H0, W0, 'mixed'),
                                                _window(_rng, 1, H0, W0, 'none')])
_case('all-ones', H0, W0, [_window(_rng, 200, H0, W0, 'ones')])
_case('crowded-pixels', 33, 40, [_window(_rng, 2000, 3, 4, 'mixed'), _window(_rng, 2000, 3, 4, 'none')])      # cntmax counts w > 0 only
_case('all-zero-weights', H0, W0, [_window(_rng, 50, H0, W0, np.zeros(50))])


def _bad(value, at=17, n=40):
    w = np.full(n, 0.5, np.float32)
    w[at] = value
    return w


for _name, _v in (('nan', np.nan), ('inf', np.inf), ('minus-inf', -np.inf), ('just-below-zero', -1e-9), ('just-above-one', 1.0 + 1e-6),
                  ('two', 2.0)):
    _case('refuses-' + _name, H0, W0, [_window(_rng, 10, H0, W0, 'none'), _window(_rng, 40, H0, W0, _bad(_v))], refused=(1, 17))
_case('first-refusal-wins', H0, W0, [_window(_rng, 40, H0, W0, _bad(np.nan, 30)), _window(_rng, 40, H0, W0, _bad(-1.0, 2))], refused=(0, 30))
_case('bounds-are-allowed', H0, W0, [_window(_rng, 40, H0, W0, _bad(0.0)), _window(_rng, 40, H0, W0, _bad(1.0))])
_case('smallest-positive', H0, W0, [_window(_rng, 40, H0, W0, _bad(np.float32(1e-45)))])


@pytest.fixture(scope='module')
def out(weights_check, tmp_path_factory):
    return HC.run(weights_check, CASES, tmp_path_factory, 'weights_cases')


@pytest.mark.parametrize('name', sorted(CASES))
def test_weighted_staging_rules(out, name):
    weighted, refused, sxy, sw, cntmax = EXPECT[name]
    head, got_xy, got_w, got_c = out[name]
    assert [int(v) for v in head] == [weighted, weighted, refused[0], refused[1] if refused[0] >= 0 else 0]
    if refused[0] >= 0:
        assert got_xy == [] and got_w == [] and got_c == []
        return
    assert np.array_equal(HC.i(got_xy), np.array(sxy, dtype=np.int64))
    assert np.array_equal(HC.i(got_w), np.array(sw, dtype=np.int64))
    assert np.array_equal(HC.i(got_c), np.array(cntmax, dtype=np.int64))
