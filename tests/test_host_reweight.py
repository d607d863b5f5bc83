"""The HIP-free side of a keep-order staging (csrc/eincm_plan.h) on the CPU: EINCM_SW_KEEP_ORDER makes a weighted
batch of any batch (plan_staging), and the host counting sort (bin_events) carries, beside the weights, the index of every sorted slot
back into the batch as it was handed over:

  * the index is a permutation of range(N) that maps every window's range into itself;
  * packed(xs[idx[i]], ys[idx[i]]) == sxy[i], ts[idx[i]] == st[i], weights[idx[i]] == sw[i] (ones for a window without weights);
  * inside a tile the indices ascend: the sort is stable;
  * most_on_one_pixel, with which a re-weighting of a host-binned batch counts, gives bin_events' cntmax.

tests/host/reweight.cpp is built once per session with the address and undefined-behaviour sanitizers through tests/_host_check.build,
as tests/test_host_plan.py builds plan_check, and run once, as a child process, over every case of this module; nothing is preloaded.
The program counts the violations of the rules above itself, and its index is compared with numpy's stable sort here."""
import numpy as np
import pytest

import _host_check as HC

TS = 32


@pytest.fixture(scope='session')
def reweight_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'reweight')


CASES, EXPECT = {}, {}


def _window(rng, n, H, W, weights, crowd=None):
    """(x, y, t, w | None).  crowd: (h, w), the corner that holds the events - repeated pixels."""
    h, w = crowd or (H, W)
    x, y, t = rng.integers(0, w, n), rng.integers(0, h, n), np.sort(rng.uniform(0.0, 1.0, n))
    wt = None
    if weights == 'mixed':          # exact zeros, exact ones and values between
        wt = np.where(rng.random(n) < 0.3, 0.0, np.where(rng.random(n) < 0.3, 1.0, rng.uniform(0.05, 0.95, n))).astype(np.float32)
    return x, y, t, wt


def _case(name, H, W, wins):
    tokens = ['order', H, W, len(wins)] + [len(w[0]) for w in wins] + [int(w[3] is not None) for w in wins]
    for x, y, t, w in wins:
        tokens += list(x) + list(y) + list(t) + ([float(v) for v in w] if w is not None else [])
    HC.add_case(CASES, name, *tokens)
    tilesX, idx, base = (W + TS - 1) // TS, [], 0
    for x, y, t, w in wins:
        idx += list(base + np.argsort((y // TS) * tilesX + (x // TS), kind='stable'))
        base += len(x)
    EXPECT[name] = idx


_rng = np.random.default_rng(29)
H0, W0 = 70, 100                    # 3 x 4 tiles, the last row and column partial
_case('mixed-batch-with-an-empty-window', H0, W0, [_window(_rng, 700, H0, W0, 'mixed'), _window(_rng, 0, H0, W0, None),
                                                    _window(_rng, 300, H0, W0, None), _window(_rng, 900, H0, W0, 'mixed', crowd=(5, 6))])
_case('empty-window-first-and-last', H0, W0, [_window(_rng, 0, H0, W0, 'mixed'), _window(_rng, 257, H0, W0, 'mixed'), _window(_rng, 0, H0, W0, None)])
_case('no-events-at-all', H0, W0, [_window(_rng, 0, H0, W0, None), _window(_rng, 0, H0, W0, None)])
_case('one-pixel', 33, 40, [_window(_rng, 400, 33, 40, 'mixed', crowd=(1, 1)), _window(_rng, 3, 33, 40, None)])
_case('one-event', H0, W0, [_window(_rng, 1, H0, W0, 'mixed')])


@pytest.fixture(scope='module')
def out(reweight_check, tmp_path_factory):
    return HC.run(reweight_check, CASES, tmp_path_factory, 'reweight_cases')


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_host_sort_keeps_the_index_of_every_slot(out, name):
    plan, faults, idx = out[name]
    # the flag alone makes the batch a keep-order one and a weighted one; without it (and without weights) it is neither
    assert [int(v) for v in plan] == [1, 1, 0]
    names = ('not a permutation', 'leaves its window', 'xy differs', 't differs', 'w differs', 'descends inside a tile', 'cntmax differs')
    assert dict(zip(names, (int(v) for v in faults))) == dict.fromkeys(names, 0)
    assert np.array_equal(HC.i(idx), np.array(EXPECT[name], dtype=np.int64))


# ---- the payload state of a staging (StagePlan.payload): what (weights, EINCM_SW_KEEP_ORDER) make of a batch ---------------------------
NONE, WEIGHTS, WEIGHTS_ORDER = 0, 1, 2
PAYLOADS = {    # name: (events per window, which windows were handed weights, the flag) -> the state
    'no-weights-no-flag': ((700, 0, 300), (0, 0, 0), 0, NONE),
    'weights-on-one-window': ((700, 0, 300), (0, 0, 1), 0, WEIGHTS),
    'weights-on-every-window': ((700, 5, 300), (1, 1, 1), 0, WEIGHTS),
    'weights-only-on-an-empty-window': ((700, 0, 300), (0, 1, 0), 0, NONE),
    'no-events-at-all-with-weights': ((0, 0), (1, 1), 0, NONE),
    'the-flag-alone': ((700, 0, 300), (0, 0, 0), 1, WEIGHTS_ORDER),
    'the-flag-and-weights': ((700, 0, 300), (1, 0, 1), 1, WEIGHTS_ORDER),
    'the-flag-and-weights-only-on-an-empty-window': ((700, 0, 300), (0, 1, 0), 1, WEIGHTS_ORDER),
    'the-flag-without-events': ((0,), (0,), 1, WEIGHTS_ORDER),
}
PAYLOAD_CASES = {}
for _name, (_n, _has, _keep, _) in PAYLOADS.items():
    HC.add_case(PAYLOAD_CASES, _name, 'payload', len(_n), *_n, *_has, _keep)


def test_the_plan_names_one_payload_state_and_sets_both_flags_from_it(reweight_check, tmp_path_factory):
    out = HC.run(reweight_check, PAYLOAD_CASES, tmp_path_factory, 'payload_cases')
    for name, (_n, _has, _keep, want) in PAYLOADS.items():
        state, weighted, keep_order = (int(v) for v in out[name][0])
        assert state == want, name
        assert (weighted, keep_order) == (int(want != NONE), int(want == WEIGHTS_ORDER)), name
