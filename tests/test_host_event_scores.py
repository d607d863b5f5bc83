"""The HIP-free rules of the per-event scores (csrc/eincm_event_scores.h) on the CPU: the argument check in its
stated order, one refusal at a time and several at once, and the layout of the output blocks for empty windows, one window and many
windows in both forms.

tests/host/event_scores_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_event_filter.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import numpy as np
import pytest

import _host_check as HC

OK, IN_FLIGHT, NULL_SCORES, NO_EVAL, FP64, SPLAT, SHARDED, REF_WEIGHT, MASKED = range(9)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NULL_SCORES: ERR_ARG, NO_EVAL: ERR_STATE, FP64: ERR_UNSUPPORTED, SPLAT: ERR_UNSUPPORTED,
        SHARDED: ERR_UNSUPPORTED, REF_WEIGHT: ERR_ARG, MASKED: ERR_STATE}


@pytest.fixture(scope='session')
def event_scores_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'event_scores_check')


CASES, EXPECT = {}, {}


def _check(name, fault, in_flight=0, has_scores=1, staged=1, have_eval=1, fp64=0, splat=3, sharded=0, has_images=0, masked=0, rw=None,
           n_refs=3):
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, has_scores, staged, have_eval, fp64, splat, sharded, has_images, masked, n_refs,
                int(rw is not None), *([] if rw is None else [float(v) for v in rw]))
    EXPECT['check-' + name] = fault
    return 'check-' + name


ALL_BAD = dict(in_flight=1, has_scores=0, staged=0, have_eval=0, fp64=1, splat=5, sharded=1, masked=1, rw=[1.0, np.nan, 1.0])
_order = ['in_flight', 'has_scores', 'staged', 'fp64', 'splat', 'sharded', 'rw', 'masked']
_good = dict(in_flight=0, has_scores=1, staged=1, fp64=0, splat=3, sharded=0, rw=None, masked=0)


def _from(i):
    """every fault from the i-th of the order on, the earlier ones mended"""
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw[k] = _good[k]
        if k == 'staged':
            kw['have_eval'] = 1
    return kw


CHECKS = [_check('ok', OK), _check('ok-images', OK, has_images=1), _check('ok-combined', OK, rw=[0.25, 0.5, 0.25]),
          _check('ok-negative-and-zero-weights', OK, rw=[-1.0, 0.0, 1e300]), _check('in-flight', IN_FLIGHT, in_flight=1),
          _check('null-scores', NULL_SCORES, has_scores=0), _check('not-staged', NO_EVAL, staged=0, have_eval=0),
          _check('no-eval', NO_EVAL, have_eval=0), _check('fp64', FP64, fp64=1), _check('splat1', SPLAT, splat=1),
          _check('splat5', SPLAT, splat=5), _check('sharded', SHARDED, sharded=1), _check('rw-nan', REF_WEIGHT, rw=[1.0, 1.0, np.nan]),
          _check('rw-inf', REF_WEIGHT, rw=[np.inf, 1.0, 1.0]), _check('rw-neg-inf', REF_WEIGHT, rw=[1.0, -np.inf, 1.0]),
          _check('masked-iwe', MASKED, masked=1), _check('masked-with-images', OK, masked=1, has_images=1),
          _check('r1', OK, rw=[2.0], n_refs=1), _check('r1-nan', REF_WEIGHT, rw=[np.nan], n_refs=1),
          # the first of the order in flight, scores, staged / evaluated, fp64, splat window, sharded, ref_weights, masked
          _check('first-of-all', IN_FLIGHT, **_from(0)), _check('second', NULL_SCORES, **_from(1)), _check('third', NO_EVAL, **_from(2)),
          _check('fourth', FP64, **_from(3)), _check('fifth', SPLAT, **_from(4)), _check('sixth', SHARDED, **_from(5)),
          _check('seventh', REF_WEIGHT, **_from(6)), _check('eighth', MASKED, **_from(7))]


def _layout(name, n_refs, n_events):
    for combined in (0, 1):
        HC.add_case(CASES, f'layout-{name}-{combined}', 'layout', n_refs, combined, len(n_events), *n_events)
        EXPECT[f'layout-{name}-{combined}'] = (n_refs, combined, list(n_events))
    return name


LAYOUTS = [_layout('no-windows', 3, []), _layout('one-empty-window', 3, [0]), _layout('one-window', 3, [7]), _layout('one-window-r1', 1, [7]),
           _layout('three-middle-empty', 3, [5, 0, 9]), _layout('all-empty', 2, [0, 0, 0]), _layout('first-and-last-empty', 4, [0, 3, 0]),
           _layout('many', 5, list(range(1, 40, 3)) + [0, 1000000, 1]), _layout('beyond-2^31', 8, [400000000, 1, 400000000])]


@pytest.fixture(scope='module')
def out(event_scores_check, tmp_path_factory):
    return HC.run(event_scores_check, CASES, tmp_path_factory, 'event_scores_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code = (int(v) for v in out[name][0])
    assert fault == EXPECT[name] and code == CODE[fault]


@pytest.mark.parametrize('combined', [0, 1], ids=['per-reference', 'combined'])
@pytest.mark.parametrize('name', LAYOUTS)
def test_layout_of_the_blocks(out, name, combined):
    n_refs, _, ne = EXPECT[f'layout-{name}-{combined}']
    total, off, length = out[f'layout-{name}-{combined}']
    want_len = [n * (1 if combined else n_refs) for n in ne]              # (Python integers: no overflow)
    want_off = [sum(want_len[:b]) for b in range(len(ne))]
    assert int(total[0]) == sum(want_len)
    assert [int(v) for v in off] == want_off and [int(v) for v in length] == want_len
