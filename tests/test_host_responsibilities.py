"""The HIP-free rules of the E-step operator (csrc/eincm_responsibilities.h) on the CPU: the argument check in its
stated order, one refusal at a time and with every later fault present, and the layout of the weights' and the labels' blocks for no
window, empty groups, many groups and a total beyond 2^31.

tests/host/responsibilities_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_event_scores.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import numpy as np
import pytest

import _host_check as HC

(OK, IN_FLIGHT, NULL_OUTPUTS, NO_EVAL, FP64, SPLAT, SHARDED, MODELS, GROUPS, UNEQUAL, REF_WEIGHT, PRIOR, MASKED) = range(13)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NULL_OUTPUTS: ERR_ARG, NO_EVAL: ERR_STATE, FP64: ERR_UNSUPPORTED, SPLAT: ERR_UNSUPPORTED,
        SHARDED: ERR_UNSUPPORTED, MODELS: ERR_ARG, GROUPS: ERR_ARG, UNEQUAL: ERR_ARG, REF_WEIGHT: ERR_ARG, PRIOR: ERR_ARG, MASKED: ERR_STATE}


@pytest.fixture(scope='session')
def responsibilities_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'responsibilities_check')


CASES, EXPECT = {}, {}
RW3 = (0.25, 0.5, 0.25)


def _check(name, fault, in_flight=0, has_outputs=1, staged=1, have_eval=1, fp64=0, splat=3, sharded=0, has_images=0, masked=0, n_models=2,
           rw=RW3, n_refs=3, ne=(5, 5, 0, 0), prior=None):
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, has_outputs, staged, have_eval, fp64, splat, sharded, has_images, masked, n_models,
                n_refs, int(rw is not None), *([] if rw is None else [float(v) for v in rw]), int(prior is not None), len(ne), *ne,
                *([] if prior is None else [float(v) for v in prior]))
    EXPECT['check-' + name] = fault
    return 'check-' + name


# every fault at once: each of the order's twelve, the later ones still present when the earlier ones are mended
ALL_BAD = dict(in_flight=1, has_outputs=0, staged=0, have_eval=0, fp64=1, splat=5, sharded=1, n_models=9, ne=(5, 4, 3), rw=(1.0, np.nan, 1.0),
               prior=(1.0, -1.0, 1.0), masked=1)
_order = ['in_flight', 'has_outputs', 'staged', 'fp64', 'splat', 'sharded', 'n_models', 'groups', 'unequal', 'rw', 'prior', 'masked']
_mend = {'in_flight': dict(in_flight=0), 'has_outputs': dict(has_outputs=1), 'staged': dict(staged=1, have_eval=1), 'fp64': dict(fp64=0),
         'splat': dict(splat=3), 'sharded': dict(sharded=0), 'n_models': dict(n_models=2), 'groups': dict(ne=(5, 4, 3, 3), prior=(1.0, -1.0, 1.0, 1.0)),
         'unequal': dict(ne=(5, 5, 3, 3)), 'rw': dict(rw=RW3), 'prior': dict(prior=(1.0, 0.0, 0.5, 0.5)), 'masked': dict(masked=0)}


def _from(i):
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw.update(_mend[k])
    return kw


CHECKS = [_check('ok', OK), _check('ok-images', OK, has_images=1), _check('ok-k1', OK, n_models=1, ne=(3, 0, 7)),
          _check('ok-k8', OK, n_models=8, ne=(2,) * 16), _check('ok-no-windows-of-events', OK, ne=(0, 0)),
          _check('ok-prior', OK, prior=(1.0, 0.0, 0.0, 2.5)), _check('ok-signed-ref-weights', OK, rw=(-1.0, 0.0, 1e300)),
          _check('in-flight', IN_FLIGHT, in_flight=1), _check('null-outputs', NULL_OUTPUTS, has_outputs=0),
          _check('not-staged', NO_EVAL, staged=0, have_eval=0), _check('no-eval', NO_EVAL, have_eval=0), _check('fp64', FP64, fp64=1),
          _check('splat1', SPLAT, splat=1), _check('splat5', SPLAT, splat=5), _check('sharded', SHARDED, sharded=1),
          _check('k0', MODELS, n_models=0), _check('k-negative', MODELS, n_models=-2), _check('k9', MODELS, n_models=9),
          _check('k-does-not-divide', GROUPS, n_models=3), _check('k-more-than-windows', GROUPS, n_models=8),
          _check('unequal', UNEQUAL, ne=(5, 4, 0, 0)), _check('unequal-last-group', UNEQUAL, ne=(5, 5, 0, 1)),
          _check('unequal-k3', UNEQUAL, n_models=3, ne=(2, 2, 2, 4, 4, 3)), _check('equal-across-groups-only', UNEQUAL, ne=(5, 4, 5, 4)),
          _check('rw-null', REF_WEIGHT, rw=None), _check('rw-nan', REF_WEIGHT, rw=(1.0, 1.0, np.nan)), _check('rw-inf', REF_WEIGHT, rw=(np.inf, 1.0, 1.0)),
          _check('prior-negative', PRIOR, prior=(1.0, -1e-9, 1.0, 1.0)), _check('prior-nan', PRIOR, prior=(1.0, 1.0, np.nan, 1.0)),
          _check('prior-inf', PRIOR, prior=(1.0, 1.0, 1.0, np.inf)), _check('prior-too-large-for-a-float', PRIOR, prior=(1.0, 1e39, 1.0, 1.0)),
          _check('prior-group-of-zeros', PRIOR, prior=(1.0, 1.0, 0.0, 0.0)), _check('prior-sum-underflows', PRIOR, prior=(1e-300, 1e-300, 1.0, 1.0)),
          _check('prior-sum-overflows', PRIOR, prior=(3e38, 3e38, 1.0, 1.0)),
          _check('masked-iwe', MASKED, masked=1), _check('masked-with-images', OK, masked=1, has_images=1)]
CHECKS += [_check(f'from-{i + 1:02d}-{k}', i + 1, **_from(i)) for i, k in enumerate(_order)]


def _layout(name, n_models, n_events):
    HC.add_case(CASES, 'layout-' + name, 'layout', n_models, len(n_events), *n_events)
    EXPECT['layout-' + name] = (n_models, list(n_events))
    return name


LAYOUTS = [_layout('no-windows', 2, []), _layout('one-empty-group', 3, [0, 0, 0]), _layout('one-window-k1', 1, [7]), _layout('one-group-k2', 2, [7, 7]),
           _layout('three-groups-middle-empty', 3, [5, 5, 5, 0, 0, 0, 9, 9, 9]), _layout('all-empty', 2, [0, 0, 0, 0]),
           _layout('first-and-last-empty', 1, [0, 3, 0]), _layout('many', 4, [n for n in list(range(1, 40, 3)) + [0, 100000, 1] for _ in range(4)]),
           _layout('k8', 8, [3] * 8 + [11] * 8), _layout('beyond-2^31', 2, [1500000000, 1500000000, 1, 1, 1500000000, 1500000000])]


@pytest.fixture(scope='module')
def out(responsibilities_check, tmp_path_factory):
    return HC.run(responsibilities_check, CASES, tmp_path_factory, 'responsibilities_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code = (int(v) for v in out[name][0])
    assert fault == EXPECT[name] and code == CODE[fault]


@pytest.mark.parametrize('name', LAYOUTS)
def test_layout_of_the_blocks(out, name):
    K, ne = EXPECT['layout-' + name]
    totals, w_off, lab_off, lab_len = out['layout-' + name]
    groups = [ne[g * K] for g in range(len(ne) // K)]                       # (Python integers: no overflow)
    assert [int(v) for v in totals] == [sum(ne), sum(groups)]
    assert [int(v) for v in w_off] == [sum(ne[:b]) for b in range(len(ne))]
    assert [int(v) for v in lab_off] == [sum(groups[:g]) for g in range(len(groups))] and [int(v) for v in lab_len] == groups
