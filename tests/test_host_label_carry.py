"""The HIP-free rules of the label prior carried to the next window (csrc/eincm_label_carry.h) on the CPU: the
argument check in its stated order - lp_check's refusals first, then the call's own - one refusal at a time and with every later fault
present; the check of eincm_adopt_carried_prior likewise; the resolve rule lc_resolve against tests/_label_carry_witness.py at the
values where it turns; the layout of the four outputs against engine.label_carry_layout; and the constants of the overflow proof.

tests/host/label_carry_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_label_prior.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import importlib
import os
import re

import numpy as np
import pytest

import _host_check as HC
import _label_carry_witness as WIT

# lp_check's faults keep their numbers (tests/test_host_label_prior.py); the call's own start at 64
(OK, IN_FLIGHT, NOT_STAGED, FP64, SHARDED, MODELS, GROUPS, UNEQUAL, RADIUS, LP_BAD_FLAGS, CROWDED) = range(11)
(NULL, TAU, NO_MODEL, WIDTH, BAD_FLAGS, EVENTS) = range(64, 70)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5             # include/eincm.h
CODE = {OK: 0, IN_FLIGHT: ERR_STATE, NOT_STAGED: ERR_STATE, FP64: ERR_UNSUPPORTED, SHARDED: ERR_UNSUPPORTED, MODELS: ERR_ARG, GROUPS: ERR_ARG,
        UNEQUAL: ERR_ARG, RADIUS: ERR_ARG, CROWDED: ERR_UNSUPPORTED, NULL: ERR_ARG, TAU: ERR_ARG, NO_MODEL: ERR_STATE, WIDTH: ERR_ARG,
        BAD_FLAGS: ERR_ARG, EVENTS: ERR_UNSUPPORTED}
FULL = 1 << 20                                               # the tile population that is refused


@pytest.fixture(scope='session')
def label_carry_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'label_carry_check')


CASES, EXPECT = {}, {}


def _check(name, fault, where=(-1, -1), in_flight=0, staged=1, fp64=0, sharded=0, n_models=2, radius=2, flags=0, has_coeffs=1, has_tau=1,
           model_set=1, n_coeffs=6, model_coeffs=6, ne=(5, 5, 0, 0), ntiles=3, tiles=None, tau=None):
    B = len(ne)
    tc = [0] * (B * ntiles) if tiles is None else list(tiles)
    assert len(tc) == B * ntiles
    if tau is None:                                              # one per group where the check can get as far as reading them
        tau = [1.0] * (B // n_models) if has_tau and 1 <= n_models <= 8 and B % n_models == 0 else []
    HC.add_case(CASES, 'check-' + name, 'check', in_flight, staged, fp64, sharded, n_models, radius, flags, has_coeffs, has_tau, model_set,
                n_coeffs, model_coeffs, B, *ne, ntiles, *tc, *[float(t) for t in tau])
    EXPECT['check-' + name] = (fault, where)
    return 'check-' + name


# every fault at once: lp_check's nine that this call can meet, then the call's own six, the later ones still present when the
# earlier ones are mended
ALL_BAD = dict(in_flight=1, staged=0, fp64=1, sharded=1, n_models=9, ne=(5, 4, 3), radius=9, flags=4, tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0),
               has_coeffs=0, has_tau=0, model_set=0, n_coeffs=5, tau=[])
_order = ['in_flight', 'staged', 'fp64', 'sharded', 'n_models', 'groups', 'unequal', 'radius', 'crowded', 'null-coeffs', 'null-tau', 'tau',
          'model', 'width', 'flags', 'events']
_fault = [IN_FLIGHT, NOT_STAGED, FP64, SHARDED, MODELS, GROUPS, UNEQUAL, RADIUS, CROWDED, NULL, NULL, TAU, NO_MODEL, WIDTH, BAD_FLAGS, EVENTS]
_mend = {'in_flight': dict(in_flight=0), 'staged': dict(staged=1), 'fp64': dict(fp64=0), 'sharded': dict(sharded=0), 'n_models': dict(n_models=2),
         'groups': dict(ne=(5, 4, 2 ** 32, 3), tiles=(0, 0, 0, 0, FULL, 0, 0, 0, 0, 0, 0, 0)), 'unequal': dict(ne=(5, 5, 2 ** 32, 2 ** 32)),
         'radius': dict(radius=8), 'crowded': dict(tiles=None), 'null-coeffs': dict(has_coeffs=1),
         'null-tau': dict(has_tau=1, tau=[0.5, float('nan')]), 'tau': dict(tau=[0.5, -2.0]), 'model': dict(model_set=1),
         'width': dict(n_coeffs=6), 'flags': dict(flags=0), 'events': dict(ne=(5, 5, 2 ** 32 - 1, 2 ** 32 - 1))}
_where = {'crowded': (1, 1), 'tau': (1, -1), 'events': (2, -1)}


def _from(i):
    kw = dict(ALL_BAD)
    for k in _order[:i]:
        kw.update(_mend[k])
    return kw


CHECKS = [_check('ok', OK), _check('ok-k1', OK, n_models=1, ne=(3, 0, 7)), _check('ok-k8', OK, n_models=8, ne=(2,) * 16),
          _check('ok-no-events', OK, ne=(0, 0)), _check('ok-tau-zero-and-negative', OK, tau=[0.0, -1.0e300]),
          _check('ok-most-events', OK, ne=(2 ** 32 - 1,) * 2), _check('in-flight', IN_FLIGHT, in_flight=1),
          _check('not-staged', NOT_STAGED, staged=0), _check('fp64', FP64, fp64=1), _check('sharded', SHARDED, sharded=1),
          _check('k0', MODELS, n_models=0), _check('k9', MODELS, n_models=9), _check('k-does-not-divide', GROUPS, n_models=3),
          _check('unequal', UNEQUAL, ne=(5, 4, 0, 0)), _check('radius-negative', RADIUS, radius=-1), _check('radius-9', RADIUS, radius=9),
          _check('crowded', CROWDED, (3, 2), tiles=(0,) * 11 + (FULL,)), _check('crowded-before-null', CROWDED, (0, 1), tiles=(5, FULL) + (0,) * 10, has_coeffs=0),
          _check('null-coeffs', NULL, has_coeffs=0), _check('null-tau', NULL, has_tau=0), _check('tau-nan', TAU, (0, -1), tau=[float('nan'), 1.0]),
          _check('tau-inf', TAU, (1, -1), tau=[1.0, float('inf')]), _check('tau-minus-inf', TAU, (0, -1), tau=[float('-inf'), float('nan')]),
          _check('no-model', NO_MODEL, model_set=0), _check('width-short', WIDTH, n_coeffs=5), _check('width-long', WIDTH, n_coeffs=7),
          _check('flag-bit-0', BAD_FLAGS, flags=1), _check('flag-bit-31', BAD_FLAGS, flags=1 << 31),
          _check('events', EVENTS, (0, -1), ne=(2 ** 32,) * 2), _check('events-last-group', EVENTS, (2, -1), ne=(1, 1, 2 ** 40, 2 ** 40))]
CHECKS += [_check(f'from-{i + 1:02d}-{k}', _fault[i], _where.get(k, (-1, -1)), **_from(i)) for i, k in enumerate(_order)]
CHECKS += [_check('from-17-all-mended', OK, **_from(len(_order)))]


@pytest.fixture(scope='module')
def out(label_carry_check, tmp_path_factory):
    return HC.run(label_carry_check, CASES, tmp_path_factory, 'label_carry_cases')


@pytest.mark.parametrize('name', CHECKS)
def test_argument_check_in_its_order(out, name):
    fault, code, wb, wi = (int(v) for v in out[name][0])
    assert (fault, (wb, wi)) == EXPECT[name] and code == CODE[fault]


def test_the_label_prior_s_refusals_come_from_its_own_check():
    """lp_check is called, not restated, so the two cannot drift; and the header includes nothing of HIP"""
    lc = open(os.path.join(HC.CSRC, 'eincm_label_carry.h')).read()
    body = lc.split('inline int lc_check(')[1].split('\n}\n')[0]
    assert 'lp_check(' in body and 'in_flight' not in body and 'fp64' not in body and 'EINCM_LP_MAX_RADIUS' not in body
    assert 'hip' not in ''.join(re.findall(r'#include\s+[<"]([^>"]+)[>"]', lc)).lower()


# ---- eincm_adopt_carried_prior ----
(A_OK, A_IN_FLIGHT, A_NOT_STAGED, A_NONE, A_MODELS, A_WINDOWS, A_SENSOR) = range(7)
A_CODE = {A_OK: 0, A_IN_FLIGHT: ERR_STATE, A_NOT_STAGED: ERR_STATE, A_NONE: ERR_STATE, A_MODELS: ERR_ARG, A_WINDOWS: ERR_ARG, A_SENSOR: ERR_ARG}
ADOPT = {}


def _adopt(name, fault, in_flight=0, staged=1, valid=1, carried=(2, 4, 40, 72), now=(2, 4, 40, 72)):
    HC.add_case(CASES, 'adopt-' + name, 'adopt', in_flight, staged, valid, *carried, *now)
    ADOPT['adopt-' + name] = fault
    return 'adopt-' + name


_A_BAD = dict(in_flight=1, staged=0, valid=0, now=(3, 6, 41, 73))
_a_order = [dict(in_flight=0), dict(staged=1), dict(valid=1), dict(now=(2, 6, 41, 73)), dict(now=(2, 4, 41, 73)), dict(now=(2, 4, 40, 73))]
ADOPTS = [_adopt('ok', A_OK), _adopt('in-flight', A_IN_FLIGHT, in_flight=1), _adopt('not-staged', A_NOT_STAGED, staged=0),
          _adopt('none', A_NONE, valid=0), _adopt('none-whatever-it-remembers', A_NONE, valid=0, carried=(0, 0, 0, 0)),
          _adopt('another-k', A_MODELS, now=(4, 4, 40, 72)), _adopt('another-b', A_WINDOWS, now=(2, 6, 40, 72)),
          _adopt('another-height', A_SENSOR, now=(2, 4, 41, 72)), _adopt('another-width', A_SENSOR, now=(2, 4, 40, 71))]
for _i in range(7):
    _kw = dict(_A_BAD)
    for _m in _a_order[:_i]:
        _kw.update(_m)
    ADOPTS.append(_adopt(f'from-{_i + 1:02d}', _i + 1 if _i < 6 else A_OK, **(_kw if _i < 6 else dict(_kw, now=(2, 4, 40, 72)))))


@pytest.mark.parametrize('name', ADOPTS)
def test_adopt_check_in_its_order(out, name):
    fault, code = (int(v) for v in out[name][0])
    assert fault == ADOPT[name] and code == A_CODE[fault]


# ---- the resolve rule ----
FIRST_SATURATING = ((2 ** 32 - 1) << 20) + 2 ** 19           # the smallest A with (A + 2^19) >> 20 == 2^32
RESOLVE = [0, 2 ** 19 - 1, 2 ** 19, 2 ** 20, ((2 ** 32 - 1) << 20) + 2 ** 19 - 1, FIRST_SATURATING, 2 ** 64 - 1,
           1, 2 ** 20 - 1, 2 ** 20 + 2 ** 19 - 1, 2 ** 20 + 2 ** 19, 3 * 2 ** 19, 5 * 2 ** 19, FIRST_SATURATING - 2 ** 20, FIRST_SATURATING + 1,
           2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2 ** 19 - 1, 2 ** 64 - 2 ** 19, 1200000 * 4096 << 20]
RESOLVE += [int(v) for v in np.random.default_rng(5).integers(0, 2 ** 63, 40, dtype=np.uint64) >> np.random.default_rng(6).integers(0, 60, 40).astype(np.uint64)]
HC.add_case(CASES, 'resolve', 'resolve', *RESOLVE)


def test_resolve_rule_is_the_witness_s(out):
    got = [int(v) for v in out['resolve'][1]]
    want = WIT.resolve(np.array(RESOLVE, dtype=np.uint64))
    assert want.dtype == np.uint32 and got == [int(v) for v in want]
    assert got == [min((a + 2 ** 19) >> 20, 2 ** 32 - 1) for a in RESOLVE]          # the contract's formula in Python integers
    # half up, and where it saturates
    assert got[:7] == [0, 0, 1, 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1]
    assert ((2 ** 32 - 1) << 20) + 2 ** 19 - 1 + 2 ** 19 >> 20 == 2 ** 32 - 1 and (FIRST_SATURATING + 2 ** 19) >> 20 == 2 ** 32
    assert got[RESOLVE.index(3 * 2 ** 19)] == 2 and got[RESOLVE.index(5 * 2 ** 19)] == 3               # ties go up, to odd and to even alike


# ---- the layout ----
LAYOUTS = [(0, 2, 40, 72), (1, 1, 40, 72), (2, 3, 40, 72), (3, 8, 5, 7), (5, 2, 480, 640), (2, 8, 20000, 30000)]
for _l in LAYOUTS:
    HC.add_case(CASES, 'layout-%d-%d-%d-%d' % _l, 'layout', *_l)


@pytest.mark.parametrize('G,K,H,W', LAYOUTS)
def test_python_layout_is_the_headers(out, G, K, H, W):
    eng = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
    lay = eng.label_carry_layout(G, K, (H, W))
    _, pr, ca, ac, dr = out['layout-%d-%d-%d-%d' % (G, K, H, W)]
    assert tuple(lay) == eng.LC_OUTPUTS == ('prior', 'carried', 'accum', 'dropped')
    assert [lay[n][0] for n in eng.LC_OUTPUTS] == [(G * K, H, W), (G, K, H, W), (G, K, H, W), (G, K)]
    assert [lay[n][1] for n in eng.LC_OUTPUTS] == [np.float32, np.uint32, np.uint64, np.uint64]
    # the header gives every window's block of prior and every (group, model) block of the others; Python's are the groups' (model 0)
    for name, words, step in (('prior', pr, H * W), ('carried', ca, H * W), ('accum', ac, H * W), ('dropped', dr, 1)):
        assert [int(v) for v in words] == [int(lay[name][2][g]) + l * step for g in range(G) for l in range(K)], name


# ---- the overflow proof's constants ----
HC.add_case(CASES, 'constants', 'constants')


def test_overflow_bound_constants(out):
    shift, full, half, carried_max, events_max, staging_max, q_one = (int(v) for v in out['constants'][1])
    hi, lo = (int(v) for v in out['constants'][2])
    assert (shift, full, half, carried_max, q_one) == (20, 2 ** 20, 2 ** 19, 2 ** 32 - 1, 4096)
    assert (shift, full, half, carried_max, events_max) == (WIT.SHIFT, WIT.FULL, WIT.HALF, WIT.CARRIED_MAX, WIT.EVENTS_MAX)
    # a cell holds at most full * q_one * n_events: below 2^64 at events_max, not at one event more; staging's own limit lies below
    assert (hi << 64) + lo == full * q_one * events_max < 2 ** 64 <= full * q_one * (events_max + 1)
    assert staging_max == 2000000000 <= events_max and full * q_one * staging_max < 2 ** 63
    api = open(os.path.join(HC.CSRC, 'eincm_api.hip')).read()
    assert 'max_events_total > (int64_t)2000000000' in api                           # eincm_create's limit, which the header restates
