"""The HIP-free rules of the refractory and polarity-aware event filter (csrc/eincm_event_filter.h) on the CPU:
the argument checks in their order, the refractory rule at -inf, at equal times and at t - prev == refractory exactly, and a
sequential filter built from the header's functions and walked chunk by chunk, which equals the numpy witness
(tests/_event_filter_witness.py) in keep, support, weight bits and all three carried maps.

tests/host/event_filter_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_event_support.py builds its checker, and run once, as a child process, over every case of this module; nothing is
preloaded."""
import numpy as np
import pytest

import _host_check as HC
import _event_filter_witness as EF


@pytest.fixture(scope='session')
def event_filter_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'event_filter_check')


CASES, EXPECT = {}, {}
ARG_OK, ARG_N, ARG_RHO, ARG_TAU, ARG_RADIUS, ARG_FULL, ARG_FLAGS = range(7)


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _args(name, fault, n=5, rho=0.5, tau=1.0, radius=1, fs=1, flags=0, has_p=1):
    HC.add_case(CASES, 'args-' + name, 'args', n, float(rho), float(tau), radius, fs, flags, has_p)
    EXPECT['args-' + name] = fault
    return 'args-' + name


ARGS = [_args('ok', ARG_OK), _args('n0', ARG_OK, n=0), _args('n-max', ARG_OK, n=1 << 30), _args('n-neg', ARG_N, n=-1),
        _args('n-over', ARG_N, n=(1 << 30) + 1), _args('rho0', ARG_OK, rho=0.0), _args('rho-neg', ARG_RHO, rho=-1e-300),
        _args('rho-nan', ARG_RHO, rho=np.nan), _args('rho-inf', ARG_RHO, rho=np.inf), _args('tau0', ARG_OK, tau=0.0),
        _args('tau-neg', ARG_TAU, tau=-1.0), _args('tau-nan', ARG_TAU, tau=np.nan), _args('tau-inf', ARG_TAU, tau=np.inf),
        _args('r0-k1', ARG_OK, radius=0), _args('r0-k2', ARG_FULL, radius=0, fs=2), _args('r-neg', ARG_RADIUS, radius=-1),
        _args('r4', ARG_RADIUS, radius=4), _args('k0', ARG_FULL, fs=0), _args('k9-r1', ARG_FULL, fs=9), _args('k8-r1', ARG_OK, fs=8),
        _args('k24-r2', ARG_OK, radius=2, fs=24), _args('k25-r2', ARG_FULL, radius=2, fs=25), _args('k48-r3', ARG_OK, radius=3, fs=48),
        _args('k49-r3', ARG_FULL, radius=3, fs=49), _args('polarity', ARG_OK, flags=1), _args('polarity-without-p', ARG_FLAGS, flags=1, has_p=0),
        _args('no-flag-without-p', ARG_OK, has_p=0), _args('flag2', ARG_FLAGS, flags=2), _args('flag3', ARG_FLAGS, flags=3),
        _args('flag-neg', ARG_FLAGS, flags=-1),
        # the first of the order n, refractory, tau, radius, full_support, flags
        _args('n-first', ARG_N, n=-1, rho=np.nan, tau=np.nan, radius=9, fs=0, flags=8),
        _args('rho-second', ARG_RHO, rho=np.nan, tau=np.nan, radius=9, fs=0, flags=8),
        _args('tau-third', ARG_TAU, tau=np.nan, radius=9, fs=0, flags=8), _args('radius-fourth', ARG_RADIUS, radius=9, fs=0, flags=8),
        _args('full-fifth', ARG_FULL, fs=0, flags=8)]


# ---- the refractory rule -----------------------------------------------------------------------------------------------------
def _kept(name, t, prev, rho, masked, expect):
    HC.add_case(CASES, 'kept-' + name, 'kept', float(t), float(prev), float(rho), int(masked))
    EXPECT['kept-' + name] = int(expect)
    return 'kept-' + name


KEPT = [_kept('first-event', 3.0, -np.inf, 1e300, 0, 1), _kept('first-event-masked', 3.0, -np.inf, 1.0, 1, 0),
        _kept('equal-times', 3.0, 3.0, 0.5, 0, 0), _kept('equal-times-rho0', 3.0, 3.0, 0.0, 0, 1),
        _kept('exactly-rho', 3.5, 3.0, 0.5, 0, 1), _kept('one-ulp-inside', 3.5 - 2.0 ** -51, 3.0, 0.5, 0, 0),
        _kept('outside', 9.0, 3.0, 0.5, 0, 1), _kept('outside-masked', 9.0, 3.0, 0.5, 1, 0), _kept('rho0-masked', 9.0, 3.0, 0.0, 1, 0)]


# ---- the sequential filter, chunk by chunk ---------------------------------------------------------------------------------------
def _filter(name, spec_name, chunks, polarity, n=None, with_p=True, rho=None):
    xs, ys, ts, ps, mask, s = EF.generated(spec_name)
    if n is not None:
        xs, ys, ts, ps = xs[-n:], ys[-n:], ts[-n:], ps[-n:]           # (the end of a stream is a chatter phase)
    n = len(xs)
    if not with_p:
        ps = None
    rho = s['refractory'] if rho is None else rho
    lens, left = [], n
    for c in chunks:
        lens.append(min(left, c))
        left -= lens[-1]
    lens.append(left)
    H, W = s['shape']
    HC.add_case(CASES, 'filter-' + name, 'filter', H, W, float(rho), float(s['tau']), s['radius'], s['full_support'], int(polarity),
                int(ps is not None), int(mask is not None), len(lens), *lens, n, *list(xs), *list(ys), *[float(v) for v in ts],
                *([] if ps is None else list(ps)), *([] if mask is None else list(mask.ravel())))
    EXPECT['filter-' + name] = EF.event_filter(xs, ys, ts, ps, s['shape'], rho, s['tau'], s['radius'], s['full_support'], polarity, mask)
    return 'filter-' + name


FILTERS = [_filter('3x3-whole', '3x3-r1-k3', [], False), _filter('3x3-whole-polarity', '3x3-r1-k3', [], True),
           _filter('3x3-r3-in-ones', '3x3-r3-k8', [1] * 80, True, n=80), _filter('5x7-r2-split', '5x7-r2-k5', [7, 1, 0, 300], True),
           _filter('5x7-tau0', '5x7-r1-k1-tau0', [100, 101], False), _filter('5x7-tau0-polarity', '5x7-r1-k1-tau0', [100, 101], True),
           _filter('5x7-ties-split-inside-a-run', '5x7-r2-k3-ties', [75, 80, 500], True),
           _filter('5x7-split-inside-a-chatter-phase', '5x7-r2-k5', [660, 5, 40], False), _filter('5x7-mask', '5x7-r1-k4-mask', [450], True),
           _filter('5x7-no-p', '5x7-r1-k1', [333], False, with_p=False), _filter('5x7-rho0', '5x7-r2-k5', [400], True, rho=0.0),
           _filter('5x7-r0', '5x7-r0', [100, 650], False), _filter('33x65-r3-kmax', '33x65-r3-kmax', [1024, 1025], True, n=3000),
           _filter('33x65-mask', '33x65-r2-k4-mask', [1500], False)]


@pytest.fixture(scope='module')
def out(event_filter_check, tmp_path_factory):
    return HC.run(event_filter_check, CASES, tmp_path_factory, 'event_filter_cases')


@pytest.mark.parametrize('name', ARGS)
def test_argument_checks_in_their_order(out, name):
    assert int(out[name][0][0]) == EXPECT[name]


@pytest.mark.parametrize('name', KEPT)
def test_refractory_rule(out, name):
    assert int(out[name][0][0]) == EXPECT[name]


@pytest.mark.parametrize('name', FILTERS)
def test_sequential_filter_in_chunks_equals_the_witness(out, name):
    keep, w, sup, st = EXPECT[name]
    _, got_k, got_s, got_w, got_m = out[name]
    assert 0 < keep.sum() < len(keep) or name.endswith('rho0')
    assert np.array_equal(HC.i(got_k), keep.astype(np.int64))
    assert np.array_equal(HC.i(got_s), sup.astype(np.int64))
    assert np.array_equal(HC.i(got_w), w.view(np.uint32).astype(np.int64))
    assert np.array([int(v) for v in got_m], dtype=np.uint64).tobytes() == st.tobytes()
