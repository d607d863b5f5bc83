"""The HIP-free rules of the event-support filter (csrc/eincm_event_support.h) on the CPU: the argument checks,
the geometry of the sort by pixel (es_sort_plan) up to 2^30 events and 2^24 pixels, the first refused event of a chunk, the
neighbour window at corners, edges and inside for r = 1, 2, 3, and the carried-time rule walked chunk by chunk (the previous event of
a neighbour: its last one in the chunk, else the carried map's).

tests/host/event_support_check.cpp is built once per session with the address and undefined-behaviour sanitizers, as
tests/test_host_plan.py builds plan_check, and run once, as a child process, over every case of this module; nothing is preloaded.
Its lines equal numpy (tests/_event_support_witness.py and the Python-side checks of engine.py)."""
import importlib

import numpy as np
import pytest

import _host_check as HC
import _event_support_witness as ES

E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')


@pytest.fixture(scope='session')
def event_support_check(tmp_path_factory):
    return HC.build(tmp_path_factory, 'event_support_check')


CASES, EXPECT = {}, {}
ARG_OK, ARG_N, ARG_TAU, ARG_RADIUS, ARG_FULL = range(5)
EV_COORD, EV_TIME, EV_ORDER = 1, 2, 3


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _args(name, n, tau, radius, fs, fault):
    HC.add_case(CASES, 'args-' + name, 'args', n, float(tau), radius, fs)
    EXPECT['args-' + name] = fault
    return 'args-' + name


ARGS = [_args('ok', 10, 1.0, 1, 1, ARG_OK), _args('n0', 0, 0.0, 3, 48, ARG_OK), _args('n-max', 1 << 30, 1.0, 1, 8, ARG_OK),
        _args('n-neg', -1, 1.0, 1, 1, ARG_N), _args('n-over', (1 << 30) + 1, 1.0, 1, 1, ARG_N),
        _args('tau-neg', 5, -1e-300, 1, 1, ARG_TAU), _args('tau-nan', 5, np.nan, 1, 1, ARG_TAU), _args('tau-inf', 5, np.inf, 1, 1, ARG_TAU),
        _args('r0', 5, 1.0, 0, 1, ARG_RADIUS), _args('r4', 5, 1.0, 4, 1, ARG_RADIUS),
        _args('k0', 5, 1.0, 1, 0, ARG_FULL), _args('k9-r1', 5, 1.0, 1, 9, ARG_FULL), _args('k24-r2', 5, 1.0, 2, 24, ARG_OK),
        _args('k25-r2', 5, 1.0, 2, 25, ARG_FULL), _args('k48-r3', 5, 1.0, 3, 48, ARG_OK), _args('k49-r3', 5, 1.0, 3, 49, ARG_FULL),
        _args('n-before-tau', -1, np.nan, 0, 0, ARG_N)]


# ---- the geometry of the sort by pixel ---------------------------------------------------------------------------------------------
SORT_BLOCK, RADIX_BITS, SCAN_TILE = 1024, 8, 4096      # ES_SORT_BLOCK, ES_RADIX_BITS, ES_SCAN_TILE (csrc/eincm_event_support.h)


def _plan(n, npix):
    name = f'plan-n{n}-npix{npix}'
    HC.add_case(CASES, name, 'plan', n, npix)
    nblk = -(-n // SORT_BLOCK)
    nhist = (1 << RADIX_BITS) * nblk
    passes = next(k for k in range(1, 5) if npix <= 1 << (RADIX_BITS * k))     # the fewest 8-bit digits that tell npix keys apart
    EXPECT[name] = (nblk, nhist, -(-nhist // SCAN_TILE), passes, 1)
    return name


PLANS = [_plan(n, npix) for npix in (1, 2, 256, 257, 65536, 65537, 1 << 24) for n in (0, 1, 1024, 1025, 16384, 16385, 1 << 30)]


# ---- first offender ------------------------------------------------------------------------------------------------------------
def _first(name, H, W, x, y, t, carried=-np.inf):
    x, y, t = np.asarray(x, dtype=np.int16), np.asarray(y, dtype=np.int16), np.asarray(t, dtype=np.float64)
    HC.add_case(CASES, 'first-' + name, 'first', H, W, float(carried), len(x), *list(x), *list(y), *[float(v) for v in t])
    got = E.event_support_first_offender(x, y, t, (H, W), carried)
    # the sequential rule, in Python: the first event that is outside, not finite, or earlier than its predecessor
    prev, ref = carried, (-1, 0)
    for e in range(len(x)):
        f = EV_COORD if not (0 <= x[e] < W and 0 <= y[e] < H) else EV_TIME if not np.isfinite(t[e]) else EV_ORDER if t[e] < prev else 0
        if f:
            ref = (e, f)
            break
        prev = t[e]
    assert (got is None and ref[0] == -1) or (got is not None and got[0] == ref[0]), (got, ref)
    EXPECT['first-' + name] = ref
    return 'first-' + name


_rng = np.random.default_rng(3)


def _good(n, H=5, W=7):
    return _rng.integers(0, W, n), _rng.integers(0, H, n), np.sort(_rng.integers(0, 50, n)).astype(np.float64)


def _with(arrs, which, at, value):
    a = [np.array(v, dtype=np.float64 if i == 2 else np.int64) for i, v in enumerate(arrs)]
    a[which][at] = value
    return a


FIRST = [_first('none', 5, 7, *_good(40)), _first('empty', 5, 7, [], [], []),
         _first('x-neg', 5, 7, *_with(_good(40), 0, 13, -1)), _first('x-w', 5, 7, *_with(_good(40), 0, 13, 7)),
         _first('y-neg', 5, 7, *_with(_good(40), 1, 0, -1)), _first('y-h', 5, 7, *_with(_good(40), 1, 39, 5)),
         _first('nan', 5, 7, *_with(_good(40), 2, 20, np.nan)), _first('inf', 5, 7, *_with(_good(40), 2, 20, np.inf)),
         _first('minus-inf', 5, 7, *_with(_good(40), 2, 0, -np.inf)),
         _first('order', 5, 7, [1, 1, 1, 1], [2, 2, 2, 2], [1.0, 2.0, 1.5, 0.0]),
         _first('equal-times-are-fine', 5, 7, [1, 1, 1], [2, 2, 2], [1.0, 1.0, 1.0]),
         _first('carried-equal', 5, 7, [1, 1], [2, 2], [3.0, 4.0], carried=3.0),
         _first('carried-above', 5, 7, [1, 1], [2, 2], [3.0, 4.0], carried=3.0000000000000004),
         _first('after-inf-reports-the-inf', 5, 7, [1, 1, 1], [2, 2, 2], [1.0, np.inf, 2.0]),
         _first('after-nan-is-not-ordered', 5, 7, [1, 1, 9], [2, 2, 2], [1.0, np.nan, 0.5]),
         _first('coord-before-time', 5, 7, [1, 9], [2, 2], [1.0, np.nan]),
         _first('earlier-order-beats-later-coord', 5, 7, [1, 1, 9], [2, 2, 2], [2.0, 1.0, 3.0])]


# ---- neighbour window ------------------------------------------------------------------------------------------------------------
def _window(name, H, W, r):
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (W // 2, H // 2),
           (min(W - 1, r), min(H - 1, r)), (max(0, W - 1 - r), max(0, H - 1 - r)), (min(W - 1, r - 1), min(H - 1, r - 1))]
    HC.add_case(CASES, 'window-' + name, 'window', H, W, r, len(pts), *[p[0] for p in pts], *[p[1] for p in pts])
    exp = []
    for x, y in pts:
        inside = np.zeros((H, W), dtype=bool)
        yy, xx = np.mgrid[0:H, 0:W]
        inside[np.maximum(np.abs(yy - y), np.abs(xx - x)) <= r] = True        # Chebyshev distance <= r inside the sensor
        ys_, xs_ = np.nonzero(inside)
        exp += [xs_.min(), xs_.max(), ys_.min(), ys_.max(), int(inside.sum()) - 1]
    EXPECT['window-' + name] = exp
    return 'window-' + name


WINDOWS = [_window(f'{H}x{W}-r{r}', H, W, r) for (H, W) in ((3, 3), (5, 7), (33, 65), (1, 1), (2, 9)) for r in (1, 2, 3)]


# ---- the carried-time rule, chunk by chunk ---------------------------------------------------------------------------------------
def _filter(name, spec_name, chunks, n=None):
    xs, ys, ts, mask, s = ES.generated(spec_name)
    if n is not None:
        xs, ys, ts = xs[:n], ys[:n], ts[:n]
    n = len(xs)
    lens, left = [], n
    for c in chunks:
        lens.append(min(left, c))
        left -= lens[-1]
    lens.append(left)
    H, W = s['shape']
    HC.add_case(CASES, 'filter-' + name, 'filter', H, W, float(s['tau']), s['radius'], s['full_support'], int(mask is not None), len(lens), *lens,
                n, *list(xs), *list(ys), *[float(v) for v in ts], *([] if mask is None else list(mask.ravel())))
    EXPECT['filter-' + name] = ES.support_filter(xs, ys, ts, s['shape'], s['tau'], s['radius'], s['full_support'], mask)
    return 'filter-' + name


FILTERS = [_filter('3x3-whole', '3x3-r1-k3', []), _filter('3x3-r3-in-ones', '3x3-r3-k8', [1] * 60, n=60),
           _filter('5x7-r2-split', '5x7-r2-k5', [7, 1, 0, 300]), _filter('5x7-tau0', '5x7-r1-k1-tau0', [100, 101]),
           _filter('5x7-ties-split-inside-a-run', '5x7-r2-k3-ties', [75, 80, 500]), _filter('5x7-mask', '5x7-r1-k4-mask', [450]),
           _filter('33x65-r3-kmax', '33x65-r3-kmax', [1024, 1025], n=3000), _filter('33x65-mask', '33x65-r2-k4-mask', [1500])]


@pytest.fixture(scope='module')
def out(event_support_check, tmp_path_factory):
    return HC.run(event_support_check, CASES, tmp_path_factory, 'event_support_cases')


@pytest.mark.parametrize('name', ARGS)
def test_argument_checks(out, name):
    assert int(out[name][0][0]) == EXPECT[name]


@pytest.mark.parametrize('name', PLANS)
def test_sort_plan_and_that_its_numbers_fit_their_types(out, name):
    assert tuple(int(v) for v in out[name][0]) == EXPECT[name]


@pytest.mark.parametrize('name', FIRST)
def test_first_offender(out, name):
    assert tuple(int(v) for v in out[name][0]) == EXPECT[name]


@pytest.mark.parametrize('name', WINDOWS)
def test_neighbour_window(out, name):
    assert np.array_equal(HC.i(out[name][1]), np.array(EXPECT[name], dtype=np.int64))


@pytest.mark.parametrize('name', FILTERS)
def test_carried_time_rule_gives_the_unsplit_bytes(out, name):
    w, sup, last = EXPECT[name]
    _, got_s, got_w, got_m = out[name]
    assert np.array_equal(HC.i(got_s), sup.astype(np.int64))
    assert np.array_equal(HC.i(got_w), w.view(np.uint32).astype(np.int64))
    assert np.array_equal(np.array([int(v) for v in got_m], dtype=np.uint64), last.ravel().view(np.uint64))
