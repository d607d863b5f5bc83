"""The event-support filter on the GPU against the sequential numpy witness tests/_event_support_witness.py,
byte for byte, weights and support alike: the arithmetic is integer counts, one exact compare and one correctly rounded division, so
no tolerance applies.  tests/test_event_support_interface.py asserts on the CPU that every generated case has zeros, ones and values
between, so a kernel that returns a constant fails here.  Every test runs under its own time limit."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import _event_support_witness as ES

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
edges_mod = importlib.import_module(pkg + '.edges')
staging = importlib.import_module(pkg + '.staging')
synth = importlib.import_module(pkg + '.synth')

TIME_LIMIT_S = 60
_engines = {}


def _eng(shape, precision='fp32'):
    key = (tuple(shape), precision)
    if key not in _engines:
        _engines[key] = E.Engine(tuple(shape), max_events_total=1, max_refs=1, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    edges_mod.clear_engines()


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f'test exceeded {TIME_LIMIT_S} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TIME_LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


_witness = {}


def _case(name):
    """(xs, ys, ts, mask, spec, witness weights, witness support) of a generated case, computed once"""
    if name not in _witness:
        xs, ys, ts, mask, s = ES.generated(name)
        w, sup, _ = ES.support_filter(xs, ys, ts, s['shape'], s['tau'], s['radius'], s['full_support'], mask)
        for a in (xs, ys, ts, w, sup):
            a.setflags(write=False)
        _witness[name] = (xs, ys, ts, mask, s, w, sup)
    return _witness[name]


def _equal(got, w, sup):
    gw, gs = got
    assert gw.dtype == np.float32 and gs.dtype == np.uint8 and gw.shape == w.shape and gs.shape == sup.shape
    bad = np.nonzero(gs != sup)[0]
    assert bad.size == 0, f'{bad.size} of {len(sup)} supports differ, first at {bad[0]}: {gs[bad[0]]} for {sup[bad[0]]}'
    assert gw.tobytes() == w.tobytes()


def _run(eng, xs, ys, ts, s, mask=None, **kw):
    return eng.event_support(xs, ys, ts, s['tau'], radius=s['radius'], full_support=s['full_support'], pixel_mask=mask, return_support=True, **kw)


# ---- every generated case: sensors 3x3, 5x7, 33x65, 260x346; r = 1, 2, 3; full_support 1, middle, maximum; masks; ties; tau = 0;
# n on both sides of the trip and block sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ES.GENERATED))
def test_generated_case_equals_the_witness_and_repeats(name):
    xs, ys, ts, mask, s, w, sup = _case(name)
    eng = _eng(s['shape'])
    first = _run(eng, xs, ys, ts, s, mask)
    _equal(first, w, sup)
    again = _run(eng, xs, ys, ts, s, mask)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    assert eng.event_support(xs, ys, ts, s['tau'], radius=s['radius'], full_support=s['full_support'], pixel_mask=mask).tobytes() == w.tobytes()


@pytest.mark.parametrize('name', ['5x7-r2-k5', '33x65-r3-kmax', '33x65-r2-k4-mask', '5x7-r1-k1-tau0'])
def test_fp64_context_gives_the_same_bytes(name):
    xs, ys, ts, mask, s, w, sup = _case(name)
    _equal(_run(_eng(s['shape'], 'fp64'), xs, ys, ts, s, mask), w, sup)


def test_no_event_and_one_event():
    eng = _eng((5, 7))
    w, sup = eng.event_support(np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0), 1.0, return_support=True)
    assert w.shape == (0,) and w.dtype == np.float32 and sup.shape == (0,) and sup.dtype == np.uint8
    for x, y in ((0, 0), (6, 4), (3, 2)):
        w, sup = eng.event_support([x], [y], [3.5], 1.0, radius=3, full_support=7, return_support=True)
        assert w.tolist() == [0.0] and sup.tolist() == [0]


# ---- runs of equal timestamps longer than a wave, at one pixel and spread over a neighbourhood --------------------------------------
@pytest.mark.parametrize('tau', [0.0, 1.0])
@pytest.mark.parametrize('n_one,n_spread', [(65, 70), (100, 200), (1030, 1100)])
def test_runs_of_equal_timestamps(n_one, n_spread, tau):
    xs, ys, ts = ES.tie_stream((5, 7), n_one, n_spread)
    for r, k in ((1, 1), (1, 8), (2, 5)):
        w, sup, _ = ES.support_filter(xs, ys, ts, (5, 7), tau, r, k)
        assert 0 < sup.max() and (sup == 0).any()
        _equal(_eng((5, 7)).event_support(xs, ys, ts, tau, radius=r, full_support=k, return_support=True), w, sup)


# ---- list lengths on both sides of the sort's trip (64) and block (1024): two adjacent pixels alternate, so each list holds n / 2 ----
@pytest.mark.parametrize('n', [1, 2, 3, 127, 128, 129, 130, 2047, 2048, 2049, 2050])
def test_list_lengths_around_the_sort_sizes(n):
    i = np.arange(n)
    xs, ys = (i % 2).astype(np.int16), np.ones(n, np.int16)
    ts = np.cumsum(np.where(i % 5 == 0, 1.5, 0.25))                  # every fifth step is longer than tau: support ages out
    w, sup, _ = ES.support_filter(xs, ys, ts, (3, 3), 1.0)
    if n > 10:
        assert (w == 0).any() and (w == 1).any()
    _equal(_eng((3, 3)).event_support(xs, ys, ts, 1.0, return_support=True), w, sup)


def test_two_hot_pixels_with_2e5_events_finish_in_normal_time():
    """Alternating and in bursts, ~10^5 indices in each of two lists: only a search that is not linear in the list finishes inside the
    time limit of a test (a linear walk reads ~10^10 list entries)."""
    xs, ys, ts = ES.two_pixel_stream(200000)
    w, sup, _ = ES.support_filter(xs, ys, ts, (3, 3), 1.0)
    assert (w == 0).mean() >= 0.2 and (w == 1).mean() >= 0.2
    _equal(_eng((3, 3)).event_support(xs, ys, ts, 1.0, return_support=True), w, sup)


# ---- chunking and the carried state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['5x7-r2-k3-ties', '33x65-r2-k4-mask'])
def test_result_does_not_depend_on_chunk(name):
    xs, ys, ts, mask, s, w, sup = _case(name)
    n = 1500
    xs, ys, ts = xs[:n], ys[:n], ts[:n]
    for chunk in (1, 7, 1024, 1025, n):
        _equal(_run(_eng(s['shape']), xs, ys, ts, s, mask, chunk=chunk), w[:n], sup[:n])


def _raw(eng, xs, ys, ts, tau, radius, k, mask, reset, w, sup):
    xs, ys, ts = np.ascontiguousarray(xs, np.int16), np.ascontiguousarray(ys, np.int16), np.ascontiguousarray(ts, np.float64)
    return eng._lib.eincm_event_support(eng._ctx, xs.ctypes.data, ys.ctypes.data, ts.ctypes.data, len(xs), tau, radius, k,
                                        None if mask is None else mask.ctypes.data, reset, w.ctypes.data, None if sup is None else sup.ctypes.data)


def test_reset_clears_the_carried_map_and_the_carried_time():
    xs, ys, ts, mask, s, w, sup = _case('5x7-r2-k5')
    eng, n, cut = _eng((5, 7)), len(xs), 333
    gw, gs = np.empty(n, np.float32), np.empty(n, np.uint8)
    args = (s['tau'], s['radius'], s['full_support'], None)
    assert _raw(eng, xs[:cut], ys[:cut], ts[:cut], *args, 1, gw[:cut], gs[:cut]) == L.OK
    assert _raw(eng, xs[cut:], ys[cut:], ts[cut:], *args, 0, gw[cut:], gs[cut:]) == L.OK
    _equal((gw, gs), w, sup)
    # without a reset the stream's start is older than the carried time: refused, naming event 0, outputs untouched
    gw[:] = -1.0
    assert _raw(eng, xs, ys, ts, *args, 0, gw, gs) == L.ERR_ARG
    assert 'event 0' in eng._lib.eincm_last_error(eng._ctx).decode() and np.all(gw == -1.0)
    # every pixel fires once at the carried time: without a reset the old events support them through the map; with a reset they do not
    assert _raw(eng, xs, ys, ts, *args, 1, gw, gs) == L.OK
    x2, y2, t2 = np.tile(np.arange(7), 5), np.repeat(np.arange(5), 7), np.full(35, ts[-1])
    last = ES.support_filter(xs, ys, ts, (5, 7), *args[:3])[2]
    w_carry, sup_carry, _ = ES.support_filter(x2, y2, t2, (5, 7), *args[:3], last=last)
    w_fresh, sup_fresh, _ = ES.support_filter(x2, y2, t2, (5, 7), *args[:3])
    assert sup_carry.tobytes() != sup_fresh.tobytes()
    hw, hs = np.empty(35, np.float32), np.empty(35, np.uint8)
    assert _raw(eng, x2, y2, t2, *args, 0, hw, hs) == L.OK
    _equal((hw, hs), w_carry, sup_carry)
    assert _raw(eng, x2, y2, t2, *args, 1, hw, None) == L.OK             # (support may be NULL)
    assert hw.tobytes() == w_fresh.tobytes()


def test_refusals_of_the_library_name_the_first_offender_and_leave_the_state():
    xs, ys, ts, mask, s, w, sup = _case('5x7-r1-k1')
    eng, n = _eng((5, 7)), len(xs)
    args = (s['tau'], s['radius'], s['full_support'], None)
    gw, gs = np.empty(n, np.float32), np.empty(n, np.uint8)
    half = n // 2
    assert _raw(eng, xs[:half], ys[:half], ts[:half], *args, 1, gw[:half], gs[:half]) == L.OK
    for which, at, value in ((0, 301, 7), (0, 5, -1), (1, 64, 5), (2, 200, np.nan), (2, 255, np.inf), (2, 300, ts[half + 299] - 1e-9)):
        a = [xs[half:].copy(), ys[half:].copy(), ts[half:].copy()]
        a[which][at] = value
        a[0][340] = 99                                                   # a later offender never wins
        out = np.full(n - half, -1.0, np.float32)
        assert _raw(eng, *a, *args, 0, out, None) == L.ERR_ARG
        assert f'event {at}:' in eng._lib.eincm_last_error(eng._ctx).decode() and np.all(out == -1.0)
    for bad in (dict(tau=-1.0), dict(tau=np.nan), dict(radius=0), dict(radius=4), dict(k=0), dict(k=9)):
        kw = dict(dict(tau=1.0, radius=1, k=1), **bad)
        assert _raw(eng, xs[half:], ys[half:], ts[half:], kw['tau'], kw['radius'], kw['k'], None, 0, gw[half:], None) == L.ERR_ARG
    assert eng._lib.eincm_event_support(eng._ctx, None, None, None, -1, 1.0, 1, 1, None, 0, None, None) == L.ERR_ARG
    assert eng._lib.eincm_event_support(eng._ctx, None, ys.ctypes.data, ts.ctypes.data, 4, 1.0, 1, 1, None, 0, gw.ctypes.data, None) == L.ERR_ARG
    # the carried state is what the first half left: the second half completes the unsplit result
    assert _raw(eng, xs[half:], ys[half:], ts[half:], *args, 0, gw[half:], gs[half:]) == L.OK
    _equal((gw, gs), w, sup)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def test_masking_a_pixel_silences_the_neighbours_that_lived_on_its_support():
    n = 300
    i = np.arange(n)
    xs, ys, ts = np.where(i % 2 == 0, 30, 31).astype(np.int16), np.full(n, 16, np.int16), i * 0.1      # across the 32-pixel tile edge
    eng = _eng((33, 65))
    w = eng.event_support(xs, ys, ts, 1.0)
    assert w[0] == 0 and np.all(w[1:] == 1)
    mask = np.zeros((33, 65), np.uint8)
    mask[16, 31] = 255
    w, sup = eng.event_support(xs, ys, ts, 1.0, pixel_mask=mask, return_support=True)
    assert not w.any() and not sup.any()
    ww, ws, _ = ES.support_filter(xs, ys, ts, (33, 65), 1.0, pixel_mask=mask)
    _equal((w, sup), ww, ws)


# ---- beside the evaluation --------------------------------------------------------------------------------------------------------------
def _window(n=3000, shape=(33, 65)):
    return synth.make_window(4, shape, n, 2, flow='smooth', flow_mag=3.0)


def test_operator_between_two_evaluations_leaves_value_and_gradient_bits():
    shape = (33, 65)
    win = _window()
    xs, ys, ts, mask, s, w, sup = _case('33x65-r2-k12')
    theta = synth.theta_near_truth(1, win, (4, 4))
    p = E.make_params(20.0, 35.0, 2.5e-4, 0.0, 0)
    with E.Engine(shape, len(win['xs']), max_refs=2) as eng:
        eng.set_window(win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])
        v0, g0, _ = eng.loss_grad(theta, p)
        _equal(_run(eng, xs, ys, ts, s), w, sup)
        v1, g1, _ = eng.loss_grad(theta, p)
        assert v0.tobytes() == v1.tobytes() and g0.tobytes() == g1.tobytes()
        # an evaluation in flight: refused as the other one-shot operators refuse it, and the evaluation is untouched
        eng.loss_grad_async(theta, p)
        with pytest.raises(E.EincmError, match='in flight') as ei:
            _run(eng, xs, ys, ts, s)
        assert ei.value.code == L.ERR_STATE
        v2, g2, _ = eng.loss_grad_wait()
        assert v0.tobytes() == v2.tobytes() and g0.tobytes() == g2.tobytes()
        _equal(_run(eng, xs, ys, ts, s), w, sup)


def test_weights_end_to_end_through_staging_into_one_loss_grad():
    shape = (33, 65)
    win = _window()
    n = len(win['xs'])
    raw_t = 1.0e6 + win['ts'] * 5.0e4                                      # raw times in "microseconds"; tau in their unit
    order = np.argsort(raw_t, kind='stable')
    ev = dict(x=win['xs'][order], y=win['ys'][order], t=raw_t[order])
    mask = staging.hot_pixel_mask(ev['x'], ev['y'], shape, 6)
    tau, r, k = 4000.0, 2, 3
    w_ref, sup_ref, _ = ES.support_filter(ev['x'], ev['y'], ev['t'], shape, tau, r, k, mask)
    assert (w_ref == 0).mean() >= 0.2 and (w_ref == 1).mean() >= 0.2
    w_gpu, sup_gpu = staging.event_support_weights(ev, shape, tau, radius=r, full_support=k, pixel_mask=mask, return_support=True)
    _equal((w_gpu, sup_gpu), w_ref, sup_ref)
    ds = dict(events=ev, image_ts=np.array([raw_t.min(), raw_t.max()]), eval_ts=(raw_t.min(), raw_t.max()))
    theta = synth.theta_near_truth(1, win, (1, 1))
    p = E.make_params(20.0, 35.0, 0.0, 0.0, 0)
    res = []
    with E.Engine(shape, n, max_refs=2) as eng:
        for wts in (w_gpu, w_ref):
            tup = staging.stage_datasample(ds, edges=win['edges'], event_weights=wts)
            assert len(tup) == 6
            eng.set_windows([tup])
            assert eng.weighted
            v, g, _ = eng.loss_grad(theta, p)
            res.append((v.tobytes(), g.tobytes()))
        eng.set_windows([staging.stage_datasample(ds, edges=win['edges'])])
        v_plain, _, _ = eng.loss_grad(theta, p)
    assert res[0] == res[1] and np.isfinite(np.frombuffer(res[0][0])).all()
    assert v_plain.tobytes() != res[0][0]                                  # the weights did reach the loss
