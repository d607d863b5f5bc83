"""The event-support filter without a GPU: the entry point in header, binding and cross-compiled library, the
refusals that Python raises before a library call, properties of the sequential witness (tests/_event_support_witness.py), the
hot-pixel mask, and the condition that keeps tests/test_gpu_event_support.py honest: from the witness alone, every generated case
has at least 20 % of its events at weight 0, at least 20 % at weight 1 and, where full_support > 1, at least 10 % strictly between."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import _event_support_witness as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')
E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
staging = importlib.import_module('edge-informed-contrast-maximization_amd.staging')

NAME = 'eincm_event_support'


# ---- the entry point ---------------------------------------------------------------------------------------------------------
def test_entry_point_in_header_binding_and_library(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    m = re.search(r'int\s+' + NAME + r'\s*\(([^)]*)\)', hdr)
    assert m, 'not declared'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert args == ['eincm_ctx* ctx', 'const int16_t* x', 'const int16_t* y', 'const double* t', 'int64_t n', 'double tau', 'int radius',
                    'int full_support', 'const uint8_t* pixel_mask', 'int reset', 'float* weights', 'uint8_t* support']
    assert int(dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)\b', hdr))['EINCM_ABI_VERSION']) == 6
    assert NAME in hdr.split('#define EINCM_ABI_VERSION')[1].split('*/')[0], 'not in the name list after EINCM_ABI_VERSION'
    assert [n for n, _, _ in L.SIGNATURES].count(NAME) == 1
    res, a = {n: (r, a) for n, r, a in L.SIGNATURES}[NAME]
    assert res is C.c_int and a == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p]
    fn = getattr(built_lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == a
    assert built_lib.eincm_abi_version() == 6
    assert hasattr(C.CDLL(os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'libeincm_hip.so')), NAME)
    assert fn(None, None, None, None, 0, 1.0, 1, 1, None, 0, None, None) == L.ERR_ARG        # no context: refused without a GPU


def test_kernels_live_in_their_own_header_and_the_rules_in_a_hip_free_one():
    csrc = os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc')
    rules = open(os.path.join(csrc, 'eincm_event_support.h')).read()
    assert 'hip' not in ''.join(re.findall(r'#include\s+[<"]([^>"]+)[>"]', rules)).lower()
    kern = open(os.path.join(csrc, 'eincm_event_support.hip.h')).read()
    assert '__global__' in kern and 'k_es_support' in kern
    api = open(os.path.join(csrc, 'eincm_api.hip')).read()
    body = api.split('int eincm_event_support(')[1].split('\n}\n')[0]
    assert 'not_in_flight(c, "eincm_event_support")' in body and 'OneShot op(c);' in body
    assert 'c->ef.' not in body                                          # the carried state is its own
    # the geometry of the sort is host arithmetic: stated in the HIP-free header (where tests/host/event_support_check.cpp reaches
    # it) and in no kernel header
    hip_headers = [f for f in os.listdir(csrc) if f.endswith('.hip.h')]
    assert 'eincm_event_support.hip.h' in hip_headers and 'eincm_event_filter.hip.h' in hip_headers
    for name in ('ES_RADIX_BITS', 'ES_RADIX', 'ES_SORT_BLOCK', 'ES_SCAN_NT', 'ES_SCAN_TILE'):
        define = r'constexpr\s+int\s+' + name + r'\s*='
        assert len(re.findall(define, rules)) == 1, name
        for f in hip_headers:
            assert not re.search(define, open(os.path.join(csrc, f)).read()), (name, f)
    for fn in ('es_sort_passes', 'es_sort_plan'):
        define = r'inline\s+\w+\s+' + fn + r'\s*\('
        assert len(re.findall(define, rules)) == 1, fn
        for f in hip_headers:
            assert not re.search(define, open(os.path.join(csrc, f)).read()), (fn, f)


# ---- the refusals, with a stub in the library's place ---------------------------------------------------------------------------
class NoGpu:
    """Stands where the library is: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


def stub_engine(H=5, W=7):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = 'fp32', 3, 0, 0, H, W
    eng._io = {}
    return eng


def _ok(n=6):
    return np.arange(n) % 7, np.arange(n) % 5, np.arange(n, dtype=np.float64)


def test_a_good_call_reaches_the_library():
    with pytest.raises(AssertionError, match=NAME + ' was reached'):
        stub_engine().event_support(*_ok(), 1.0)
    with pytest.raises(AssertionError, match=NAME + ' was reached'):
        stub_engine().event_support(*_ok(), 0.0, radius=3, full_support=48, pixel_mask=np.zeros((5, 7), bool), chunk=1, return_support=True)
    with pytest.raises(AssertionError, match=NAME + ' was reached'):
        stub_engine().event_support(_ok()[0], _ok()[1], np.arange(6, dtype=np.int64) + (1 << 53) - 5, 1)


def _set(arr, at, v, dtype=None):
    a = np.array(arr, dtype=dtype)
    a[at] = v
    return a


X, Y, T = _ok()
BAD_EVENTS = [
    ('x-negative', (_set(X, 3, -1), Y, T), 'event 3'), ('x-at-W', (_set(X, 2, 7), Y, T), 'event 2'),
    ('y-negative', (X, _set(Y, 0, -1), T), 'event 0'), ('y-at-H', (X, _set(Y, 5, 5), T), 'event 5'),
    ('nan', (X, Y, _set(T, 4, np.nan)), 'event 4'), ('inf', (X, Y, _set(T, 1, np.inf)), 'event 1'),
    ('minus-inf', (X, Y, _set(T, 0, -np.inf)), 'event 0'), ('order', (X, Y, _set(T, 3, 1.5)), 'event 3'),
    ('the-first-of-two', (_set(X, 4, 99), Y, _set(T, 2, 0.0)), 'event 2'),
]


@pytest.mark.parametrize('name,args,match', BAD_EVENTS, ids=[b[0] for b in BAD_EVENTS])
def test_bad_events_are_value_errors_with_the_first_index_before_any_library_call(name, args, match):
    with pytest.raises(ValueError, match=match + r'\b'):
        stub_engine().event_support(*args, 1.0)
    with pytest.raises(ValueError, match=match + r'\b'):
        staging.event_support_weights(dict(x=args[0], y=args[1], t=args[2]), (5, 7), 1.0, engine=stub_engine())


@pytest.mark.parametrize('kw', [dict(tau=-1.0), dict(tau=np.nan), dict(tau=np.inf), dict(tau='a'), dict(radius=0), dict(radius=4),
                                dict(radius=1.0), dict(radius=True), dict(full_support=0), dict(full_support=9),
                                dict(radius=2, full_support=25), dict(radius=3, full_support=49), dict(chunk=0), dict(chunk=(1 << 30) + 1),
                                dict(chunk=1.5), dict(pixel_mask=np.zeros((7, 5), np.uint8)), dict(pixel_mask=np.zeros((5, 7)))],
                         ids=lambda kw: '-'.join(f'{k}={v if np.ndim(v) == 0 else np.shape(v)}' for k, v in kw.items()))
def test_bad_arguments_are_value_errors_before_any_library_call(kw):
    kw = dict(dict(tau=1.0), **kw)
    with pytest.raises(ValueError):
        stub_engine().event_support(*_ok(), **kw)
    with pytest.raises(ValueError):
        staging.event_support_weights(dict(zip('xyt', _ok())), (5, 7), engine=stub_engine(), **kw)


def test_bad_arrays_are_value_errors_before_any_library_call():
    x, y, t = _ok()
    for args in ((x[:-1], y, t), (x, y, t[:-1]), (x, y, t[:, None]), (x.astype(np.float64), y, t), (x, y, t.astype(str)),
                 (x, y, t.astype(bool)), (x, y, _set(t.astype(np.int64), 5, (1 << 53) + 2)), (x, y, _set(-t.astype(np.int64), 5, -(1 << 53) - 2)),
                 (x, y, _set(t.astype(np.uint64), 5, (1 << 63)))):
        with pytest.raises(ValueError):
            stub_engine().event_support(*args, 1.0)
    with pytest.raises(ValueError, match='lack'):
        staging.event_support_weights(dict(x=x, y=y), (5, 7), 1.0, engine=stub_engine())
    with pytest.raises(ValueError, match='sensor_size'):
        staging.event_support_weights(dict(x=x, y=y, t=t), (7, 5), 1.0, engine=stub_engine())


def test_integer_times_convert_exactly_or_not_at_all():
    t = np.array([-(1 << 53), 0, (1 << 53)], dtype=np.int64)
    got = E.check_event_times(t, 3)
    assert got.dtype == np.float64 and [int(v) for v in got] == [int(v) for v in t]
    assert E.check_event_times(np.array([1, 2], dtype=np.uint16), 2).dtype == np.float64
    assert E.check_event_times(np.array([1, 2], dtype=np.float32), 2).dtype == np.float64


def test_signatures_of_the_python_layer():
    p = inspect.signature(E.Engine.event_support).parameters
    assert list(p) == ['self', 'xs', 'ys', 'ts', 'tau', 'radius', 'full_support', 'pixel_mask', 'chunk', 'return_support']
    assert (p['radius'].default, p['full_support'].default, p['pixel_mask'].default, p['chunk'].default, p['return_support'].default) == (
        1, 1, None, 1 << 22, False)
    p = inspect.signature(staging.event_support_weights).parameters
    assert list(p)[:3] == ['events', 'sensor_size', 'tau'] and p['engine'].default is None
    assert list(inspect.signature(staging.hot_pixel_mask).parameters) == ['xs', 'ys', 'sensor_size', 'max_count']
    assert 'event_support' not in inspect.getsource(staging.stage_datasample)        # stage_datasample is not changed


# ---- hot_pixel_mask ------------------------------------------------------------------------------------------------------------
def test_hot_pixel_mask_against_a_hand_count():
    #                  (x, y): (1, 0) x 4, (6, 4) x 3, (0, 0) x 1, (2, 3) x 2
    xs = np.array([1, 6, 1, 0, 2, 6, 1, 2, 6, 1])
    ys = np.array([0, 4, 0, 0, 3, 4, 0, 3, 4, 0])
    m = staging.hot_pixel_mask(xs, ys, (5, 7), 2)
    assert m.dtype == np.uint8 and m.shape == (5, 7)
    exp = np.zeros((5, 7), np.uint8)
    exp[0, 1] = exp[4, 6] = 1
    assert np.array_equal(m, exp)
    assert staging.hot_pixel_mask(xs, ys, (5, 7), 3).sum() == 1 and staging.hot_pixel_mask(xs, ys, (5, 7), 4).sum() == 0
    assert staging.hot_pixel_mask(xs, ys, (5, 7), 0).sum() == 4
    assert staging.hot_pixel_mask(xs[:0], ys[:0], (5, 7), 0).sum() == 0
    with pytest.raises(ValueError):
        staging.hot_pixel_mask([7], [0], (5, 7), 1)
    assert E.check_pixel_mask(m * 200, (5, 7)).max() == 1                  # any non-zero value masks


# ---- witness properties ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize('name', ['3x3-r3-k8', '5x7-r2-k3-ties', '5x7-r1-k4-mask', '5x7-r1-k1-tau0'])
def test_witness_split_at_any_index_gives_the_unsplit_result(name):
    xs, ys, ts, mask, s = ES.generated(name)
    n = 160
    xs, ys, ts = xs[-n:], ys[-n:], ts[-n:]
    kw = dict(tau=s['tau'], radius=s['radius'], full_support=s['full_support'], pixel_mask=mask)
    whole = ES.support_filter(xs, ys, ts, s['shape'], **kw)
    for cut in range(n + 1):
        a = ES.support_filter(xs[:cut], ys[:cut], ts[:cut], s['shape'], **kw)
        b = ES.support_filter(xs[cut:], ys[cut:], ts[cut:], s['shape'], last=a[2], **kw)
        assert _same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), b[2]), whole), cut


def test_witness_isolated_pixel_gets_weight_zero_however_often_it_fires():
    n = 500
    for r in (1, 2, 3):
        w, sup, _ = ES.support_filter(np.full(n, 3), np.full(n, 2), np.arange(n) * 1e-3, (5, 7), 10.0, r, 1)
        assert not w.any() and not sup.any()


def test_witness_masked_pixel_neither_receives_nor_gives_support():
    # pixel a = (2, 2) and its neighbour b = (3, 2) alternate: each lives on the other's support
    xs, ys, ts = np.array([2, 3] * 20), np.full(40, 2), np.arange(40) * 0.1
    w, _, _ = ES.support_filter(xs, ys, ts, (5, 7), 1.0)
    assert w[0] == 0 and np.all(w[1:] == 1)
    mask = np.zeros((5, 7), np.uint8)
    mask[2, 3] = 1
    w, sup, last = ES.support_filter(xs, ys, ts, (5, 7), 1.0, pixel_mask=mask)
    assert not w.any() and not sup.any()
    assert last[2, 3] == ts[-1]                                              # its events still happened


def test_witness_tau_zero_supports_equal_timestamps_only():
    xs, ys = np.array([1, 2, 1, 2, 3]), np.full(5, 1)
    ts = np.array([1.0, 1.0, 1.0 + 2.0 ** -52, 2.0, 2.0])
    _, sup, _ = ES.support_filter(xs, ys, ts, (3, 5), 0.0)
    assert list(sup) == [0, 1, 0, 0, 1]                                      # the earlier index supports the later, never the reverse


def test_witness_is_invariant_under_an_exact_translation_of_the_times():
    xs, ys, ts, mask, s = ES.generated('33x65-r2-k12')
    ts = np.round(ts * 1024.0) / 1024.0                                      # multiples of 2^-10 below 2^20: adding 2^30 is exact
    assert ts.max() < 2.0 ** 20
    shifted = ts + 2.0 ** 30
    assert np.array_equal(shifted - 2.0 ** 30, ts)
    tau = 0.5
    a = ES.support_filter(xs, ys, ts, s['shape'], tau, s['radius'], s['full_support'])
    b = ES.support_filter(xs, ys, shifted, s['shape'], tau, s['radius'], s['full_support'])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert 0.0 < a[0].mean() < 1.0


# ---- the condition that keeps the GPU tests honest ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ES.GENERATED))
def test_every_generated_case_has_zeros_ones_and_values_between(name):
    xs, ys, ts, mask, s = ES.generated(name)
    assert len(xs) == s['n'] and np.all(np.diff(ts) >= 0) and np.isfinite(ts).all()
    w, sup, _ = ES.support_filter(xs, ys, ts, s['shape'], s['tau'], s['radius'], s['full_support'], mask)
    zero, one, between = ES.weight_fractions(w, s['full_support'])
    assert zero >= 0.20 and one >= 0.20, (zero, one, between)
    if s['full_support'] > 1:
        assert between >= 0.10, (zero, one, between)


def test_generated_cases_cover_the_shapes_and_parameters():
    specs = list(ES.GENERATED.values())
    assert {s['shape'] for s in specs} == {(3, 3), (5, 7), (33, 65), (260, 346)}
    assert {s['radius'] for s in specs} == {1, 2, 3}
    for r in (1, 2, 3):
        ks = {s['full_support'] for s in specs if s['radius'] == r}
        assert 1 in ks or r > 1
        assert ES.max_support(r) in ks and any(1 < k < ES.max_support(r) for k in ks), (r, ks)
    assert any(s['mask'] is not None for s in specs) and any(s['tau'] == 0.0 for s in specs) and any(s['tie_run'] > 64 for s in specs)
    # the corners and the edge middles carry events in every case of at least 256 events
    for name, s in ES.GENERATED.items():
        if s['n'] < 256:
            continue
        xs, ys, _, _, _ = ES.generated(name)
        H, W = s['shape']
        have = set(zip(ys.tolist(), xs.tolist()))
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= have, name


def test_two_pixel_and_tie_streams_are_not_constant_either():
    xs, ys, ts = ES.two_pixel_stream(4000)
    w, _, _ = ES.support_filter(xs, ys, ts, (3, 3), 1.0)
    zero, one, _ = ES.weight_fractions(w, 1)
    assert zero >= 0.20 and one >= 0.20
    assert set(zip(ys.tolist(), xs.tolist())) == {(1, 0), (1, 1)}
    xs, ys, ts = ES.tie_stream((5, 7), 100, 200)
    w, sup, _ = ES.support_filter(xs, ys, ts, (5, 7), 0.0)
    zero, one, _ = ES.weight_fractions(w, 1)
    assert zero >= 0.20 and one >= 0.20 and sup.max() == 8
