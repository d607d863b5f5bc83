"""Who holds a context's memory, read through Engine.memory(): nothing is allocated in steady state, a buffer
grows once and keeps its operator's results, the one-shot operators share one scratch block, no state rides in it (the rectify map and
the NL-means table have buffers of their own), and a refused call allocates nothing."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _dsec_witness as DW
import _gt_flow_witness as GW
import _preprocess_witness as PW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
ev = importlib.import_module(pkg + '.evaluation')
synth = importlib.import_module(pkg + '.synth')

SENSOR = (40, 56)
H, W = SENSOR
B, R, N_EVENTS = 2, 2, 3000
N_MAX = 3                                   # the largest stack any test hands to an operator
_engines = {}


@functools.lru_cache(maxsize=None)
def _windows():
    wins = [synth.make_window(700 + b, SENSOR, N_EVENTS, R, flow='smooth', flow_mag=2.0) for b in range(B)]
    return [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]


def _params(**kw):
    a = dict(alpha=20.0, beta=35.0, gamma=0.0, delta=0.0, cur_pyr_lvl=0)
    a.update(kw)
    return E.make_params(**a)


def _staged(precision='fp32'):
    """A context with the two windows staged and one evaluation behind it (identity theta: no buffer grows for it)."""
    eng = E.Engine(SENSOR, B * N_EVENTS, max_refs=R, max_windows=B, precision=precision)
    eng.set_windows(_windows())
    eng.loss_grad(_theta((H, W)), _params())
    return eng


def _eng(precision='fp32'):
    if precision not in _engines:
        _engines[precision] = _staged(precision)
    return _engines[precision]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


def _theta(hw, seed=3):
    return np.random.default_rng(seed).normal(0.0, 1.5, (B,) + tuple(hw) + (2,))


# -- the one-shot operators: inputs made once, each operator a function of (engine, n) ------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(21)
    d = {'u8': rng.integers(0, 256, (N_MAX, H, W)).astype(np.uint8), 'f64': rng.normal(0.0, 1.0, (N_MAX, H, W)),
         'edge': (rng.random((N_MAX, H, W)) < 0.1).astype(np.uint8)}
    gt_ts, gx, gy = GW.random_sequence(4, H, W, n_gt=40)
    a, b = GW.random_windows(4, gt_ts, N_MAX, 4)
    d['gt'] = (gx.astype(np.float32), gy.astype(np.float32), gt_ts, a, b)
    d['xy'] = (rng.integers(0, W, N_MAX * 1000).astype(np.int16), rng.integers(0, H, N_MAX * 1000).astype(np.int16))
    d['map'] = DW.distortion_map(H, W)
    d['map2'] = DW.distortion_map(H, W, k=-0.1, shift=(-0.5, 1.0))
    d['src'] = rng.integers(0, 256, (N_MAX, 61, 83)).astype(np.uint8)
    ident = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).astype(np.float32)
    d['remap'] = np.ascontiguousarray(ident * np.float32(1.3) + np.float32(2.25))
    f16 = rng.integers(0, 65536, (N_MAX, H, W, 3)).astype(np.uint16)
    f16[..., 2] = rng.random((N_MAX, H, W)) < 0.6
    d['f16'] = f16
    d['theta'] = rng.normal(0.0, 3.0, (N_MAX, 4, 6, 2))
    d['valid'] = rng.random((N_MAX, H, W)) < 0.5
    return d


def _gt_flow(e, n):
    gx, gy, gt_ts, a, b = _inputs()['gt']
    return ev.estimate_gt_flow(gx, gy, gt_ts, a[:n], b[:n], engine=e)


OPS = {
    'inv_dist_transform': lambda e, n: e.inv_dist_transform(_inputs()['edge'][:n]),
    'gaussian_blur': lambda e, n: e.gaussian_blur(_inputs()['f64'][:n], 1.5),
    'canny': lambda e, n: e.canny(_inputs()['u8'][:n], 50.0, 120.0),
    'preprocess_image': lambda e, n: e.preprocess_image(_inputs()['u8'][:n]),
    'gt_flow': _gt_flow,
    'rectify_events': lambda e, n: e.rectify_events(_inputs()['xy'][0][:n * 1000], _inputs()['xy'][1][:n * 1000], _inputs()['map'])[:3],
    'remap_cubic': lambda e, n: e.remap_cubic(_inputs()['src'][:n], _inputs()['remap']),
    'flow_decode': lambda e, n: e.flow_decode(_inputs()['f16'][:n]),
    'flow_encode': lambda e, n: e.flow_encode(_inputs()['theta'][:n], _inputs()['valid'][:n]),
    'get_warped_events': lambda e, n: e.warped_events(1),               # (no n: the staged window's events)
    'tiled_objectives': lambda e, n: tuple(v for d in e.tiled_objectives((8, 8)) for _, v in sorted(d.items())),
}


def _same(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() and np.shape(p) == np.shape(q) for p, q in zip(a, b))


# -- 1. nothing is allocated in steady state ------------------------------------------------------------------------------------
def _bfgs(e):
    e.bfgs_begin(_theta((4, 4)))
    zero, step = np.zeros(B), np.full(B, 1e-3)
    e.bfgs_eval(_params(), zero)
    e.bfgs_accept(zero, [L.BFGS_INIT] * B)
    e.bfgs_eval(_params(), step)
    e.bfgs_accept(step, [L.BFGS_UPDATE] * B)


EVALS = {
    'identity': ('fp32', lambda e: e.loss_grad(_theta((H, W)), _params())),
    '1x1': ('fp32', lambda e: e.loss_grad(_theta((1, 1)), _params())),
    '4x4': ('fp32', lambda e: e.loss_grad(_theta((4, 4)), _params())),
    '4x4_delta': ('fp32', lambda e: e.loss_grad(_theta((4, 4)), _params(delta=0.3))),
    '4x4_gamma': ('fp32', lambda e: e.loss_grad(_theta((4, 4)), _params(gamma=2.5e-4))),
    '4x4_adaptive_variance': ('fp32', lambda e: e.loss_grad(_theta((4, 4)), _params(contrast_kind='adaptive_variance'))),
    '4x4_fp64': ('fp64', lambda e: e.loss_grad(_theta((4, 4)), _params())),
    'bfgs_4x4': ('fp32', _bfgs),
}


@pytest.mark.parametrize('name', list(EVALS))
def test_steady_state_evaluations(name):
    precision, run = EVALS[name]
    eng = _eng(precision)
    run(eng)
    m1 = eng.memory()
    run(eng)
    m2 = eng.memory()
    print(name, m1, m2)
    assert m1 == m2
    assert m1.device_bytes > 0 and m1.pinned_bytes > 0 and m1.allocations > 50


@pytest.mark.parametrize('name', list(OPS))
def test_steady_state_operators(name):
    eng = _eng()
    OPS[name](eng, 2)
    m1 = eng.memory()
    OPS[name](eng, 2)
    m2 = eng.memory()
    print(name, m1, m2)
    assert m1 == m2 and m1.scratch_bytes > 0


# -- 2. growth happens once and keeps results -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['canny', 'preprocess_image', 'flow_decode'])
def test_growth_once(name):
    with _staged() as eng:
        first = OPS[name](eng, 1)
        m1 = eng.memory()
        OPS[name](eng, 3)
        m2 = eng.memory()
        third = OPS[name](eng, 1)
        m3 = eng.memory()
    print(name, m1, m2, m3)
    assert m2.scratch_bytes > m1.scratch_bytes and m2.device_bytes - m1.device_bytes == m2.scratch_bytes - m1.scratch_bytes
    assert m2.allocations == m1.allocations                    # the old block was freed
    assert m3 == m2
    assert _same(first, third)


# -- 3. the scratch is shared, not summed ---------------------------------------------------------------------------------------
def _nlm_table_bytes():
    """The NL-means weight table of the default parameters: one int32 per entry of the witness's table."""
    d = E.PREPROCESS_DEFAULTS
    return 4 * len(PW.nlm_table(d['denoise_h'], d['denoise_template_win'], d['denoise_search_win'])[0])


def test_scratch_is_the_maximum_and_only_two_buffers_persist():
    with E.Engine(SENSOR, B * N_EVENTS, max_refs=R, max_windows=B) as eng:
        fresh = eng.memory()
    with _staged() as eng:
        staged = eng.memory()
    # staging's theta = 0 pass is a (1, 1, 2) evaluation: it sizes the two resample matrices, (H, 1) and (W, 1) doubles, and nothing
    # else; the identity evaluation adds nothing.  That is all a context holds beyond a fresh one before its first operator.
    assert fresh.scratch_bytes == 0 and staged.scratch_bytes == 0
    assert staged == fresh._replace(device_bytes=fresh.device_bytes + (H + W) * 8, allocations=fresh.allocations + 2)
    alone = {}
    for name, op in OPS.items():
        with _staged() as eng:
            op(eng, 2)
            alone[name] = eng.memory().scratch_bytes
    with _staged() as eng:
        for op in OPS.values():
            op(eng, 2)
        m = eng.memory()
    print(alone, fresh, staged, m)
    assert all(v > 0 for v in alone.values()) and len(set(alone.values())) > 3
    assert m.scratch_bytes == max(alone.values())
    persistent = H * W * 4 + _nlm_table_bytes()      # the rectify map, the NL-means table
    assert m.device_bytes - m.scratch_bytes == staged.device_bytes + persistent
    assert m.pinned_bytes == staged.pinned_bytes
    assert m.allocations == staged.allocations + 3             # the scratch block and the two


# -- 4. no state rides in the scratch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('small,large', [('gaussian_blur', 'preprocess_image'), ('canny', 'gt_flow'), ('flow_encode', 'flow_decode'),
                                         ('tiled_objectives', 'remap_cubic'), ('inv_dist_transform', 'get_warped_events')])
def test_an_operator_between_two_calls_of_another(small, large):
    with _staged() as eng:
        a1 = OPS[small](eng, 1)
        s1 = eng.memory().scratch_bytes
        b1 = OPS[large](eng, 3)
        s2 = eng.memory().scratch_bytes
        a2 = OPS[small](eng, 1)
        b2 = OPS[large](eng, 3)
    print(small, s1, large, s2)
    assert s2 > s1                                             # the second one's footprint is the larger: the block was replaced
    assert _same(a1, a2) and _same(b1, b2)


def _rectify_raw(eng, rectify_map, x, y):
    """One chunk through the C-ABI, with or without a map"""
    n = len(x)
    rx, ry, keep, k = np.empty(n, np.int16), np.empty(n, np.int16), np.empty(n, np.uint8), C.c_int64(0)
    rc = L.load().eincm_rectify_events(eng._ctx, None if rectify_map is None else rectify_map.ctypes.data, x.ctypes.data, y.ctypes.data, n,
                                       rx.ctypes.data, ry.ctypes.data, keep.ctypes.data, C.byref(k))
    assert rc == L.OK, rc
    return rx[:k.value], ry[:k.value], keep


def test_rectify_map_survives_other_operators():
    d = _inputs()
    x, y = d['xy']
    with _staged() as eng:
        first = _rectify_raw(eng, d['map'], x, y)
        eng.remap_cubic(d['src'], np.ascontiguousarray(d['map2'] * np.float32(1.4)))      # another float map through the scratch, a larger footprint
        OPS['flow_decode'](eng, 3)
        last = _rectify_raw(eng, None, x, y)
    want = DW.rectify_events(x, y, d['map'])
    assert _same(first, last)
    assert np.array_equal(last[0], want[0]) and np.array_equal(last[1], want[1]) and np.array_equal(last[2].view(np.bool_), want[2])
    assert not np.array_equal(want[2], DW.rectify_events(x, y, d['map2'])[2])            # (the two maps differ on these events)


def test_nlmeans_table_survives_other_operators():
    yy, xx = np.mgrid[0:H, 0:W]             # a smooth image with a little noise: patches resemble each other, the filter changes it
    u8 = np.clip(np.rint(120 + 40 * np.sin(xx / 7.0) + np.random.default_rng(5).normal(0, 2, (2, H, W))), 0, 255).astype(np.uint8)
    with _staged() as eng:
        first = eng.preprocess_image(u8[:2], stages=('nlmeans',))
        m1 = eng.memory()
        OPS['gaussian_blur'](eng, 3)
        second = eng.preprocess_image(u8[:2], stages=('nlmeans',))       # the cached table: not built or uploaded again
        m2 = eng.memory()
    assert _same(first, second) and not np.array_equal(first, u8[:2])
    assert m2.device_bytes - m2.scratch_bytes == m1.device_bytes - m1.scratch_bytes and m2.scratch_bytes > m1.scratch_bytes


# -- 5. a refused call allocates nothing ----------------------------------------------------------------------------------------
def test_refused_calls_allocate_nothing():
    lib = L.load()
    u8p = C.POINTER(C.c_uint8)
    with E.Engine(SENSOR, 1, max_refs=1) as eng:
        before = eng.memory()
        img = np.zeros((1, H, W), np.uint8)
        out = np.zeros((1, H, W), np.uint8)
        d = np.zeros((1, H, W))
        k = C.c_int64(0)
        pp = E.make_preprocess_params(SENSOR)
        refused = [
            lib.eincm_canny(eng._ctx, img.ctypes.data_as(u8p), 0, 50.0, 100.0, 3, 1, out.ctypes.data_as(u8p)),
            lib.eincm_canny(eng._ctx, img.ctypes.data_as(u8p), 1, 50.0, 100.0, 5, 1, out.ctypes.data_as(u8p)),
            lib.eincm_gaussian_blur(eng._ctx, E._dp(d), 0, 1.5, E._dp(d)),
            lib.eincm_gaussian_blur(eng._ctx, E._dp(d), 1, -1.0, E._dp(d)),
            lib.eincm_inv_dist_transform(eng._ctx, img.ctypes.data_as(u8p), 0, 0, 6.0, 6.0, E._dp(d), None),
            lib.eincm_preprocess_image(eng._ctx, img.ctypes.data_as(u8p), 0, C.byref(pp), out.ctypes.data_as(u8p)),
            lib.eincm_flow_decode(eng._ctx, img.ctypes.data, 0, d.ctypes.data, out.ctypes.data, C.byref(k)),
            lib.eincm_flow_encode(eng._ctx, d.ctypes.data, 0, 1, 1, None, out.ctypes.data, C.byref(k)),
            lib.eincm_remap_cubic(eng._ctx, img.ctypes.data, 0, H, W, d.ctypes.data, E.remap_cubic_table().ctypes.data, out.ctypes.data),
            lib.eincm_rectify_events(eng._ctx, None, img.ctypes.data, img.ctypes.data, 4, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                     C.byref(k)),                     # no map yet
        ]
        after = eng.memory()
    assert refused == [L.ERR_ARG, L.ERR_UNSUPPORTED] + [L.ERR_ARG] * 7 + [L.ERR_STATE]
    assert after == before and before.scratch_bytes == 0


# -- 6. a call refused after work has run on the GPU leaves the context as an accepted call of the same sizes does ---------------------
def _changed(a, index, value):
    a = a.copy()
    a[index] = value
    return a


def _rectify(e, x, y, m):
    return e.rectify_events(x, y, m)[:3]


def _fe_stage(e, x_outside=None):
    d = _inputs()
    x, y = d['xy'] if x_outside is None else (_changed(d['xy'][0], x_outside, W), d['xy'][1])
    gt = np.random.default_rng(33).normal(0.0, 2.0, (N_MAX, H, W, 2))
    e.flow_eval_stage(gt, [(x[b * 1000:(b + 1) * 1000], y[b * 1000:(b + 1) * 1000]) for b in range(N_MAX)], d['valid'])


def _fe_read(e):
    res, emap = e.flow_errors(_inputs()['theta'], ee_map=True)
    return tuple(np.array(list(r['errors'].values()) + list(r['counts'].values())) for r in res) + (emap,)


# name: (the refused call, a piece of its message, the accepted call of the same sizes, how that one's results are read if it returns none)
LATE_REFUSALS = {
    'inv_dist_transform_empty_image': (lambda e: e.inv_dist_transform(_changed(_inputs()['edge'][:2], 1, 0)), 'has no edge pixel',
                                       lambda e: e.inv_dist_transform(_inputs()['edge'][:2]), None),
    'rectify_events_nan_in_map': (lambda e: _rectify(e, *_inputs()['xy'], _changed(_inputs()['map'], (7, 9, 1), np.nan)), 'rectify map',
                                  lambda e: _rectify(e, *_inputs()['xy'], _inputs()['map']), None),
    'rectify_events_x_equals_W': (lambda e: _rectify(e, _changed(_inputs()['xy'][0], 1234, W), _inputs()['xy'][1], _inputs()['map']),
                                  'events have a coordinate outside', lambda e: _rectify(e, *_inputs()['xy'], _inputs()['map']), None),
    'flow_decode_third_channel_2': (lambda e: e.flow_decode(_changed(_inputs()['f16'], (1, 5, 6, 2), 2)), 'third channel',
                                    lambda e: e.flow_decode(_inputs()['f16']), None),
    'flow_encode_nonfinite_theta': (lambda e: e.flow_encode(_changed(_inputs()['theta'], (1, 2, 3, 0), np.inf), _inputs()['valid']),
                                    'not finite', lambda e: e.flow_encode(_inputs()['theta'], _inputs()['valid']), None),
    'flow_eval_stage_event_outside': (lambda e: _fe_stage(e, x_outside=1017), 'evaluation events have a coordinate outside',
                                      _fe_stage, _fe_read),
}


@pytest.mark.parametrize('name', list(LATE_REFUSALS))
def test_a_late_refusal_leaves_the_context_as_an_accepted_call_does(name):
    refuse, message, accept, read = LATE_REFUSALS[name]
    with E.Engine(SENSOR, 1, max_refs=1) as twin:              # never sees the refusal
        want = accept(twin)
        m_want = twin.memory()
        want = read(twin) if read else want
    with E.Engine(SENSOR, 1, max_refs=1) as eng:
        with pytest.raises((ValueError, E.EincmError), match=message):
            refuse(eng)
        m_got = eng.memory()
        if read is _fe_read:                                   # nothing is staged now: the library says so, and so does the wrapper
            th = _inputs()['theta']
            out = (L.FlowErrorOut * N_MAX)()
            assert L.load().eincm_flow_errors(eng._ctx, th.ctypes.data, th.shape[1], th.shape[2], L.METHODS['bilinear'], out,
                                              None) == L.ERR_STATE
            with pytest.raises(E.EincmError):
                eng.flow_errors(th)
            assert eng.memory() == m_got
        got = accept(eng)
        m_after = eng.memory()
        got = read(eng) if read else got
    print(name, m_want, m_got, m_after)
    assert m_got._asdict() == m_want._asdict()                 # field by field
    assert m_after == m_want
    assert _same(got, want)
