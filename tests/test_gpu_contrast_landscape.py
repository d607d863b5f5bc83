"""The contrast landscape and the seeding driver on the GPU.

The criterion is equality: ``sumsq`` and ``n_in`` equal the numpy witness (tests/_contrast_landscape_witness.py) integer for integer.
No tolerance exists or is needed: every result is a count or a sum of squared counts.  Beside the generated cases stand constructed
events whose answer is also written out by hand (half-integers in both parities, the four sides, the first and last row of every
band, candidates that drop everything), the cross-check against the engine's own count images, every refusal on pattern-filled
outputs, and the driver against the driver run on the witness.  Every test runs under its own time limit."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import _contrast_landscape_witness as CW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
synth = importlib.import_module(pkg + '.synth')
motion = importlib.import_module(pkg + '.motion')
segmentation = importlib.import_module(pkg + '.segmentation')
contrast_landscape = E.Engine.contrast_landscape              # a tree without the operator has nothing that this module could test

TIME_LIMIT_S = 30
R = 2
EDGE_TS = np.array([0.0, 1.0])
P = E.make_params(1.0, 0.0, 0.0, 0.0, 1)
CELLS = (1, 2, 4, 8)
S_SENT, N_SENT = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0x5A5A5A5A)
_engines = {}


def _eng(shape, precision='fp32'):
    key = (tuple(shape), precision)
    if key not in _engines:
        _engines[key] = E.Engine(tuple(shape), max_events_total=16384, max_refs=R, max_windows=4, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f'test exceeded {TIME_LIMIT_S} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TIME_LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def bands(H, W, cell):
    """(rows per band, row bands) of cl_bands (csrc/eincm_contrast_landscape.h), restated for the sensors of this module, all of
    which keep the table and hold a whole cell row; tests/test_host_contrast_landscape.py checks the header's own."""
    Hc, Wc = -(-H // cell), -(-W // cell)
    words = (65536 - 2 * 16 * 8 - (W + H) * 8) // 4
    assert W + H <= 2048 and Wc <= words
    rows = min(Hc, words // Wc)
    return rows, -(-Hc // rows)


def random_events(rng, shape, n, margin=0):
    H, W = shape
    return (rng.integers(margin, W - margin, n).astype(np.int16), rng.integers(margin, H - margin, n).astype(np.int16),
            np.sort(rng.uniform(0.0, 1.0, n)))


def window_of(ev, shape, seed=0):
    return ev + (np.random.default_rng(seed).random((R,) + tuple(shape)), EDGE_TS)


def random_coeffs(rng, model, B, V):
    """Candidates whose fields stay within about +-9 px over the sensor"""
    K, s = model.n_coeffs, model.scale
    if model.kind == 'translation':
        return rng.uniform(-9, 9, (B, V, K))
    if model.kind == 'affine':
        return np.concatenate([rng.uniform(-5, 5, (B, V, 2)), rng.uniform(-2, 2, (B, V, 4))], axis=2)      # zoom and shear, none zero
    if model.kind == 'rotation':
        return rng.uniform(-3 / s, 3 / s, (B, V, K))
    return rng.uniform(-1.5, 1.5, (B, V, K))                                                               # polynomial2


def keep_of(rng, mode, ns):
    if mode is None:
        return None
    if mode == 'random':
        return [rng.random(n) < 0.6 for n in ns]
    if mode == 'zero':
        return [np.zeros(n, dtype=bool) for n in ns]
    return [None if b % 2 == 0 else (rng.integers(0, 3, n).astype(np.uint8)) for b, n in enumerate(ns)]   # 'mixed': NULL beside a mask, bytes > 1


def evaluate(eng, model, events, coeffs, t_ref, keep, cells=CELLS):
    """Stage, run every cell size, compare with the witness; returns {cell: (sumsq, n_in)} of the GPU"""
    shape = model.sensor_size
    eng.set_windows([window_of(ev, shape) for ev in events])
    eng.set_motion_model(model)
    want = CW.landscapes(model, events, coeffs, t_ref, cells, keep)
    got = {}
    for cell in cells:
        r = eng.contrast_landscape(coeffs, t_ref=t_ref, cell=cell, keep=keep)
        assert r['sumsq'].dtype == np.uint64 and r['n_in'].dtype == np.uint32 and r['sumsq'].shape == r['n_in'].shape == coeffs.shape[:2]
        assert np.array_equal(r['sumsq'], want[cell][0]), (cell, r['sumsq'], want[cell][0])
        assert np.array_equal(r['n_in'], want[cell][1]), (cell, r['n_in'], want[cell][1])
        got[cell] = (r['sumsq'], r['n_in'])
    return got


#          name                       sensor      model          events per window   V   keep
CASES = [('33x65-translation-b1',    (33, 65),   'translation', (700,),             65, None),
         ('33x65-affine-b3',         (33, 65),   'affine',      (257, 0, 63),       2,  'random'),
         ('33x65-rotation-small-n',  (33, 65),   'rotation',    (1, 0, 64),         2,  'mixed'),
         ('33x65-empty',             (33, 65),   'translation', (0,),               2,  None),
         ('60x80-polynomial2-b3',    (60, 80),   'polynomial2', (255, 0, 256),      65, 'mixed'),
         ('60x80-affine-v1',         (60, 80),   'affine',      (65,),              1,  'zero'),
         ('60x80-rotation-b1',       (60, 80),   'rotation',    (700,),             2,  'random'),
         ('130x173-translation-b3',  (130, 173), 'translation', (700, 0, 257),      65, 'random'),
         ('130x173-polynomial2-b1',  (130, 173), 'polynomial2', (256,),             2,  None),
         ('130x173-affine-b3',       (130, 173), 'affine',      (64, 0, 65),        2,  'mixed'),
         ('260x346-translation-b1',  (260, 346), 'translation', (2000,),            65, None),
         ('260x346-rotation-b3',     (260, 346), 'rotation',    (2000, 0, 63),      2,  'random')]


def test_the_cases_cover_what_they_are_meant_to():
    assert {c[1] for c in CASES} == {(33, 65), (60, 80), (130, 173), (260, 346)} and {c[2] for c in CASES} == {'translation', 'affine', 'rotation', 'polynomial2'}
    assert {n for c in CASES for n in c[3]} >= {0, 1, 63, 64, 65, 255, 256, 257, 700, 2000} and {c[4] for c in CASES} == {1, 2, 65}
    assert {len(c[3]) for c in CASES} == {1, 3} and all(c[3][1] == 0 for c in CASES if len(c[3]) == 3) and {c[5] for c in CASES} == {None, 'random', 'zero', 'mixed'}
    assert all(bands(33, 65, c)[1] == 1 and bands(60, 80, c)[1] == 1 for c in CELLS)
    assert bands(130, 173, 1)[1] >= 2 and bands(260, 346, 1)[1] >= 6 and bands(260, 346, 2)[1] >= 2 and bands(260, 346, 8)[1] == 1


@pytest.mark.parametrize('name,shape,kind,ns,V,keep', CASES, ids=[c[0] for c in CASES])
def test_generated_case_equals_the_witness(name, shape, kind, ns, V, keep):
    rng = np.random.default_rng(sum(map(ord, name)))
    model = motion.MotionModel(kind, shape)
    events = [random_events(rng, shape, n) for n in ns]
    coeffs = random_coeffs(rng, model, len(ns), V)
    t_ref = rng.uniform(0.0, 1.0, len(ns))
    got = evaluate(_eng(shape), model, events, coeffs, t_ref, keep_of(rng, keep, ns))
    total = sum(int(g[1].sum()) for g in got.values())
    assert (total > 0) == (keep != 'zero' and sum(ns) > 0)                              # the comparison was not one of zeros
    for b, n in enumerate(ns):
        if n == 0 or keep == 'zero':
            assert all(not g[0][b].any() and not g[1][b].any() for g in got.values())   # a window without (kept) events: zeros


def test_half_integers_round_to_even_in_both_parities():
    """Theta = 1 and dt = +-1/2: w = x -+ 1/2 is a half-integer for every event; rint takes it to the even neighbour"""
    shape = (33, 65)
    model = motion.MotionModel('translation', shape)
    xs = np.array([2, 3, 3, 4, 10, 11], dtype=np.int16)
    ys = np.array([5, 5, 5, 5, 20, 21], dtype=np.int16)
    ts = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    # candidate (1, 0), t_ref 1/2: x 2 -> 2.5 -> 2, 3 -> 3.5 -> 4, 3 -> 2.5 -> 2, 4 -> 3.5 -> 4, 10 -> 9.5 -> 10, 11 -> 10.5 -> 10
    # candidate (0, 1): y 5 -> 5.5 -> 6, 5 -> 6, 5 -> 4.5 -> 4, 5 -> 4, 20 -> 19.5 -> 20, 21 -> 20.5 -> 20; (1, 1): the last two meet in (20, 10)
    coeffs = np.array([[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]])
    got = evaluate(_eng(shape), model, [(xs, ys, ts)], coeffs, np.array([0.5]), None)
    assert got[1][0].tolist() == [[2 * 2 + 2 * 2 + 1 + 1, 6, 2 * 2 + 4]] and got[1][1].tolist() == [[6, 6, 6]]
    rng = np.random.default_rng(3)
    ev = (rng.integers(1, 64, 700).astype(np.int16), rng.integers(1, 32, 700).astype(np.int16), np.sort(rng.integers(0, 2, 700).astype(np.float64)))
    evaluate(_eng(shape), model, [ev], np.array([[[1.0, 1.0], [-1.0, 1.0], [3.0, -1.0], [1.0, 0.0]]]), np.array([0.5]), None)


@pytest.mark.parametrize('shape', [(33, 65), (130, 173)])
def test_events_leave_over_each_side_by_one_pixel(shape):
    H, W = shape
    model = motion.MotionModel('translation', shape)
    xs = np.array([0, W - 1, 7, 7, 1, W - 2, 7, 7], dtype=np.int16)
    ys = np.array([5, 5, 0, H - 1, 5, 5, 1, H - 2], dtype=np.int16)
    ts = np.array([1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    order = np.argsort(ts, kind='stable')
    coeffs = np.array([[[2.0, 0.0], [0.0, 2.0], [-2.0, 0.0], [0.0, -2.0], [2.0, 2.0]]])       # a shift of one pixel at dt = +-1/2
    got = evaluate(_eng(shape), model, [(xs[order], ys[order], ts[order])], coeffs, np.array([0.5]), None)
    for cell in CELLS:
        assert got[cell][1].tolist() == [[6, 6, 8, 8, 4]]


@pytest.mark.parametrize('shape', [(130, 173), (260, 346)])
def test_first_and_last_row_of_every_band(shape):
    H, W = shape
    model = motion.MotionModel('translation', shape)
    rng = np.random.default_rng(11)
    rows = set()
    for cell in CELLS:
        per, nb = bands(H, W, cell)
        for k in range(nb):
            first, last = k * per * cell, min((k + 1) * per * cell, H) - 1            # pixel rows
            rows |= {first, last, max(first - 1, 0), min(last + 1, H - 1)}
    ys = np.repeat(np.array(sorted(rows), dtype=np.int16), 8)
    xs = rng.integers(0, W, len(ys)).astype(np.int16)
    ts = rng.integers(0, 2, len(ys)).astype(np.float64)
    order = np.argsort(ts, kind='stable')
    coeffs = np.array([[[0.0, 0.0], [0.0, 2.0], [0.0, -2.0], [0.0, 4.0], [3.0, -6.0]]])       # rows move by 0, 1, 2 and 3 across the cuts
    got = evaluate(_eng(shape), model, [(xs[order], ys[order], ts[order])], coeffs, np.array([0.5]), None)
    assert got[1][1][0, 0] == len(ys)


def test_far_candidates_drop_everything():
    shape = (33, 65)
    rng = np.random.default_rng(5)
    ev = random_events(rng, shape, 700)
    model = motion.MotionModel('translation', shape)
    coeffs = np.array([[[1e5, 0.0], [0.0, -1e5], [1e5, 1e5], [0.0, 0.0]]])
    got = evaluate(_eng(shape), model, [ev], coeffs, np.array([2.0]), None)                    # |dt| >= 1: 1e5 px away
    for cell in CELLS:
        assert got[cell][0][0, :3].tolist() == [0, 0, 0] and got[cell][1].tolist() == [[0, 0, 0, 700]]


def test_inf_times_zero_is_dropped():
    """polynomial2 with a small normalising length: u u >= 1e9 a few pixels off the centre, so 1e300 u u is inf.  An event at
    dt = 0 then has inf * 0 = NaN as its shift and is dropped; on the centre column u = 0, the field is 0 and the event stays."""
    shape = (33, 65)
    model = motion.MotionModel('polynomial2', shape, scale=1e-4)
    assert model.cx == 32.0
    xs = np.array([32, 32, 10, 50, 60, 32], dtype=np.int16)
    ys = np.array([3, 30, 3, 16, 30, 16], dtype=np.int16)
    ts = np.array([0.25, 0.5, 0.5, 0.5, 0.5, 0.75])
    c = np.zeros((1, 2, 12))
    c[0, 0, 3] = 1e300                                                                        # Theta_x = 1e300 u u
    with np.errstate(over='ignore', invalid='ignore'):
        th = model.field(c[0, 0])
    assert np.isinf(th[3, 10, 0]) and th[3, 32, 0] == 0.0
    got = evaluate(_eng(shape), model, [(xs, ys, ts)], c, np.array([0.5]), None)
    assert got[1][1].tolist() == [[3, 6]] and got[1][0].tolist() == [[3, 6]]


def test_affine_with_translation_coefficients_equals_translation():
    shape = (60, 80)
    rng = np.random.default_rng(8)
    events = [random_events(rng, shape, n) for n in (700, 0, 257)]
    ct = rng.uniform(-9, 9, (3, 65, 2))
    ca = np.concatenate([ct, np.zeros((3, 65, 4))], axis=2)
    t_ref = np.array([0.5, 0.5, 0.1])
    eng = _eng(shape)
    a = evaluate(eng, motion.MotionModel('affine', shape), events, ca, t_ref, None)
    t = evaluate(eng, motion.MotionModel('translation', shape), events, ct, t_ref, None)
    assert all(np.array_equal(a[c][0], t[c][0]) and np.array_equal(a[c][1], t[c][1]) for c in CELLS)


def test_repeated_call_gives_equal_bytes_and_allocates_nothing():
    shape = (130, 173)
    rng = np.random.default_rng(9)
    model = motion.MotionModel('polynomial2', shape)
    events = [random_events(rng, shape, n) for n in (700, 0, 700)]
    coeffs, t_ref = random_coeffs(rng, model, 3, 65), np.array([0.5, 0.5, 0.5])
    eng = _eng(shape)
    keep = keep_of(rng, 'random', (700, 0, 700))
    evaluate(eng, model, events, coeffs, t_ref, keep, cells=(1,))
    first = eng.contrast_landscape(coeffs, cell=1, keep=keep)
    mem = eng.memory()
    again = eng.contrast_landscape(coeffs, cell=1, keep=keep)
    assert eng.memory() == mem
    assert first['sumsq'].tobytes() == again['sumsq'].tobytes() and first['n_in'].tobytes() == again['n_in'].tobytes()
    one = eng.contrast_landscape(coeffs, cell=1, keep=keep, want='n_in')
    assert list(one) == ['n_in'] and one['n_in'].tobytes() == first['n_in'].tobytes()
    one = eng.contrast_landscape(coeffs, cell=1, keep=keep, want='sumsq')
    assert list(one) == ['sumsq'] and one['sumsq'].tobytes() == first['sumsq'].tobytes()


@pytest.mark.parametrize('precision,splat', [('fp32', 5), ('fp64', 3)])
def test_allowed_on_fp64_contexts_and_with_any_splat_window(precision, splat):
    shape = (33, 65)
    rng = np.random.default_rng(10)
    model = motion.MotionModel('affine', shape)
    events = [random_events(rng, shape, 257)]
    eng = _eng(shape, precision)
    eng.set_splat_window(splat)
    try:
        evaluate(eng, model, events, random_coeffs(rng, model, 1, 2), np.array([0.3]), None)
    finally:
        eng.set_splat_window(3)


def test_sumsq_is_the_sum_of_the_squared_count_images():
    """Every warped event stays inside (margin 10 px, |Theta| <= 9, |dt| <= 1): at cell 1 and t_ref = edge_ts[r] the operator counts
    what the evaluation's own count image of reference time r counts."""
    shape = (60, 80)
    rng = np.random.default_rng(12)
    model = motion.MotionModel('translation', shape)
    events = [random_events(rng, shape, n, margin=10) for n in (700, 0, 257)]
    coeffs = rng.uniform(-9, 9, (3, 2))
    eng = _eng(shape)
    eng.set_windows([window_of(ev, shape) for ev in events])
    eng.set_motion_model(model)
    eng.loss_grad_motion(coeffs, P, want_grad=False)
    cnt = eng.count_images().astype(np.uint64)
    assert cnt.shape == (3, R) + shape and [int(cnt[b, r].sum()) for b in range(3) for r in range(R)] == [700, 700, 0, 0, 257, 257]
    for r in range(R):
        got = eng.contrast_landscape(coeffs[:, None, :], t_ref=np.full(3, EDGE_TS[r]), cell=1)
        assert got['sumsq'][:, 0].tolist() == [int((cnt[b, r] ** 2).sum()) for b in range(3)] and got['n_in'][:, 0].tolist() == [700, 0, 257]


# ---- refusals: each returns its code and leaves the outputs untouched ----------------------------------------------------------------------
def _raw(eng, V, coeffs, t_ref, cell, outs=('sumsq', 'n_in'), B=1):
    s, n = np.full(B * max(V, 1) + 1, S_SENT, np.uint64), np.full(B * max(V, 1) + 1, N_SENT, np.uint32)
    addr = lambda a: None if a is None else a.ctypes.data
    rc = eng._lib.eincm_contrast_landscape(eng._ctx, V, addr(coeffs), addr(t_ref), cell, None, s.ctypes.data if 'sumsq' in outs else None,
                                           n.ctypes.data if 'n_in' in outs else None)
    return rc, eng._lib.eincm_last_error(eng._ctx).decode(), bool(np.all(s == S_SENT) and np.all(n == N_SENT))


def _refused(eng, code, match, V=2, coeffs='good', t_ref='good', cell=1, **kw):
    c = np.array([[1.0, 2.0], [-3.0, 0.5]]) if isinstance(coeffs, str) else coeffs
    t = np.array([0.5]) if isinstance(t_ref, str) else t_ref
    rc, msg, untouched = _raw(eng, V, c, t, cell, **kw)
    assert rc == code and match in msg and untouched, (rc, msg, untouched)


def test_refusals_leave_the_outputs_untouched():
    shape = (33, 65)
    model = motion.MotionModel('translation', shape)
    win = window_of(random_events(np.random.default_rng(13), shape, 257), shape)
    with E.Engine(shape, 1024, max_refs=R, max_windows=2) as eng:
        eng.set_motion_model(model)
        _refused(eng, L.ERR_STATE, 'before eincm_set_windows')
        eng.set_windows([win])
        eng.set_motion_model(None)
        _refused(eng, L.ERR_STATE, 'no motion model')
        with pytest.raises(ValueError, match='no motion model'):
            eng.contrast_landscape(np.zeros((1, 2)))
        eng.set_motion_model(model)
        eng.loss_grad_async(np.zeros((1, 4, 4, 2)), P, want_grad=False)
        _refused(eng, L.ERR_STATE, 'in flight')
        _refused(eng, L.ERR_STATE, 'in flight', outs=())                                       # the first of the order wins
        eng.loss_grad_wait()
        _refused(eng, L.ERR_ARG, 'sumsq and n_in both', outs=())
        for V in (0, -1, 4097):
            _refused(eng, L.ERR_ARG, 'n_candidates', V=V)
        for cell in (0, 3, 16, -1):
            _refused(eng, L.ERR_ARG, 'cell', cell=cell)
        _refused(eng, L.ERR_ARG, 'coeffs or t_ref', coeffs=None)
        _refused(eng, L.ERR_ARG, 'coeffs or t_ref', t_ref=None)
        _refused(eng, L.ERR_ARG, 'window 0, candidate 1, coefficient 0', coeffs=np.array([[1.0, 2.0], [np.nan, 0.5]]))
        _refused(eng, L.ERR_ARG, 'window 0, candidate 0, coefficient 1', coeffs=np.array([[1.0, -np.inf], [np.nan, 0.5]]))
        _refused(eng, L.ERR_ARG, 't_ref of window 0', t_ref=np.array([np.inf]))
        rc, msg, untouched = _raw(eng, 2, np.array([[1.0, 2.0], [-3.0, 0.5]]), np.array([0.5]), 1)
        assert rc == L.OK and not untouched, msg
        eng.set_windows([win], defer_constants=True)
        _refused(eng, L.ERR_UNSUPPORTED, 'event-sharded')
        with pytest.raises(E.EincmError, match='event-sharded') as e:                          # the Python layer reports the library's refusal
            eng.contrast_landscape(np.zeros((1, 2)))
        assert e.value.code == L.ERR_UNSUPPORTED
        eng.set_windows([win])
        assert _raw(eng, 2, np.array([[1.0, 2.0], [-3.0, 0.5]]), np.array([0.5]), 8)[0] == L.OK


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def test_the_driver_returns_the_witness_drivers_seeds_and_the_segmentation_runs_from_them():
    window, flows, shape = CW.scene(synth, 1)
    model = motion.MotionModel('translation', shape)
    want = segmentation.seed_motions(None, [window], model, 2, 16, landscape=CW.landscape_callable(model, [window]))
    n = len(window[0])
    with E.Engine(shape, 2 * n, max_refs=CW.SCENE_R, max_windows=2) as eng:
        got = segmentation.seed_motions(eng, [window], model, 2, 16)
        for k in ('coeffs0', 'sumsq', 'n_kept', 'n_found'):
            assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
        assert got['n_found'][0] == 2 and max(np.abs(got['coeffs0'][0] - f).max(axis=1).min() for f in flows) <= 1.0
        hist = segmentation.segment_motions(eng, [window], model, got['coeffs0'], P, n_iters=1, maxiter=5, prior='uniform')
    c = hist[-1]['coeffs'][0]
    print(f'seeds {got["coeffs0"][0].tolist()} -> after one EM iteration {c.round(3).tolist()}')
    assert np.isfinite(c).all() and abs(hist[-1]['mass'].sum() - n) <= 1e-3
