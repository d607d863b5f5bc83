"""Batched flow errors of solved thetas on the GPU against the numpy witness tests/_flow_error_witness.py, which
restates the per-pixel arithmetic, the tap order of the up-sampling and the summation order: every field of eincm_flow_error_out and
the error map are compared bit for bit.  Shapes are chosen for where the kernel can go wrong (fewer pixels than one workgroup, fewer
than the 8192 threads of a window, chains of one and two terms, several windows), not for the workload."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _flow_error_witness as FW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
ev = importlib.import_module(pkg + '.evaluation')
synth = importlib.import_module(pkg + '.synth')

METHODS = ('bilinear', 'cubic', 'lanczos3', 'lanczos5')
_engines = {}


def _eng(sensor, precision='fp32'):
    key = (tuple(sensor), precision)
    if key not in _engines:
        _engines[key] = E.Engine(sensor, 4000, max_refs=2, max_windows=3, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()


# -- the C ABI, called as a C program would -----------------------------------------------------------------------------------------
def c_stage(eng, gts, events, masks=None):
    gts = np.ascontiguousarray(gts, dtype=np.float64)
    n_ev = np.array([len(e[0]) for e in events], dtype=np.int64)
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(e[k], dtype=np.int16) for e in events] + [np.zeros(1, np.int16)]))  # noqa: E731
    xs, ys = cat(0), cat(1)
    m = None if masks is None else np.ascontiguousarray(np.asarray(masks) != 0).astype(np.uint8)
    return eng._lib.eincm_flow_eval_stage(eng._ctx, len(events), gts.ctypes.data, n_ev.ctypes.data, xs.ctypes.data, ys.ctypes.data,
                                          None if m is None else m.ctypes.data)


FIELDS = ('n_ee', 'n_pred', 'n_gt', 'n_over', 'sum_ee', 'sum_ree', 'aee', 'aree', 'anpe')


def c_errors(eng, thetas, n, method='bilinear', want_map=True):
    """(rc, list of dicts with every field of eincm_flow_error_out + 'ee_map', the raw bytes of outputs and map)."""
    t = np.ascontiguousarray(thetas, dtype=np.float64)
    out = (L.FlowErrorOut * n)()
    emap = np.full((n, eng.H, eng.W), -1.0) if want_map else None
    rc = eng._lib.eincm_flow_errors(eng._ctx, t.ctypes.data, t.shape[1], t.shape[2], L.METHODS[method], out,
                                    None if emap is None else emap.ctypes.data)
    res = []
    for b, o in enumerate(out):
        d = {k: (list(getattr(o, k)) if k in ('n_over', 'anpe') else getattr(o, k)) for k in FIELDS}
        if want_map:
            d['ee_map'] = emap[b]
        res.append(d)
    raw = bytes(out) + (emap.tobytes() if want_map else b'')
    return rc, res, raw


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def assert_same(got, want, what=''):
    """Every field: integers equal, doubles bit for bit (a NaN is a NaN), the map's NaN positions and the bits of the rest."""
    for k in ('n_ee', 'n_pred', 'n_gt', 'n_over'):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ('sum_ee', 'sum_ree', 'aee', 'aree', 'anpe'):
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and bits(g[~np.isnan(g)]) == bits(w[~np.isnan(w)]), (what, k, got[k], want[k])
    if 'ee_map' in got and 'ee_map' in want:
        g, w = got['ee_map'], want['ee_map']
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, 'NaN positions of ee_map')
        assert bits(g[~np.isnan(g)]) == bits(w[~np.isnan(w)]), (what, 'ee_map')


def to_sensor(theta, sensor, method):
    h, w = theta.shape[:2]
    if (h, w) == tuple(sensor):
        return theta
    return FW.upsample(theta, E.resample_matrix(h, sensor[0], method), E.resample_matrix(w, sensor[1], method))


def check_batch(eng, thetas, gts, events, masks=None, method='bilinear', what=''):
    sensor = (eng.H, eng.W)
    assert c_stage(eng, gts, events, masks) == L.OK, eng._lib.eincm_last_error(eng._ctx)
    rc, got, raw = c_errors(eng, thetas, len(events), method)
    assert rc == L.OK, eng._lib.eincm_last_error(eng._ctx)
    for b in range(len(events)):
        want = FW.flow_errors(to_sensor(np.asarray(thetas[b]), sensor, method), gts[b], events[b], None if masks is None else masks[b])
        assert_same(got[b], want, (what, b))
    return got, raw


# -- 1. bit-exact against the witness, full-resolution theta ------------------------------------------------------------------------
@pytest.mark.parametrize('sensor,n', [((3, 5), 1), ((5, 3), 1), ((7, 13), 1), ((31, 37), 1), ((64, 80), 1), ((97, 131), 1), ((260, 346), 3)])
def test_bit_exact_full_resolution(sensor, n):
    H, W = sensor
    cases = [FW.random_case(10 * H + b, H, W, special=H * W > 100) for b in range(n)]
    got, _ = check_batch(_eng(sensor), [c[0] for c in cases], np.stack([c[1] for c in cases]), [c[2] for c in cases], what=sensor)
    assert all(g['n_ee'] > 0 for g in got)


# -- 2. special values ----------------------------------------------------------------------------------------------------------------
def _special_batches():
    th, gt, events, expect = FW.special_case()
    yield (7, 13), th, gt, events, expect
    th, gt, events = FW.random_case(77, 37, 53, special=True)
    yield (37, 53), th, gt, events, None


@pytest.mark.parametrize('which', [0, 1])
def test_special_values_and_masks(which):
    sensor, th, gt, events, expect = list(_special_batches())[which]
    H, W = sensor
    eng = _eng(sensor)
    none = (np.zeros(0, np.int16), np.zeros(0, np.int16))
    # window 0: the case; window 1: the same fields and no events; window 2: events, but no valid ground truth (an empty intersection)
    thetas, gts, evs = [th, th, th], np.stack([gt, gt, np.zeros_like(gt)]), [events, none, events]
    got, raw_none = check_batch(eng, thetas, gts, evs, None, what='no mask')
    if expect:
        for k, v in expect.items():
            assert got[0][k] == v, k
        assert got[0]['ee_map'][2, :6].tolist() == [1.0, 2.0, 3.0, 5.0, 10.0, 20.0]            # on a threshold: not over it
    assert (got[1]['n_ee'], got[1]['n_pred']) == (0, 0) and got[1]['n_gt'] == got[0]['n_gt']
    assert got[2]['n_ee'] == 0 and got[2]['n_gt'] == 0 and got[2]['n_pred'] == got[0]['n_pred']
    for g in got[1:]:
        assert np.isnan(g['aee']) and np.isnan(g['aree']) and g['anpe'] == [0.0] * 6 and np.isnan(g['ee_map']).all()
    _, raw_ones = check_batch(eng, thetas, gts, evs, np.ones((3, H, W), np.uint8), what='mask of ones')
    assert raw_ones == raw_none
    masks = np.random.default_rng(5).random((3, H, W)) < 0.5
    got_m, raw_m = check_batch(eng, thetas, gts, evs, masks, what='random mask')
    assert 0 < got_m[0]['n_pred'] < got[0]['n_pred'] and raw_m != raw_none
    # a mask that removes every event pixel: events, valid fields, and still an empty intersection
    plane = FW.event_plane(events[0], events[1], sensor)
    got_z, _ = check_batch(eng, thetas, gts, evs, np.stack([~plane] * 3), what='mask off the events')
    assert got_z[0]['n_pred'] == 0 and got_z[0]['n_gt'] == got[0]['n_gt'] and np.isnan(got_z[0]['aee'])


# -- 3. pyramid thetas ----------------------------------------------------------------------------------------------------------------
PYR_SENSOR = (37, 53)


@functools.lru_cache(maxsize=None)
def _pyr_case():
    cases = [FW.random_case(300 + b, *PYR_SENSOR, special=True) for b in range(2)]
    return np.stack([c[1] for c in cases]), [c[2] for c in cases]


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('hw', [(1, 1), (2, 2), (4, 4), (5, 3), (16, 16)])
def test_pyramid_thetas(hw, method):
    gts, events = _pyr_case()
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    thetas = rng.normal(0.0, 6.0, size=(2,) + hw + (2,))
    if hw[0] >= 4:                                       # NaN and inf in a coarse theta are data: they spread over their taps' pixels
        thetas[1, 0, 0, 0], thetas[1, hw[0] - 1, hw[1] - 1, 1] = np.nan, np.inf
    got, _ = check_batch(_eng(PYR_SENSOR), thetas, gts, events, method=method, what=(hw, method))
    assert got[0]['n_ee'] > 0
    # the witness's tap-ordered field against the matrix product, at the project's tolerance for scaled_theta
    A_H, A_W = E.resample_matrix(hw[0], PYR_SENSOR[0], method), E.resample_matrix(hw[1], PYR_SENSOR[1], method)
    assert np.abs(FW.upsample(thetas[0], A_H, A_W) - np.einsum('yi,xj,ijc->yxc', A_H, A_W, thetas[0])).max() <= 1e-13


# -- 4. the same bytes ------------------------------------------------------------------------------------------------------------
def _three():
    cases = [FW.random_case(500 + b, *PYR_SENSOR, special=True) for b in range(3)]
    thetas = np.random.default_rng(9).normal(0.0, 6.0, size=(3, 4, 4, 2))
    return thetas, np.stack([c[1] for c in cases]), [c[2] for c in cases], np.stack([c[0] for c in cases])


def _run(eng, thetas, gts, events, method='cubic'):
    assert c_stage(eng, gts, events) == L.OK
    rc, _, raw = c_errors(eng, thetas, len(events), method)
    assert rc == L.OK
    return raw


def _split(raw, n, npix):
    """Window b's bytes of a raw result: its struct and its map."""
    s = C.sizeof(L.FlowErrorOut)
    return [raw[b * s:(b + 1) * s] + raw[n * s + b * npix * 8:n * s + (b + 1) * npix * 8] for b in range(n)]


def test_same_bytes_alone_repeated_fresh_and_fp64():
    thetas, gts, events, full = _three()
    npix = PYR_SENSOR[0] * PYR_SENSOR[1]
    eng = _eng(PYR_SENSOR)
    for th in (thetas, full):                                            # a pyramid level and the sensor's size
        raw = _run(eng, th, gts, events)
        rc, _, again = c_errors(eng, th, 3, 'cubic')                      # a repeated call on the same staging
        assert rc == L.OK and again == raw
        per = _split(raw, 3, npix)
        for b in range(3):                                               # window b staged alone
            assert _run(eng, th[b:b + 1], gts[b:b + 1], events[b:b + 1]) == per[b], b
        with E.Engine(PYR_SENSOR, 1, max_refs=1, max_windows=1) as fresh:
            assert _run(fresh, th, gts, events) == raw
        assert _run(_eng(PYR_SENSOR, 'fp64'), th, gts, events) == raw


def test_staging_survives_other_work_on_the_context():
    thetas, gts, events, _ = _three()
    H, W = PYR_SENSOR
    eng = _eng(PYR_SENSOR)
    raw = _run(eng, thetas, gts, events)
    scratch0 = eng.memory().scratch_bytes
    wins = [synth.make_window(40 + b, PYR_SENSOR, 1500, 2, flow='smooth', flow_mag=3.0) for b in range(2)]
    eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
    eng.loss_grad(np.zeros((2, 2, 2, 2)), E.make_params(20.0, 35.0, 0.0, 0.0, 0))
    rng = np.random.default_rng(2)
    eng.canny(rng.integers(0, 256, (40, H, W)).astype(np.uint8), 50.0, 120.0)         # a stack large enough to grow the scratch
    eng.flow_encode(rng.normal(0, 3, (40, 4, 4, 2)))
    assert eng.memory().scratch_bytes > scratch0
    rc, _, after = c_errors(eng, thetas, 3, 'cubic')
    assert rc == L.OK and after == raw


# -- 5. memory ------------------------------------------------------------------------------------------------------------------------
def test_memory():
    H, W = PYR_SENSOR
    thetas, gts, events, _ = _three()
    with E.Engine(PYR_SENSOR, 1, max_refs=1, max_windows=1) as eng:
        eng.flow_eval_stage(gts[:1], events[:1])
        eng.flow_errors(thetas[:1], ee_map=True)
        m1 = eng.memory()
        eng.flow_errors(thetas[:1], ee_map=True)
        eng.flow_eval_stage(gts[:1], events[:1])
        assert eng.memory() == m1                                        # nothing is allocated in steady state
        # refused calls allocate nothing
        assert eng._lib.eincm_flow_eval_stage(eng._ctx, 0, gts.ctypes.data, None, None, None, None) == L.ERR_ARG
        t = np.zeros((1, H + 1, 2, 2))
        out = (L.FlowErrorOut * 1)()
        assert eng._lib.eincm_flow_errors(eng._ctx, t.ctypes.data, H + 1, 2, 0, out, None) == L.ERR_ARG
        with pytest.raises(ValueError):
            eng.flow_errors(np.zeros((1, 2, 2, 2)), method='nearest')
        assert eng.memory() == m1
        eng.flow_eval_stage(gts, events)                                 # a larger batch: the staged block grows once, by 17 bytes a pixel
        eng.flow_errors(thetas)
        m3 = eng.memory()
        assert (m3.device_bytes - m3.scratch_bytes) - (m1.device_bytes - m1.scratch_bytes) == 2 * 17 * H * W
        assert m3.allocations == m1.allocations
        eng.flow_eval_stage(gts, events)
        eng.flow_errors(thetas)
        eng.flow_eval_stage(gts[:1], events[:1])                         # a smaller one fits what is there
        eng.flow_errors(thetas[:1])
        assert eng.memory() == m3


# -- 6. refusals through the C ABI ----------------------------------------------------------------------------------------------------
def test_refusals():
    H, W = PYR_SENSOR
    thetas, gts, events, _ = _three()
    with E.Engine(PYR_SENSOR, 4000, max_refs=2, max_windows=2) as eng:
        lib, ctx = eng._lib, eng._ctx
        n_ev = np.array([len(e[0]) for e in events], dtype=np.int64)
        xs = np.ascontiguousarray(np.concatenate([e[0] for e in events]))
        ys = np.ascontiguousarray(np.concatenate([e[1] for e in events]))
        out = (L.FlowErrorOut * 3)()
        g, n, x, y, t = gts.ctypes.data, n_ev.ctypes.data, xs.ctypes.data, ys.ctypes.data, thetas.ctypes.data
        stage = lambda *a: lib.eincm_flow_eval_stage(ctx, *a)            # noqa: E731
        errors = lambda *a: lib.eincm_flow_errors(ctx, *a)               # noqa: E731
        m0 = eng.memory()
        assert errors(t, 4, 4, 0, out, None) == L.ERR_STATE              # nothing staged yet
        for args in ((3, None, n, x, y, None), (3, g, None, x, y, None), (3, g, n, None, y, None), (3, g, n, x, None, None),
                     (0, g, n, x, y, None), (-1, g, n, x, y, None)):
            assert stage(*args) == L.ERR_ARG, args
        neg = n_ev.copy()
        neg[1] = -1
        assert stage(3, g, neg.ctypes.data, x, y, None) == L.ERR_ARG
        assert eng.memory() == m0
        assert stage(3, g, n, x, y, None) == L.OK
        for args in ((None, 4, 4, 0, out, None), (t, 4, 4, 0, None, None), (t, 4, 4, 4, out, None), (t, 4, 4, -1, out, None),
                     (t, 0, 4, 0, out, None), (t, 4, 0, 0, out, None), (t, H + 1, 4, 0, out, None), (t, 4, W + 1, 0, out, None)):
            assert errors(*args) == L.ERR_ARG, args
        assert errors(t, 4, 4, 0, out, None) == L.OK
        # an evaluation in flight
        wins = [synth.make_window(60 + b, PYR_SENSOR, 1500, 2, flow='smooth', flow_mag=3.0) for b in range(2)]
        eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
        eng.loss_grad_async(np.zeros((2, 2, 2, 2)), E.make_params(20.0, 35.0, 0.0, 0.0, 0))
        assert stage(3, g, n, x, y, None) == L.ERR_STATE
        assert errors(t, 4, 4, 0, out, None) == L.ERR_STATE
        eng.loss_grad_wait()
        assert errors(t, 4, 4, 0, out, None) == L.OK                     # the staging outlived both refusals
        # an event outside the sensor: refused, and nothing is staged afterwards
        for bad_x, bad_y in ((W, 0), (0, H), (-1, 0), (0, -1)):
            assert stage(3, g, n, x, y, None) == L.OK
            bx, by = xs.copy(), ys.copy()
            bx[len(bx) // 2], by[len(by) // 2] = bad_x, bad_y
            assert stage(3, g, n, bx.ctypes.data, by.ctypes.data, None) == L.ERR_ARG
            assert b'outside' in lib.eincm_last_error(ctx)
            assert errors(t, 4, 4, 0, out, None) == L.ERR_STATE
        with pytest.raises(ValueError, match='outside'):
            eng.flow_eval_stage(gts[:1], [(np.array([W]), np.array([0]))])
        with pytest.raises(E.EincmError):
            eng.flow_errors(thetas[:1])


# -- 7. the evaluator -------------------------------------------------------------------------------------------------------------------
def test_batch_theta_evaluator():
    H, W = 96, 128
    wins = [synth.make_window(b, (H, W), 6000, 3, flow='smooth', flow_mag=10.0) for b in range(3)]
    windows = [(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins]
    gts = np.stack([w['flow_gt'] for w in wins])
    thetas = np.stack([synth.theta_near_truth(b, w, (4, 4)) for b, w in enumerate(wins)])
    params = (20.0, 35.0, 2.5e-4, 0.1)
    masks = np.random.default_rng(1).random((3, H, W)) < 0.8
    A_H, A_W = E.resample_matrix(4, H, 'bilinear'), E.resample_matrix(4, W, 'bilinear')
    with ev.BatchThetaEvaluator((H, W), windows, gts, *params, err_eval_event_masks=masks) as be:
        res = be.evaluate(thetas)
        fe = be.flow_errors(thetas)
        assert np.abs(be.scaled_thetas(thetas)[0] - FW.upsample(thetas[0], A_H, A_W)).max() <= 1e-13
    assert len(res) == 3
    for b in range(3):
        evals, lo = res[b]
        # the per-window path on the same full-resolution field the kernel forms (the witness's tap order)
        Theta = FW.upsample(thetas[b], A_H, A_W)
        want, want_lo = ev.evaluate_theta_array(Theta, *windows[b], gts[b], *params, (H, W), err_eval_event_mask=masks[b])
        assert set(evals) == set(want) and set(lo) == set(want_lo)
        assert {k: evals[k] for k in fe[b]['errors']} == fe[b]['errors']          # .flow_errors alone gives the same figures
        for k in ('n_ee', 'n_pred', 'n_gt', 'n_pixels'):
            assert evals[k] == want[k] and type(evals[k]) is type(want[k]), k
        for n in FW.THRESHOLDS:
            assert bits(evals[f'A{n}PE']) == bits(want[f'A{n}PE']) and type(evals[f'A{n}PE']) is float
        assert evals['n_ee'] > 100
        tol = evals['n_ee'] * 2.0 ** -52                                 # tests/test_flow_error_witness.py derives it
        for k in ('AEE', 'AREE'):
            rel = abs(evals[k] - want[k]) / abs(want[k])
            print(f'window {b} {k}: relative difference {rel:.3g}, bound {tol:.3g}')
            assert rel <= tol, k
        for k in sorted(set(want) - set(fe[b]['errors']) - set(fe[b]['counts']) - {'n_pixels'}):
            a, w = np.asarray(evals[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
            rel = np.max(np.abs(a - w) / np.where(w != 0, np.abs(w), 1.0))
            print(f'window {b} {k}: largest relative difference {rel:.3g}')
            assert rel <= 1e-5, k
    # without ground truth the flow keys are absent
    with ev.BatchThetaEvaluator((H, W), windows[:1], None, *params) as be:
        evals, _ = be.evaluate(thetas[:1])[0]
        want, _ = ev.evaluate_theta_array(FW.upsample(thetas[0], A_H, A_W), *windows[0], None, *params, (H, W))
        assert set(evals) == set(want) and 'AEE' not in evals
        with pytest.raises(ValueError):
            be.flow_errors(thetas[:1])
