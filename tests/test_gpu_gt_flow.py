"""GPU ground-truth flow (eincm_gt_flow) bit-exact against the numpy witness tests/_gt_flow_witness.py: sensors
from a few pixels to 480x640, dt = 1, 2, 4, 20 image steps over non-uniform GT timestamps, float32 and float64 stacks, ties, NaN,
inf and flows that leave the frame; batches against single windows, repeated calls and fp32 / fp64 contexts, the C-ABI's refusals,
and a synthetic MVSEC-like sequence through mvsec_datasamples -> stage_datasample -> evaluate_theta_array."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _gt_flow_witness as GW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
ev = importlib.import_module(pkg + '.evaluation')
edges_mod = importlib.import_module(pkg + '.edges')
staging = importlib.import_module(pkg + '.staging')
synth = importlib.import_module(pkg + '.synth')

_engines = {}


def _eng(shape, precision='fp32'):
    key = (tuple(shape), precision)
    if key not in _engines:
        _engines[key] = E.Engine(shape, max_events_total=1, max_refs=1, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    edges_mod.clear_engines()


def _check(shape, dt_img, dtype, seed, n_win, big=False):
    H, W = shape
    gt_ts, gx, gy = GW.random_sequence(seed, H, W, n_gt=40 if dt_img < 20 else 60, nan_inf=True, big=big)
    gx, gy = gx.astype(dtype), gy.astype(dtype)
    a, b = GW.random_windows(seed, gt_ts, n_win, dt_img)
    got = ev.estimate_gt_flow(gx, gy, gt_ts, a, b, engine=_eng(shape))
    assert got.shape == (n_win, H, W, 2) and got.dtype == np.float64
    for k in range(n_win):
        want = GW.estimate_gt_flow(gx, gy, gt_ts, a[k], b[k])
        assert GW.same_bytes(got[k], want), (shape, dt_img, dtype, k, np.argwhere(got[k] != want)[:5])
    return got


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('dt_img', [1, 2, 4, 20])
@pytest.mark.parametrize('shape', [(3, 5), (5, 3), (7, 13), (31, 37), (256, 336)])
def test_bit_exact_against_witness(shape, dt_img, dtype):
    _check(shape, dt_img, dtype, seed=dt_img * 7 + shape[0], n_win=6)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('dt_img', [1, 4, 20])
def test_bit_exact_480x640(dt_img, dtype):
    _check((480, 640), dt_img, dtype, seed=dt_img + 1000, n_win=2)


@pytest.mark.parametrize('shape', [(4, 6), (33, 47), (256, 336)])
def test_flows_leaving_the_frame(shape):
    got = _check(shape, 4, np.float32, seed=5, n_win=4, big=True)
    assert np.mean(got == 0.0) > 0.2            # many pixels leave the frame and are masked


def test_direct_and_propagate_in_one_batch():
    H, W = 40, 52
    gt_ts, gx, gy = GW.random_sequence(11, H, W, nan_inf=True)
    a = np.array([gt_ts[3] + 0.001, gt_ts[3] + 0.001, gt_ts[5], gt_ts[7]])
    b = np.array([gt_ts[3] + 0.005, gt_ts[9] + 0.01, gt_ts[6], gt_ts[7] + 0.001])
    modes = [ev.gt_flow_plan(gt_ts, s, e).mode for s, e in zip(a, b)]
    assert modes == ['direct', 'propagate', 'direct', 'direct']
    got = ev.estimate_gt_flow(gx, gy, gt_ts, a, b, engine=_eng((H, W)))
    for k in range(4):
        assert GW.same_bytes(got[k], GW.estimate_gt_flow(gx, gy, gt_ts, a[k], b[k]))


def test_batch_of_64_equals_single_windows():
    H, W = 256, 336
    gt_ts, gx, gy = GW.random_sequence(21, H, W, n_gt=60, nan_inf=True)
    img_ts = np.linspace(gt_ts[0] + 0.003, gt_ts[-1] - 0.2, 68)
    a, b = img_ts[:64], img_ts[4:68]
    eng = _eng((H, W))
    batch = ev.estimate_gt_flow(gx, gy, gt_ts, a, b, engine=eng)
    for k in range(64):
        assert GW.same_bytes(batch[k], ev.estimate_gt_flow(gx, gy, gt_ts, a[k], b[k], engine=eng)), k
    for k in (0, 31, 63):
        assert GW.same_bytes(batch[k], GW.estimate_gt_flow(gx, gy, gt_ts, a[k], b[k]))


def test_repeatable_and_precision_independent():
    H, W = 96, 128
    gt_ts, gx, gy = GW.random_sequence(31, H, W, nan_inf=True)
    a, b = GW.random_windows(31, gt_ts, 8, 4)
    first = ev.estimate_gt_flow(gx, gy, gt_ts, a, b, engine=_eng((H, W)))
    for precision in ('fp32', 'fp64', 'fp32'):
        again = ev.estimate_gt_flow(gx, gy, gt_ts, a, b, engine=_eng((H, W), precision))
        assert GW.same_bytes(first, again), precision
    assert GW.same_bytes(first, ev.estimate_gt_flow(gx.astype(np.float64), gy.astype(np.float64), gt_ts, a, b, engine=_eng((H, W))))
    assert GW.same_bytes(first, ev.estimate_gt_flow(gx, gy, gt_ts, a, b))          # the cached context


def test_only_the_touched_frames_are_used():
    H, W = 16, 20
    gt_ts, gx, gy = GW.random_sequence(41, H, W)
    plan = ev.gt_flow_plan(gt_ts, gt_ts[20] + 0.001, gt_ts[24] + 0.001)
    gx2, gy2 = gx.copy(), gy.copy()
    gx2[:20], gy2[:20], gx2[26:], gy2[26:] = np.nan, np.nan, np.nan, np.nan
    eng = _eng((H, W))
    assert GW.same_bytes(eng.gt_flow(gx, gy, plan), eng.gt_flow(gx2, gy2, plan))
    assert GW.same_bytes(eng.gt_flow(gx, gy, [plan])[0], GW.flow_from_plan(gx, gy, plan))


def test_c_abi_refusals():
    H, W = 6, 7
    eng = _eng((H, W))
    lib = L.load()
    gx = np.ones((3, H, W))
    gy = np.ones((3, H, W))
    out = np.zeros((2, H, W, 2))
    i32, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def call(mode=(0, 1), off=(0, 1, 3), frame=(0, 1, 2), num=(0.5, 0.5, 1.0), den=(1.0, 1.0, 1.0), elem=8, n_frames=3,
             n_windows=2, null=None):
        m = np.array(mode, dtype=np.int32)
        o = np.array(off, dtype=np.int32)
        f = np.array(frame, dtype=np.int32)
        nm = np.array(num, dtype=np.float64)
        dn = np.array(den, dtype=np.float64)
        args = [gx.ctypes.data, gy.ctypes.data, elem, n_frames, n_windows, m.ctypes.data_as(i32), o.ctypes.data_as(i32),
                f.ctypes.data_as(i32), nm.ctypes.data_as(dp), dn.ctypes.data_as(dp), out.ctypes.data_as(dp)]
        if null is not None:
            args[null] = None
        return lib.eincm_gt_flow(eng._ctx, *args)

    assert call() == L.OK
    want = out.copy()
    for null in (0, 1, 5, 6, 7, 8, 9, 10):
        assert call(null=null) == L.ERR_ARG, null
    assert lib.eincm_gt_flow(None, gx.ctypes.data, gy.ctypes.data, 8, 3, 2, None, None, None, None, None, None) == L.ERR_ARG
    bad = [dict(n_frames=0), dict(n_windows=0), dict(elem=2), dict(elem=16),
           dict(frame=(3, 1, 2)), dict(frame=(0, -1, 2)),                                   # frame outside [0, n_frames)
           dict(off=(0, 0, 3)), dict(off=(0, 3, 3)),                                        # a window with no steps
           dict(mode=(0, 0)),                                                               # a direct window with two steps
           dict(mode=(2, 1)), dict(off=(1, 1, 3)),
           dict(num=(np.nan, 0.5, 1.0)), dict(num=(0.5, np.inf, 1.0)),
           dict(den=(0.0, 1.0, 1.0)), dict(den=(np.nan, 1.0, 1.0)), dict(den=(np.inf, 1.0, 1.0))]
    out[:] = -7.0
    for kw in bad:
        assert call(**kw) == L.ERR_ARG, kw
        assert lib.eincm_last_error(eng._ctx)
    assert np.all(out == -7.0)                     # refused before any device work
    assert call(den=(1.0, np.nan, 0.0)) == L.OK    # a propagate window's den is not read
    assert GW.same_bytes(out, want)


def test_engine_argument_errors():
    eng = _eng((6, 7))
    gx = np.ones((3, 6, 7))
    plan = E.GtFlowPlan('direct', ((3, 1.0, 1.0),))
    with pytest.raises(ValueError):
        eng.gt_flow(gx, gx, plan)
    with pytest.raises(ValueError):
        eng.gt_flow(np.ones((3, 7, 6)), np.ones((3, 7, 6)), E.GtFlowPlan('direct', ((0, 1.0, 1.0),)))


# -- end to end -------------------------------------------------------------------------------
def _synthetic_mvsec(seed, H, W):
    """Images, events and GT of a sequence: moving-edge frames from synth, a smooth GT flow per GT frame, events on the edges."""
    rng = np.random.default_rng(seed)
    gt_ts = 10.0 + np.cumsum(rng.uniform(0.045, 0.055, 24))
    image_ts = gt_ts[0] + 0.004 + np.cumsum(rng.uniform(0.028, 0.036, 32))
    image_ts = image_ts[image_ts < gt_ts[-1] - 0.06]
    win = synth.make_window(seed, (H, W), 90000, len(image_ts), flow='smooth', flow_mag=6.0)
    images = np.clip(np.rint(40.0 + 170.0 * win['edges']), 0, 255).astype(np.uint8)
    gx = np.stack([synth._bilinear_field(rng.uniform(-3, 3, (16, 16, 2)), H, W)[..., 0] for _ in gt_ts]).astype(np.float32)
    gy = np.stack([synth._bilinear_field(rng.uniform(-3, 3, (16, 16, 2)), H, W)[..., 1] for _ in gt_ts]).astype(np.float32)
    t = image_ts[0] - 0.05 + win['ts'] * (image_ts[-1] - image_ts[0] + 0.1)
    events = {'x': win['xs'], 'y': win['ys'], 't': t, 'p': rng.random(len(t)) < 0.5}
    return events, images, image_ts, gx, gy, gt_ts


@pytest.mark.parametrize('des', [30000, 3000])
def test_end_to_end_mvsec_window(des):
    H, W = 96, 128
    seq = _synthetic_mvsec(7, H, W)
    gx, gy, gt_ts = seq[3], seq[4], seq[5]
    samples = staging.mvsec_datasamples(*seq, [1, 6], 4, des_n_events=des)
    assert (samples[0]['n_event_deficiency'] > 0) == (des == 30000)
    params = (20.0, 35.0, 2.5e-4, 0.0)
    for s in samples:
        t0, t1 = s['eval_ts']
        wit = GW.estimate_gt_flow(gx, gy, gt_ts, t0, t1)
        assert GW.same_bytes(s['flow_gt'], wit)
        xs, ys, ts, edges, edge_ts = staging.stage_datasample(s)
        sl = staging.eval_event_slice(s['events']['t'], s['eval_ts'], s['n_event_deficiency'])
        exs, eys, ets = xs[sl], ys[sl], ts[sl]
        assert len(exs) > 1000
        evals, _ = ev.evaluate_theta_array(s['flow_gt'], exs, eys, ets, edges, edge_ts, s['flow_gt'], *params, (H, W))
        assert evals['n_ee'] > 500
        assert evals['AEE'] == 0.0 and evals['AREE'] == 0.0
        for n in (1, 2, 3, 5, 10, 20):
            assert evals[f'A{n}PE'] == 0.0
        theta = s['flow_gt'] + np.random.default_rng(3).normal(0.0, 1.5, s['flow_gt'].shape)
        evals, _ = ev.evaluate_theta_array(theta, exs, eys, ets, edges, edge_ts, s['flow_gt'], *params, (H, W))
        fe = ev.sparse_flow_error(ev.per_pix_theta_to_flow(theta, exs, eys), wit)
        for k, v in list(fe['errors'].items()) + list(fe['counts'].items()):
            assert evals[k] == v, k
        assert evals['AEE'] > 0.5
