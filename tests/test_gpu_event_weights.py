"""Per-event weights on the GPU against the fp64 witness of tests/_event_weights_witness.py.

The weighted forms of k_splat / k_gather / k_count / k_mask and the payload that staging carries through both event layouts: at
every trip boundary of the event loops and at the image borders (tests/_event_loop_edge_cases.py's windows, window 0 weighted and
window 1 not, in one batch), on the dense and the device-resident paths, through the handover loss, the objectives, the masked
evaluation, the expanded motion path and the lockstep BFGS state.  Beside the witness: all-ones weights give the unweighted engine's
bits, a weight of 0 gives what the batch without that event gives, weights k/4 give what the list with every event repeated k times
gives, and a context staged without weights after a weighted batch gives a fresh context's bits.

The bar is TOL = 1e-5 relative (tests/test_gpu_parity.py) wherever two different computations are compared.  Weights are drawn from
{0} u [1/8, 1], about a fifth of them zero.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import _event_loop_edge_cases as EC
import _event_weights_witness as EW
from oracle import eincm_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5                      # tests/test_gpu_parity.py

synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
losses = importlib.import_module('edge-informed-contrast-maximization_amd.losses')
motion = importlib.import_module('edge-informed-contrast-maximization_amd.motion')
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')


@pytest.fixture(scope='module', autouse=True)
def _lib(built_lib):
    return built_lib


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def win_args(win):
    return (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])


def draw_weights(n, seed, lo=0.125):
    """{0} u [lo, 1], about a fifth zero; never all zero (an empty window has no loss)."""
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(lo, 1.0, n))
    if not w.any():
        w[0] = rng.uniform(lo, 1.0)
    return w.astype(np.float32)


def mats(hw, H, W, method='bilinear'):
    return (O.resample_matrix(hw[0], H, H / hw[0], method), O.resample_matrix(hw[1], W, W / hw[1], method))


def same_bits(a, b):
    a, b = np.ascontiguousarray(np.atleast_1d(a)), np.ascontiguousarray(np.atleast_1d(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. loop and border shapes -------------------------------------------------------------------------------------------------
COUNTS = (1, 255, 256, 257, 512, 513, 1025, 1537)
RUNS = [(n, None) for n in COUNTS] + [(n, EC.SEG) for n in (513, 1537)]


def mixed_windows(n):
    """The two windows of the edge cases: window 0 weighted, window 1 with None, in one batch."""
    w0, w1 = EC.windows(n)
    return [w0 + (draw_weights(n, 900 + n),), w1 + (None,)]


def stage(wins, seg=None, B=None, binning='device'):
    with pytest.MonkeyPatch.context() as mp:
        for k in EC.ENV:
            mp.delenv(k, raising=False)
        if binning == 'host':           # (read when the context is created)
            mp.setenv('EINCM_HOST_BINNING', '1')
        if seg is not None:
            for k in ('EINCM_SEG', 'EINCM_SEG_SPLAT', 'EINCM_SEG_2DOF'):
                mp.setenv(k, str(seg))
        eng = engine.Engine((EC.H, EC.W), max(sum(len(w[0]) for w in wins), 1), max_refs=EC.R, max_windows=B or len(wins))
        try:
            eng.set_windows(wins)
        except Exception:
            eng.close()
            raise
    return eng


def edge_params(gamma=0.0, lvl=0):
    return engine.make_params(EC.ALPHA, EC.BETA, gamma, 0.0, lvl)


_WIT = {}


def edge_witness(n, setting, mode):
    """Per window (value, gradient, IWE stack, zero-warp IWE) of the mixed batch; once per (n, theta): segment lengths do not change it."""
    k = (n, setting, mode)
    if k not in _WIT:
        th = EC.theta(setting, mode)
        out = []
        for b, win in enumerate(mixed_windows(n)):
            v, g, _, I, t = EW.loss_and_grad(th[b], *win[:5], EC.ALPHA, EC.BETA, 0.0, 0.0, 0, *mats(th[b].shape[:2], EC.H, EC.W), weights=win[5])
            out.append((v, g, I, t['zero_iwe']))
        _WIT[k] = out
    return _WIT[k]


@pytest.mark.parametrize('n,seg', RUNS, ids=[f'n{n}' + (f'-seg{seg}' if seg else '') for n, seg in RUNS])
def test_event_count_at_a_trip_boundary(n, seg):
    eng = stage(mixed_windows(n), seg=seg)
    try:
        assert eng.weighted
        for setting in EC.SETTINGS:
            for mode in EC.MODES:
                v, g, _ = eng.loss_grad(EC.theta(setting, mode), edge_params())
                iw, z = eng.iwes(), eng.zero_iwe()
                for b, (v_w, g_w, I_w, z_w) in enumerate(edge_witness(n, setting, mode)):
                    e = (abs(v[b] - v_w) / abs(v_w), rel(g[b], g_w), rel(iw[b], I_w), rel(z[b], z_w))
                    print(f'WEIGHTS n{n} seg{seg or 0} {setting} {mode} window {b} value={e[0]:.2e} grad={e[1]:.2e} iwe={e[2]:.2e} zero={e[3]:.2e}')
                    assert max(e) <= TOL, (n, seg, setting, mode, b, e)
    finally:
        eng.close()


# ---- 2. all-ones weights are the unweighted engine, bit for bit ------------------------------------------------------------------
def test_all_ones_is_the_unweighted_engine_bit_for_bit():
    n = 1537
    plain = EC.windows(n)
    ones = [w + (np.ones(n, dtype=np.float32),) for w in plain]
    a, b = stage(ones), stage(plain)
    try:
        assert a.weighted and not b.weighted
        for setting in EC.SETTINGS:
            for mode in EC.MODES:
                for gamma in (0.0, 2.5e-4):
                    va, ga, _ = a.loss_grad(EC.theta(setting, mode), edge_params(gamma))
                    vb, gb, _ = b.loss_grad(EC.theta(setting, mode), edge_params(gamma))
                    tag = (setting, mode, gamma)
                    assert same_bits(va, vb) and same_bits(ga, gb), tag
                    assert same_bits(a.iwes(), b.iwes()) and same_bits(a.image_grad(), b.image_grad()), tag
        assert same_bits(a.zero_iwe(), b.zero_iwe())
        assert np.array_equal(a.count_images(), b.count_images())
    finally:
        a.close()
        b.close()


DENSE = ((60, 80), 20000, 3, 8.0, 2000.0, 4000.0, 2.5e-3)          # the dense_small row of tests/test_gpu_parity.py


def dense_case():
    (H, W), N, R, mag, al, be, ga = DENSE
    win = synth.make_window(11, (H, W), N, R, flow='smooth', flow_mag=mag)
    th = win['flow_gt'] * np.random.default_rng(2).uniform(0.5, 1.5, (H, W, 2))
    return win, th, engine.make_params(al, be, ga, 0.0, 0)


def test_all_ones_dense_bit_for_bit():
    win, th, p = dense_case()
    (H, W), N, R = DENSE[:3]
    with engine.Engine((H, W), N, max_refs=R) as a, engine.Engine((H, W), N, max_refs=R) as b:
        a.set_window(*win_args(win), weights=np.ones(N))
        b.set_window(*win_args(win))
        va, ga, _ = a.loss_grad(th, p)
        vb, gb, _ = b.loss_grad(th, p)
        assert same_bits(va, vb) and same_bits(ga, gb)
        assert same_bits(a.iwes(), b.iwes()) and same_bits(a.image_grad(), b.image_grad())


# ---- 3. weight 0 is absence --------------------------------------------------------------------------------------------------------
def weight_zero_batch(hw):
    """(full, cut, ws, theta, params): two weighted windows, the same without their weight-0 events, the weights, a theta near the truth."""
    H, W, N, R = EC.H, EC.W, 1500, 2
    wins = [synth.make_window(60 + b, (H, W), N, R, flow='smooth', flow_mag=5.0) for b in range(2)]
    ws = [draw_weights(N, 70 + b) for b in range(2)]
    keep = [w > 0 for w in ws]
    full = [win_args(v) + (w,) for v, w in zip(wins, ws)]
    cut = [(v['xs'][k], v['ys'][k], v['ts'][k], v['edges'], v['edge_ts'], w[k]) for v, w, k in zip(wins, ws, keep)]
    for v, k in zip(wins, keep):        # some pixels hold nothing but weight-0 events: the TV mask must leave them out
        on = np.zeros((H, W), bool)
        on[v['ys'][k], v['xs'][k]] = True
        assert (~on[v['ys'][~k], v['xs'][~k]]).any()
    th = np.stack([synth.theta_near_truth(60 + b, v, hw) for b, v in enumerate(wins)])
    return full, cut, ws, th, engine.make_params(20.0, 35.0, 2.5e-4, 0.0, 0)


def check_weight_zero_is_absence(hw, binning='device'):
    """The body of test_weight_zero_is_absence on either binning path (tests/test_gpu_event_weights_cells.py runs it on the host's);
    returns the weighted batch's value and gradient."""
    H, W, N = EC.H, EC.W, 1500
    full, cut, ws, th, p = weight_zero_batch(hw)
    a, b = stage(full, binning=binning), stage(cut, binning=binning)
    try:
        va, ga, xa = a.loss_grad(th, p, want_aux=True)
        vb, gb, xb = b.loss_grad(th, p, want_aux=True)
        assert np.array_equal(a.n_events, [N, N]) and all(len(a.warped_events(i)[0][0]) == N for i in range(2))
        assert rel(va, vb) <= TOL and rel(a.iwes(), b.iwes()) <= TOL and rel(a.zero_iwe(), b.zero_iwe()) <= TOL
        for i in range(2):
            assert rel(ga[i], gb[i]) <= TOL, i
            assert xa[i]['theta_total_variation'] == pytest.approx(xb[i]['theta_total_variation'], rel=TOL)
            assert xa[i]['theta_total_variation'] > 0.0
        assert np.array_equal(a.count_images(), b.count_images())
        # ... and the witness agrees with both, the TV term included
        for i in range(2):
            v_w, g_w, _, _, t = EW.loss_and_grad(th[i], *full[i][:5], 20.0, 35.0, 2.5e-4, 0.0, 0, *mats(hw, H, W), weights=ws[i])
            assert abs(va[i] - v_w) <= TOL * abs(v_w) and rel(ga[i], g_w) <= TOL
            assert xa[i]['theta_total_variation'] == pytest.approx(t['theta_total_variation'], rel=TOL)
            Theta = O.scale_theta_to_sensor_size(th[i], (H, W), 'bilinear')
            assert np.array_equal(a.count_images()[i], EW.count_images(Theta, *full[i][:3], full[i][4], ws[i]))
    finally:
        a.close()
        b.close()
    return va, ga


@pytest.mark.parametrize('hw', [(1, 1), (4, 4)])
def test_weight_zero_is_absence(hw):
    check_weight_zero_is_absence(hw)


# ---- 4. dense theta and the device path -------------------------------------------------------------------------------------------
def test_dense_theta_host_and_device_paths():
    import torch
    win, th, p = dense_case()
    (H, W), N, R, _, al, be, ga = DENSE
    w = draw_weights(N, 5)
    eye = (np.eye(H), np.eye(W))
    v_w, g_w, G_w, I_w, _ = EW.loss_and_grad(th, *win_args(win), al, be, ga, 0.0, 0, *eye, weights=w)
    with engine.Engine((H, W), N, max_refs=R) as eng:
        eng.set_window(*win_args(win), weights=w)
        v, g, _ = eng.loss_grad(th, p)
        assert abs(v[0] - v_w) <= TOL * abs(v_w) and rel(g[0], g_w) <= TOL
        assert rel(eng.iwes()[0], I_w) <= TOL and rel(eng.image_grad()[0], G_w) <= TOL
        vd, gd, _ = eng.loss_grad_device(torch.from_numpy(th).cuda(), p, theta_abs_max=float(np.abs(th).max()))
        assert abs(vd[0] - v_w) <= TOL * abs(v_w) and rel(gd.cpu().numpy(), g_w) <= TOL
        assert rel(eng.iwes()[0], I_w) <= TOL


def test_partial_tiles_and_odd_sizes():
    (H, W), N, R, hw = (33, 65), 3000, 2, (3, 5)          # the odd_sizes row of tests/test_gpu_parity.py
    win = synth.make_window(11, (H, W), N, R, flow='smooth', flow_mag=5.0)
    th = synth.theta_near_truth(11, win, hw)
    w = draw_weights(N, 6)
    v_w, g_w, G_w, I_w, t = EW.loss_and_grad(th, *win_args(win), 60.0, 60.0, 1e-3, 0.0, 0, *mats(hw, H, W, 'cubic'), weights=w)
    with engine.Engine((H, W), N, max_refs=R) as eng:
        eng.set_window(*win_args(win), weights=w)
        v, g, _ = eng.loss_grad(th, engine.make_params(60.0, 60.0, 1e-3, 0.0, 0, 'cubic'))
        assert abs(v[0] - v_w) <= TOL * abs(v_w) and rel(g[0], g_w) <= TOL
        assert rel(eng.iwes()[0], I_w) <= TOL and rel(eng.image_grad()[0], G_w) <= TOL and rel(eng.zero_iwe()[0], t['zero_iwe']) <= TOL


# ---- 5. - 7. handover, objectives, masked evaluation ----------------------------------------------------------------------------------
def small_window(seed=3, n=1500):
    return synth.make_window(seed, (EC.H, EC.W), n, EC.R, flow='smooth', flow_mag=5.0)


def test_handover_matches_witness():
    win = small_window()
    w = draw_weights(1500, 8)
    prev, th = synth.theta_near_truth(8, win, (2, 2)), synth.theta_near_truth(9, win, (2, 2))
    v_w, dv_w = EW.handover_loss_and_grad(0.4, prev, th, *win_args(win), 20.0, 35.0, 0.0, 0.0, 1, *mats((2, 2), EC.H, EC.W), weights=w)
    with engine.Engine((EC.H, EC.W), 1500, max_refs=EC.R) as eng:
        eng.set_window(*win_args(win), weights=w)
        v, dv = eng.handover_loss_grad(0.4, prev, th, engine.make_params(20.0, 35.0, 0.0, 0.0, 1))
    assert abs(v[0] - v_w) <= TOL * abs(v_w)
    assert abs(dv[0] - dv_w) <= TOL * max(abs(dv_w), 1e-12 * abs(v_w))
    # the same through the losses callable, whose engine cache keys on the weights
    v2, dv2 = losses.value_and_grad_handover_loss_func(0.4, prev, th, *win_args(win), 20.0, 35.0, 0.0, 0.0, 1, 3, (EC.H, EC.W), event_weights=w)
    v3 = losses.handover_loss_func(0.4, prev, th, *win_args(win), 20.0, 35.0, 0.0, 0.0, 1, 3, (EC.H, EC.W))
    losses.clear_engine_cache()
    assert v2 == v[0] and dv2 == dv[0]
    assert v3 != v2                                   # (the unweighted window is another objective, and another entry of the cache)


def test_objectives_match_witness():
    win = small_window(12, 3000)
    w = draw_weights(3000, 9)
    Theta = win['flow_gt'] * 0.8
    t = EW.objectives(Theta, *win_args(win), weights=w)
    d = losses.compute_loss_objectives(Theta, *win_args(win), (EC.H, EC.W), event_weights=w)
    losses.clear_engine_cache()
    per = t['per_ref']
    assert d['zero_contrast'] == pytest.approx(t['zero_contrast'], rel=TOL)
    assert d['zero_iwe_divergence'] == pytest.approx(t['zero_iwe_divergence'], rel=TOL)
    assert rel(d['zero_correlations'], [q['zero_correlation'] for q in per]) <= TOL
    assert rel(d['correlations'], [q['correlation'] for q in per]) <= TOL
    assert rel(d['contrasts'], [q['contrast'] for q in per]) <= TOL
    assert rel(d['iwe_divergences'], [q['divergence'] for q in per]) <= TOL
    assert rel(d['flow_warp_losses'], [q['variance'] / t['zero_variance'] for q in per]) <= TOL
    assert d['theta_total_variation'] == pytest.approx(t['theta_total_variation'], rel=TOL)
    assert d['warped_xs'].shape == (EC.R, 3000)          # weight-0 events are still returned, in the order handed over


def test_masked_evaluation_of_a_mixed_batch():
    eng = stage(mixed_windows(1537))
    try:
        for mode in EC.MODES:
            th = EC.theta('small', mode)
            v, g, _ = eng.loss_grad(th, edge_params())
            for act in ([0, 1], [1, 0]):
                vm, gm, _ = eng.loss_grad(th, edge_params(), active=act)
                on = int(np.argmax(act))
                assert same_bits(vm[on], v[on]) and same_bits(gm[on], g[on]), (mode, act)
                assert np.isnan(vm[1 - on]) and not gm[1 - on].any()
    finally:
        eng.close()


# ---- 8. motion ---------------------------------------------------------------------------------------------------------------------
def test_motion_expanded_matches_witness_and_fused_refuses():
    H, W, N = EC.H, EC.W, 1500
    model = motion.MotionModel('affine', (H, W))
    c = np.array([[1.5, 0.8, -0.6, -1.0, 0.5, 0.9]])
    win = synth.make_window(21, (H, W), N, EC.R, flow=model.field(c[0]))
    w = draw_weights(N, 10)
    p = engine.make_params(20.0, 35.0, 0.0, 0.0, 1)
    v_w, gT = EW.loss_and_grad_Theta(model.field(c[0]), *win_args(win), 20.0, 35.0, 0.0, 0.0, 1, weights=w)
    g_w = model.project(gT)
    with engine.Engine((H, W), N, max_refs=EC.R) as eng:
        eng.set_window(*win_args(win), weights=w)
        eng.set_motion_model(model)
        v, g, _ = eng.loss_grad_motion(c, p)
        assert abs(v[0] - v_w) <= TOL * abs(v_w) and rel(g[0], g_w) <= TOL
        eng.set_motion_path('auto')
        va, ga, _ = eng.loss_grad_motion(c, p)
        assert same_bits(va, v) and same_bits(ga, g)
        eng.set_motion_path('fused')
        with pytest.raises(ValueError, match='weight'):
            eng.loss_grad_motion(c, p)
        # the library refuses by itself too
        val, grd = np.empty(1), np.empty((1, 6))
        rc = eng._lib.eincm_loss_grad_motion_fused(eng._ctx, c.ctypes.data, C.byref(p), None, val.ctypes.data, grd.ctypes.data, None)
        assert rc == L.ERR_UNSUPPORTED and b'weight' in eng._lib.eincm_last_error(eng._ctx)
        # without weights the fused path serves the same context again
        eng.set_window(*win_args(win))
        assert not eng.weighted
        eng.loss_grad_motion(c, p)


# ---- 9. lockstep state ---------------------------------------------------------------------------------------------------------------
def test_bfgs_eval_at_alpha_zero_is_loss_grad():
    eng = stage(mixed_windows(1537))
    try:
        th = EC.theta('small', 'grid')
        p = edge_params()
        v, g, _ = eng.loss_grad(th, p)
        eng.bfgs_begin(th)
        vb, _, gmax = eng.bfgs_eval(p, np.zeros(EC.B))
        # two assemblies of one evaluation (host and k_final): the bar the suite sets between two paths of the same evaluation
        assert rel(vb, v) <= 1e-6
        assert rel(gmax, np.abs(g.reshape(EC.B, -1)).max(1)) <= 1e-6
        for b, (v_w, g_w, _, _) in enumerate(edge_witness(1537, 'small', 'grid')):
            assert abs(vb[b] - v_w) <= TOL * abs(v_w) and abs(gmax[b] - np.abs(g_w).max()) <= TOL * np.abs(g_w).max()
    finally:
        eng.close()


# ---- 10. / 11. determinism and re-staging ------------------------------------------------------------------------------------------------
def test_two_evaluations_and_two_stagings_give_equal_bytes():
    wins = mixed_windows(1537)
    a, b = stage(wins), stage(wins)
    try:
        for mode in EC.MODES:
            th = EC.theta('border', mode)
            out = []
            for eng in (a, a, b):
                v, g, _ = eng.loss_grad(th, edge_params(2.5e-4))
                out.append((v.copy(), g.copy(), eng.iwes().copy()))
            a.set_windows(wins)                 # ... and the same context staged again
            v, g, _ = a.loss_grad(th, edge_params(2.5e-4))
            out.append((v, g, a.iwes()))
            for o in out[1:]:
                assert all(same_bits(x, y) for x, y in zip(o, out[0])), mode
    finally:
        a.close()
        b.close()


def test_restaging_without_weights_drops_the_weighted_state():
    n = 1537
    plain = EC.windows(n)
    a, b = stage(mixed_windows(n)), stage(plain)
    try:
        assert a.weighted
        a.loss_grad(EC.theta('small', 'grid'), edge_params())
        a.set_windows(plain)
        assert not a.weighted
        for mode in EC.MODES:
            th = EC.theta('small', mode)
            va, ga, _ = a.loss_grad(th, edge_params(2.5e-4))
            vb, gb, _ = b.loss_grad(th, edge_params(2.5e-4))
            assert same_bits(va, vb) and same_bits(ga, gb) and same_bits(a.iwes(), b.iwes()), mode
        assert np.array_equal(a.count_images(), b.count_images())
    finally:
        a.close()
        b.close()


# ---- 12. the repetition identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (4, 4)])
def test_repetition_identity(hw):
    """Weights k/4 against the unweighted engine on the list with event e repeated k_e times: the same loss and gradient."""
    win = small_window()
    N, K = 1500, 4
    k = np.random.default_rng(11).integers(0, K + 1, N)
    rep = np.repeat(np.arange(N), k)
    th = synth.theta_near_truth(1, win, hw)
    p = engine.make_params(20.0, 35.0, 2.5e-4, 0.0, 0)
    with engine.Engine((EC.H, EC.W), N, max_refs=EC.R) as a, engine.Engine((EC.H, EC.W), len(rep), max_refs=EC.R) as b:
        a.set_window(*win_args(win), weights=k / K)
        b.set_window(win['xs'][rep], win['ys'][rep], win['ts'][rep], win['edges'], win['edge_ts'])
        va, ga, _ = a.loss_grad(th, p)
        vb, gb, _ = b.loss_grad(th, p)
        assert abs(va[0] - vb[0]) <= TOL * abs(vb[0]) and rel(ga[0], gb[0]) <= TOL
        assert rel(a.iwes() * K, b.iwes()) <= TOL


# ---- the library's own refusals ---------------------------------------------------------------------------------------------------
def test_library_refuses_by_itself():
    win = small_window(3, 200)
    n = np.array([200], dtype=np.int64)
    xs, ys, ts, ed, et = (np.ascontiguousarray(a) for a in win_args(win))
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)

    def call(eng, w, flags=0):
        return eng._lib.eincm_set_windows_weighted(eng._ctx, 1, EC.R, n.ctypes.data_as(C.POINTER(C.c_int64)), one(xs), one(ys), one(ts), one(ed),
                                                   et.ctypes.data_as(C.POINTER(C.c_double)), one(w) if w is not None else None, flags)
    good = np.full(200, 0.5, dtype=np.float32)
    with engine.Engine((EC.H, EC.W), 200, max_refs=EC.R) as eng:
        for bad in (np.nan, np.inf, -1e-9, 1.0 + 1e-6):
            w = good.copy()
            w[17] = bad
            assert call(eng, w) == L.ERR_ARG
            assert b'weight 17 of window 0' in eng._lib.eincm_last_error(eng._ctx)
        assert call(eng, good, L.SW_DEFER_CONSTANTS) == L.ERR_UNSUPPORTED
        assert call(eng, None) == L.OK and call(eng, good) == L.OK
        assert eng._lib.eincm_set_splat_window(eng._ctx, 5) == L.ERR_UNSUPPORTED
        assert eng._lib.eincm_set_splat_window(eng._ctx, 3) == L.OK
    with engine.Engine((EC.H, EC.W), 200, max_refs=EC.R) as eng:
        eng.set_splat_window(5)
        assert call(eng, good) == L.ERR_UNSUPPORTED and call(eng, None) == L.OK
    with engine.Engine((EC.H, EC.W), 200, max_refs=EC.R, precision='fp64') as eng:
        assert call(eng, good) == L.ERR_UNSUPPORTED and b'fp64' in eng._lib.eincm_last_error(eng._ctx)
        assert call(eng, None) == L.OK
