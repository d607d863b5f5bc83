"""The selectable splat window size on the GPU: parity with the fp64 autograd witness
(tests/_splat_window_witness.py) at sizes 1, 5 and 7 for every theta mode, the border and wide-flow paths of the new event kernels,
batches, the entry points, bitwise properties, the refusals and a lockstep solve.  Tolerance and `rel` as tests/test_gpu_parity.py:
1e-5, max-norm relative."""
import importlib

import numpy as np
import pytest

from oracle import eincm_oracle as O
import _splat_window_witness as SW

pytestmark = pytest.mark.gpu

TOL = 1e-5
SIZES = (1, 5, 7)

synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')
engine = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
losses = importlib.import_module('edge-informed-contrast-maximization_amd.losses')
evaluation = importlib.import_module('edge-informed-contrast-maximization_amd.evaluation')
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')

A, B_, GAMMA = 20.0, 35.0, 2.5e-3


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def same_aux(a, b):
    return len(a) == len(b) and all(x.keys() == y.keys() and all(np.array_equal(x[k], y[k], equal_nan=True) for k in x) for x, y in zip(a, b))


def win_args(win):
    return (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])


@pytest.fixture(scope='module', autouse=True)
def _lib(built_lib):
    yield built_lib
    losses.clear_engine_cache()


_WINS = {}


def window(shape=(120, 160), n=30000, R=3, seed=5, mag=8.0):
    key = (shape, n, R, seed, mag)
    if key not in _WINS:
        _WINS[key] = synth.make_window(seed, shape, n, R, flow='smooth', flow_mag=mag)
    return _WINS[key]


def mats(theta, H, W, method='bilinear'):
    h, w = theta.shape[:2]
    if (h, w) == (H, W):
        return np.eye(H), np.eye(W)
    return O.resample_matrix(h, H, H / h, method), O.resample_matrix(w, W, W / w, method)


def witness(win, theta, size, method='bilinear', gamma=0.0, delta=0.0, lvl=1, ck=0, rk=0):
    H, W = win['sensor_size']
    return SW.loss_and_grad(theta, *win_args(win), A, B_, gamma, delta, lvl, *mats(theta, H, W, method), window_size=size,
                            contrast_kind=ck, correlation_kind=rk)


def check(win, theta, size, method='bilinear', gamma=0.0, delta=0.0, lvl=1, ck=0, rk=0):
    H, W = win['sensor_size']
    v_w, g_w, G_w, I_w, t_w = witness(win, theta, size, method, gamma, delta, lvl, ck, rk)
    with engine.Engine((H, W), len(win['xs']), max_refs=len(win['edge_ts'])) as eng:
        eng.set_splat_window(size)
        eng.set_window(*win_args(win))
        p = engine.make_params(A, B_, gamma, delta, lvl, method, ck, correlation_kind=rk)
        v, g, aux = eng.loss_grad(theta, p, want_aux=True)
        I, G = eng.iwes()[0], eng.image_grad()[0]
        v_f, _, _ = eng.loss_grad(theta, p, want_grad=False, want_aux=True)
    tag = (size, theta.shape, method, gamma, delta, ck, rk)
    assert abs(v[0] - v_w) <= TOL * abs(v_w), (tag, v[0], v_w)
    assert rel(g[0], g_w) <= TOL, (tag, rel(g[0], g_w))
    assert rel(I, I_w) <= TOL, (tag, rel(I, I_w))
    # delta != 0: dL/dIWE holds sign(div n) (k_divgrad, unchanged), which flips wherever the divergence of the normalised fp32 image
    # is within rounding of zero - a few pixels, each off by one stencil weight / HW (the default path's parity tests leave G out there)
    assert rel(G, G_w) <= (TOL if delta == 0.0 else 1e-4), (tag, rel(G, G_w))
    assert abs(v_f[0] - v_w) <= TOL * abs(v_w), tag
    assert aux[0]['mean_rel_corr'] == pytest.approx(t_w['mean_rel_corr'], rel=TOL), tag
    assert aux[0]['mean_rel_contrast'] == pytest.approx(t_w['mean_rel_contrast'], rel=TOL), tag
    return v, g


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES)
def test_2dof(size):
    win = window()
    check(win, synth.theta_near_truth(1, win, (1, 1)), size)


@pytest.mark.parametrize('method', ['bilinear', 'lanczos3'])
@pytest.mark.parametrize('size', SIZES)
def test_16x16_grid(size, method):
    win = window()
    check(win, synth.theta_near_truth(2, win, (16, 16)), size, method)


@pytest.mark.parametrize('size', SIZES)
def test_dense_theta(size):
    win = window((48, 64), 6000, 2, seed=7)
    check(win, win['flow_gt'] * 0.9, size)


@pytest.mark.parametrize('size', SIZES)
def test_level0_with_tv_and_divergence(size):
    win = window((64, 80), 8000, 3, seed=11)
    check(win, synth.theta_near_truth(3, win, (4, 4)), size, gamma=GAMMA, delta=0.7, lvl=0)


@pytest.mark.parametrize('ck,rk', [(3, 1), (2, 3)])
@pytest.mark.parametrize('size', SIZES)
def test_objective_kinds(size, ck, rk):
    win = window()
    check(win, synth.theta_near_truth(4, win, (2, 2)), size, ck=ck, rk=rk)


def _border_window(shape, n, R, seed):
    """Half the events on the outermost two rows / columns, so that every radius puts taps past both ends of both axes."""
    win = dict(synth.make_window(seed, shape, n, R, flow='smooth', flow_mag=2.0))
    H, W = shape
    rng = np.random.default_rng(seed)
    xs, ys = win['xs'].copy(), win['ys'].copy()
    m = n // 2
    side = rng.integers(0, 4, m)
    pos_x, pos_y = rng.integers(0, W, m), rng.integers(0, H, m)
    edge = rng.integers(0, 2, m)
    xs[:m] = np.where(side == 0, edge, np.where(side == 1, W - 1 - edge, pos_x))
    ys[:m] = np.where(side == 2, edge, np.where(side == 3, H - 1 - edge, pos_y))
    win['xs'], win['ys'] = xs.astype(win['xs'].dtype), ys.astype(win['ys'].dtype)
    return win


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('shape,hw', [((40, 52), (1, 1)), ((40, 52), (2, 2)), ((6, 5), (1, 1)), ((3, 4), (3, 4))])
def test_border_events_wrap_and_drop(size, shape, hw):
    """Taps past the left / top wrap once, past the right / bottom are dropped; on sensors no wider than 2w (6x5 and 3x4 at sizes 5
    and 7) one event's taps wrap onto pixels it already covers."""
    win = _border_window(shape, 400 if shape[0] < 10 else 3000, 2, seed=21)
    check(win, synth.theta_near_truth(5, win, hw) if hw != shape else win['flow_gt'], size)


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('hw', [(1, 1), (2, 2)])
def test_wide_theta_leaves_the_lds_window(size, hw):
    """theta far beyond the capacity of the LDS windows: most taps take the direct-to-HBM path of both kernels."""
    win = window((96, 128), 12000, 2, seed=23)
    check(win, synth.theta_near_truth(6, win, hw) * 25.0, size)


@pytest.mark.parametrize('size', SIZES)
def test_batch_of_unequal_windows(size):
    H, W, R = 96, 128, 3
    Ns = [1, 40, 2000, 40000]
    wins = []
    for b, n in enumerate(Ns):
        w = dict(synth.make_window(60 + b, (H, W), max(n, 2), R, flow='smooth', flow_mag=4.0 + 2 * b))
        for k in ('xs', 'ys', 'ts'):
            w[k] = w[k][:n]
        wins.append(w)
    thetas = np.stack([synth.theta_near_truth(b, w, (2, 2)) for b, w in enumerate(wins)])
    with engine.Engine((H, W), sum(Ns), max_refs=R, max_windows=len(Ns)) as eng:
        eng.set_splat_window(size)
        eng.set_windows([win_args(w) for w in wins])
        v, g, _ = eng.loss_grad(thetas, engine.make_params(A, B_, 0.0, 0.0, 1))
        I = eng.iwes()
    for b in range(len(Ns)):
        if Ns[b] < 10:        # a handful of events: the normalisation's arg-min / arg-max dominate; value and IWE only
            v_w, _, _, I_w, _ = witness(wins[b], thetas[b], size)
            assert abs(v[b] - v_w) <= 1e-4 * abs(v_w), (b, v[b], v_w)
            assert rel(I[b], I_w) <= TOL, b
            continue
        v_w, g_w, _, I_w, _ = witness(wins[b], thetas[b], size)
        assert abs(v[b] - v_w) <= TOL * abs(v_w), (b, v[b], v_w)
        assert rel(g[b], g_w) <= TOL, (b, rel(g[b], g_w))
        assert rel(I[b], I_w) <= TOL, b


def test_65_windows_masked():
    """B = 65 at size 5: past the 64-bit window mask.  Masked windows below 64 return NaN and a zero gradient, the active ones the
    unmasked bits, and windows 0, 63 and 64 match the witness."""
    H, W, R, B = 40, 50, 2, 65
    wins = [synth.make_window(300 + b, (H, W), 1500 + 37 * b, R, flow='constant', flow_mag=3.0 + 0.05 * b) for b in range(B)]
    thetas = np.stack([synth.theta_near_truth(b, w, (2, 2)) for b, w in enumerate(wins)])
    p = engine.make_params(A, B_, 0.0, 0.0, 1)
    active = np.ones(B, dtype=np.uint8)
    active[[0, 5, 31, 32, 62]] = 0
    with engine.Engine((H, W), sum(len(w['xs']) for w in wins), max_refs=R, max_windows=B) as eng:
        eng.set_splat_window(5)
        eng.set_windows([win_args(w) for w in wins])
        v, g, _ = eng.loss_grad(thetas, p)
        G = eng.image_grad()
        vm, gm, _ = eng.loss_grad(thetas, p, active=active)
    on = active == 1
    assert np.all(np.isfinite(v))
    assert np.all(np.isnan(vm[~on])) and not gm[~on].any()
    assert np.array_equal(vm[on], v[on]) and np.array_equal(gm[on], g[on])
    for b in (0, 63, 64):
        v_w, g_w, G_w, _, _ = witness(wins[b], thetas[b], 5)
        assert abs(v[b] - v_w) <= TOL * abs(v_w), (b, v[b], v_w)
        assert rel(g[b], g_w) <= TOL, (b, rel(g[b], g_w))
        assert rel(G[b], G_w) <= TOL, b


def test_fullsize_size5():
    """260 x 346, 10^6 events, R = 5 at size 5 (2-DoF): value, gradient and IWE stack against the witness."""
    win = synth.make_window(31, (260, 346), 1_000_000, 5, flow='smooth', flow_mag=10.0)
    check(win, synth.theta_near_truth(7, win, (1, 1)), 5)


# ---- 2. entry points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES)
def test_async_and_device_entry_point(size):
    import torch
    win = window()
    for hw in ((1, 1), (4, 4)):
        th = synth.theta_near_truth(7, win, hw)
        p = engine.make_params(A, B_, GAMMA, 0.0, 0)
        with engine.Engine((120, 160), 30000, max_refs=3) as eng:
            eng.set_splat_window(size)
            eng.set_window(*win_args(win))
            v, g, a = eng.loss_grad(th, p, want_aux=True)
            eng.loss_grad_async(th, p)
            va, ga, aa = eng.loss_grad_wait(want_aux=True)
            assert np.array_equal(v, va) and np.array_equal(g, ga) and same_aux(a, aa), (size, hw)
            vd, gd, ad = eng.loss_grad_device(torch.from_numpy(th[None].copy()).cuda(), p, theta_abs_max=float(np.abs(th).max()),
                                              want_aux=True)
            assert np.array_equal(v, vd) and same_aux(a, ad), (size, hw)
            assert rel(gd.cpu().numpy(), g) <= 1e-12, (size, hw)


@pytest.mark.parametrize('size', SIZES)
def test_handover_matches_witness(size):
    win = window()
    H, W = win['sensor_size']
    prev = synth.theta_near_truth(8, win, (2, 2))
    th = synth.theta_near_truth(9, win, (2, 2))
    v_w, dv_w = SW.handover_loss_and_grad(0.4, prev, th, *win_args(win), A, B_, 0.0, 0.0, 1, *mats(th, H, W), window_size=size)
    v, dv = losses.value_and_grad_handover_loss_func(0.4, prev, th, *win_args(win), A, B_, 0.0, 0.0, 1, 3, (H, W), window_size=size)
    assert abs(v - v_w) <= TOL * abs(v_w)
    assert abs(dv - dv_w) <= TOL * max(abs(dv_w), 1e-12 * abs(v_w))
    # forward only: the default kinds' statistics come from another kernel there (k_stats), so the value agrees to rounding, not bitwise
    v2 = losses.handover_loss_func(0.4, prev, th, *win_args(win), A, B_, 0.0, 0.0, 1, 3, (H, W), window_size=size)
    assert abs(v2 - v_w) <= TOL * abs(v_w) and abs(v2 - v) <= 1e-8 * abs(v)
    (vl, _), gl = losses.value_and_grad_loss_func(th, *win_args(win), A, B_, 0.0, 0.0, 1, 3, (H, W), window_size=size)
    v_w2, g_w2, _, _, _ = witness(win, th, size)
    assert abs(vl - v_w2) <= TOL * abs(v_w2) and rel(gl, g_w2) <= TOL
    assert losses.loss_func(th, *win_args(win), A, B_, 0.0, 0.0, 1, 3, (H, W), window_size=size)[0] == pytest.approx(v_w2, rel=TOL)


@pytest.mark.parametrize('size', SIZES)
def test_loss_objectives_and_evaluation(size):
    win = window((64, 80), 8000, 3, seed=12)
    H, W = win['sensor_size']
    Theta = win['flow_gt'] * 0.8
    t = SW.objectives(Theta, *win_args(win), window_size=size)
    d = losses.compute_loss_objectives(Theta, *win_args(win), (H, W), warped_events=False, window_size=size)
    per = t['per_ref']
    assert d['zero_contrast'] == pytest.approx(t['zero_contrast'], rel=TOL)
    assert d['zero_iwe_divergence'] == pytest.approx(t['zero_iwe_divergence'], rel=TOL)
    assert rel(d['zero_correlations'], [q['zero_correlation'] for q in per]) <= TOL
    assert rel(d['correlations'], [q['correlation'] for q in per]) <= TOL
    assert rel(d['contrasts'], [q['contrast'] for q in per]) <= TOL
    assert rel(d['iwe_divergences'], [q['divergence'] for q in per]) <= TOL
    assert rel(d['flow_warp_losses'], [q['variance'] / t['zero_variance'] for q in per]) <= TOL
    assert d['theta_total_variation'] == pytest.approx(t['theta_total_variation'], rel=TOL)
    ev, lo = evaluation.evaluate_theta_array(Theta, *win_args(win), None, A, B_, GAMMA, 0.0, (H, W), window_size=size)
    # (theta_eval.py: plain means of the relative terms, no multi-reference weights)
    assert ev['mean_rel_contrast'] == pytest.approx(np.mean([q['contrast'] for q in per]) / t['zero_contrast'], rel=TOL)
    assert ev['mean_rel_corr'] == pytest.approx(np.mean([q['correlation'] / q['zero_correlation'] for q in per]), rel=TOL)
    assert ev['iwe_var'] == pytest.approx(per[0]['variance'], rel=TOL)


def test_sharded_world1_equals_engine():
    sh = importlib.import_module('edge-informed-contrast-maximization_amd.sharding')
    win = window()
    a = win_args(win)
    with engine.Engine((120, 160), 30000, max_refs=3) as e1, engine.Engine((120, 160), 30000, max_refs=3) as e2:
        e1.set_splat_window(5)
        e1.set_window(*a)
        se = sh.ShardedEngine(e2, window_size=5)
        se.set_windows([a])
        for hw in ((1, 1), (4, 4)):
            th = synth.theta_near_truth(11, win, hw)
            p = engine.make_params(A, B_, 0.0, 0.0, 1)
            v1, g1, _ = e1.loss_grad(th, p)
            v2, g2 = se.loss_grad(th, p)
            assert v2[0] == v1[0], hw
            assert np.array_equal(np.asarray(g2).reshape(g1.shape), g1), hw
        with pytest.raises(engine.EincmError) as ei:     # the sharded staging's constants cannot be formed again by one rank
            e2.set_splat_window(3)
        assert ei.value.code == L.ERR_STATE


# ---- 3. bitwise properties and refusals -----------------------------------------------------------------------------------------
def _evaluate(eng, win, hw):
    out = []
    for k, h in enumerate(hw):
        th = synth.theta_near_truth(20 + k, win, h)
        v, g, a = eng.loss_grad(th, engine.make_params(A, B_, GAMMA, 0.0, 0), want_aux=True)
        out.append((v, g, a, eng.iwes(), eng.image_grad()))
    return out


def _same(x, y):
    return all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_aux(a[2], b[2]) and np.array_equal(a[3], b[3])
               and np.array_equal(a[4], b[4]) for a, b in zip(x, y))


def test_even_sizes_equal_odd_sizes_bitwise():
    win = window()
    hw = ((1, 1), (4, 4), (16, 16))
    res = {}
    for s in (2, 3, 4, 5, 6, 7):
        with engine.Engine((120, 160), 30000, max_refs=3) as eng:
            eng.set_splat_window(s)
            eng.set_window(*win_args(win))
            res[s] = _evaluate(eng, win, hw)
    assert _same(res[2], res[3]) and _same(res[4], res[5]) and _same(res[6], res[7])
    assert not np.array_equal(res[5][0][3], res[7][0][3])


def test_repeat_and_switch_bitwise():
    """Repeated evaluations are bit-identical; 3 -> 5 -> 3 on a staged batch returns a fresh context's bits at either size."""
    win = window()
    hw = ((1, 1), (4, 4))
    fresh = {}
    for s in (3, 5):
        with engine.Engine((120, 160), 30000, max_refs=3) as eng:
            eng.set_splat_window(s)
            eng.set_window(*win_args(win))
            fresh[s] = _evaluate(eng, win, hw)
            assert _same(fresh[s], _evaluate(eng, win, hw)), s
    with engine.Engine((120, 160), 30000, max_refs=3) as eng:
        eng.set_window(*win_args(win))
        assert eng.splat_window == 3 and _same(_evaluate(eng, win, hw), fresh[3])
        eng.set_splat_window(5)
        assert eng.splat_window == 5 and _same(_evaluate(eng, win, hw), fresh[5])
        z5 = eng.zero_iwe()
        eng.set_splat_window(3)
        assert _same(_evaluate(eng, win, hw), fresh[3])
        assert not np.array_equal(z5, eng.zero_iwe())
        with pytest.raises(ValueError):
            eng.set_splat_window(8)
        for bad in (0, 8, -1):                 # the C function checks too
            with pytest.raises(engine.EincmError) as ei:
                eng._check(eng._lib.eincm_set_splat_window(eng._ctx, bad))
            assert ei.value.code == L.ERR_ARG
        assert eng.splat_window == 3 and _same(_evaluate(eng, win, hw), fresh[3])


def test_counts_and_warped_events_do_not_depend_on_the_size():
    win = window()
    th = synth.theta_near_truth(3, win, (4, 4))
    out = []
    for s in (1, 3, 7):
        with engine.Engine((120, 160), 30000, max_refs=3) as eng:
            eng.set_splat_window(s)
            eng.set_window(*win_args(win))
            eng.loss_grad(th, engine.make_params(A, B_, 0.0, 0.0, 1))
            out.append((eng.count_images(), eng.warped_events(0)))
    for c, w in out[1:]:
        assert np.array_equal(c, out[0][0]) and all(np.array_equal(a, b) for a, b in zip(w, out[0][1]))


def test_async_in_flight_refuses_a_change():
    win = window()
    th = synth.theta_near_truth(3, win, (1, 1))
    with engine.Engine((120, 160), 30000, max_refs=3) as eng:
        eng.set_window(*win_args(win))
        eng.loss_grad_async(th, engine.make_params(A, B_, 0.0, 0.0, 1))
        with pytest.raises(engine.EincmError) as ei:
            eng.set_splat_window(5)
        assert ei.value.code == L.ERR_STATE
        eng.loss_grad_wait()
        eng.set_splat_window(5)
        assert eng.splat_window == 5


def test_fp64_refuses_other_sizes():
    win = window((48, 64), 4000, 2, seed=13)
    th = synth.theta_near_truth(12, win, (1, 1))
    with engine.Engine((48, 64), 4000, max_refs=2, precision='fp64') as eng:
        eng.set_window(*win_args(win))
        eng.set_splat_window(3)
        for s in (1, 2, 5, 7):
            with pytest.raises(engine.EincmError) as ei:
                eng.set_splat_window(s)
            assert ei.value.code == L.ERR_UNSUPPORTED and 'fp64' in str(ei.value)
        assert eng.splat_window == 3
        eng.loss_grad(th, engine.make_params(A, B_, 0.0, 0.0, 1))


# ---- 4. solver ------------------------------------------------------------------------------------------------------------------
def test_lockstep_solve_size5():
    sol = importlib.import_module('edge-informed-contrast-maximization_amd.solver')
    bsol = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
    H, W, N, R, n_lvls = 96, 128, 12000, 3, 2
    wins = [synth.make_window(80 + b, (H, W), N, R, flow='constant', flow_mag=3.0 + b) for b in range(2)]
    loss = dict(alpha=A, beta=B_, gamma=0.0, delta=0.0, scale_to_sensor_size_method='bilinear', window_size=5)
    bs = bsol.BatchedMultipleLevelEINCMSolver(
        2, (H, W), n_lvls, sol.growing_maxiters(n_lvls, 3, 12), loss,
        {'method': 'BFGS', 'options': {'gtol': 1e-7}, 'n_extra_attempts': {'pyr_lvl_0': 0, 'pyr_lvl_1': 0}},
        handover_opt_maxiters=sol.growing_maxiters(n_lvls, 4, 20), handover_opt_solver_params={'method': 'L-BFGS-B', 'options': {'gtol': 1e-6}},
        handover_settings=None, pyramid_downscale_method='lanczos3', pyramid_upscale_method='repeat', pyramid_bases=[2])
    bs.set_datasamples([win_args(w) for w in wins])
    assert all(e.splat_window == 5 for e in bs.engines)
    out = bs.solve()
    bs.close()
    for b in range(2):
        for k in range(n_lvls):
            key = f'pyr_lvl_{k}'
            fv = out[b]['theta_opt_state_pyr'][key].fun_val
            start = out[b]['pre_opt_theta_pyr'][key]
            (v0, _), _ = losses.value_and_grad_loss_func(start, *win_args(wins[b]), A, B_, 0.0, 0.0, k, n_lvls, (H, W), window_size=5)
            assert np.isfinite(fv) and np.all(np.isfinite(out[b]['final_theta_pyr'][key])), (b, key)
            assert fv <= v0 + 1e-9 * abs(v0), (b, key, fv, v0)
