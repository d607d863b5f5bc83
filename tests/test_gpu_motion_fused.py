"""The fused evaluation of a motion model on the GPU: k_splat and k_gather in their polynomial theta mode, with
no Theta image and no dense gradient during the evaluation.

Against the expanded path of the same build: value and IWE stack bit for bit (integer accumulation: a tap does not depend on the LDS
window it landed in), also with delta != 0 and the tiled objective kinds.  Gradient: against the exact moments (math.fsum) of the
dense gradient of the same build on the witness's field, within the bound of the summation scheme built (``moment_bound``), and
against the fp64 oracle at the project's tolerances (1e-5; the 7-event case 1e-4).  Then determinism, masking, a context shared with
the other theta modes, the accessors, every refusal and a lockstep solve.  Batches are three windows with the middle one masked unless
a test says otherwise; scenes and coefficients: tests/_motion_cases.py."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

from oracle import eincm_oracle as O
import _motion_cases as MC
from _motion_bounds import moment_bound, slots_per_window
import _splat_window_witness as SW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
engine = importlib.import_module(pkg + '.engine')
motion = importlib.import_module(pkg + '.motion')
bs = importlib.import_module(pkg + '.batch_solver')
synth = importlib.import_module(pkg + '.synth')
L = importlib.import_module(pkg + '._lib')

A, B_ = 20.0, 35.0
MASK = np.array([1, 0, 1], dtype=np.uint8)
ON = [0, 2]
# sensor size -> events per window: one partial tile (wide) / four tiles, three partial / six full tiles / a tile of two gather segments
SHAPES = {(5, 7): 7, (37, 53): 4000, (64, 96): 20000, (32, 40): 40000}


@pytest.fixture(scope='module', autouse=True)
def _lib(built_lib):
    return built_lib


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def open_engine(model, wins, window_size=None, **kw):
    H, W = model.sensor_size
    eng = engine.Engine((H, W), max(sum(len(w['xs']) for w in wins), 1), max_refs=len(wins[0]['edge_ts']), max_windows=len(wins), **kw)
    if window_size is not None:
        eng.set_splat_window(window_size)
    eng.set_windows([MC.win_args(w) for w in wins])
    eng.set_motion_model(model)
    return eng


def lgm(eng, coeffs, p, path='expanded', **kw):
    """loss_grad_motion by `path` (the engine's setting, Engine.set_motion_path)."""
    eng.set_motion_path(path)
    return eng.loss_grad_motion(coeffs, p, **kw)


def params(gamma=0.0, delta=0.0, lvl=1, ck=0, rk=0, full_aux=False):
    return engine.make_params(A, B_, gamma, delta, lvl, 'bilinear', ck, full_aux=full_aux, correlation_kind=rk)


# ---- the bound of the fused gradient: tests/_motion_bounds.py (shared with the motion sweep of tests/dev/fuzz_gpu.py) ----


# ---- 1. against the expanded path and the dense path of the same build ----
#            name -> (kind, shape, R, params keywords)
SAME_BUILD = {
    'poly2-5x7-wide': ('polynomial2', (5, 7), 3, {}),
    'zoom-37x53': ('zoom', (37, 53), 3, {}),
    'translation-37x53': ('translation', (37, 53), 3, {}),
    'similarity-37x53-divergence': ('similarity', (37, 53), 3, dict(delta=0.5)),
    'affine-64x96': ('affine', (64, 96), 3, {}),
    'rotation-64x96-tiled-kinds': ('rotation', (64, 96), 3, dict(ck=3, rk=2)),
    'quadratic-32x40-two-segments': ('quadratic', (32, 40), 3, {}),
    'poly2-32x40-one-reference-time': ('polynomial2', (32, 40), 1, {}),
}


@pytest.mark.parametrize('name', sorted(SAME_BUILD))
def test_equals_the_expanded_and_the_dense_path(name):
    kind, shape, R, kw = SAME_BUILD[name]
    model, wins, c = MC.batch(kind, shape, SHAPES[shape], R=R)
    p = params(**kw)
    slots, all_r = slots_per_window(wins, shape, R)
    with open_engine(model, wins) as eng:
        ve, ge, _ = lgm(eng, c, p, active=MASK)
        iwe_e = eng.iwes()
        vf, gf, aux = lgm(eng, c, p, active=MASK, path='fused', want_aux=True)
        iwe_f = eng.iwes()
        v0, g0, _ = lgm(eng, c, p, active=MASK, path='fused', want_grad=False)
        v0e, _, _ = lgm(eng, c, p, active=MASK, want_grad=False)
        vd, gd, _ = eng.loss_grad_device(torch.from_numpy(model.field(c)).cuda(), p, theta_abs_max=model.abs_bound(c))
    gd = gd.cpu().numpy()
    assert not all_r and (min(len(w['xs']) for w in wins) * R < 4096) == (shape == (5, 7))     # the instantiation this case reaches
    assert np.isnan(vf[1]) and np.array_equal(gf[1], np.zeros(model.n_coeffs)) and np.isnan(aux[1]['final_loss'])
    assert np.array_equal(vf[ON], ve[ON]) and np.array_equal(vf[ON], vd[ON]), (vf, ve, vd)
    assert all(aux[b]['final_loss'] == vf[b] for b in ON)
    assert np.array_equal(iwe_f[ON], iwe_e[ON])
    assert g0 is None and np.array_equal(v0[ON], v0e[ON])            # forward only: the same image passes as the expanded path's
    want, bound = moment_bound(model, gd, slots)
    err = np.abs(gf - want)[ON]
    print(f'{name}: |fused gradient - exact moments M| / bound = {(err / bound[ON]).max():.4f}; max-norm rel to the exact moments '
          f'{rel(gf[ON], want[ON]):.2e}, to the expanded path {rel(gf[ON], ge[ON]):.2e}; slots per window {slots.tolist()}')
    assert np.all(np.abs(want[ON]).max(axis=1) > 0.0)
    assert np.all(err <= bound[ON]), (err, bound[ON])


def test_more_windows_than_ride_in_the_arguments():
    """65 windows: q of up to 10 rides in the event kernels' arguments, beyond that they read it from pinned host memory.  The batch
    repeats three windows, so every window must give the bits of its first copy - value and gradient."""
    model, wins, c = MC.batch('polynomial2', (5, 7), 7)
    idx = np.arange(65) % 3
    with open_engine(model, wins) as eng:
        v3, g3, _ = lgm(eng, c, params(), path='fused')
    with open_engine(model, [wins[i] for i in idx]) as eng:
        v, g, _ = lgm(eng, c[idx], params(), path='fused')
        ve, _, _ = lgm(eng, c[idx], params())
        T = eng.scaled_theta()
    assert np.array_equal(v, v3[idx]) and np.array_equal(g, g3[idx]) and np.all(np.isfinite(v)) and np.array_equal(v, ve)
    assert np.array_equal(T, model.field(c[idx]))


@pytest.mark.parametrize('sparse', [False, True])
def test_one_workgroup_for_all_reference_times(sparse):
    """180 windows of four tiles: 720 segments, so one gather workgroup per segment walks all reference times (a slot per segment).
    With one window of seven events the staging is `wide` (61-bit sums) and still has 700 segments and more."""
    model, wins, c = MC.batch('affine', (37, 53), 4000)
    few = synth.make_window(9, (37, 53), 7, 3, flow=model.field(MC.true_of('affine', (37, 53), 4000)))
    idx = np.arange(180) % 3
    batch = [wins[i] for i in idx]
    cb = c[idx].copy()
    if sparse:
        batch[5] = few
    slots, all_r = slots_per_window(batch, (37, 53), 3)
    assert all_r and slots.sum() >= 700 and (min(len(w['xs']) for w in batch) * 3 < 4096) == sparse
    p = params()
    with open_engine(model, batch) as eng:
        vf, gf, _ = lgm(eng, cb, p, path='fused')
        vf2, gf2, _ = lgm(eng, cb, p, path='fused')
        ve, ge, _ = lgm(eng, cb, p)
        _, gd, _ = eng.loss_grad_device(torch.from_numpy(model.field(cb)).cuda(), p, theta_abs_max=model.abs_bound(cb))
    assert np.array_equal(vf, ve) and np.array_equal(vf, vf2) and np.array_equal(gf, gf2) and np.all(np.isfinite(vf))
    want, bound = moment_bound(model, gd.cpu().numpy(), slots)
    err = np.abs(gf - want)
    print(f'all reference times, 180 windows (sparse={sparse}): |fused gradient - exact moments M| / bound = {(err / bound).max():.4f}; '
          f'against the expanded gradient, max-norm rel {rel(gf, ge):.2e}')
    assert np.all(err <= bound)


# ---- 2. against the oracle ----
ORACLE_CASES = {                        # name -> (kind, shape, R, params keywords, tolerance)
    'translation': ('translation', (37, 53), 3, {}, 1e-5),
    'affine': ('affine', (64, 96), 3, {}, 1e-5),
    'rotation': ('rotation', (37, 53), 3, {}, 1e-5),
    'quadratic': ('quadratic', (37, 53), 3, {}, 1e-5),
    'divergence': ('rotation', (37, 53), 3, dict(delta=0.5), 1e-5),
    'tiled-kinds': ('similarity', (64, 96), 3, dict(ck=3, rk=2), 1e-5),
    'two-segments': ('quadratic', (32, 40), 3, {}, 1e-5),
    'seven-events': ('affine', (5, 7), 3, {}, 1e-4),
}
_REF = {}


def oracle_reference(name):
    """(value, dL/dc) of the case's active windows by the fp64 oracle on model.field(c), projected by the witness; computed once.  The
    tiled objective kinds are outside oracle.eincm_oracle: there the fp64 autograd witness of those kinds takes its place."""
    if name not in _REF:
        kind, shape, R, kw, _ = ORACLE_CASES[name]
        model, wins, c = MC.batch(kind, shape, SHAPES[shape], R=R)
        out = {}
        for b in ON:
            F = model.field(c[b])
            if kw.get('ck', 0) or kw.get('rk', 0):
                v, g = SW.loss_and_grad(F, *MC.win_args(wins[b]), A, B_, 0.0, kw.get('delta', 0.0), 1, np.eye(shape[0]), np.eye(shape[1]),
                                        window_size=3, contrast_kind=kw.get('ck', 0), correlation_kind=kw.get('rk', 0), tile=(32, 42))[:2]
            else:
                v, g, _ = O.loss_and_grad(F, *MC.win_args(wins[b]), A, B_, 0.0, kw.get('delta', 0.0), 1, 5, shape, 'bilinear')
            out[b] = (v, model.project(g))
        _REF[name] = out
    return _REF[name]


@pytest.mark.parametrize('name', sorted(ORACLE_CASES))
def test_against_the_oracle(name):
    kind, shape, R, kw, tol = ORACLE_CASES[name]
    model, wins, c = MC.batch(kind, shape, SHAPES[shape], R=R)
    ref = oracle_reference(name)
    with open_engine(model, wins) as eng:
        v, g, _ = lgm(eng, c, params(**kw), active=MASK, path='fused')
    ev = max(abs(v[b] - ref[b][0]) / abs(ref[b][0]) for b in ref)
    eg = max(rel(g[b], ref[b][1]) for b in ref)
    print(f'{name}: {kind} {shape} value rel {ev:.2e}, gradient max-norm rel {eg:.2e}')
    assert ev <= tol and eg <= tol, (name, ev, eg)


# ---- 3. determinism, masking, a shared context ----
@pytest.mark.parametrize('kind,shape', [('affine', (37, 53)), ('polynomial2', (32, 40)), ('zoom', (5, 7))])
def test_same_bits_on_every_call_and_in_every_context(kind, shape):
    model, wins, c = MC.batch(kind, shape, SHAPES[shape])
    p = params()
    with open_engine(model, wins) as eng:
        v1, g1, _ = lgm(eng, c, p, path='fused')
        v2, g2, _ = lgm(eng, c, p, path='fused')
        vm, gm, _ = lgm(eng, c, p, active=MASK, path='fused')
        garbage = c.copy()
        garbage[1] = np.nan                                       # the coefficients of a masked window are not read
        vn, gn, _ = lgm(eng, garbage, p, active=MASK, allow_nonfinite=False, path='fused')
        va, ga, _ = lgm(eng, c, p, path='auto')
    with open_engine(model, wins) as eng:
        v3, g3, _ = lgm(eng, c, p, path='fused')
    assert np.all(np.isfinite(v1)) and np.all(np.abs(g1).max(axis=1) > 0.0)
    assert np.array_equal(v1, v2) and np.array_equal(g1, g2) and np.array_equal(v1, v3) and np.array_equal(g1, g3)
    assert np.isnan(vm[1]) and np.array_equal(gm[1], np.zeros(model.n_coeffs))
    assert np.array_equal(vm[ON], v1[ON]) and np.array_equal(gm[ON], g1[ON])
    assert np.array_equal(vn, vm, equal_nan=True) and np.array_equal(gn, gm)
    assert np.array_equal(va, v1)                                 # 'auto' takes one of the two paths: the value is the same bits


def test_a_context_shared_with_the_other_theta_modes():
    """fused, a theta-grid loss_grad, a 2-DoF loss_grad, a dense loss_grad_device, fused again on one context: each result equals the
    bits that evaluation gives on a fresh context, so no accumulator, ticket or table is left dirty or stale by any of them."""
    model, wins, c = MC.batch('affine', (37, 53), 4000)
    p = params()
    rng = np.random.default_rng(3)
    th44, th11 = rng.normal(size=(3, 4, 4, 2)) * 3.0, rng.normal(size=(3, 1, 1, 2)) * 3.0
    dense = model.field(c)

    def steps(eng):
        return {'fused': lambda: lgm(eng, c, p, active=MASK, path='fused')[:2],
                'grid': lambda: eng.loss_grad(th44, p)[:2],
                'two_dof': lambda: eng.loss_grad(th11, p)[:2],
                'dense': lambda: tuple(np.asarray(x.cpu() if torch.is_tensor(x) else x)
                                       for x in eng.loss_grad_device(torch.from_numpy(dense).cuda(), p, theta_abs_max=model.abs_bound(c))[:2])}
    fresh = {}
    for k in ('fused', 'grid', 'two_dof', 'dense'):
        with open_engine(model, wins) as eng:
            fresh[k] = steps(eng)[k]()
    with open_engine(model, wins) as eng:
        s = steps(eng)
        for k in ('fused', 'grid', 'two_dof', 'dense', 'fused', 'dense', 'fused', 'two_dof', 'fused', 'grid', 'fused'):
            v, g = s[k]()
            assert np.array_equal(v, fresh[k][0], equal_nan=True) and np.array_equal(g, fresh[k][1]), k


# ---- 4. the accessors ----
def test_accessors_build_the_field_from_the_evaluations_q():
    model, wins, c = MC.batch('quadratic', (37, 53), 4000)
    p = params()
    with open_engine(model, wins) as eng:
        lgm(eng, c, p)
        T_e, W_e, N_e = eng.scaled_theta(), [eng.warped_events(b) for b in range(3)], eng.count_images()
        lgm(eng, c, p, path='fused')
        T_f, W_f, N_f = eng.scaled_theta(), [eng.warped_events(b) for b in range(3)], eng.count_images()
        eng.loss_grad(np.ones((3, 1, 1, 2)), p)                   # another evaluation's theta in between ...
        lgm(eng, c, p, path='fused')
        W_2 = eng.warped_events(1)                                # ... and an accessor other than scaled_theta asked first
        T_2 = eng.scaled_theta()
    assert np.array_equal(T_f, model.field(c)) and np.array_equal(T_f, T_e) and np.array_equal(T_2, T_e)
    for b in range(3):
        assert all(np.array_equal(a, e) for a, e in zip(W_f[b], W_e[b]))
    assert all(np.array_equal(a, e) for a, e in zip(W_2, W_e[1]))
    assert np.array_equal(N_f, N_e) and N_f.sum() > 0


# ---- 5. refusals ----
def test_refusals():
    model, wins, c = MC.batch('affine', (37, 53), 4000)
    H, W = model.sensor_size
    theta = np.zeros((3, 1, 1, 2))
    val, grd = np.empty(3), np.empty((3, 6))

    def refused(eng, code, word, p):
        rc = eng._lib.eincm_loss_grad_motion_fused(eng._ctx, c.ctypes.data, C.byref(p), None, val.ctypes.data, grd.ctypes.data, None)
        msg = eng._lib.eincm_last_error(eng._ctx).decode()
        assert rc == code and 'eincm_loss_grad_motion_fused' in msg and word in msg, (rc, msg)

    def plain_ok(eng):
        v, g, _ = eng.loss_grad(theta, params())
        assert np.all(np.isfinite(v)) and g.shape == theta.shape

    def auto_is_expanded(eng, p):
        va, ga, _ = lgm(eng, c, p, path='auto')
        ve, ge, _ = lgm(eng, c, p)
        assert np.array_equal(va, ve) and np.array_equal(ga, ge) and np.all(np.isfinite(va))

    with open_engine(model, wins) as eng:
        v0, g0, _ = lgm(eng, c, params(), path='fused')
        # EINCM_ERR_UNSUPPORTED: the TV term active, the full aux
        for p, word in ((params(gamma=2.5e-3, lvl=0), 'TV term'), (params(full_aux=True), 'EINCM_PF_FULL_AUX')):
            refused(eng, L.ERR_UNSUPPORTED, word, p)
            with pytest.raises(ValueError):
                lgm(eng, c, p, path='fused')
            auto_is_expanded(eng, p)
            plain_ok(eng)
        # ... a null pointer
        rc = eng._lib.eincm_loss_grad_motion_fused(eng._ctx, None, C.byref(params()), None, val.ctypes.data, None, None)
        assert rc == L.ERR_ARG and eng._lib.eincm_last_error(eng._ctx).decode()
        plain_ok(eng)
        # EINCM_ERR_STATE: eincm_set_device_results on, an evaluation in flight, no model set
        eng.set_device_results(True)
        refused(eng, L.ERR_STATE, 'eincm_set_device_results', params())
        eng.set_device_results(False)
        plain_ok(eng)
        eng.loss_grad_async(theta, params())
        refused(eng, L.ERR_STATE, 'in flight', params())
        assert np.all(np.isfinite(eng.loss_grad_wait()[0]))
        plain_ok(eng)
        eng.set_motion_model(None)
        refused(eng, L.ERR_STATE, 'no motion model', params())
        for path in ('fused', 'auto'):
            with pytest.raises(ValueError, match='no motion model'):
                lgm(eng, c, params(), path=path)
        plain_ok(eng)
        eng.set_motion_model(model)
        v1, g1, _ = lgm(eng, c, params(), path='fused')
        assert np.array_equal(v1, v0) and np.array_equal(g1, g0)
    # ... another splat window
    with open_engine(model, wins, window_size=5) as eng:
        refused(eng, L.ERR_UNSUPPORTED, '3x3 splat window', params())
        with pytest.raises(ValueError, match='3x3 splat window'):
            lgm(eng, c, params(), path='fused')
        auto_is_expanded(eng, params())
        plain_ok(eng)
    # ... a float64 context (the expanded path does not exist there either: 'auto' gives its refusal)
    with engine.Engine((H, W), 3 * 4000, max_refs=3, max_windows=3, precision='fp64') as eng:
        eng.set_windows([MC.win_args(w) for w in wins])
        eng.set_motion_model(model)
        refused(eng, L.ERR_UNSUPPORTED, 'fp64', params())
        with pytest.raises(ValueError, match='fp64'):
            lgm(eng, c, params(), path='fused')
        with pytest.raises(engine.EincmError):
            lgm(eng, c, params(), path='auto')
        plain_ok(eng)
    # ... no staged windows
    with engine.Engine((H, W), 4000, max_refs=3, max_windows=3) as eng:
        eng.set_motion_model(model)
        refused(eng, L.ERR_STATE, 'eincm_set_windows', params())


def test_nonfinite_coefficients_are_reported():
    model, wins, c = MC.batch('affine', (37, 53), 4000)
    bad = c.copy()
    bad[2, 3] = np.nan
    huge, over = c.copy(), c.copy()
    huge[0, 0] = 1e308                                            # finite, with a finite bound: evaluated, every tap of the window dropped
    over[0, 0] = over[0, 2] = 1.7e308                             # finite coefficients whose field's bound is not: treated as a NaN is
    with open_engine(model, wins) as eng:
        v0, g0, _ = lgm(eng, c, params(), path='fused', allow_nonfinite=False)
        v, g, aux = lgm(eng, bad, params(), path='fused', want_aux=True)     # (allow_nonfinite: the outputs are written)
        assert np.isnan(v[2]) and np.isnan(g[2]).all() and np.isnan(aux[2]['final_loss'])
        assert np.array_equal(v[:2], v0[:2]) and np.array_equal(g[:2], g0[:2])
        with pytest.raises(engine.NonFiniteLoss):
            lgm(eng, bad, params(), path='fused', allow_nonfinite=False)
        vo, go, _ = lgm(eng, over, params(), path='fused')
        assert np.isnan(vo[0]) and np.isnan(go[0]).all() and np.array_equal(vo[1:], v0[1:]) and np.array_equal(go[1:], g0[1:])
        vh, gh, _ = lgm(eng, huge, params(), path='fused')
        vhe, _, _ = lgm(eng, huge, params())
        assert np.all(np.isfinite(vh)) and np.array_equal(vh, vhe) and np.array_equal(vh[1:], v0[1:]) and np.array_equal(gh[1:], g0[1:])
        v2, g2, _ = lgm(eng, c, params(), path='fused', allow_nonfinite=False)
        assert np.array_equal(v2, v0) and np.array_equal(g2, g0)


def test_a_large_finite_field_takes_the_clamped_path():
    """Coefficients that throw most events out of every LDS window and many off the sensor: the windows are clamped to their capacity
    and the taps outside them go to HBM, so value and IWE stack still equal the expanded path's."""
    model, wins, c = MC.batch('affine', (64, 96), 20000)
    big = c * np.array([40.0, -30.0, 25.0, 1.0, 1.0, -20.0])
    with open_engine(model, wins) as eng:
        ve, ge, _ = lgm(eng, big, params())
        iwe_e = eng.iwes()
        vf, gf, _ = lgm(eng, big, params(), path='fused')
        iwe_f = eng.iwes()
        _, gd, _ = eng.loss_grad_device(torch.from_numpy(model.field(big)).cuda(), params(), theta_abs_max=model.abs_bound(big))
    assert np.abs(model.field(big)).max() > 100.0
    assert np.array_equal(vf, ve) and np.array_equal(iwe_f, iwe_e) and np.all(np.isfinite(vf))
    want, bound = moment_bound(model, gd.cpu().numpy(), slots_per_window(wins, (64, 96), 3)[0])
    err = np.abs(gf - want)
    print(f'large field: |fused gradient - exact moments M| / bound = {(err / bound).max():.4f}; against the expanded gradient {rel(gf, ge):.2e}')
    assert np.all(err <= bound)


def test_the_loss_callables_by_path():
    """losses.motion_loss_funcs(path): the pair of callables on another path, the arguments of the module's own pair."""
    losses = importlib.import_module(pkg + '.losses')
    model, wins, c = MC.batch('affine', (37, 53), 4000)
    w = wins[0]
    args = (*MC.win_args(w), A, B_, 0.0, 0.0, 1, 5, model.sensor_size)
    (v_e, _), g_e = losses.value_and_grad_motion_loss_func(c[0], *args, model=model)
    f_fused, vg_fused = losses.motion_loss_funcs('fused')
    f_auto, vg_auto = losses.motion_loss_funcs('auto')
    (v_f, _), g_f = vg_fused(c[0], *args, model=model)
    (v_a, _), g_a = vg_auto(c[0], *args, model=model)
    (v_e2, _), g_e2 = losses.value_and_grad_motion_loss_func(c[0], *args, model=model)      # the module's own pair stays expanded
    with open_engine(model, wins[:1]) as eng:
        v_d, g_d, _ = lgm(eng, c[:1], params(), path='fused')
    assert v_f == v_e == v_a == v_e2 == v_d[0] and np.array_equal(g_f, g_d[0]) and np.array_equal(g_e2, g_e)
    assert np.array_equal(g_a, g_f if engine.motion_auto_takes_fused(1, 4000, 3) else g_e)
    with pytest.raises(ValueError, match='full_aux'):              # forward only evaluates every aux entry: the Theta image is needed
        f_fused(c[0], *args, model=model)
    assert f_auto(c[0], *args, model=model)[0] == losses.motion_loss_func(c[0], *args, model=model)[0]
    losses.clear_engine_cache()


# ---- 6. a solve ----
def test_lockstep_solve_on_the_fused_path():
    """Three windows whose flow is an affine field, from c = 0: minimize_motion on an engine set to the fused path in lockstep walks the iterates of three
    sequential SciPy BFGS runs over the same fused callable on single-window engines, ends below the starting loss, and ends where the
    expanded-path solve ends (tests/test_gpu_batch_solver.py's tolerances: objective 1e-4 relative, field 0.05 px)."""
    H, W, N, R = 64, 96, 8000, 3
    model = motion.MotionModel('affine', (H, W))
    rng = np.random.default_rng(42)
    c_true = rng.uniform(0.4, 1.0, (3, 6)) * rng.choice([-1.0, 1.0], (3, 6)) * np.array([3.0, 3.0, 2.0, 2.0, 2.0, 2.0])
    wins = [synth.make_window(70 + b, (H, W), N, R, flow=model.field(c_true[b])) for b in range(3)]
    p = params()
    maxiter, gtol = 30, 1e-5
    with open_engine(model, wins) as eng:
        v0, _, _ = lgm(eng, np.zeros((3, 6)), p, path='fused')
        eng.set_motion_path('fused')
        res = bs.minimize_motion(eng, model, np.zeros((3, 6)), p, maxiter, gtol)
        eng.set_motion_path('expanded')
        exp = bs.minimize_motion(eng, model, np.zeros((3, 6)), p, maxiter, gtol)
    for b in range(3):
        with open_engine(model, wins[b:b + 1]) as eng:
            def fun(x):
                v, g, _ = lgm(eng, x, p, path='fused')
                return float(v[0]), g[0]
            seq = minimize(fun, np.zeros(6), jac=True, method='BFGS', options={'maxiter': maxiter, 'gtol': gtol})
        d_seq = np.abs(model.field(res[b].x) - model.field(seq.x)).max()
        d_exp = np.abs(model.field(res[b].x) - model.field(exp[b].x)).max()
        print(f'window {b}: start {v0[b]:.6f} fused lockstep {res[b].fun:.6f} ({res[b].nit} it) sequential {seq.fun:.6f} ({seq.nit} it) '
              f'expanded {exp[b].fun:.6f} ({exp[b].nit} it); field difference to sequential {d_seq:.2e} px, to expanded {d_exp:.2e} px')
        assert np.array_equal(res[b].x, seq.x) and res[b].nit == seq.nit and res[b].fun == seq.fun, b
        assert res[b].fun < v0[b], b
        assert res[b].fun == pytest.approx(exp[b].fun, rel=1e-4) and d_exp < 0.05, (b, d_exp)
