"""The per-event scores on the GPU against the numpy float64 witness tests/_event_scores_witness.py.

Tolerance: |gpu - witness| <= 1e-5 * M per output cell, M = sum_d k |F| the witness's magnitude of the cell (sum_d k^2 for selfs; each
weighted by |omega_r| in the combined form): the project's standing fp32 bar (DESIGN.md sections 2 and 6, the IWE's own bound).  F is
what the GPU itself holds - Engine.iwes() for the IWE source, the caller's stack otherwise - and the witness warps with
Engine.scaled_theta(), fetched AFTER the scores so that the call builds the Theta image itself where the evaluation left none.  Cells
with M == 0 must be exactly 0.  tests/test_event_scores_interface.py asserts on the CPU that every generated case has wrapped and
dropped taps, mostly positive scores and a theta that matters, so a kernel that ignores any of them fails here.

The launch does not cap its grid (one thread per event, grid x = ceil(max_b n_b / 256)), so there is no case beyond a cap.  Every test
runs under its own time limit; the largest ratio |gpu - witness| / M of the session is printed when the module ends."""
import ctypes as C
import importlib
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import _event_scores_witness as ES
import _motion_cases as MC
from oracle import eincm_oracle as O

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
staging = importlib.import_module(pkg + '.staging')
evaluation = importlib.import_module(pkg + '.evaluation')
losses = importlib.import_module(pkg + '.losses')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 30
P = E.make_params(20.0, 35.0, 2.5e-4, 0.0, 1)
_engines = {}
_worst = {'ratio': 0.0, 'where': ''}


def _eng(shape, precision='fp32'):
    key = (tuple(shape), precision)
    if key not in _engines:
        _engines[key] = E.Engine(tuple(shape), max_events_total=16384, max_refs=3, max_windows=3, precision=precision)
    return _engines[key]


@pytest.fixture(scope='module', autouse=True)
def _close_engines(built_lib):
    yield
    for e in _engines.values():
        e.close()
    _engines.clear()
    print(f"\nevent scores: largest |gpu - witness| / M = {_worst['ratio']:.3e} ({_worst['where']})")


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError(f'test exceeded {TIME_LIMIT_S} s')
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TIME_LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


SENTINEL = np.float32(-777.0)


def _raw(eng, images=None, ref_weights=None, want_selfs=True):
    """The library call itself: (rc, [scores per window], [selfs per window] | None), arrays pre-filled with a sentinel"""
    off, length, total = E.event_scores_layout(eng.n_events, eng.R, ref_weights is not None)
    scores = np.full(total + 1, SENTINEL, dtype=np.float32)                    # (one cell more: nothing is written past the end)
    selfs = np.full(total + 1, SENTINEL, dtype=np.float32) if want_selfs else None
    img = None if images is None else np.ascontiguousarray(images, dtype=np.float32)
    rw = None if ref_weights is None else np.ascontiguousarray(ref_weights, dtype=np.float64)
    rc = eng._lib.eincm_event_scores(eng._ctx, None if img is None else img.ctypes.data, None if rw is None else rw.ctypes.data,
                                     scores.ctypes.data, None if selfs is None else selfs.ctypes.data)

    def split(a):
        assert a[total] == SENTINEL
        shape = (lambda n: (n,)) if ref_weights is not None else (lambda n: (eng.R, n))
        return [a[off[b]:off[b] + length[b]].reshape(shape(int(eng.n_events[b]))) for b in range(eng.B)]
    return rc, split(scores), (split(selfs) if want_selfs else None), scores, selfs


def _close(got, ref, M, what):
    ok, ratio = ES.within(got, ref, M)
    if ratio > _worst['ratio']:
        _worst.update(ratio=ratio, where=what)
    print(f'{what}: largest |gpu - witness| / M = {ratio:.3e}')
    assert ok, f'{what}: ratio {ratio:.3e} > {ES.TOL}, or a cell with M == 0 is not 0'


def _check_batch(eng, wins, stack, what, forms=(None, 'omega')):
    """Every form of the call on the staged and evaluated batch `wins` (dicts with xs, ys, ts, edge_ts) against the witness.
    stack None: the IWE source."""
    R = eng.R
    omega = np.linspace(-0.5, 1.0, R) if R > 1 else np.array([0.75])
    out = {}
    for form in forms:
        rw = None if form is None else omega
        rc, s, q, flat_s, flat_q = _raw(eng, stack, rw, True)
        assert rc == L.OK, eng._lib.eincm_last_error(eng._ctx).decode()
        rc2, s2, _, flat_s2, _ = _raw(eng, stack, rw, False)                   # selfs not requested: the same scores
        rc3, _, _, flat_s3, flat_q3 = _raw(eng, stack, rw, True)               # a call repeated: the same bytes
        assert rc2 == L.OK and rc3 == L.OK
        assert flat_s2.tobytes() == flat_s.tobytes() and flat_s3.tobytes() == flat_s.tobytes() and flat_q3.tobytes() == flat_q.tobytes()
        out[form] = (s, q)
    Theta = eng.scaled_theta()
    F = eng.iwes() if stack is None else np.asarray(stack, dtype=np.float32).reshape(eng.B, R, eng.H, eng.W)
    for form, (s, q) in out.items():
        rw = None if form is None else omega
        for b, w in enumerate(wins):
            ref = ES.event_scores(F[b], Theta[b], w['xs'], w['ys'], w['ts'], w['edge_ts'], rw)
            assert s[b].dtype == np.float32 and s[b].shape == ref['scores'].shape
            _close(s[b], ref['scores'], ref['M'], f'{what} window {b} {"combined" if form else "per-r"} scores')
            _close(q[b], ref['selfs'], ref['M_self'], f'{what} window {b} {"combined" if form else "per-r"} selfs')
    return out


# ---- every generated case: both sources, both forms, selfs asked for and not, a call repeated ------------------------------------
@pytest.mark.parametrize('source', ['iwe', 'stack'])
@pytest.mark.parametrize('name', sorted(ES.GENERATED))
def test_generated_case_is_the_witness_in_every_form(name, source):
    c = ES.generated(name)
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    eng.loss_grad(c['theta'], P, want_grad=False)
    out = _check_batch(eng, [c], None if source == 'iwe' else c['stack'], f'{name} {source}')
    # the Python layer hands out the same bytes, shaped
    got = eng.event_scores(images=None if source == 'iwe' else c['stack'])
    assert len(got) == 1 and got[0].dtype == np.float32 and got[0].tobytes() == out[None][0][0].tobytes()
    if source == 'stack':
        assert eng.event_scores(images=c['stack'][None])[0].tobytes() == got[0].tobytes()      # (B,R,H,W) and (R,H,W) alike


def test_batch_of_three_windows_the_middle_one_empty():
    a, b = ES.generated('60x80-dense-r3'), ES.generated('60x80-n65')
    empty = dict(xs=np.zeros(0, np.int16), ys=np.zeros(0, np.int16), ts=np.zeros(0), edges=a['edges'], edge_ts=a['edge_ts'])
    wins = [a, empty, b]
    eng = _eng((60, 80))
    eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
    theta = np.stack([a['theta'], np.zeros_like(a['theta']), b['theta']])
    eng.loss_grad(theta, P, want_grad=False)
    rng = np.random.default_rng(5)
    stack = rng.uniform(-0.5, 1.0, (3, 3, 60, 80)).astype(np.float32)
    for st, what in ((None, 'batch iwe'), (stack, 'batch stack')):
        out = _check_batch(eng, wins, st, what)
        assert out[None][0][1].shape == (3, 0) and out['omega'][0][1].shape == (0,)
    got = eng.event_scores(ref_weights=[0.25, 0.5, 0.25], exclude_self=True)
    assert [g.shape for g in got] == [(700,), (0,), (65,)]
    with pytest.raises(ValueError, match='images must be'):
        eng.event_scores(images=stack[0])                                                   # (R,H,W) stands for a batch of one only


def test_a_batch_without_events_is_valid_and_writes_nothing():
    a = ES.generated('60x80-dense-r3')
    z = (np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0), a['edges'], a['edge_ts'])
    eng = _eng((60, 80))
    eng.set_windows([z, z])
    eng.loss_grad(np.zeros((2, 1, 1, 2)), P, want_grad=False)
    rc, s, q, flat_s, flat_q = _raw(eng, None, None, True)
    assert rc == L.OK and [x.shape for x in s] == [(3, 0), (3, 0)] and flat_s[0] == SENTINEL and flat_q[0] == SENTINEL
    assert [g.shape for g in eng.event_scores(ref_weights=[1, 1, 1])] == [(0,), (0,)]


# ---- the borders: a wrap on one side, a drop on the other -------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(33, 65), (60, 80)], ids=['33x65', '60x80'])
def test_events_on_the_outermost_rows_and_columns_moved_one_and_two_pixels(shape):
    H, W = shape
    rng = np.random.default_rng(3)
    n = 4 * 40
    xs = np.concatenate([np.zeros(40), np.full(40, W - 1), rng.integers(0, W, 80)]).astype(np.int16)
    ys = np.concatenate([rng.integers(0, H, 80), np.zeros(40), np.full(40, H - 1)]).astype(np.int16)
    ts = np.full(n, 0.5) + np.arange(n) * 1e-9
    edge_ts = np.array([0.0])
    w = dict(xs=xs, ys=ys, ts=ts, edge_ts=edge_ts)
    eng = _eng(shape)
    eng.set_window(xs, ys, ts, rng.uniform(0, 1, (1, H, W)), edge_ts)
    stack = rng.uniform(-0.5, 1.0, (1, 1, H, W)).astype(np.float32)
    seen_wrap = seen_drop = False
    for vx, vy in ((2.0, 2.0), (-2.0, 4.0), (4.0, -2.0), (-4.0, -4.0), (2.5, -3.5)):         # displacements of -+1, -+2 px (and between)
        eng.loss_grad(np.array([[[[vx, vy]]]]), P, want_grad=False)
        for st in (None, stack):
            _check_batch(eng, [w], st, f'border {shape} v=({vx},{vy}) {"iwe" if st is None else "stack"}')
        ref = ES.event_scores(stack[0], eng.scaled_theta()[0], xs, ys, ts, edge_ts)
        seen_wrap |= bool((ref['wrapped'] > 0).any())
        seen_drop |= bool(((ref['dropped'] > 0) & (ref['dropped'] < 9)).any())
    assert seen_wrap and seen_drop


def test_theta_far_out_of_frame_scores_exactly_zero():
    c = ES.generated('60x80-dense-r1')
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    ones = np.ones((1, 1, 60, 80), np.float32)
    for th in (np.full((1, 1, 1, 2), 1e5), np.array([[[[-1e5, 1e5]]]]), np.full((1, 60, 80, 2), 1e5)):
        eng.loss_grad(th, P, want_grad=False)
        for st in (None, ones):
            for rw in (None, [2.0]):
                rc, s, q, _, _ = _raw(eng, st, rw, True)
                assert rc == L.OK and not s[0].any() and not q[0].any() and not np.signbit(s[0]).any()


# ---- the Theta image built on demand: 2-DoF, a motion model, the fused motion path ----------------------------------------------------
def test_two_dof_theta_builds_its_image_for_the_scores():
    c = ES.generated('60x80-dense-r3')
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    eng.loss_grad(np.full((1, 60, 80, 2), 1.0), P, want_grad=False)          # a dense theta's image first ...
    eng.loss_grad(np.array([[[[5.5, -3.25]]]]), P, want_grad=False)           # ... which the 2-DoF evaluation does not rewrite
    _check_batch(eng, [c], c['stack'], 'two-dof stack')
    eng.loss_grad(np.array([[[[-2.5, 7.0]]]]), P)
    _check_batch(eng, [c], None, 'two-dof iwe')


@pytest.mark.parametrize('path', ['expanded', 'fused'])
def test_after_a_motion_model_evaluation(path):
    model, wins, coeffs = MC.batch('affine', (37, 53), 2000)
    n = sum(len(w['xs']) for w in wins)
    rng = np.random.default_rng(9)
    stack = rng.uniform(-0.5, 1.0, (3, 3, 37, 53)).astype(np.float32)
    with E.Engine((37, 53), n, max_refs=3, max_windows=3) as eng:
        eng.set_windows([MC.win_args(w) for w in wins])
        eng.set_motion_model(model)
        eng.set_motion_path(path)
        eng.loss_grad(np.ones((3, 1, 1, 2)), P, want_grad=False)              # another evaluation's theta in between
        eng.loss_grad_motion(coeffs, P)
        _check_batch(eng, wins, stack, f'motion {path} stack', forms=(None,))
        assert np.array_equal(eng.scaled_theta(), model.field(coeffs))
        eng.loss_grad_motion(coeffs, P, want_grad=False)
        _check_batch(eng, wins, None, f'motion {path} iwe', forms=('omega',))


# ---- leave-one-out on a weighted batch; weight-0 events still get scores ----------------------------------------------------------------
def test_exclude_self_on_a_weighted_batch():
    c = ES.generated('60x80-dense-r3')
    n = len(c['xs'])
    rng = np.random.default_rng(21)
    w = rng.uniform(0.0, 1.0, n).astype(np.float32)
    w[::5] = 0.0
    w[1::7] = 1.0
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'], w)
    assert eng.weighted
    for rw in (None, np.array([0.2, 0.5, 0.3])):
        got = eng.event_scores(ref_weights=rw, exclude_self=True, theta=c['theta'], params=P)[0]
        plain = eng.event_scores(ref_weights=rw)[0]
        ref = ES.event_scores(eng.iwes()[0], eng.scaled_theta()[0], c['xs'], c['ys'], c['ts'], c['edge_ts'], rw)
        w64 = w.astype(np.float64)
        _close(got, ref['scores'] - w64 * ref['selfs'], ref['M'] + w64 * ref['M_self'], f'exclude_self {"combined" if rw is not None else "per-r"}')
        _close(plain, ref['scores'], ref['M'], 'weighted batch, plain scores')
        # an event of weight 0 is absent from the IWE and is scored all the same: its leave-one-out score is its score
        z = w == 0
        assert np.array_equal(got[..., z], plain[..., z]) and (plain[..., z] > 0).mean() > 0.5
        assert not np.array_equal(got[..., ~z], plain[..., ~z])
    # the engine no longer holds the weights: refused before the library
    eng._staged_weights = None
    with pytest.raises(ValueError, match='does not hold them'):
        eng.event_scores(exclude_self=True)
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])                     # without weights: ones
    got = eng.event_scores(exclude_self=True, theta=c['theta'], params=P)[0]
    ref = ES.event_scores(eng.iwes()[0], eng.scaled_theta()[0], c['xs'], c['ys'], c['ts'], c['edge_ts'])
    _close(got, ref['scores'] - ref['selfs'], ref['M'] + ref['M_self'], 'exclude_self, unweighted')


# ---- properties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['33x65-grid-r3', '60x80-dense-r1'])
def test_adjoint_identity_against_the_oracle_s_splat(name):
    """<splat(1), F> = sum_e s_e: the scores against a random stack, summed over the window's events, are the inner product of that
    stack with the oracle's unweighted IWE"""
    c = ES.generated(name)
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    eng.loss_grad(c['theta'], P, want_grad=False)
    s = eng.event_scores(images=c['stack'])[0].astype(np.float64)
    Theta = eng.scaled_theta()[0]
    ev = (c['xs'], c['ys'], c['ts'], c['edge_ts'])
    iwes = ES.oracle_iwes(Theta, *ev, c['shape'])
    F = c['stack'].astype(np.float64)
    lhs = (iwes * F).sum(axis=(1, 2))
    bound = ES.TOL * ES.event_scores(F, Theta, *ev)['M'].sum(axis=1)
    print(f'{name}: sum_e s_e - <IWE, F> = {s.sum(axis=1) - lhs}, bound {bound}')
    assert np.all(np.abs(s.sum(axis=1) - lhs) <= bound)
    ones = eng.event_scores(images=np.ones_like(c['stack']))[0].astype(np.float64)          # F = 1: the sum of the IWE itself
    assert np.all(np.abs(ones.sum(axis=1) - iwes.sum(axis=(1, 2))) <= ES.TOL * iwes.sum(axis=(1, 2)))


def test_a_call_between_two_evaluations_changes_nothing_and_allocates_once():
    c = ES.generated('33x65-grid-r3')
    eng = _eng(c['shape'])
    eng.set_window(c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    th2 = c['theta'] * 0.5 + 1.0
    eng.loss_grad(c['theta'], P)
    want = eng.loss_grad(th2, P)
    want_iwe = eng.iwes()
    eng.loss_grad(c['theta'], P)
    first = eng.event_scores(images=c['stack'], ref_weights=[1.0, 2.0, 3.0], exclude_self=True)
    mem = eng.memory()
    again = eng.event_scores(images=c['stack'], ref_weights=[1.0, 2.0, 3.0], exclude_self=True)
    assert eng.memory() == mem and again[0].tobytes() == first[0].tobytes()
    eng.event_scores()
    got = eng.loss_grad(th2, P)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert eng.iwes().tobytes() == want_iwe.tobytes()


# ---- refusals: each leaves the outputs untouched -----------------------------------------------------------------------------------
def _refused(eng, code, match, images=None, ref_weights=None):
    rc, _, _, flat_s, flat_q = _raw(eng, images, ref_weights, True)
    assert rc == code, (rc, eng._lib.eincm_last_error(eng._ctx).decode())
    assert match in eng._lib.eincm_last_error(eng._ctx).decode()
    assert np.all(flat_s == SENTINEL) and np.all(flat_q == SENTINEL)
    with pytest.raises(E.EincmError, match=match) as e:
        eng.event_scores(images=images, ref_weights=ref_weights)
    assert e.value.code == code


def test_refusals_leave_the_outputs_untouched():
    c = ES.generated('60x80-dense-r3')
    args = (c['xs'], c['ys'], c['ts'], c['edges'], c['edge_ts'])
    stack = c['stack'][None]
    eng = _eng(c['shape'])
    eng.set_window(*args)
    _refused(eng, L.ERR_STATE, 'no evaluation yet')                            # staged, not evaluated
    _refused(eng, L.ERR_STATE, 'no evaluation yet', images=stack)
    eng.loss_grad_async(c['theta'], P, want_grad=False)
    _refused(eng, L.ERR_STATE, 'in flight', images=stack)                      # an evaluation in flight
    eng.loss_grad_wait()
    assert _raw(eng, stack)[0] == L.OK
    # null scores, and a ref_weights entry that is not finite, straight at the library
    assert eng._lib.eincm_event_scores(eng._ctx, None, None, None, None) == L.ERR_ARG
    rc, _, _, flat_s, flat_q = _raw(eng, None, [1.0, np.inf, 1.0], True)
    assert rc == L.ERR_ARG and np.all(flat_s == SENTINEL) and np.all(flat_q == SENTINEL)
    # a splat window other than 3
    eng.set_splat_window(5)
    try:
        eng.set_window(*args)
        eng.loss_grad(c['theta'], P, want_grad=False)
        _refused(eng, L.ERR_UNSUPPORTED, '3x3 splat window', images=stack)
    finally:
        eng.set_splat_window(3)
    # an fp64 context
    e64 = _eng(c['shape'], 'fp64')
    e64.set_window(*args)
    e64.loss_grad(c['theta'], P, want_grad=False)
    _refused(e64, L.ERR_UNSUPPORTED, 'fp64', images=stack)
    _refused(e64, L.ERR_UNSUPPORTED, 'fp64')


def test_a_masked_evaluation_refuses_the_iwe_source_and_serves_a_stack():
    a, b = ES.generated('60x80-dense-r3'), ES.generated('60x80-n65')
    wins = [a, b]
    eng = _eng((60, 80))
    eng.set_windows([(w['xs'], w['ys'], w['ts'], w['edges'], w['edge_ts']) for w in wins])
    theta = np.stack([a['theta'], b['theta']])
    eng.loss_grad(theta, P, want_grad=False)
    eng.loss_grad(theta * 0.5, P, want_grad=False, active=[1, 0])
    _refused(eng, L.ERR_STATE, 'left windows out')
    eng.loss_grad(np.array([[[[3.0, 1.0]]], [[[1.0, -2.0]]]]), P, want_grad=False, active=[0, 1])      # 2-DoF: the image on demand ...
    _refused(eng, L.ERR_STATE, 'left windows out')
    _refused(eng, L.ERR_STATE, 'left windows out')                             # ... does not make the second call forget the mask
    stack = np.random.default_rng(2).uniform(-0.5, 1.0, (2, 3, 60, 80)).astype(np.float32)
    _check_batch(eng, wins, stack, 'masked evaluation, stack', forms=(None,))
    eng.loss_grad(theta, P, want_grad=False, active=[1, 1])
    _check_batch(eng, wins, None, 'all windows active again', forms=(None,))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_scores_become_weights_and_the_weighted_window_is_solved_again():
    synth = importlib.import_module(pkg + '.synth')
    shape = (60, 80)
    win, is_noise = ES.noisy_window(synth, shape, 3000, 1000, 3, flow_mag=6.0)
    args = (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])
    th = win['flow_gt'][:1, :1]
    s = evaluation.event_scores(th, *args, source='iwe', exclude_self=True, engine=_eng(shape))
    assert s.shape == (3, 4000) and s.dtype == np.float32
    assert s[:, ~is_noise].mean() > s[:, is_noise].mean()
    e = evaluation.event_scores(th, *args, source='edges', ref_weights=E.multi_ref_weights(3), engine=_eng(shape))
    assert e.shape == (4000,) and e[~is_noise].mean() > e[is_noise].mean()
    w = staging.weights_from_scores(s)
    assert w.dtype == np.float32 and w[~is_noise].mean() > w[is_noise].mean()
    eng = _eng(shape)
    eng.set_window(*args, w)
    v, g, _ = eng.loss_grad(th[None], P)
    assert eng.weighted and np.isfinite(v).all() and np.isfinite(g).all()


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'event_scores.py'), '--events', '6000', '--noise', '2000'],
                       capture_output=True, text=True, timeout=TIME_LIMIT_S - 5)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'mean leave-one-out score' in r.stdout and 'flow error' in r.stdout
