"""The E-step with a prior image on the GPU: eincm_event_responsibilities_spatial and the EM driver on it.

Every comparison is byte equality: with the float32 restatement of tests/_label_prior_witness.py fed with the GPU's own
Engine.event_scores scores and selfs (as tests/test_gpu_responsibilities.py feeds the plain rule), with the plain E-step, or between two
routes to the same result; there is no tolerance.  The sensor is the 40 x 72 of tests/test_gpu_motion_layers.py and a window holds a few
thousand events.  Every test runs under its own time limit."""
import importlib
import signal

import numpy as np
import pytest

import _label_prior_witness as WIT
import _responsibilities_witness as RW

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
motion = importlib.import_module(pkg + '.motion')
segmentation = importlib.import_module(pkg + '.segmentation')
synth = importlib.import_module(pkg + '.synth')

H, W = 40, 72
NS = (3000, 1100)                            # the events of the two groups: several blocks of 256 each, the last one partial
TIME_LIMIT_S = 60
ALL = ('weights', 'labels', 'mass', 'n_unsupported')
MODEL = motion.MotionModel('affine', (H, W))
P = E.make_params(20.0, 35.0, 2.5e-4, 0.0, 1)
OMEGA = np.array([1.0])
_engines = {}


def _eng(fresh=False):
    if fresh:
        return E.Engine((H, W), max_events_total=40000, max_refs=1, max_windows=16)
    if 'e' not in _engines:
        _engines['e'] = E.Engine((H, W), max_events_total=40000, max_refs=1, max_windows=16)
    return _engines['e']


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


# ---- the case: G = 2 groups of K windows on shared events, complementary random weights, small affine motions ----
_cases = {}


def _case(K):
    if K not in _cases:
        rng = np.random.default_rng(900 + K)
        groups, ws = [], []
        for n in NS:
            xs, ys = rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16)
            groups.append((xs, ys, np.sort(rng.random(n)), rng.random((1, H, W)), np.array([0.5])))
            w = rng.random((K, n)).astype(np.float32)
            w[:, ::7] = 0.0
            ws.append([np.ascontiguousarray((w[l] / np.maximum(w.sum(axis=0), 1e-6)).astype(np.float32).clip(0, 1)) for l in range(K)])
        coeffs = rng.standard_normal((2 * K, MODEL.n_coeffs)) * np.array([4.0, 4.0, 1.5, 1.5, 1.5, 1.5])
        pi = rng.uniform(0.2, 2.0, 2 * K)
        stack = rng.uniform(0.05, 1.0, (2 * K, H, W)).astype(np.float32)
        _cases[K] = (groups, ws, coeffs, pi, stack)
    return _cases[K]


def _stage(eng, K, keep_order=False):
    groups, ws, coeffs, _, _ = _case(K)
    eng.set_motion_model(MODEL)
    eng.set_motion_path('expanded')
    if keep_order:
        eng.set_windows([groups[g] for g in range(2) for l in range(K)], keep_order=True)
        eng.set_weights([ws[g][l] for g in range(2) for l in range(K)])
    else:
        eng.set_windows([groups[g] + (ws[g][l],) for g in range(2) for l in range(K)])
    eng.loss_grad_motion(coeffs, P, want_grad=False, allow_nonfinite=True)


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x = np.concatenate(a[k]) if isinstance(a[k], list) else a[k]
        y = np.concatenate(b[k]) if isinstance(b[k], list) else b[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, int((x != y).sum()))


def _gpu_scores(eng):
    """The GPU's own combined scores and selfs of every window under OMEGA: ([s_b], [q_b]) float32"""
    off, length, total = E.event_scores_layout(eng.n_events, eng.R, True)
    s, q = np.empty(total, np.float32), np.empty(total, np.float32)
    rc = eng._lib.eincm_event_scores(eng._ctx, None, OMEGA.ctypes.data, s.ctypes.data, q.ctypes.data)
    assert rc == L.OK, eng._lib.eincm_last_error(eng._ctx).decode()
    return [s[off[b]:off[b] + length[b]] for b in range(eng.B)], [q[off[b]:off[b] + length[b]] for b in range(eng.B)]


def _witness(eng, K, pi, stack, exclude_self):
    """The four outputs of the restatement for the staged and evaluated case(K), in the shapes of the Python layer, and the per-group
    fallback codes."""
    groups, ws, _, _, _ = _case(K)
    s, q = _gpu_scores(eng)
    out = dict(weights=[], labels=[], mass=np.zeros((2, K)), n_unsupported=np.zeros(2, np.int64))
    fallback = []
    for g in range(2):
        b0 = g * K
        Pe = WIT.prior_at_events(stack[b0:b0 + K], [(groups[g][0], groups[g][1])] * K)
        r = WIT.responsibilities_spatial_f32(np.stack(s[b0:b0 + K]), np.stack(q[b0:b0 + K]), np.stack(ws[g]),
                                             None if pi is None else pi[b0:b0 + K], Pe, exclude_self)
        out['weights'] += [r['weights'][l] for l in range(K)]
        out['labels'].append(r['labels'])
        out['mass'][g] = RW.ordered_mass(r['weights'])
        out['n_unsupported'][g] = int(r['unsupported'].sum())
        fallback.append(r['fallback'])
    return out, fallback


# ---- 1. a prior of ones is the plain E-step ----
@pytest.mark.parametrize('exclude_self', [True, False])
@pytest.mark.parametrize('K', [1, 2, 8])
def test_a_prior_of_ones_gives_the_plain_bytes(K, exclude_self):
    _, _, _, pi, _ = _case(K)
    eng = _eng()
    _stage(eng, K)
    ones = np.ones((2 * K, H, W), np.float32)
    for prior in (None, pi):
        plain = eng.event_responsibilities(K, ref_weights=OMEGA, prior=prior, exclude_self=exclude_self, want=ALL)
        got = eng.event_responsibilities_spatial(K, ones, ref_weights=OMEGA, prior=prior, exclude_self=exclude_self, want=ALL)
        _same(got, plain, (K, exclude_self, prior is None))
    assert K == 1 or any((w > 0).any() and (w < 1).any() for w in plain['weights'])


# ---- 2. a random positive prior stack against the witness ----
@pytest.mark.parametrize('exclude_self', [True, False])
@pytest.mark.parametrize('K', [2, 3, 8])
def test_a_random_prior_stack_equals_the_witness(K, exclude_self):
    _, _, _, pi, stack = _case(K)
    eng = _eng()
    _stage(eng, K)
    for prior in (None, pi):
        got = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=prior, exclude_self=exclude_self, want=ALL)
        ref, _ = _witness(eng, K, prior, stack, exclude_self)
        print(f'K {K} exclude_self {exclude_self} prior {prior is not None}: mass gpu {got["mass"].tolist()} witness {ref["mass"].tolist()}, '
              f'unsupported {got["n_unsupported"].tolist()}')
        _same(got, ref, (K, exclude_self, prior is None))
        plain = eng.event_responsibilities(K, ref_weights=OMEGA, prior=prior, exclude_self=exclude_self, want='weights')['weights']
        assert np.concatenate(plain).tobytes() != np.concatenate(got['weights']).tobytes()      # the prior stack does something
    for k in ALL:                                                                  # each output alone: the bytes of the full call
        one = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, exclude_self=exclude_self, want=k)
        _same(one, {k: got[k]}, k)


# ---- 3. the prior from the host and the same prior staged ----
def test_host_prior_and_staged_prior_give_the_same_bytes():
    K = 3
    _, _, _, pi, _ = _case(K)
    eng = _eng()
    _stage(eng, K)
    prior = eng.label_prior(K, 2, want='prior')['prior']
    assert prior.min() > 0 and prior.max() < 1 and len(np.unique(prior)) > 100
    host = eng.event_responsibilities_spatial(K, prior, ref_weights=OMEGA, prior=pi, want=ALL)
    staged = eng.event_responsibilities_spatial(K, ref_weights=OMEGA, prior=pi, want=ALL)
    _same(staged, host, 'staged')
    ref, _ = _witness(eng, K, pi, prior, True)
    _same(host, ref, 'witness')


# ---- 4. the fallbacks ----
def test_a_block_without_prior_takes_the_pi_fallback_and_counts_once():
    K = 2
    groups, _, coeffs, pi, stack = _case(K)
    stack = stack.copy()
    stack[:, 10:20, 30:50] = 0.0
    eng = _eng()
    _stage(eng, K)
    far = coeffs.copy()                                                             # group 1: every model throws the events out of the sensor,
    far[K:] = 0.0                                                                   # so no model supports them and the c_l shares decide
    far[K:, 0] = RW.FAR
    eng.loss_grad_motion(far, P, want_grad=False, allow_nonfinite=True)
    got = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)
    ref, fallback = _witness(eng, K, pi, stack, True)
    _same(got, ref, 'block')
    for g in range(2):
        xs, ys = groups[g][0], groups[g][1]
        block = (ys >= 10) & (ys < 20) & (xs >= 30) & (xs < 50)
        assert block.sum() > 20 and np.array_equal(fallback[g] == 2, block)
        pi32 = pi[g * K:(g + 1) * K].astype(np.float32)
        share = pi32 / np.float32(np.float32(0) + pi32[0] + pi32[1])
        assert all(np.all(got['weights'][g * K + l][block] == share[l]) for l in range(K))
        assert int(got['n_unsupported'][g]) == int((fallback[g] > 0).sum())          # once, whichever fallback
    assert (fallback[1] == 1).sum() > 0.9 * (fallback[1] != 2).sum() and (fallback[0] == 0).sum() > 0.5 * NS[0]


def test_a_model_without_prior_gets_exact_zeros():
    K = 3
    _, _, _, pi, stack = _case(K)
    stack = stack.copy()
    stack[1] = 0.0
    stack[K + 2] = 0.0
    eng = _eng()
    _stage(eng, K)
    got = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)
    _same(got, _witness(eng, K, pi, stack, True)[0], 'model')
    assert not got['weights'][1].any() and not got['weights'][K + 2].any() and got['weights'][0].any() and got['weights'][K].any()
    assert (got['labels'][0] != 1).all() and (got['labels'][1] != 2).all() and got['mass'][0, 1] == 0.0 and got['mass'][1, 2] == 0.0


def test_a_tie_goes_to_the_lowest_label():
    K = 2
    groups, ws, coeffs, _, stack = _case(K)
    eng = _eng()
    eng.set_motion_model(MODEL)
    eng.set_windows([groups[0] + (ws[0][0],)] * K)                                   # the same window twice, under the same motion
    eng.loss_grad_motion(coeffs[[0, 0]], P, want_grad=False, allow_nonfinite=True)
    got = eng.event_responsibilities_spatial(K, stack[[0, 0]], ref_weights=OMEGA, want=ALL)
    assert not got['labels'][0].any()
    assert np.all(got['weights'][0] == 0.5) and np.all(got['weights'][1] == 0.5) and got['mass'].tolist() == [[NS[0] / 2, NS[0] / 2]]


# ---- 5. applying in place ----
def test_apply_leaves_the_engine_as_a_staging_with_its_weights_would():
    K = 2
    groups, _, coeffs, pi, stack = _case(K)
    eng = _eng()
    _stage(eng, K, keep_order=True)
    ref = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)
    applied = eng.apply_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)
    _same(applied, ref, 'the applying call returns the same bytes')
    a_w = [np.array(w) for w in eng.staged_weights()]
    a_v = eng.loss_grad_motion(coeffs, P, allow_nonfinite=True)
    with _eng(fresh=True) as other:
        other.set_motion_model(MODEL)
        other.set_motion_path('expanded')
        other.set_windows([groups[g] + (ref['weights'][g * K + l],) for g in range(2) for l in range(K)], keep_order=True)
        b_w = other.staged_weights()
        b_v = other.loss_grad_motion(coeffs, P, allow_nonfinite=True)
    assert np.concatenate(a_w).tobytes() == np.concatenate(b_w).tobytes() == np.concatenate(ref['weights']).tobytes()
    assert a_v[0].tobytes() == b_v[0].tobytes() and a_v[1].tobytes() == b_v[1].tobytes()
    # on the staged prior too, and the staged prior outlives the application
    _stage(eng, K, keep_order=True)
    prior = eng.label_prior(K, 2, want='prior')['prior']
    want_w = eng.event_responsibilities_spatial(K, prior, ref_weights=OMEGA, want='weights')['weights']
    assert eng.apply_responsibilities_spatial(K, ref_weights=OMEGA, want=()) == {}
    assert np.concatenate(eng.staged_weights()).tobytes() == np.concatenate(want_w).tobytes()
    assert eng.staged_prior().tobytes() == prior.tobytes()


# ---- 6. the driver ----
def test_the_spatial_driver_in_place_and_restaging_give_equal_histories():
    flows = np.array([[6.0, 1.5], [-4.0, -5.0]])
    layers = [synth.make_window(seed, (H, W), 1500, 2, flow=np.broadcast_to(v, (H, W, 2)).copy(), n_segments=6, n_circles=1, jitter_px=0.3,
                                noise_frac=0) for seed, v in zip((3, 4), flows)]
    ts = np.concatenate([l['ts'] for l in layers])
    order = np.argsort(ts, kind='stable')
    win = (np.concatenate([l['xs'] for l in layers])[order], np.concatenate([l['ys'] for l in layers])[order], ts[order],
           np.maximum(layers[0]['edges'], layers[1]['edges']), layers[0]['edge_ts'])
    model = motion.MotionModel('translation', (H, W))
    params = E.make_params(1.0, 0.0, 0.0, 0.0, 1)
    coeffs0 = (flows * np.array([[0.6], [1.4]]))[None]
    hist = {}
    for in_place in (True, False):
        with E.Engine((H, W), max_events_total=8000, max_refs=2, max_windows=2) as eng:
            hist[in_place] = segmentation.segment_motions_spatial(eng, [win], model, coeffs0, params, radius=2, n_iters=2, maxiter=5,
                                                                  in_place=in_place)
    assert len(hist[True]) == len(hist[False]) == 2
    for a, b in zip(hist[True], hist[False]):
        for k in ('coeffs', 'mass', 'n_unsupported', 'active'):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a['labels'], b['labels']))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a['weights'][0], b['weights'][0]))
    with E.Engine((H, W), max_events_total=8000, max_refs=2, max_windows=2) as eng:
        plain = segmentation.segment_motions_in_place(eng, [win], model, coeffs0, params, n_iters=2, maxiter=5)
    assert plain[-1]['weights'][0][0].tobytes() != hist[True][-1]['weights'][0][0].tobytes()     # the prior image takes part


# ---- 7. the plain E-step is untouched by a spatial call in between ----
def test_the_plain_e_step_before_and_after_a_spatial_one():
    K = 3
    _, _, _, pi, stack = _case(K)
    eng = _eng()
    _stage(eng, K)
    before = eng.event_responsibilities(K, ref_weights=OMEGA, prior=pi, want=ALL)
    eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)
    eng.label_prior(K, 8, want=())
    eng.event_responsibilities_spatial(K, ref_weights=OMEGA, prior=pi, want=ALL)
    _same(eng.event_responsibilities(K, ref_weights=OMEGA, prior=pi, want=ALL), before, 'after')


# ---- 8. the refusals of the library ----
def test_refusals_leave_the_outputs_untouched():
    K = 2
    _, _, _, pi, stack = _case(K)
    eng = _eng()
    _stage(eng, K)
    n = int(eng.n_events.sum())
    good = eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL)

    def raw(prior_images, flags):
        w, lab = np.full(n, -3.0, np.float32), np.full(n // K, 77, np.uint8)
        rc = eng._lib.eincm_event_responsibilities_spatial(eng._ctx, K, None, OMEGA.ctypes.data, None, None,
                                                           None if prior_images is None else prior_images.ctypes.data, flags,
                                                           w.ctypes.data, lab.ctypes.data, None, None)
        return rc, bool((w == -3.0).all() and (lab == 77).all()), eng._lib.eincm_last_error(eng._ctx).decode()

    rc, untouched, why = raw(stack, L.RS_PRIOR_STAGED)
    assert (rc, untouched) == (L.ERR_ARG, True) and 'one source' in why
    rc, untouched, why = raw(None, 0)
    assert (rc, untouched) == (L.ERR_ARG, True) and 'no prior stack' in why
    rc, untouched, why = raw(None, L.RS_PRIOR_STAGED)
    assert (rc, untouched) == (L.ERR_STATE, True) and 'without a staged prior' in why
    for value in (np.nan, np.inf, -1.0e-30):
        bad = stack.copy()
        bad[3, 17, 41] = value
        rc, untouched, why = raw(bad, 0)
        assert (rc, untouched) == (L.ERR_ARG, True) and 'window 3, pixel (x 41, y 17)' in why, why
        with pytest.raises(ValueError, match=r'window 3, pixel \(x 41, y 17\)'):
            eng.event_responsibilities_spatial(K, bad, ref_weights=OMEGA)
    rc, untouched, why = raw(stack, L.RS_APPLY)                                      # the keep-order flags are refused as the plain call refuses them
    assert (rc, untouched) == (L.ERR_STATE, True) and 'EINCM_SW_KEEP_ORDER' in why
    _same(eng.event_responsibilities_spatial(K, stack, ref_weights=OMEGA, prior=pi, want=ALL), good, 'after the refusals')
