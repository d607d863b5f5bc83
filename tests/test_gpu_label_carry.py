"""eincm_carry_label_prior and eincm_adopt_carried_prior on the GPU: a segmentation's label prior carried along
every model's own motion to the next window.

Every comparison is byte equality of all pixels of all four outputs with tests/_label_carry_witness.py; there is no tolerance.  The
sensor, the events, the weights and the affine coefficients are those of tests/test_gpu_motion_layers.py, imported from it: 40 x 72 is
2 x 3 source tiles with a partial tile in both axes; 1500 events lie on one pixel of the corner partial tile, one whole tile is empty,
and every sensor corner holds an event; the weights hold exact 0 and 1, the halves of the 1/4096 grid and values that quantise to 0.
Every test runs under its own time limit."""
import importlib
import signal

import numpy as np
import pytest

import _label_carry_witness as WIT
import _label_prior_witness as LPW
import _reweight_scene as RS
from test_gpu_motion_layers import GROUP_EVENTS, H, MODEL, W, _main_case

pytestmark = pytest.mark.gpu

pkg = 'edge-informed-contrast-maximization_amd'
E = importlib.import_module(pkg + '.engine')
L = importlib.import_module(pkg + '._lib')
motion = importlib.import_module(pkg + '.motion')
segmentation = importlib.import_module(pkg + '.segmentation')
synth = importlib.import_module(pkg + '.synth')

TIME_LIMIT_S = 60
ALL = ('prior', 'carried', 'accum', 'dropped')
MODELS, RADII, FLOORS = (1, 2, 3, 8), (0, 3, 8), (0, 4096)
TAUS = (0.37, 1.0, -0.5, (0.75, -1.25))                      # (the last: one per group)
P = E.make_params(20.0, 35.0, 2.5e-4, 0.0, 1)
_engines = {}


def _eng(precision='fp32', fresh=False):
    if fresh:
        return E.Engine((H, W), max_events_total=80000, max_refs=1, max_windows=16, precision=precision)
    if precision not in _engines:
        _engines[precision] = E.Engine((H, W), max_events_total=80000, max_refs=1, max_windows=16, precision=precision)
    return _engines[precision]


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


def _same(got, want, what):
    for name in got:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name)
        assert got[name].tobytes() == want[name].tobytes(), (what, name, int((got[name] != want[name]).sum()))


def _stage(eng, groups, ws, K, model=MODEL):
    eng.set_motion_model(model)
    eng.set_windows([groups[g] + (None if ws is None else ws[g][l],) for g in range(len(groups)) for l in range(K)])


def _wit_groups(groups, ws):
    return [(groups[g][0], groups[g][1], ws[g]) for g in range(len(groups))]


def _conserved(out, mass, what):
    """accum.sum() + dropped == total << 20 per (group, model), in Python integers"""
    G, K = out['dropped'].shape
    for g in range(G):
        for l in range(K):
            total = sum(int(v) for v in mass[g, l].reshape(-1))
            assert sum(int(v) for v in out['accum'][g, l].reshape(-1)) + int(out['dropped'][g, l]) == total << 20, (what, g, l)


# ---- 1. the main case, and 4. conservation in every case of it ----
@pytest.mark.parametrize('K', MODELS)
def test_main_case_equals_the_witness(K):
    groups, ws, coeffs = _main_case(K)
    eng = _eng()
    _stage(eng, groups, ws, K)
    staged = eng.label_prior(K, 2, want='prior')['prior']                          # the staged prior of this batch: it must stay
    assert eng.staged_prior().tobytes() == staged.tobytes()
    claims = dict(partial=0, taps_dropped=0, shared=0, rejected=0)
    for tau in TAUS:
        ref = WIT.carry(MODEL, _wit_groups(groups, ws), coeffs, tau, RADII[0], FLOORS[0])
        for r in RADII:
            for floor in FLOORS:
                ref['prior'] = WIT.prior_of(ref['carried'], r, floor)
                got = eng.carry_label_prior(K, coeffs, tau, radius=r, floor_mass=floor, want=ALL)
                assert tuple(got) == ALL
                _same(got, ref, (K, tau, r, floor))
                assert eng.carried_prior().tobytes() == got['prior'].tobytes()
                assert np.isfinite(got['prior']).all() and got['prior'].min() >= 0.0 and got['prior'].max() <= 1.0
                _conserved(got, ref['mass'], (K, tau, r, floor))
        for info in (i for grp in ref['info'] for i in grp):
            claims['partial'] += info['partial']
            claims['taps_dropped'] += info['taps_dropped']
            claims['rejected'] += info['rejected']
            claims['shared'] += int((info['sources'] > 4).sum())                     # more taps than one source has: several sources
    assert eng.staged_prior().tobytes() == staged.tobytes()                        # the staged prior of the batch is as it was
    # the case holds what it claims to: a source in row / column -1 that still deposits, taps that leave, pixels that several sources feed
    assert claims['partial'] > 0 and claims['taps_dropped'] > 0 and claims['shared'] > 0 and claims['rejected'] > 0, claims


# ---- 2. tau = 0 is the identity ----
def test_tau_zero_is_the_identity():
    K = 3
    groups, ws, coeffs = _main_case(K)
    eng = _eng()
    _stage(eng, groups, ws, K)
    mass = eng.compose_motions(K, coeffs, want='mass')['mass']
    for r, floor in ((0, 0), (3, 4096), (8, 1)):
        want = eng.label_prior(K, r, floor_mass=floor, want='prior')['prior']
        got = eng.carry_label_prior(K, coeffs, 0.0, radius=r, floor_mass=floor, want=ALL)
        assert got['carried'].tobytes() == mass.tobytes() and got['prior'].tobytes() == want.tobytes()
        assert not got['dropped'].any() and got['accum'].tobytes() == (mass.astype(np.uint64) << np.uint64(20)).tobytes()


# ---- 3. an integer shift ----
def test_an_integer_shift_moves_the_mass_image():
    K, dx, dy = 2, 3, -2
    groups, ws, _ = _main_case(K)
    model = motion.MotionModel('translation', (H, W))
    coeffs, tau = np.tile([6.0, -4.0], (2 * K, 1)), 0.5
    assert (model.field(coeffs) * tau == np.array([float(dx), float(dy)])).all()    # exactly (+3, -2) px at every pixel
    eng = _eng()
    _stage(eng, groups, ws, K, model)
    mass = eng.compose_motions(K, coeffs, want='mass')['mass']
    got = eng.carry_label_prior(K, coeffs, tau, radius=0, floor_mass=0, want=ALL)
    want = np.zeros_like(mass)
    want[:, :, :H + dy, dx:] = mass[:, :, -dy:, :W - dx]                            # shifted right and up, zeros shifted in
    assert got['carried'].tobytes() == want.tobytes()
    left = mass.astype(np.uint64).sum(axis=(2, 3)) - want.astype(np.uint64).sum(axis=(2, 3))
    assert (left > 0).all() and got['dropped'].tobytes() == (left << np.uint64(20)).tobytes()
    _same(got, WIT.carry(model, _wit_groups(groups, ws), coeffs, tau, 0, 0), 'shift')
    eng.set_motion_model(MODEL)


# ---- 5. saturation ----
def test_a_converging_field_saturates_one_pixel():
    model, window, coeffs, tau = WIT.saturation_case(motion)
    n = len(window[0])
    tx, ty = WIT.SAT_TARGET
    ref = WIT.carry(model, [(window[0], window[1], [None])], coeffs, tau, 2, 4096)
    with E.Engine(WIT.SAT_SENSOR, max_events_total=1300000, max_refs=1, max_windows=1) as eng:
        eng.set_motion_model(model)
        eng.set_windows([window])
        got = eng.carry_label_prior(1, coeffs, tau, radius=2, floor_mass=4096, want=ALL)
    assert n == 1200000 and int(got['accum'][0, 0, ty, tx]) == (1200000 * 4096) << 20 and int(got['carried'][0, 0, ty, tx]) == 2 ** 32 - 1
    assert int(got['dropped'][0, 0]) == 0 and int((got['accum'] != 0).sum()) == 1
    _same(got, ref, 'saturation')


# ---- 6. fields that are not finite ----
def test_sources_whose_landing_is_not_finite_are_dropped():
    K = 2
    groups, ws, coeffs = _main_case(K)
    coeffs = coeffs.copy()
    coeffs[0] = [0.0, 0.0, 1.0e306, 0.0, 0.0, -1.0e306]                             # finite everywhere; times tau = 1e3 it overflows
    coeffs[2] = [1.7e308, 0.0, 1.7e308, 0.0, 0.0, 0.0]                              # the field itself overflows right of the centre
    tau = np.array([1.0e3, 0.0])                                                    # ... and inf * 0 is a NaN
    with np.errstate(all='ignore'):
        f = MODEL.field(coeffs)
        assert np.isinf(f[0] * tau[0]).any() and np.isfinite(f[0]).all() and np.isnan(f[2] * tau[1]).any() and np.isfinite(f[2] * tau[1]).any()
    eng = _eng()
    _stage(eng, groups, ws, K)
    ref = WIT.carry(MODEL, _wit_groups(groups, ws), coeffs, tau, 3, 4096)
    got = eng.carry_label_prior(K, coeffs, tau, radius=3, floor_mass=4096, want=ALL)
    _same(got, ref, 'non-finite')
    _conserved(got, ref['mass'], 'non-finite')
    assert not got['accum'][0, 0].any() and int(got['dropped'][0, 0]) == int(ref['mass'][0, 0].astype(np.uint64).sum()) << 20
    assert ref['info'][1][0]['rejected'] > 0 and got['accum'][1, 0].any() and got['dropped'][1, 0] > 0
    assert np.isfinite(got['prior']).all()


# ---- 7. the edges ----
def test_a_group_without_events_beside_one_with():
    K = 8
    none = (np.zeros(0, np.int16), np.zeros(0, np.int16), np.zeros(0), np.ones((1, H, W)), np.array([0.5]))
    groups, ws, coeffs = _main_case(K)
    eng = _eng()
    eng.set_motion_model(MODEL)
    eng.set_windows([none] * K + [groups[1] + (ws[1][l],) for l in range(K)])
    wit = [(none[0], none[1], [None] * K), (groups[1][0], groups[1][1], ws[1])]
    for r, floor in ((8, 0), (8, 4096), (0, 4096)):
        got = eng.carry_label_prior(K, coeffs, 0.6, radius=r, floor_mass=floor, want=ALL)
        _same(got, WIT.carry(MODEL, wit, coeffs, 0.6, r, floor), (r, floor))
        assert not got['accum'][0].any() and not got['dropped'][0].any() and got['accum'][1].any()
        share = np.float32(1.0) if floor == 0 else np.float32(np.float64(floor) / np.float64(K * floor))
        assert got['prior'][:K].tobytes() == np.full((K, H, W), share, np.float32).tobytes()


def test_a_sensor_of_a_single_tile():
    h = w = 24
    K = 2
    rng = np.random.default_rng(9)
    n = 700
    xs, ys = rng.integers(0, w, n).astype(np.int16), rng.integers(0, h, n).astype(np.int16)
    win = (xs, ys, np.sort(rng.random(n)), np.ones((1, h, w)), np.array([0.5]))
    a = rng.random(n, dtype=np.float32)
    ws = [a, (np.float32(1.0) - a).astype(np.float32)]
    model = motion.MotionModel('affine', (h, w))
    coeffs = np.array([[4.0, -2.5, 3.0, 1.0, -1.0, 2.0], [-3.25, 5.0, -2.0, 0.5, 1.5, -3.0]])
    with E.Engine((h, w), max_events_total=2 * n, max_refs=1, max_windows=2) as eng:
        eng.set_motion_model(model)
        eng.set_windows([win + (ws[l],) for l in range(K)])
        for tau in (1.0, -0.7):
            got = eng.carry_label_prior(K, coeffs, tau, radius=8, floor_mass=1, want=ALL)
            ref = WIT.carry(model, [(xs, ys, ws)], coeffs, tau, 8, 1)
            _same(got, ref, tau)
            _conserved(got, ref['mass'], tau)
            assert got['dropped'].all() and got['accum'].any()


# ---- 8. adopt ----
def test_the_carried_prior_survives_a_staging_and_becomes_the_staged_one():
    K = 2
    groups, ws, coeffs = _main_case(K)
    eng = _eng()
    _stage(eng, groups, ws, K)
    carried = eng.carry_label_prior(K, coeffs, 0.8, radius=2, want='prior')['prior']
    other = [GROUP_EVENTS[1], GROUP_EVENTS[0]]                                      # other events, the same B and sensor
    answers = []
    for _ in range(2):
        eng.set_windows([other[g] for g in range(2) for l in range(K)])
        with pytest.raises(E.EincmError, match='no staged prior'):
            eng.staged_prior()                                                      # the staging dropped the staged prior ...
        assert eng.carried_prior().tobytes() == carried.tobytes()                   # ... and not the carried one
        eng.adopt_carried_prior(K)
        assert eng.staged_prior().tobytes() == carried.tobytes()
        eng.loss_grad_motion(coeffs, P, want_grad=False, allow_nonfinite=True)
        staged = eng.event_responsibilities_spatial(K, prior_images=None, want=E.RS_OUTPUTS)
        handed = eng.event_responsibilities_spatial(K, prior_images=eng.carried_prior(), want=E.RS_OUTPUTS)
        assert tuple(staged) == tuple(handed) == tuple(E.RS_OUTPUTS)
        for name in E.RS_OUTPUTS:
            a, b = (np.concatenate(o[name]) if isinstance(o[name], list) else o[name] for o in (staged, handed))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
        answers.append(np.concatenate(staged['weights']).tobytes())
        assert eng.carried_prior().tobytes() == carried.tobytes()                   # still valid after the adopt
    assert answers[0] == answers[1]
    uniform = eng.label_prior(K, 2, want='prior')['prior']                          # what this window would have started from
    assert uniform.tobytes() != carried.tobytes() and eng.carried_prior().tobytes() == carried.tobytes()


# ---- 9. the refusals ----
def _raw(eng, K, coeffs, tau, r=2, floor=4096, flags=0, n_coeffs=None):
    n = max(eng.B, 1) * H * W
    sent = dict(prior=np.full(n, -7.0, np.float32), carried=np.full(n, 0xA5A5, np.uint32), accum=np.full(n, 0xA5A5, np.uint64),
                dropped=np.full(max(eng.B, 1), 0xA5A5, np.uint64))
    c = None if coeffs is None else np.ascontiguousarray(coeffs, dtype=np.float64)
    t = None if tau is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (max(eng.B // max(K, 1), 1),)))
    rc = eng._lib.eincm_carry_label_prior(eng._ctx, K, None if c is None else c.ctypes.data, (c.shape[1] if c is not None else 6) if n_coeffs is None else n_coeffs,
                                          None if t is None else t.ctypes.data, r, floor, flags, *[sent[k].ctypes.data for k in ALL])
    untouched = bool((sent['prior'] == -7.0).all() and all((sent[k] == 0xA5A5).all() for k in ALL[1:]))
    return rc, untouched, eng._lib.eincm_last_error(eng._ctx).decode()


def _adopt_raw(eng, K):
    return eng._lib.eincm_adopt_carried_prior(eng._ctx, K), eng._lib.eincm_last_error(eng._ctx).decode()


def test_refusals_leave_everything_as_it_was():
    K = 2
    groups, ws, coeffs = _main_case(K)
    xs, ys, ts, edges, ets = GROUP_EVENTS[1]
    win, short = (xs, ys, ts, edges, ets), (xs[:100], ys[:100], ts[:100], edges, ets)
    with _eng(fresh=True) as eng:
        rc, untouched, why = _raw(eng, K, coeffs, 1.0)
        assert (rc, untouched) == (L.ERR_STATE, True) and 'needs staged windows' in why                   # nothing staged
        assert _adopt_raw(eng, K)[0] == L.ERR_STATE and 'needs staged windows' in _adopt_raw(eng, K)[1]
        eng.set_windows([groups[g] + (ws[g][l],) for g in range(2) for l in range(K)])
        rc, untouched, why = _raw(eng, K, coeffs, 1.0)
        assert (rc, untouched) == (L.ERR_STATE, True) and 'motion model' in why                            # no motion model
        rc, why = _adopt_raw(eng, K)
        assert rc == L.ERR_STATE and 'no carried prior' in why                                             # adopt with no carried prior
        with pytest.raises(E.EincmError, match='no carried prior') as err:
            eng.carried_prior()
        assert err.value.code == L.ERR_STATE
        eng.set_motion_model(MODEL)
        before = eng.carry_label_prior(K, coeffs, 1.0, want=ALL)
        for kw, code, words in ((dict(K=0), L.ERR_ARG, 'n_models'), (dict(K=3), L.ERR_ARG, 'whole number of groups'),      # K not dividing B
                                (dict(r=9), L.ERR_ARG, 'radius'), (dict(r=-1), L.ERR_ARG, 'radius'),
                                (dict(coeffs=None), L.ERR_ARG, 'null pointer'), (dict(tau=None), L.ERR_ARG, 'null pointer'),
                                (dict(tau=np.nan), L.ERR_ARG, 'tau must be finite'), (dict(tau=[1.0, np.inf]), L.ERR_ARG, 'group 1'),
                                (dict(n_coeffs=5), L.ERR_ARG, 'n_coeffs'), (dict(flags=1), L.ERR_ARG, 'flag bits'),
                                (dict(flags=1 << 31), L.ERR_ARG, 'flag bits')):
            a = dict(K=K, coeffs=coeffs, tau=1.0)
            a.update(kw)
            rc, untouched, why = _raw(eng, **a)
            assert (rc, untouched) == (code, True) and words in why, (kw, rc, why)
            assert eng.carried_prior().tobytes() == before['prior'].tobytes(), kw    # the carried prior is valid and as it was
        eng.loss_grad_async(np.zeros((2 * K, 1, 1, 2)), P)
        rc, untouched, why = _raw(eng, K, coeffs, 1.0)
        assert (rc, untouched) == (L.ERR_STATE, True) and 'in flight' in why
        assert _adopt_raw(eng, K)[0] == L.ERR_STATE and 'in flight' in _adopt_raw(eng, K)[1]
        eng.loss_grad_wait()
        for bad in ('want', 'radius', 'floor', 'tau', 'coeffs'):                     # the Python layer refuses before the library
            with pytest.raises(ValueError, match=bad):
                eng.carry_label_prior(K, coeffs[:, :5] if bad == 'coeffs' else coeffs, np.nan if bad == 'tau' else 1.0, radius=9 if bad == 'radius' else 2,
                                      floor_mass=-1 if bad == 'floor' else 0, want=('mass',) if bad == 'want' else ())
        _same(eng.carry_label_prior(K, coeffs, 1.0, want=ALL), before, 'after the refusals')
        rc, why = _adopt_raw(eng, 1)
        assert rc == L.ERR_ARG and 'another n_models' in why                                               # adopt with another K
        rc, why = _adopt_raw(eng, 4)
        assert rc == L.ERR_ARG and 'another n_models' in why
        eng.set_windows([win, short])
        rc, untouched, why = _raw(eng, K, coeffs[:2], 1.0)
        assert (rc, untouched) == (L.ERR_ARG, True) and 'equal n_events' in why                            # unequal groups
        rc, why = _adopt_raw(eng, K)
        assert rc == L.ERR_ARG and 'another number of windows' in why                                      # adopt after staging another B
        assert eng.carried_prior().tobytes() == before['prior'].tobytes()
        with pytest.raises(E.EincmError, match='no staged prior'):
            eng.staged_prior()                                                       # no refused adopt staged anything
    with _eng('fp64', fresh=True) as eng:
        eng.set_motion_model(MODEL)
        eng.set_windows([win, win])
        rc, untouched, why = _raw(eng, K, coeffs[:2], 1.0)
        assert (rc, untouched) == (L.ERR_UNSUPPORTED, True) and 'fp64' in why


# ---- 10. determinism ----
def test_same_bytes_on_every_run_and_engine():
    K = 3
    groups, ws, coeffs = _main_case(K)
    eng = _eng()
    _stage(eng, groups, ws, K)
    a = eng.carry_label_prior(K, coeffs, (0.75, -1.25), radius=3, want=ALL)
    _same(eng.carry_label_prior(K, coeffs, (0.75, -1.25), radius=3, want=ALL), a, 'second call')
    with _eng(fresh=True) as other:
        _stage(other, groups, ws, K)
        _same(other.carry_label_prior(K, coeffs, (0.75, -1.25), radius=3, want=ALL), a, 'fresh engine')
        assert other.carry_label_prior(K, coeffs, (0.75, -1.25), radius=3, want=()) == {}                  # carried only
        assert other.carried_prior().tobytes() == a['prior'].tobytes()


# ---- 11. the drivers ----
def _equal_histories(a, b, what):
    assert len(a) == len(b), what
    for ra, rb in zip(a, b):
        for k in ('coeffs', 'mass', 'n_unsupported', 'active'):
            assert ra[k].dtype == rb[k].dtype and ra[k].tobytes() == rb[k].tobytes(), (what, k)
        assert RS.as_bytes(ra['labels']) == RS.as_bytes(rb['labels']) and RS.as_bytes(ra['weights']) == RS.as_bytes(rb['weights']), what


def test_the_drivers():
    first, second = RS.two_layer(synth), RS.two_layer(synth, seeds=(5, 6))
    model = motion.MotionModel('translation', (RS.H, RS.W))
    params = E.make_params(1.0, 0.0, 0.0, 0.0, 1)
    n = max(len(first['window'][0]), len(second['window'][0]))
    assert 1900 <= n <= 2100
    em = dict(n_iters=2, maxiter=5)
    with E.Engine((RS.H, RS.W), max_events_total=2 * n, max_refs=RS.R, max_windows=2) as eng:
        # first_prior=None is the call without the keyword
        plain = segmentation.segment_motions_spatial(eng, [first['window']], model, first['coeffs0'], params, **em)
        _equal_histories(segmentation.segment_motions_spatial_primed(eng, [first['window']], model, first['coeffs0'], params, first_prior=None, **em),
                         plain, 'first_prior=None')
        # the sequence over two windows, against the same engine calls made by hand
        seq = segmentation.segment_sequence(eng, [[first['window']], [second['window']]], model, first['coeffs0'], params, tau=1.0, **em)
        assert len(seq) == 2 and all(len(h) == 2 for h in seq)
        _equal_histories(seq[0], plain, 'step 0')
        last = plain[-1]['coeffs']
        h0 = segmentation.segment_motions_spatial(eng, [first['window']], model, first['coeffs0'], params, **em)
        assert eng.carry_label_prior(2, h0[-1]['coeffs'].reshape(2, -1), 1.0, 2, 4096, want=()) == {}
        h1 = segmentation.segment_motions_spatial_primed(eng, [second['window']], model, h0[-1]['coeffs'], params, first_prior='carried', **em)
        _equal_histories(seq[1], h1, 'step 1 by hand')
        # ... and the carry takes part: the second window without it starts from another first E-step
        alone = segmentation.segment_motions_spatial(eng, [second['window']], model, last, params, **em)
        assert RS.as_bytes(alone[0]['weights']) != RS.as_bytes(seq[1][0]['weights'])
