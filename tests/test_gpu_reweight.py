"""Re-weighting a staged batch in place on the GPU.  The contract is byte equality: after set_weights(w) - or
after an E-step that applies its own result - the engine answers every call with the bytes of a fresh engine staged with the same
windows, w and keep_order=True.  The engine is bit-reproducible and the two staged layouts are the same arrays, so nothing here has a
tolerance.

The batch is tests/_reweight_scene.py's: 64 x 96 (2 x 3 tiles), R = 2, B = 4 - 3000 events with 1500 in one tile and 300 on one pixel,
300 events, an empty window, and a window that is never handed weights; two weight sets with exact 0, exact 1 and values between, the
second with its zeros on other pixels.  Windows of unequal length are no group of models, so event_responsibilities(2) is compared on
the two-group batch of the applying E-step, and the main batch takes event_responsibilities(1).

The existing interface tests pin the parameter lists of Engine.event_responsibilities and segmentation.segment_motions; the applying
E-step and the in-place EM driver are therefore Engine.apply_responsibilities and segmentation.segment_motions_in_place."""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch      # at import, before any fixture loads the engine's library (tests/test_gpu_device_bfgs.py says why): mask_tensor and
                  # loss_grad_device hand out torch views  # noqa: F401

import _reweight_scene as RS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = 'edge-informed-contrast-maximization_amd'
L = importlib.import_module(PKG + '._lib')
E = importlib.import_module(PKG + '.engine')
synth = importlib.import_module(PKG + '.synth')
motion = importlib.import_module(PKG + '.motion')
segmentation = importlib.import_module(PKG + '.segmentation')

P0 = E.make_params(RS.ALPHA, RS.BETA, RS.GAMMA, 0.0, 0)           # level 0 with the TV term: the event mask is read
P1 = E.make_params(RS.ALPHA, RS.BETA, 0.0, 0.0, 1)
ONES = [None] * RS.B


def _engine(n=sum(RS.N), B=RS.B):
    return E.Engine((RS.H, RS.W), max(n, 1), max_refs=RS.R, max_windows=B)


_bytes, answers = RS.as_bytes, RS.answers


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f'{what}: {k} differs'


@pytest.fixture(scope='module')
def scene(built_lib):
    return RS.batch(synth)


@pytest.fixture(scope='module')
def fresh(scene):
    """name -> the answers of a fresh engine staged with that weight set and keep_order=True; 'plain': the unweighted engine of before"""
    out = {}
    for name, w, keep in (('w1', scene['w1'], True), ('w2', scene['w2'], True), ('ones', ONES, True), ('plain', None, False)):
        with _engine() as eng:
            eng.set_windows(RS.staged(scene, w), keep_order=keep)
            assert eng.keep_order is keep and eng.weighted is keep
            out[name] = answers(eng, scene)
    return out


def test_the_scene_is_what_the_cases_need(scene):
    xs, ys = scene['windows'][0][:2]
    tile = (ys // 32) * 3 + xs // 32
    assert [len(w[0]) for w in scene['windows']] == list(RS.N) and 1400 <= int((tile == 1).sum()) <= 1900
    assert int(((xs == RS.CROWD[0]) & (ys == RS.CROWD[1])).sum()) >= 300
    assert scene['w1'][2] is None and scene['w1'][3] is None and scene['w2'][3] is None
    for w in (scene['w1'][0], scene['w1'][1], scene['w2'][0], scene['w2'][1]):
        assert (w == 0).any() and (w == 1).any() and ((w > 0) & (w < 1)).any()
    for b in (0, 1):                                # the zeros moved to other pixels: the event mask must change
        pix = scene['windows'][b][1].astype(np.int64) * RS.W + scene['windows'][b][0]
        gone1, gone2 = (np.setdiff1d(pix, pix[w[b] > 0]) for w in (scene['w1'], scene['w2']))
        assert len(gone1) and len(gone2) and not np.intersect1d(gone1, gone2).size


def test_fresh_stagings_differ_where_they_should_and_ones_are_the_unweighted_bits(fresh):
    assert fresh['w1']['mask'] != fresh['w2']['mask'] and fresh['w1']['loss_grad_theta8'] != fresh['w2']['loss_grad_theta8']
    _same(fresh['ones'], fresh['plain'], 'keep-order staging without weights against the unweighted engine')


def test_staged_order_is_a_permutation_inside_every_window(scene):
    with _engine() as eng:
        eng.set_windows(RS.staged(scene, scene['w1']), keep_order=True)
        orders = eng.staged_order()
        w = eng.staged_weights()
    off = np.concatenate([[0], np.cumsum(RS.N)])
    for o in orders:
        assert o.dtype == np.uint32 and o.shape == (sum(RS.N),)
        assert np.array_equal(np.sort(o), np.arange(sum(RS.N)))
        for b in range(RS.B):
            assert ((o[off[b]:off[b + 1]] >= off[b]) & (o[off[b]:off[b + 1]] < off[b + 1])).all()
    assert not np.array_equal(*orders)              # the two layouts are two orders
    # the splat's copy: tile after tile; inside a tile a permutation of the time order that stays inside blocks of 256
    xs = np.concatenate([x[0] for x in scene['windows']]).astype(np.int64)
    ys = np.concatenate([x[1] for x in scene['windows']]).astype(np.int64)
    for o in orders:
        tiles = (ys[o] // 32) * 3 + xs[o] // 32
        for b in range(RS.B):
            assert (np.diff(tiles[off[b]:off[b + 1]]) >= 0).all()
    for b in range(RS.B):
        want = np.ones(RS.N[b], np.float32) if scene['w1'][b] is None else scene['w1'][b]
        assert w[b].dtype == np.float32 and np.array_equal(w[b], want)


TRANSITIONS = [('w1', 'w2'), ('none', 'w2'), ('w2', 'ones'), ('w1', 'w1')]


@pytest.mark.parametrize('start,end', TRANSITIONS, ids=['-to-'.join(t) for t in TRANSITIONS])
def test_set_weights_leaves_the_bytes_of_a_fresh_staging(scene, fresh, start, end):
    sets = dict(w1=scene['w1'], w2=scene['w2'], ones=ONES, none=None)
    with _engine() as eng:
        eng.set_windows(RS.staged(scene, sets[start]), keep_order=True)
        eng.loss_grad(scene['theta8'], P0)                              # an evaluation, a policy and a BFGS that the call must drop
        eng.bfgs_begin(scene['theta8'])
        eng.set_weights(sets[end])
        with pytest.raises(E.EincmError):
            eng.iwes()                                                  # the last evaluation is gone, as after a staging
        got = answers(eng, scene)
        w = eng.staged_weights()
    _same(got, fresh[end], f'{start} -> {end}')
    if end == 'ones':
        _same(got, fresh['plain'], 'back to all ones against the unweighted engine')
    for b in range(RS.B):
        assert np.array_equal(w[b], np.ones(RS.N[b], np.float32) if sets[end][b] is None else sets[end][b])


def test_a_refused_set_weights_leaves_the_batch_and_its_evaluation(scene):
    with _engine() as eng:
        eng.set_windows(RS.staged(scene, scene['w1']), keep_order=True)
        before = _bytes(eng.loss_grad(scene['theta8'], P0, want_aux=True))
        iwes = eng.iwes().tobytes()
        bad = [w if w is None else w.copy() for w in scene['w2']]
        bad[1][7] = 1.5
        with pytest.raises(ValueError, match=r'within \[0, 1\]'):
            eng.set_weights(bad)
        nan = np.array(bad[1], dtype=np.float32)
        nan[7] = np.nan
        wp = (E.C.c_void_p * RS.B)(scene['w2'][0].ctypes.data, nan.ctypes.data, None, None)
        assert eng._lib.eincm_set_weights(eng._ctx, wp) == L.ERR_ARG     # the library's own check, past Python's
        assert 'weight 7 of window 1' in eng._lib.eincm_last_error(eng._ctx).decode()
        assert eng.iwes().tobytes() == iwes                             # the last evaluation is still there
        assert _bytes(eng.loss_grad(scene['theta8'], P0, want_aux=True)) == before
        assert all(np.array_equal(a, np.ones(len(a), np.float32) if b is None else b) for a, b in zip(eng.staged_weights(), scene['w1']))


def test_without_keep_order_the_calls_raise_and_name_the_flag(scene):
    with _engine() as eng:
        eng.set_windows(RS.staged(scene, scene['w1']))
        eng.loss_grad(scene['theta8'], P1, want_grad=False)
        for call in (lambda: eng.set_weights(scene['w2']), eng.staged_order, eng.staged_weights, lambda: eng.apply_responsibilities(1)):
            with pytest.raises(ValueError, match='keep_order=True'):
                call()
        # the library's own refusals, past Python's
        assert eng._lib.eincm_set_weights(eng._ctx, None) == L.ERR_STATE
        assert 'EINCM_SW_KEEP_ORDER' in eng._lib.eincm_last_error(eng._ctx).decode()
        mass = np.zeros(RS.B)
        rw = np.ascontiguousarray(E.multi_ref_weights(RS.R), dtype=np.float64)
        for flag in (L.RS_APPLY, L.RS_STAGED_WEIGHTS | L.RS_EXCLUDE_SELF):
            rc = eng._lib.eincm_event_responsibilities(eng._ctx, 1, None, rw.ctypes.data, None, None, flag, None, None, mass.ctypes.data, None)
            assert rc == L.ERR_STATE and 'EINCM_SW_KEEP_ORDER' in eng._lib.eincm_last_error(eng._ctx).decode()
        a = np.zeros(sum(RS.N), np.uint32)
        assert eng._lib.eincm_get_stage_order(eng._ctx, a.ctypes.data, None) == L.ERR_STATE
        # a later keep-order staging of the same engine serves them, and one without drops the state again
        eng.set_windows(RS.staged(scene, scene['w1']), keep_order=True)
        eng.set_weights(scene['w2'])
        eng.set_windows(RS.staged(scene, scene['w1']))
        assert eng.keep_order is False
        with pytest.raises(ValueError, match='keep_order=True'):
            eng.set_weights(scene['w2'])


# ---- the E-step that applies its own result ----------------------------------------------------------------------------------------
def test_the_applying_e_step_equals_the_e_step_followed_by_a_staging(built_lib):
    c = RS.e_step_batch(synth)
    n = sum(len(w[0]) for w in c['windows'])
    model = motion.MotionModel('translation', (RS.H, RS.W))
    wins = [w + (c['w0'][b],) for b, w in enumerate(c['windows'])]
    prior = np.array([0.7, 0.3, 0.5, 0.5])

    def evaluate(eng):
        eng.set_motion_model(model)
        eng.set_motion_path('expanded')
        return eng.loss_grad_motion(c['coeffs'], P1, want_aux=True)

    with _engine(n) as eng:                          # the route of before: E-step, download, stage again
        eng.set_windows(wins)
        evaluate(eng)
        ref = eng.event_responsibilities(2, prior=prior, want=E.RS_OUTPUTS)
        eng.set_windows([w + (ref['weights'][b],) for b, w in enumerate(c['windows'])])
        ref_next = _bytes(evaluate(eng))
        ref_iwes = eng.iwes().tobytes()
        ref_again = _bytes(eng.event_responsibilities(2, prior=prior, want=E.RS_OUTPUTS))
    with _engine(n) as eng:
        eng.set_windows(wins, keep_order=True)
        evaluate(eng)
        plain = eng.event_responsibilities(2, prior=prior, want=E.RS_OUTPUTS)      # (reads the staged weights on the device)
        assert _bytes(plain) == _bytes(ref)
        got = eng.apply_responsibilities(2, prior=prior, want=E.RS_OUTPUTS)
        assert _bytes(got) == _bytes(ref)
        with pytest.raises(E.EincmError):
            eng.iwes()
        staged = eng.staged_weights()
        assert all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(staged, ref['weights']))
        assert _bytes(evaluate(eng)) == ref_next and eng.iwes().tobytes() == ref_iwes
        assert _bytes(eng.event_responsibilities(2, prior=prior, want=E.RS_OUTPUTS)) == ref_again
        # nothing per-event downloaded, nothing at all downloaded: the same weights are applied
        eng.set_weights(c['w0'])
        evaluate(eng)
        part = eng.apply_responsibilities(2, prior=prior)
        assert sorted(part) == ['labels', 'mass'] and _bytes(part['labels']) == _bytes(ref['labels']) and part['mass'].tobytes() == ref['mass'].tobytes()
        assert all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(eng.staged_weights(), ref['weights']))
        eng.set_weights(c['w0'])
        evaluate(eng)
        assert eng.apply_responsibilities(2, prior=prior, want=()) == {}
        assert _bytes(evaluate(eng)) == ref_next
        # set_weights on this batch against the fresh staging, with the two-model E-step among the answers
        eng.set_weights(c['w0'])
        evaluate(eng)
        assert _bytes(eng.event_responsibilities(2, prior=prior, want=E.RS_OUTPUTS)) == _bytes(ref)


def test_the_in_place_driver_returns_the_restaging_drivers_bytes(built_lib):
    case = RS.two_layer(synth)
    n = len(case['window'][0])
    assert 1900 <= n <= 2100
    model = motion.MotionModel('translation', (RS.H, RS.W))
    params = E.make_params(1.0, 0.0, 0.0, 0.0, 1)
    runs = {}
    with _engine(2 * n, 2) as eng:
        for name, drive, kw in (('restage', segmentation.segment_motions, {}), ('in_place', segmentation.segment_motions_in_place, {}),
                                ('unrecorded', segmentation.segment_motions_in_place, dict(record_weights=False))):
            runs[name] = drive(eng, [case['window']], model, case['coeffs0'], params, n_iters=2, maxiter=5, **kw)
        w0 = [[np.asarray(w) for w in runs['restage'][0]['weights'][0]]]
        for name, drive in (('restage_w0', segmentation.segment_motions), ('in_place_w0', segmentation.segment_motions_in_place)):
            runs[name] = drive(eng, [case['window']], model, case['coeffs0'], params, n_iters=1, maxiter=5, weights0=w0, prior='uniform')
    for a, b in (('in_place', 'restage'), ('unrecorded', 'restage'), ('in_place_w0', 'restage_w0')):
        assert len(runs[a]) == len(runs[b])
        for ra, rb in zip(runs[a], runs[b]):
            for k in ('coeffs', 'mass', 'n_unsupported', 'active'):
                assert ra[k].dtype == rb[k].dtype and ra[k].tobytes() == rb[k].tobytes(), (a, k)
            assert _bytes(ra['labels']) == _bytes(rb['labels']), a
            if a == 'unrecorded':
                assert ra['weights'] is None
            else:
                assert _bytes(ra['weights']) == _bytes(rb['weights']), a
            assert [[r is None for r in g] for g in ra['results']] == [[r is None for r in g] for g in rb['results']]
    assert runs['restage'][0]['coeffs'].tobytes() != runs['restage'][1]['coeffs'].tobytes()     # the iterations did move the models


# ---- the launch switches, each in a fresh child process -------------------------------------------------------------------------------
SWITCHES = [('host-binning', {'EINCM_HOST_BINNING': '1'}), ('no-segsort', {'EINCM_NO_SEGSORT': '1'}), ('no-spread', {'EINCM_NO_SPREAD': '1'})]


@pytest.mark.parametrize('tag,env_extra', SWITCHES, ids=[s[0] for s in SWITCHES])
def test_set_weights_under_a_launch_switch(built_lib, tmp_path, tag, env_extra):
    out = str(tmp_path / f'{tag}.npz')
    env = {k: v for k, v in os.environ.items() if not k.startswith('EINCM_') or k == 'EINCM_LIB'}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, '_reweight_probe.py'), out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
    got = dict(np.load(out))
    assert json.loads(str(got.pop('env'))) == env_extra                  # the child saw this switch and no other
    off = np.concatenate([[0], np.cumsum(RS.N)])
    for o in (got.pop('order_splat'), got.pop('order_gather')):
        assert np.array_equal(np.sort(o), np.arange(sum(RS.N)))
        assert all(((o[off[b]:off[b + 1]] >= off[b]) & (o[off[b]:off[b + 1]] < off[b + 1])).all() for b in range(RS.B))
    keys = sorted(k[len('fresh_'):] for k in got if k.startswith('fresh_'))
    assert len(keys) == 10 and sorted(got) == sorted(['fresh_' + k for k in keys] + ['inplace_' + k for k in keys])
    for k in keys:
        a, b = got['inplace_' + k], got['fresh_' + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k)


# ---- an engine that never asks for it pays nothing -------------------------------------------------------------------------------------
def test_an_engine_that_never_keeps_order_holds_the_memory_of_before(scene):
    """Engine.memory() of Engine((64, 96), 4000, max_refs=2, max_windows=4) at the parent commit 893d349, read there once on an MI355X:
    after the constructor PARENT_MEMORY[0]; after an unweighted staging of the scene and a loss_grad at the 8 x 8 theta
    PARENT_MEMORY[1]; after a staging with the first weight set and the same loss_grad PARENT_MEMORY[2].  A keep-order staging adds
    three arrays of 4 B per event of the engine's capacity, once."""
    got = []
    with _engine() as eng:
        got.append(tuple(eng.memory()))
        eng.set_windows(RS.staged(scene, None))
        eng.loss_grad(scene['theta8'], P0)
        got.append(tuple(eng.memory()))
        eng.set_windows(RS.staged(scene, scene['w1']))
        eng.loss_grad(scene['theta8'], P0)
        got.append(tuple(eng.memory()))
        print('MEMORY', got)
        assert got == PARENT_MEMORY
        eng.set_windows(RS.staged(scene, scene['w1']), keep_order=True)
        m = eng.memory()
        assert m.device_bytes == got[2][0] + 3 * 4 * sum(RS.N) and m.pinned_bytes == got[2][1] and m.scratch_bytes == got[2][3]
        eng.set_weights(scene['w2'])
        eng.loss_grad(scene['theta8'], P0)
        eng.set_windows(RS.staged(scene, scene['w2']), keep_order=True)
        assert eng.memory() == m                                         # once: neither a re-weighting nor a second staging allocates


# (device_bytes, pinned_bytes, allocations, scratch_bytes) at 893d349
PARENT_MEMORY = [(4187980, 797024, 63, 0), (4198220, 797024, 65, 0), (4230220, 797024, 67, 0)]
