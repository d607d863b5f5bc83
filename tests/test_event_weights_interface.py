"""Per-event weights without a GPU: the host-side check of a weight array, the new entry point in header,
binding and cross-compiled library, the refusals that Python reaches before a library call, and self-checks of the fp64 witness
(tests/_event_weights_witness.py): all-ones weights against the oracle, the repetition identity (weights k/K against the oracle on
the list with event e repeated k_e times), and the autograd gradient against central differences."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

from oracle import eincm_oracle as O
import _event_weights_witness as EW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')
E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
losses = importlib.import_module('edge-informed-contrast-maximization_amd.losses')
staging = importlib.import_module('edge-informed-contrast-maximization_amd.staging')
sharding = importlib.import_module('edge-informed-contrast-maximization_amd.sharding')
synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')

NAME = 'eincm_set_windows_weighted'


# ---- check_event_weights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [np.array([0.0, 0.25, 1.0], dtype=np.float32), np.array([0.0, 0.1, 1.0], dtype=np.float64),
                               np.array([0, 1, 1], dtype=np.int64), np.array([1, 0, 1], dtype=np.uint8), np.array([True, False, True]),
                               [0.5, 0.5, 0.5]])
def test_check_event_weights_accepts(w):
    got = E.check_event_weights(w, 3)
    assert got.dtype == np.float32 and got.shape == (3,) and got.flags.c_contiguous
    assert np.array_equal(got, np.asarray(w, dtype=np.float64).astype(np.float32))


def test_check_event_weights_rounds_to_float32_once():
    w = np.array([0.1, 1.0 / 3.0, 0.7], dtype=np.float64)
    assert np.array_equal(E.check_event_weights(w, 3), w.astype(np.float32))
    assert np.array_equal(EW.staged_weights(w, 3), w.astype(np.float32).astype(np.float64))
    assert E.check_event_weights(np.zeros(0), 0).shape == (0,)


class NoGpu:
    """Stands where the library is: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


def stub_engine(precision='fp32', splat_window=3, H=20, W=26):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = precision, splat_window, 0, 0, H, W
    eng._io = {}
    return eng


def _tiny_window(n=5, H=20, W=26, R=2):
    return (np.arange(n, dtype=np.int16), np.arange(n, dtype=np.int16), np.linspace(0.0, 1.0, n), np.zeros((R, H, W)), np.array([0.0, 1.0]))


@pytest.mark.parametrize('bad', [np.ones(4), np.ones(6), np.ones((5, 1)), np.array([1, 1, np.nan, 1, 1]), np.array([1, 1, np.inf, 1, 1]),
                                 np.array([1, 1, -np.inf, 1, 1]), np.array([1, 1, -1e-9, 1, 1]), np.array([1, 1, 1 + 1e-6, 1, 1]),
                                 np.array(['a'] * 5)])
def test_bad_weights_are_value_errors_before_any_library_call(bad):
    with pytest.raises(ValueError):
        E.check_event_weights(bad, 5)
    with pytest.raises(ValueError):
        stub_engine().set_windows([_tiny_window() + (bad,)])
    with pytest.raises(ValueError):
        stub_engine().set_window(*_tiny_window(), weights=bad)


def test_tuples_of_other_lengths_are_refused():
    with pytest.raises(ValueError, match='elements'):
        stub_engine().set_windows([_tiny_window()[:4]])
    with pytest.raises(ValueError, match='elements'):
        stub_engine().set_windows([_tiny_window() + (None, None)])


def test_staging_takes_the_weighted_entry_point_only_with_weights():
    with pytest.raises(AssertionError, match='eincm_set_windows_ptrs was reached'):
        stub_engine().set_windows([_tiny_window()])
    with pytest.raises(AssertionError, match='eincm_set_windows_ptrs was reached'):
        stub_engine().set_windows([_tiny_window() + (None,)])
    with pytest.raises(AssertionError, match=NAME + ' was reached'):
        stub_engine().set_windows([_tiny_window() + (np.ones(5),), _tiny_window()])
    assert stub_engine().weighted is False


# ---- the entry point ---------------------------------------------------------------------------------------------------------
def test_entry_point_in_header_binding_and_library(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    m = re.search(r'int\s+' + NAME + r'\s*\(([^)]*)\)', hdr)
    assert m, 'not declared'
    args = [a.strip() for a in m.group(1).split(',')]
    ptrs = re.search(r'int\s+eincm_set_windows_ptrs\s*\(([^)]*)\)', hdr)
    base = [a.strip() for a in ptrs.group(1).split(',')]
    # eincm_set_windows_ptrs' shape plus the weights in front of the flags
    assert args == base[:-1] + ['const float* const* weights', 'uint32_t flags']
    assert int(dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)\b', hdr))['EINCM_ABI_VERSION']) == 6
    table = {n: (res, a) for n, res, a in L.SIGNATURES}
    assert [n for n, _, _ in L.SIGNATURES].count(NAME) == 1
    res, a = table[NAME]
    pres, pa = table['eincm_set_windows_ptrs']
    assert res is C.c_int and a == pa[:-1] + [C.POINTER(C.c_void_p), C.c_uint32]
    fn = getattr(built_lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == a
    raw = C.CDLL(os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'libeincm_hip.so'))
    assert hasattr(raw, NAME)
    assert fn(None, 1, 1, None, None, None, None, None, None, None, 0) == L.ERR_ARG        # no context: refused without a GPU


# ---- the refusals --------------------------------------------------------------------------------------------------------------
def test_fused_motion_refusal_takes_the_weighted_state():
    p = E.make_params(20.0, 35.0, 0.0, 0.0, 1)
    assert list(inspect.signature(E.motion_fused_refusal).parameters) == ['precision', 'splat_window', 'params', 'weighted']
    assert inspect.signature(E.motion_fused_refusal).parameters['weighted'].default is False
    assert E.motion_fused_refusal('fp32', 3, p) is None and E.motion_fused_refusal('fp32', 3, p, False) is None
    why = E.motion_fused_refusal('fp32', 3, p, True)
    assert 'weight' in why and 'fused' in why


def test_fused_motion_path_refuses_a_weighted_batch_and_auto_falls_back():
    motion = importlib.import_module('edge-informed-contrast-maximization_amd.motion')
    model = motion.MotionModel('affine', (20, 26))
    p = E.make_params(20.0, 35.0, 0.0, 0.0, 1)

    def eng(path, weighted):
        e = stub_engine()
        e.motion_path, e.motion_model, e.B, e.R, e.n_events, e._weighted = path, model, 2, 2, np.array([100, 100]), weighted
        return e
    with pytest.raises(ValueError, match='weight'):
        eng('fused', True).loss_grad_motion(np.zeros((2, 6)), p)
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion was reached'):
        eng('auto', True).loss_grad_motion(np.zeros((2, 6)), p)
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion was reached'):
        eng('expanded', True).loss_grad_motion(np.zeros((2, 6)), p)
    with pytest.raises(AssertionError, match='eincm_loss_grad_motion_fused was reached'):
        eng('fused', False).loss_grad_motion(np.zeros((2, 6)), p)


def test_fp64_and_other_splat_windows_refuse_weighted_batches_at_staging():
    assert E.event_weights_refusal('fp32', 3) is None
    assert 'fp64' in E.event_weights_refusal('fp64', 3)
    assert '3x3 splat window' in E.event_weights_refusal('fp32', 5)
    assert 'sharded' in E.event_weights_refusal('fp32', 3, sharded=True)
    win = _tiny_window() + (np.ones(5),)
    with pytest.raises(ValueError, match='fp64'):
        stub_engine(precision='fp64').set_windows([win])
    with pytest.raises(ValueError, match='3x3 splat window'):
        stub_engine(splat_window=5).set_windows([win])
    with pytest.raises(ValueError, match='sharded'):
        stub_engine().set_windows([win], defer_constants=True)
    # unweighted batches go on to the library on all three
    for kw in (dict(precision='fp64'), dict(splat_window=5)):
        with pytest.raises(AssertionError, match='eincm_set_windows_ptrs was reached'):
            stub_engine(**kw).set_windows([win[:5]])
    # a staged weighted batch keeps the 3x3 window
    eng = stub_engine()
    eng._weighted = True
    with pytest.raises(ValueError, match='3x3 splat window'):
        eng.set_splat_window(5)


def test_sharded_engine_refuses_weighted_batches_at_staging():
    win = _tiny_window()
    sharding.check_unweighted([win, win + (None,)])
    with pytest.raises(ValueError, match='window 1 carries per-event weights'):
        sharding.check_unweighted([win, win + (np.ones(5),)])
    sh = sharding.ShardedEngine.__new__(sharding.ShardedEngine)
    sh.eng, sh.dist = NoGpu(), NoGpu()
    with pytest.raises(ValueError, match='per-event weights'):
        sh.set_windows([win + (np.ones(5),)])


def test_c_side_states_the_same_refusals():
    api = open(os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc', 'eincm_api.hip')).read()
    for phrase in ('per-event weights are not supported in fp64 mode', 'per-event weights have the 3x3 splat window only',
                   'per-event weights are not supported in an event-sharded staging', 'weights are finite and within [0, 1]'):
        assert phrase in api, phrase
    mo = open(os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc', 'eincm_motion.h')).read()
    assert 'the fused path has no weighted form' in mo


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_loss_callables_take_event_weights():
    for f in (losses.loss_func, losses.value_and_grad_loss_func, losses.handover_loss_func, losses.value_and_grad_handover_loss_func,
              losses.compute_loss_objectives, losses.motion_loss_func, losses.value_and_grad_motion_loss_func, losses.engine_for):
        assert inspect.signature(f).parameters['event_weights'].default is None, f.__name__
    assert inspect.signature(E.Engine.set_window).parameters['weights'].default is None
    assert isinstance(E.Engine.weighted, property)


def test_engine_cache_fingerprint_includes_the_weights():
    a = tuple(np.asarray(x) for x in _tiny_window())
    w1, w2 = np.linspace(0.0, 1.0, 5), np.linspace(1.0, 0.0, 5)
    assert losses._fingerprint(a + (w1,)) != losses._fingerprint(a + (w2,))
    assert losses._fingerprint(a + (w1,)) != losses._fingerprint(a)
    assert losses._fingerprint(a + (w1,)) == losses._fingerprint(a + (w1.copy(),))


def test_stage_datasample_returns_the_six_tuple_only_with_weights():
    n, H, W = 40, 20, 26
    rng = np.random.default_rng(0)
    ds = dict(events=dict(x=rng.integers(0, W, n), y=rng.integers(0, H, n), t=np.sort(rng.uniform(10.0, 20.0, n))),
              image_ts=np.array([10.0, 20.0]), eval_ts=(10.0, 20.0))
    edges = rng.uniform(0.0, 1.0, (2, H, W))
    five = staging.stage_datasample(ds, edges=edges)
    assert len(five) == 5
    w = rng.uniform(0.0, 1.0, n)
    six = staging.stage_datasample(ds, edges=edges, event_weights=w)
    assert len(six) == 6 and six[5].dtype == np.float32 and np.array_equal(six[5], w.astype(np.float32))
    for a, b in zip(five, six):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        staging.stage_datasample(ds, edges=edges, event_weights=w[:-1])


def test_batch_solver_forwards_the_tuples():
    bs = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
    src = inspect.getsource(bs.BatchedMultipleLevelEINCMSolver.set_datasamples)
    assert 'eng.set_windows([windows[b] for b in ix])' in src
    assert 'e.set_windows(windows[sl])' in inspect.getsource(E.EngineGroup.set_windows)


# ---- witness self-checks -------------------------------------------------------------------------------------------------------
SENSOR = (70, 100)


def _case(n=1500, R=2, seed=3):
    win = synth.make_window(seed, SENSOR, n, R, flow='smooth', flow_mag=5.0)
    return win, (win['xs'], win['ys'], win['ts'], win['edges'], win['edge_ts'])


def _mats(theta_hw, H, W, method='bilinear'):
    return (O.resample_matrix(theta_hw[0], H, H / theta_hw[0], method), O.resample_matrix(theta_hw[1], W, W / theta_hw[1], method))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.mark.parametrize('delta', [0.0, 0.3])
@pytest.mark.parametrize('gamma', [0.0, 2.5e-4])
@pytest.mark.parametrize('theta_hw', [(1, 1), (4, 4)])
def test_witness_with_all_ones_is_the_oracle(theta_hw, gamma, delta):
    win, args = _case()
    H, W = SENSOR
    theta = synth.theta_near_truth(1, win, theta_hw)
    v_o, g_o, aux = O.loss_and_grad(theta, *args, 20.0, 35.0, gamma, delta, 0, 5, SENSOR, 'bilinear', return_intermediates=True)
    for weights in (None, np.ones(len(args[0]))):
        v, g, G, I, terms = EW.loss_and_grad(theta, *args, 20.0, 35.0, gamma, delta, 0, *_mats(theta_hw, H, W), weights=weights)
        assert abs(v - v_o) <= 1e-12 * abs(v_o)
        assert _rel(g, g_o) <= 1e-12
        assert _rel(I, aux['_iwes']) <= 1e-12
        assert _rel(G, aux['_G']) <= 1e-12
        assert _rel(terms['zero_iwe'], aux['_zero_iwe']) <= 1e-12


@pytest.mark.parametrize('gamma', [0.0, 2.5e-4])
@pytest.mark.parametrize('theta_hw', [(1, 1), (4, 4)])
def test_repetition_identity_against_the_oracle(theta_hw, gamma):
    """Repeating event e k_e times gives the loss and the gradient of weighting it k_e / K: the loss is built from ratios and a min-max
    normalised IWE, and the TV mask leaves out the events of weight 0 as the repeated list leaves them out."""
    win, args = _case()
    H, W = SENSOR
    K = 4
    k = np.random.default_rng(11).integers(0, K + 1, len(args[0]))
    rep = np.repeat(np.arange(len(k)), k)
    theta = synth.theta_near_truth(1, win, theta_hw)
    v_o, g_o, aux = O.loss_and_grad(theta, args[0][rep], args[1][rep], args[2][rep], args[3], args[4], 20.0, 35.0, gamma, 0.0, 0, 5, SENSOR,
                                    'bilinear', return_intermediates=True)
    v, g, _, I, _ = EW.loss_and_grad(theta, *args, 20.0, 35.0, gamma, 0.0, 0, *_mats(theta_hw, H, W), weights=k / K)
    assert abs(v - v_o) <= 1e-12 * abs(v_o)
    assert _rel(g, g_o) <= 1e-12
    assert _rel(I * K, aux['_iwes']) <= 1e-12


@pytest.mark.parametrize('lvl,gamma', [(1, 0.0), (0, 2.5e-3)])
def test_witness_gradient_matches_central_differences(lvl, gamma):
    win, args = _case(n=800)
    H, W = SENSOR
    theta = synth.theta_near_truth(5, win, (2, 2))
    AH, AW = _mats((2, 2), H, W)
    rng = np.random.default_rng(7)
    weights = np.where(rng.random(len(args[0])) < 0.2, 0.0, rng.uniform(0.125, 1.0, len(args[0])))
    v, g, _, _, _ = EW.loss_and_grad(theta, *args, 20.0, 35.0, gamma, 0.0, lvl, AH, AW, weights=weights)
    h = 1e-6
    fd = np.zeros_like(theta)
    for idx in np.ndindex(theta.shape):
        tp, tm = theta.copy(), theta.copy()
        tp[idx] += h
        tm[idx] -= h
        fd[idx] = (EW.loss_value(tp, *args, 20.0, 35.0, gamma, 0.0, lvl, AH, AW, weights=weights)
                   - EW.loss_value(tm, *args, 20.0, 35.0, gamma, 0.0, lvl, AH, AW, weights=weights)) / (2 * h)
    assert np.abs(g - fd).max() <= 1e-5 * np.abs(fd).max() + 1e-9, (g, fd)


def test_witness_count_images_leave_out_weight_zero():
    win, args = _case(n=300)
    H, W = SENSOR
    Theta = O.scale_theta_to_sensor_size(synth.theta_near_truth(1, win, (2, 2)), SENSOR, 'bilinear')
    w = np.ones(300)
    w[::3] = 0.0
    keep = w > 0
    got = EW.count_images(Theta, args[0], args[1], args[2], args[4], w)
    ref = EW.count_images(Theta, args[0][keep], args[1][keep], args[2][keep], args[4])
    assert np.array_equal(got, ref) and got.sum() <= 2 * keep.sum()
    wx, wy = O.per_pix_warp(Theta, args[0][keep].astype(np.int64), args[1][keep].astype(np.int64), args[2][keep], args[4][0], 1.0)
    assert np.array_equal(got[0], O.rounded_count_image(wx, wy, SENSOR))
