"""The per-event scores without a GPU: the entry point in the header, the binding and the library; where the
kernel and the rules live; every refusal of the Python layer with a stub in the library's place; weights_from_scores on hand-made
inputs; the Python restatement of the layout against the header's; and the conditions that keep tests/test_gpu_event_scores.py
honest, asserted from the witness alone for every generated case."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import _event_scores_witness as ES
import _host_check as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module('edge-informed-contrast-maximization_amd._lib')
E = importlib.import_module('edge-informed-contrast-maximization_amd.engine')
staging = importlib.import_module('edge-informed-contrast-maximization_amd.staging')
evaluation = importlib.import_module('edge-informed-contrast-maximization_amd.evaluation')
synth = importlib.import_module('edge-informed-contrast-maximization_amd.synth')

NAME = 'eincm_event_scores'
# the Python entry points: a tree without them has nothing that this module could test
event_scores, weights_from_scores, layout = E.Engine.event_scores, staging.weights_from_scores, E.event_scores_layout


# ---- the entry point ---------------------------------------------------------------------------------------------------------
def test_entry_point_in_header_binding_and_library(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'eincm.h')).read()
    m = re.search(r'int\s+' + NAME + r'\s*\(([^)]*)\)', hdr)
    assert m, 'not declared'
    args = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert args == ['eincm_ctx* ctx', 'const float* images', 'const double* ref_weights', 'float* scores', 'float* selfs']
    defines = dict(re.findall(r'#define\s+(EINCM_[A-Z0-9_]+)\s+(\d+)\b', hdr))
    assert int(defines['EINCM_ABI_VERSION']) == 6
    assert NAME in hdr.split('#define EINCM_ABI_VERSION')[1].split('*/')[0], 'not in the name list after EINCM_ABI_VERSION'
    doc = hdr.split('int ' + NAME)[0].rsplit('/*', 1)[1]
    for words in ('H, W >= 3', 'fixed order', 'dy = -1, 0, +1', 'No atomics', 'exactly 0', 'in this order', 'ascending r'):
        assert words in doc, words
    assert [n for n, _, _ in L.SIGNATURES].count(NAME) == 1
    res, a = {n: (r, a) for n, r, a in L.SIGNATURES}[NAME]
    assert res is C.c_int and a == [C.c_void_p] * 5
    fn = getattr(built_lib, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == a
    assert built_lib.eincm_abi_version() == 6
    assert fn(None, None, None, None, None) == L.ERR_ARG      # no context: refused without a GPU


def test_kernel_lives_in_its_own_header_and_the_rules_in_a_hip_free_one():
    csrc = os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc')
    rules = open(os.path.join(csrc, 'eincm_event_scores.h')).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', rules)
    assert 'hip' not in ''.join(includes).lower()
    for fn in ('sc_check', 'sc_code', 'sc_why', 'sc_block_len', 'sc_block_offset', 'sc_total'):
        assert re.search(r'\b' + fn + r'\(', rules), fn
    kern = open(os.path.join(csrc, 'eincm_event_scores.hip.h')).read()
    assert re.search(r'__global__[^;{]*\bk_event_scores\(', kern)
    code = re.sub(r'//[^\n]*', '', kern)
    for fn in ('warp_axis(', 'taps3x2(', 'clamp_far(', 'wrap_drop(', '#pragma clang fp contract(off)'):
        assert fn in code, fn
    assert 'atomic' not in code and '__shfl' not in code and '__shared__' not in code      # one thread owns a cell
    shared = open(os.path.join(csrc, 'eincm_kernels.hip.h')).read()
    for fn in ('warp_axis', 'taps3x2', 'clamp_far', 'wrap_drop'):                            # reused, not restated
        assert not re.search(r'__device__[^;{]*\b' + fn + r'\(', kern) and re.search(r'__device__[^;{]*\b' + fn + r'\(', shared), fn
    api = open(os.path.join(csrc, 'eincm_api.hip')).read()
    body = api.split('int ' + NAME + '(')[1].split('\n}\n')[0]
    assert 'sc_check(' in body and 'OneShot op(c);' in body and 'ensure_theta_image(c)' in body
    assert body.index('sc_check(') < body.index('ensure_theta_image(c)') < body.index('OneShot op(c);')
    assert 'sc_total(' in body and 'sc_block_offset(' in body and 'op.launch(' in body and 'hipMalloc' not in body
    assert 'd_w' not in body                                                                # the staged weights are never read


# ---- the refusals, with a stub in the library's place ---------------------------------------------------------------------------
class NoGpu:
    """Stands where the library is: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was reached: a library call')


class Reached(Exception):
    pass


class Records:
    """Stands where the library is: eincm_event_scores records its arguments and ends the call."""
    def __init__(self):
        self.calls = []

    def eincm_event_scores(self, *a):
        self.calls.append(a)
        raise Reached()


def stub_engine(lib=None, B=2, R=3, H=5, W=7, n=(4, 6), weights='ones'):
    eng = E.Engine.__new__(E.Engine)
    eng._ctx, eng._lib = None, lib or NoGpu()
    eng.precision, eng.splat_window, eng.B, eng.R, eng.H, eng.W = 'fp32', 3, B, R, H, W
    eng._io, eng.n_events = {}, np.array(n, dtype=np.int64)
    if weights == 'ones':
        eng._staged_weights = [None] * B
    elif weights is not None:
        eng._staged_weights = weights
    return eng


def test_a_good_call_reaches_the_library_with_the_layout_s_sizes():
    lib = Records()
    eng = stub_engine(lib)
    for kw in (dict(), dict(images=np.zeros((2, 3, 5, 7))), dict(ref_weights=[0.25, 0.5, 0.25]), dict(exclude_self=True),
               dict(images=np.zeros((2, 3, 5, 7), dtype=np.uint8), ref_weights=np.array([1, 0, -1]), exclude_self=True)):
        with pytest.raises(Reached):
            eng.event_scores(**kw)
        _, images, rw, scores, selfs = lib.calls[-1]
        assert (images is None) == ('images' not in kw) and (rw is None) == ('ref_weights' not in kw)
        assert scores is not None and (selfs is None) == (not kw.get('exclude_self'))
    one = stub_engine(lib, B=1, n=(4,))
    with pytest.raises(Reached):
        one.event_scores(images=np.zeros((3, 5, 7)))                       # (R,H,W) stands for the batch when B == 1
    assert lib.calls[-1][1] is not None


BAD = [('images-3d-for-a-batch', dict(images=np.zeros((3, 5, 7))), 'images must be'),
       ('images-wrong-windows', dict(images=np.zeros((1, 3, 5, 7))), 'images must be'),
       ('images-wrong-refs', dict(images=np.zeros((2, 2, 5, 7))), 'images must be'),
       ('images-transposed', dict(images=np.zeros((2, 3, 7, 5))), 'images must be'),
       ('images-strings', dict(images=np.zeros((2, 3, 5, 7), dtype='U1')), 'numbers'),
       ('ref-weights-nan', dict(ref_weights=[0.5, np.nan, 0.5]), 'finite'), ('ref-weights-inf', dict(ref_weights=[np.inf, 0.0, 0.5]), 'finite'),
       ('ref-weights-short', dict(ref_weights=[0.5, 0.5]), r'ref_weights must be \(3,\)'),
       ('ref-weights-2d', dict(ref_weights=np.ones((3, 1))), 'ref_weights must be'),
       ('theta-without-params', dict(theta=np.zeros((2, 1, 1, 2))), 'go together'), ('params-without-theta', dict(params=object()), 'go together')]


@pytest.mark.parametrize('name,kw,match', BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_value_errors_before_any_library_call(name, kw, match):
    with pytest.raises(ValueError, match=match):
        stub_engine().event_scores(**kw)


def test_exclude_self_without_the_staged_weights_is_a_value_error_before_any_library_call():
    for eng in (stub_engine(weights=None), stub_engine(weights=[None])):       # never kept; kept for another batch
        with pytest.raises(ValueError, match='does not hold them'):
            eng.event_scores(exclude_self=True)
    eng = stub_engine(Records())
    eng._staged_weights = None
    with pytest.raises(Reached):                                               # ... and nobody asks for them otherwise
        eng.event_scores()


def test_the_one_window_convenience_checks_before_it_asks_for_an_engine():
    x, y, t = np.arange(6) % 7, np.arange(6) % 5, np.linspace(0, 1, 6)
    edges, edge_ts = np.zeros((3, 5, 7)), np.array([0.0, 0.5, 1.0])
    th = np.zeros((1, 1, 2))
    for kw, match in ((dict(source='zero_iwe'), 'source'), (dict(source='edges', exclude_self=True), 'exclude_self'),
                      (dict(ref_weights=[1.0, np.nan, 1.0]), 'finite'), (dict(sensor_size=(7, 5)), 'edges must be'),
                      (dict(event_weights=np.full(6, 2.0)), r'within \[0, 1\]')):
        with pytest.raises(ValueError, match=match):
            evaluation.event_scores(th, x, y, t, edges, edge_ts, engine=stub_engine(), **kw)
    with pytest.raises(ValueError, match='theta must be'):
        evaluation.event_scores(np.zeros((1, 2)), x, y, t, edges, edge_ts, engine=stub_engine())


def test_signatures_of_the_python_layer():
    p = inspect.signature(E.Engine.event_scores).parameters
    assert list(p) == ['self', 'images', 'ref_weights', 'exclude_self', 'theta', 'params']
    assert [p[k].default for k in list(p)[1:]] == [None, None, False, None, None]
    p = inspect.signature(evaluation.event_scores).parameters
    assert list(p)[:7] == ['theta', 'xs', 'ys', 'ts', 'edges', 'edge_ts', 'source'] and p['source'].default == 'iwe' and p['engine'].default is None
    p = inspect.signature(staging.weights_from_scores).parameters
    assert list(p) == ['scores', 'ref_weights', 'full_score'] and p['ref_weights'].default is None and p['full_score'].default is None


# ---- weights_from_scores ---------------------------------------------------------------------------------------------------------
def test_weights_from_scores_on_hand_made_inputs():
    w = weights_from_scores(np.array([0.0, 1.0, 2.0, 4.0, -3.0]))
    assert w.dtype == np.float32 and np.array_equal(w, np.float32([0.0, 0.5, 1.0, 1.0, 0.0]))      # median of (1, 2, 4) = 2
    assert np.array_equal(weights_from_scores([0.5, 1.0, 3.0], full_score=2.0), np.float32([0.25, 0.5, 1.0]))
    s = np.array([[1.0, 0.0, 4.0], [3.0, 0.0, 8.0]])
    assert np.array_equal(weights_from_scores(s, ref_weights=[0.5, 0.5], full_score=4.0), np.float32([0.5, 0.0, 1.0]))
    assert np.array_equal(weights_from_scores(s, ref_weights=[1.0, -1.0], full_score=1.0), np.float32([0.0, 0.0, 0.0]))
    # the default over r is the loss's own weighting of the reference times (oracle: compute_weights_for_multi_reference)
    from oracle import eincm_oracle as O
    s3 = np.array([[1.0, 2.0], [3.0, 1.0], [5.0, 0.5]])
    want = O.compute_weights_for_multi_reference(3) @ s3
    assert np.allclose(weights_from_scores(s3, full_score=10.0), want / 10.0, rtol=1e-7, atol=0)
    assert np.array_equal(weights_from_scores(np.zeros(4)), np.zeros(4, np.float32))                # nothing positive: full_score 1
    assert weights_from_scores(np.zeros(0)).shape == (0,)
    assert E.check_event_weights(weights_from_scores(np.random.default_rng(0).normal(size=50)), 50).dtype == np.float32
    for bad, kw in (([1.0, np.nan], {}), (np.zeros((2, 2, 2)), {}), ([1.0, 2.0], dict(full_score=0.0)), ([1.0, 2.0], dict(full_score=np.inf)),
                    ([1.0, 2.0], dict(ref_weights=[1.0, 1.0])), (np.ones((2, 3)), dict(ref_weights=[1.0])),
                    (np.ones((2, 3)), dict(ref_weights=[1.0, np.nan]))):
        with pytest.raises(ValueError):
            weights_from_scores(bad, **kw)


# ---- the layout: the Python restatement against the header's ------------------------------------------------------------------
LAYOUTS = [(3, []), (3, [0]), (3, [7]), (1, [7]), (3, [5, 0, 9]), (2, [0, 0, 0]), (4, [0, 3, 0]), (5, [1, 40, 0, 1000000, 1]),
           (8, [400000000, 1, 400000000])]


def test_layout_in_python_is_the_header_s(tmp_path_factory):
    exe = HC.build(tmp_path_factory, 'event_scores_check')
    cases = {}
    for i, (R, ne) in enumerate(LAYOUTS):
        for combined in (0, 1):
            HC.add_case(cases, (i, combined), 'layout', R, combined, len(ne), *ne)
    out = HC.run(exe, cases, tmp_path_factory, 'event_scores_layouts')
    for (i, combined), (total, off, length) in out.items():
        R, ne = LAYOUTS[i]
        o, ln, tot = layout(ne, R, bool(combined))
        assert tot == int(total[0]) and o.dtype == np.int64 and ln.dtype == np.int64
        assert np.array_equal(o, HC.i(off)) and np.array_equal(ln, HC.i(length))


# ---- what keeps the GPU module honest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('source', ['iwe', 'stack'])
@pytest.mark.parametrize('name', sorted(ES.GENERATED))
def test_every_generated_case_meets_the_conditions(name, source):
    c = ES.generated(name)
    Th = ES.sensor_theta(c['theta'], c['shape'])
    ev = (c['xs'], c['ys'], c['ts'], c['edge_ts'])
    F = ES.oracle_iwes(Th, *ev, c['shape']) if source == 'iwe' else c['stack']
    w = ES.event_scores(F, Th, *ev)
    z = ES.event_scores(F, np.zeros_like(Th), *ev)
    assert w['scores'].shape == (c['R'], len(c['xs']))
    assert ((w['wrapped'] + w['dropped']) > 0).mean() >= 0.05
    assert (w['wrapped'] > 0).any() and ((w['dropped'] > 0).any() or len(c['xs']) == 1)      # (one event cannot do both)
    assert (w['scores'] > 0).mean() >= 0.5
    assert (np.abs(w['scores'] - z['scores']) > ES.TOL * np.maximum(w['M'], z['M'])).mean() >= 0.5
    alive = w['dropped'] < 9
    assert np.all((w['selfs'][alive] > 0) & (w['selfs'][alive] < w['ksum'][alive]))
    assert np.all(w['selfs'][~alive] == 0) and np.all(w['scores'][~alive] == 0) and np.all(w['M'][~alive] == 0)
    # the combined form is the weighted sum of the rows, magnitudes by |omega|
    om = np.linspace(-0.5, 1.0, c['R'])
    cw = ES.event_scores(F, Th, *ev, ref_weights=om)
    om32 = om.astype(np.float32).astype(np.float64)
    assert np.array_equal(cw['scores'], om32 @ w['scores']) and np.array_equal(cw['M'], np.abs(om32) @ w['M'])


def test_generated_cases_cover_the_shapes_and_counts():
    specs = ES.GENERATED.values()
    assert {s[0] for s in specs} == {(33, 65), (60, 80)} and {s[2] for s in specs} == {1, 3}
    assert {s[1] for s in specs if s[0] == (33, 65)} == {(3, 5)} and {s[1] for s in specs if s[0] == (60, 80)} == {None}
    assert {1, 63, 64, 65, ES.NT - 1, ES.NT, ES.NT + 1} <= {s[3] for s in specs}
    kern = open(os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc', 'eincm_types.h')).read()
    assert int(re.search(r'constexpr int NT = (\d+);', kern).group(1)) == ES.NT


def test_witness_adjoint_identity_and_the_iwe_s_own_share():
    """<splat(1), F> = sum_e s_e for any F, and against the IWE an event alone on its pixels scores exactly its self term"""
    c = ES.generated('33x65-grid-r3')
    Th = ES.sensor_theta(c['theta'], c['shape'])
    ev = (c['xs'], c['ys'], c['ts'], c['edge_ts'])
    iwes = ES.oracle_iwes(Th, *ev, c['shape'])
    w = ES.event_scores(c['stack'], Th, *ev)
    lhs = (iwes * c['stack'].astype(np.float64)).sum(axis=(1, 2))
    assert np.allclose(w['scores'].sum(axis=1), lhs, rtol=1e-12, atol=0)
    one = tuple(a[:1] for a in ev[:3]) + (ev[3],)
    alone = ES.event_scores(ES.oracle_iwes(Th, *one, c['shape']), Th, *one)
    assert np.allclose(alone['scores'], alone['selfs'], rtol=1e-14, atol=0)


def test_signal_events_outscore_noise_events_leave_one_out():
    """The example's window (examples/event_scores.py) at the true flow, the oracle's IWE and the witness: the signal events' mean
    leave-one-out score exceeds the noise events' mean.  Only the ordering is asserted."""
    shape = (260, 346)
    win, is_noise = ES.noisy_window(synth, shape, 30000, 10000, 2)
    assert is_noise.sum() == 10000 and np.all(np.diff(win['ts']) >= 0)
    ev = (win['xs'], win['ys'], win['ts'], win['edge_ts'])
    F = ES.oracle_iwes(win['flow_gt'], *ev, shape)
    w = ES.event_scores(F, win['flow_gt'], *ev)
    loo = (w['scores'] - w['selfs']).mean(axis=0)
    print(f'mean leave-one-out score: signal {loo[~is_noise].mean():.3f}, noise {loo[is_noise].mean():.3f}')
    assert loo[~is_noise].mean() > loo[is_noise].mean()
